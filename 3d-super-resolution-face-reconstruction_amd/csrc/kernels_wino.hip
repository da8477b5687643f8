// Winograd F(2x2, 3x3) for the exact-f32 3x3 / stride-1 convs of the deep UNet levels (prec 0).
//
//   Y = A^T [ (G g G^T) . (B^T d B) ] A          per 2x2 output tile, 4x4 input window d
//
//   B^T = | 1  0 -1  0 |     G = | 1    0    0  |     A^T = | 1  1  1  0 |
//         | 0  1  1  0 |         | 1/2  1/2  1/2|           | 0  1 -1 -1 |
//         | 0 -1  1  0 |         | 1/2 -1/2  1/2|
//         | 0  1  0 -1 |         | 0    0    1  |
//
// At <= 32x32 pixels, three passes per conv, all on one stream (64x64 and up: wino_fused_kernel, one pass):
//   1. the GroupNorm apply pass itself (gn_wino_input_kernel, kernels_misc.hip; ConvParams::u_ready), or
//      wino_input_kernel where no such pass precedes the conv (and under SR3_NO_GN_WINO=1):
//      U[pos][tile][Cin] = (B^T d B)[pos] over the zero-bordered input; in0 || in1 concatenated here.
//      wino_input_kernel reads the activated tensor (window origins (2ty, 2tx) in padded coordinates, so the borders
//      are already zero and nothing is masked); the apply pass activates the raw tensor on the way and never stores
//      the activated one: the same values through the same +-1 adds, so U is bit-identical either way.
//   2. launch_wino_gemm: M[pos] = U[pos] x V[pos] for the 16 positions, on the f32 implicit-GEMM kernel
//      (conv_igemm_dma_f32 as a 1x1 conv, blockIdx.z = position): fixed K order, no atomics.
//   3. wino_output_kernel: A^T M A per tile + bias + FeatureWiseAffine bias + residual into the zero-bordered output,
//      and the fused GroupNorm statistics (ConvParams::stats layout) in a fixed order.
// The fused 1x1 term (res_conv, ConvParams::in2 / in2b / w2) runs as a 1x1 conv on the direct kernel into the output
// first (with the conv's residual); the output transform then adds it as the residual.
// The operands and the accumulation stay fp32; the data transforms use only +-1, the weight transform (1/2) runs in fp64.
#include "sr3_internal.h"
#include <type_traits>

namespace sr3 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// one thread = 4 channels of one 2x2 output tile; consecutive threads take consecutive channel quads (coalesced)
__global__ __launch_bounds__(256) void wino_input_kernel(const TDesc in0, const TDesc in1, int B, float *__restrict__ U) {
    const int C0 = in0.C, C1 = in1.p ? in1.C : 0, Cin = C0 + C1, cq = Cin >> 2;
    const int th = in0.H >> 1, tw = in0.W >> 1;
    const unsigned ntiles = (unsigned)B * th * tw;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= ntiles * (unsigned)cq) return;
    const unsigned t = i / (unsigned)cq;
    const int c4 = (int)(i - t * (unsigned)cq) * 4;
    const int tx = (int)(t % (unsigned)tw);
    const unsigned r = t / (unsigned)tw;
    const int ty = (int)(r % (unsigned)th), n = (int)(r / (unsigned)th);
    const bool first = c4 < C0;
    const int C = first ? C0 : C1;
    const int Wp = in0.Wp();
    const float *b = (first ? in0.p : in1.p) + ((size_t)(n * in0.Hp() + 2 * ty) * Wp + 2 * tx) * C + (first ? c4 : c4 - C0);
    f32x4 d[4][4];
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 4; ++x) d[y][x] = *reinterpret_cast<const f32x4 *>(b + ((size_t)y * Wp + x) * C);
    f32x4 e[4][4];            // B^T d
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        e[0][x] = d[0][x] - d[2][x];
        e[1][x] = d[1][x] + d[2][x];
        e[2][x] = d[2][x] - d[1][x];
        e[3][x] = d[1][x] - d[3][x];
    }
    const size_t plane = (size_t)ntiles * Cin;
    float *o = U + (size_t)t * Cin + c4;
#pragma unroll
    for (int a = 0; a < 4; ++a) {   // (B^T d) B
        *reinterpret_cast<f32x4 *>(o + (size_t)(a * 4 + 0) * plane) = e[a][0] - e[a][2];
        *reinterpret_cast<f32x4 *>(o + (size_t)(a * 4 + 1) * plane) = e[a][1] + e[a][2];
        *reinterpret_cast<f32x4 *>(o + (size_t)(a * 4 + 2) * plane) = e[a][2] - e[a][1];
        *reinterpret_cast<f32x4 *>(o + (size_t)(a * 4 + 3) * plane) = e[a][1] - e[a][3];
    }
}

// block = 16 channel quads (64 channels) x 16 tile lanes over the tiles [slice * tps, (slice + 1) * tps) of image n
// (grid: Cout / 64, slices, B); the statistics of the block's 64 channels go to slice `slice` of the image, its
// tile lanes added in lane order
__global__ __launch_bounds__(256) void wino_output_kernel(const ConvParams p, const float *__restrict__ Mw, int slices) {
    __shared__ double2 red[16][64];
    const int Cout = p.out.C, th = p.Hout >> 1, tw = p.Wout >> 1;
    const int q = threadIdx.x & 15, tl = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + q * 4;
    const int slice = blockIdx.y, n = blockIdx.z;
    const int tps = th * tw / slices;
    const size_t plane = (size_t)p.B * th * tw * Cout;
    f32x4 bias = {0.f, 0.f, 0.f, 0.f}, cb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (p.bias) bias[j] = p.bias[c + j];
        if (p.chan_bias) cb[j] = p.chan_bias[(size_t)n * p.chan_bias_stride + c + j];
    }
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    for (int k = tl; k < tps; k += 16) {
        const int tt = slice * tps + k;
        const int ty = tt / tw, tx = tt - ty * tw;
        const float *m = Mw + ((size_t)n * th * tw + tt) * Cout + c;
        f32x4 v[16];
#pragma unroll
        for (int ps = 0; ps < 16; ++ps) v[ps] = *reinterpret_cast<const f32x4 *>(m + ps * plane);
        f32x4 u0[4], u1[4];       // A^T M
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            u0[b] = v[b] + v[4 + b] + v[8 + b];
            u1[b] = v[4 + b] - v[8 + b] - v[12 + b];
        }
        f32x4 y[2][2];            // (A^T M) A
        y[0][0] = u0[0] + u0[1] + u0[2];
        y[0][1] = u0[1] - u0[2] - u0[3];
        y[1][0] = u1[0] + u1[1] + u1[2];
        y[1][1] = u1[1] - u1[2] - u1[3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int oy = 2 * ty + r, ox = 2 * tx + cc;
                f32x4 add = bias;   // (the direct kernel's epilogue order: bias, residual, FeatureWiseAffine bias)
                if (p.resid.p) add += *reinterpret_cast<const f32x4 *>(p.resid.p + p.resid.pix(n, oy, ox) * Cout + c);
                if (p.chan_bias) add += cb;
                const f32x4 o = y[r][cc] + add;
                *reinterpret_cast<f32x4 *>(p.out.p + p.out.pix(n, oy, ox) * Cout + c) = o;
#pragma unroll
                for (int j = 0; j < 4; ++j) { s1[j] += (double)o[j]; s2[j] = fma((double)o[j], (double)o[j], s2[j]); }
            }
    }
    if (p.stats == nullptr) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) red[tl][q * 4 + j] = make_double2(s1[j], s2[j]);
    __syncthreads();
    if (threadIdx.x < 64) {
        double a = 0, b = 0;
        for (int l = 0; l < 16; ++l) { const double2 t2 = red[l][threadIdx.x]; a += t2.x; b += t2.y; }
        double *o = p.stats + (((size_t)n * p.stats_slices + slice) * Cout + blockIdx.x * 64 + threadIdx.x) * 2;
        o[0] = a; o[1] = b;
    }
}

// ---- one-pass form for the 64x64- and 128x128-pixel levels ----------------------------------------------------------
// Block = one strip of WF_T = 32 tiles along a tile row x WF_BN = 64 output channels; wave a (0..3) owns row a of the
// 4x4 positions (4a + b, b = 0..3), so U and M never leave the CU:
//   * the strip's 4 x 66 padded input pixels x 32 channels are staged per K-step by LDS-DMA (two stages, 16-B chunk c
//     of pixel column x at c ^ ((x >> 1) & 7));
//   * lane (li, h) of wave a reads the two window rows that (B^T d)[a] needs for tile li and 4 channels (same +-1 adds as
//     wino_input_kernel) and forms U[4a + b] for b = 0..3: exactly its A operands of v_mfma_f32_32x32x2_f32
//     (lane half h, element j -> channel 8kk + 4h + j, as in conv_igemm_dma_f32);
//   * the B operand comes straight from the fragment-major copy of the transformed weights [16][CinPad/8][Cout][8]
//     (make_wino_weights_frag; one 16-B load per lane, L2-resident): the 64 lanes of one load read 32 output channels
//     x 8 input channels = 1 KiB of contiguous memory, whole 128-B lines (in the [16][Cout][CinPad] layout of the
//     three-pass path the same load touches 32 rows of 32 B each, half of every L2 request);
//     the four waves multiply DIFFERENT positions, so a B tile staged in LDS would be read by one wave only, and the
//     16 positions x 64 channels x 32 input channels of one K-step (128 KiB) do not fit next to the input stages;
//   * epilogue: each wave folds its row over the columns of A (t_c = M[a] A[:, c]) in registers, the four rows meet in
//     LDS, y = A^T t, then the direct kernel's epilogue order (bias, residual, FeatureWiseAffine bias), the store and the
//     fused GroupNorm statistics (per tile in LDS, then per slice in tile order; spb slices per strip).
// Registers: 4 positions x 2 N-fragments x 16 accumulators = 128, one ring of four B pairs (32, each refilled right
// behind its MFMAs: see the K loop), two generations of window sums and one half-window landing area (48), the A operands
// of two positions (8), the nine held DMA offsets: 238 in all, 2 waves per SIMD.
// A 64-tile or 128-channel block doubles the accumulators (256: 1 wave per SIMD, nothing left for operands).
// One input tensor only (conv_plan): the engine writes x || skip as one tensor in the GroupNorm apply pass.
// Tile rows (R, as wino_up2_kernel): the block's 32 tiles are R tile rows of TPR = 32 / R tiles, R = 1 | 2 | 4 for widths
// 64k | 32 | 16 (R > 1: ConvPlan::wino_fused_rows, a form of the three-pass plan at the 32x32 and 16x16 levels). Lane li
// holds tile (li / TPR, li % TPR), which is tile li of the block in the image's row-major tile order, so the K loop, the
// fragment ring, the exchange and the statistics slices are R = 1's. A stage holds the block's 2R + 2 distinct padded
// input rows (2 ty + 0 .. 2R + 1) of 2 TPR + 2 padded columns, each once: tile row tr reads its 4 window rows from stage
// row 2 tr on, so the two rows that neighbouring tile rows share are fetched and stored once (staged per tile row they
// were 25 % | 37.5 % of the input DMA at R = 2 | 4). 264 | 204 | 180 live pixel rows of 32 floats, rounded up to whole
// LDS-DMA instructions: 264 | 208 | 184 rows, 33 | 26 | 23 instructions; the lanes of the last instruction past the
// live rows are switched off through bit 31 of their offset. At R > 1 every wave issues 7 | 6 instructions per stage,
// the 2 | 1 slots past the last instruction switched off the same way (they point behind the rows, still inside the
// stage). A stage is at least the 32 KiB that half of the epilogue exchange needs (R > 1: exactly; 28 | 24 slots of
// 1 KiB fit), two stages are at most 67584 B, so two blocks still fit in a CU's LDS.
constexpr int WF_T = 32;                    // 2x2 output tiles per block (R = 1: one strip of a tile row)
constexpr int WF_BN = 64;                   // output channels per block
template <int R>
struct WfGeom {
    static_assert(R == 1 || R == 2 || R == 4, "tile rows per block");
    static constexpr int TPR = WF_T / R;            // tiles per tile row of the block
    static constexpr int WX = 2 * TPR + 2;          // padded input columns of a tile row's windows
    static constexpr int SROWS = R == 1 ? 4 : 2 * R + 2;        // distinct padded input rows of the block's windows
    static constexpr int PIX = SROWS * WX;          // live pixel rows of 32 floats per LDS stage
    static constexpr int DMA = (PIX + 7) / 8;       // LDS-DMA instructions per stage (64 lanes x 16 B each)
    static constexpr int ROWS = DMA * 8;            // pixel rows they write (rows PIX .. ROWS - 1: lanes switched off)
    static constexpr int PER_WAVE = (DMA + 3) / 4;  // R > 1: instructions every wave issues per stage (R = 1: 8, and wave 0's 33rd)
    static constexpr int SLOTS = R == 1 ? DMA : 4 * PER_WAVE;   // 1-KiB destinations a stage needs room for
    static constexpr int XCHG = 4 * WF_T * WF_BN;   // floats of half the epilogue exchange
    static constexpr int STAGE = SLOTS * 256 > XCHG ? SLOTS * 256 : XCHG;       // floats per stage
    static constexpr size_t LDS = (size_t)2 * STAGE * sizeof(float);
    static_assert(R == 1 ? DMA == 33 && ROWS == PIX : PER_WAVE <= 8, "R = 1: eight instructions per wave and one more for wave 0");
    static_assert(LDS >= (size_t)4 * 2 * WF_T * WF_BN * sizeof(float), "epilogue exchange fits in the stages");
    static_assert(2 * LDS <= 160 * 1024, "two blocks per CU");
};

template <int N, class F>
__device__ __forceinline__ void wf_static_for(F &&f) {
    if constexpr (N > 0) {
        wf_static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// 64 lanes x 16 B from a wave-uniform base + per-lane byte offset into LDS at lds (wave-uniform) + lane * 16
__device__ __forceinline__ void wf_dma16(const char *sbase, unsigned voff, float *lds) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(sbase), 0, -1, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)lds, 16, (int)voff, 0, 0, 0);
}

template <int R>
__global__ __launch_bounds__(256, 2) void wino_fused_kernel(const ConvParams p, int spb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using G = WfGeom<R>;
    constexpr int TPR = G::TPR, WF_WX = G::WX, WF_STAGE = G::STAGE, WF_DMA = G::DMA;
    const int Cin = p.in0.C;                             // (one input tensor: conv_wino_taken)
    const int Cout = p.out.C, th = p.Hout >> 1, tw = p.Wout >> 1;
    const int spr = tw / TPR, spi = (th / R) * spr;      // blocks ("strips") per group of R tile rows / per image
    const int nbl = Cout / WF_BN;
    int bid = blockIdx.x;
    {   // XCD-aware remap (as conv_igemm_dma_f32): the channel blocks of one strip share an L2
        const int nwg = gridDim.x;
        const int xcd = bid & 7, loc = bid >> 3;
        const int qq = nwg >> 3, rr = nwg & 7;
        bid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + loc;
    }
    const int nb = bid % nbl, strip = bid / nbl;
    const int n = strip / spi, si = strip - n * spi;
    const int tg = si / spr;
    const int ty = tg * R, tx0 = (si - tg * spr) * TPR;  // the block's first tile row and column
    const int n0 = nb * WF_BN;
    const int a = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int Wp = p.in0.Wp();
    const size_t pix0 = ((size_t)n * p.in0.Hp() + 2 * ty) * Wp + 2 * tx0;     // window origin of the strip
    const char *src0 = reinterpret_cast<const char *>(p.in0.p + pix0 * Cin);
    if constexpr (R > 1) {
        // (block-uniform, but computed with vector multiplies: without this the compiler keeps the DMA descriptors in
        // vector registers and wraps every DMA instruction in a loop over their distinct values)
        const uint64_t s = reinterpret_cast<uint64_t>(src0);
        src0 = reinterpret_cast<const char *>((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)s) |
                                              ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(s >> 32)) << 32));
    }

    // LDS-DMA: wave a issues instructions i = a + 4m; lane -> pixel row 8i + (lane >> 3) of the stage (stage row r,
    // column x: padded input row 2 ty + r), stored chunk lane & 7.
    // The lane's byte offset of an instruction depends on lane, i, Wp and Cin only (the channel step c0 goes into the
    // descriptor's base), so the nine offsets of the wave are computed once here and held across the K loop: dvoff[m] for
    // i = a + 4m, dvoff[8] for the one from 32 on (R = 1; R > 1: the first 7 | 6). Recomputed per K-step they cost 13 vector instructions each (a
    // division by WF_WX, three 64-bit multiply-adds, the swizzle) beside the MFMAs, and the registers were held anyway
    // (for the row index the arithmetic started from). one() pins the offset itself, so the compiler neither
    // rematerialises it in the loop nor moves the arithmetic back in: a K-step issues its DMAs with no vector
    // arithmetic in front of them.
    // Nothing in the K loop issues a vector memory instruction under a branch that the compiler cannot count: the
    // s_waitcnt vmcnt(N) it inserts assume the fewest loads in flight, so a skipped DMA makes every later wait one
    // instruction stricter. A step with no next stage (on == false) is wave-uniform and switches its instructions off
    // in the descriptor: num_records = 0 puts every offset past its end (no memory request; the free stage may receive
    // zeros, which nobody reads); only R = 1's instruction 32 (m = 8, wave 0 alone) sits behind a wave-uniform branch,
    // and it goes first. At R > 1 nothing does: every wave issues PER_WAVE instructions, and a lane past the live rows
    // (the tail of the last instruction, the whole of a slot past it; fixed per wave, m and lane) holds an offset with
    // bit 31 set, which no live descriptor reaches.
    // A live descriptor ends at 2^31 - 1 bytes, so a live offset must stay below it:
    // (3 Wp + 65) * Cin * 4 + 128 < 2^31, i.e. Wp * Cin < 1.7e8 (the widest row of the UNet: 130 * 384 = 5e4);
    // R > 1: ((2R + 1) Wp + 2 TPR + 1) * Cin * 4 + 128 (stage row 2R + 1 is the last), with Wp = 2 TPR + 2 <= 34
    // (conv_plan checks it).
    unsigned dvoff[9];
    {
        const unsigned cs4 = (unsigned)Cin * 4u;
        auto lane_off = [&](int i) {
            const int q = 8 * i + (lane >> 3);
            const int r = q / WF_WX, x = q - r * WF_WX;
            const unsigned voff = (unsigned)(r * Wp + x) * cs4 + (unsigned)(((lane & 7) ^ ((x >> 1) & 7)) * 16);
            if constexpr (R == 1) return voff;
            else return q < G::PIX ? voff : 0x80000000u;
        };
        if constexpr (R == 1) {
#pragma unroll
            for (int m = 0; m < 8; ++m) dvoff[m] = lane_off(a + 4 * m);
            dvoff[8] = lane_off(32);
        } else {
#pragma unroll
            for (int m = 0; m < G::PER_WAVE; ++m) dvoff[m] = lane_off(a + 4 * m);
        }
    }
    auto issue = [&](int c0, int stage, bool on) {
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(src0 + (size_t)c0 * 4), 0, on ? 0x7fffffff : 0, 0x00020000);
        float *dst = smem + stage * WF_STAGE;
        auto one = [&](int i, unsigned &voff) {
            asm volatile("" : "+v"(voff));   // (held, not recomputed: see above)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst + i * 256), 16,
                                                     (int)voff, 0, 0, 0);
        };
        if constexpr (R == 1) {
            if (a == 0 && on) one(32, dvoff[8]);
        }
        wf_static_for<(R == 1 ? 8 : G::PER_WAVE)>([&](auto mc) { constexpr int m = decltype(mc)::value; one(a + 4 * m, dvoff[m]); });
    };

    // B fragments: lane (li, h) loads channels c0 + 8kk + 4h .. +3 of output channel n0 + 32ni + li, position 4a + b,
    // from w_wino_f[4a + b][(c0 + 8kk) / 8][n0 + 32ni + li][4h .. 4h + 3]
    // (buffer loads: a wave-uniform descriptor over the wave's 4 position planes, the uniform part of the offset in
    // soffset, the lane part in one VGPR — no 64-bit address arithmetic per load)
    const unsigned wlane = ((unsigned)(n0 + li) * 8u + 4u * h) * 4u;
    const size_t plane = (size_t)Cout * Cin;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w_wino_f + (size_t)(4 * a) * plane), 0, -1, 0x00020000);
    auto loadB = [&](f32x4 (&bfb)[2], int b, int c8) {      // position 4a + b, 8-channel group c8 = channel / 8
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int soff = (int)(((size_t)b * plane + ((size_t)c8 * Cout + (size_t)ni * 32) * 8) * 4);
            bfb[ni] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)wlane, soff, 0));
        }
    };

    // rows of the 4x4 window that (B^T d)[a] combines: e = d[ra] + sg * d[rb]
    const int ra = a == 0 ? 0 : (a == 2 ? 2 : 1);
    const int rb = a == 0 ? 2 : (a == 1 ? 2 : (a == 2 ? 1 : 3));
    const float sg = a == 1 ? 1.f : -1.f;
    const int ltr = li / TPR, ltc = li - ltr * TPR;       // the lane's tile in the block (R = 1: (0, li))
    int aoff[2][4];          // float offsets of the lane's window pixels (rows ra, rb; columns 0..3) in a stage
    int asw[4];              // swizzle of those columns
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        if constexpr (R == 1) {
            aoff[0][x] = (ra * WF_WX + 2 * li + x) * 32;
            aoff[1][x] = (rb * WF_WX + 2 * li + x) * 32;
            asw[x] = (li + (x >> 1)) & 7;
        } else {
            aoff[0][x] = ((2 * ltr + ra) * WF_WX + 2 * ltc + x) * 32;   // (tile row ltr: stage rows 2 ltr + 0..3)
            aoff[1][x] = ((2 * ltr + rb) * WF_WX + 2 * ltc + x) * 32;
            asw[x] = (ltc + (x >> 1)) & 7;
        }
    }

    f32x16 acc[4][2];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][ni][r] = 0.f;

    // K loop. One ring of four B pairs, bf[b] = the two N-fragments of position 4a + b: the eight MFMAs of position b
    // are followed at once by the loads of the same position's next 8-channel group (the next step's first group after
    // kk = 3; past the last step the same addresses again, never used), so every B load is issued about 24 MFMAs of
    // this wave (19-33 in the binary) before the wait that covers it. The window reads of group kk + 1 are issued in
    // two halves under the MFMAs of group kk and folded into e as they land; only a step's first group reads after the
    // barrier. The next stage's DMA goes between groups 2 and 3: every B load that a later MFMA of this step waits for
    // is older than it (vmcnt retires in order), and it has a group's time to land before the barrier that publishes
    // it. sched_barrier(0) after each position keeps the loads where they are written; the compiler places the waits.
    // The A operands u of position b + 1 (the next group's position 0 after b = 3) are formed in front of the MFMAs of
    // position b and pinned there, so no MFMA reads a register that the instruction before it wrote: formed right before
    // their use, each u[j] cost the MFMA pair behind it a padded wait (32 s_nop per K-step, 5 now: those of a step's first
    // position). Same sums, same operands, same order: the bits do not change.
    const int nk = Cin / 32;
    f32x4 bf[4][2];
    auto window = [&](const float *st, int kk, int x, f32x4 &d0, f32x4 &d1) {
        const int ch = 2 * kk + h;
        d0 = *reinterpret_cast<const f32x4 *>(st + aoff[0][x] + ((ch ^ asw[x]) << 2));
        d1 = *reinterpret_cast<const f32x4 *>(st + aoff[1][x] + ((ch ^ asw[x]) << 2));
    };
    issue(0, 0, true);
#pragma unroll
    for (int b = 0; b < 4; ++b) loadB(bf[b], b, 0);
    __syncthreads();                          // (waits for this wave's DMA; the barrier publishes everybody's)
    for (int kt = 0; kt < nk; ++kt) {
        const int c0 = kt * 32;
        const bool more = kt + 1 < nk;
        const int c8n = more ? c0 / 8 + 4 : c0 / 8;
        const float *st = smem + (kt & 1) * WF_STAGE;
        f32x4 e[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            f32x4 d0, d1;
            window(st, 0, x, d0, d1);
            e[x] = d0 + sg * d1;
        }
        f32x4 u = e[0] - e[2];
        wf_static_for<4>([&](auto kc) {
            constexpr int kk = decltype(kc)::value;
            f32x4 en[4], d0[2], d1[2];
            wf_static_for<4>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                f32x4 un;
                if constexpr (b == 0) un = e[1] + e[2];
                if constexpr (b == 1) un = e[2] - e[1];
                if constexpr (b == 2) un = e[1] - e[3];
                if constexpr (b == 3 && kk < 3) {
                    en[2] = d0[0] + sg * d1[0]; en[3] = d0[1] + sg * d1[1];
                    un = en[0] - en[2];
                }
                if constexpr (b < 3 || kk < 3) asm volatile("" : "+v"(un));
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[b][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[j], bf[b][ni][j], acc[b][ni], 0, 0, 0);
                loadB(bf[b], b, kk < 3 ? c0 / 8 + kk + 1 : c8n);
                if constexpr (kk < 3) {
                    if constexpr (b == 0) { window(st, kk + 1, 0, d0[0], d1[0]); window(st, kk + 1, 1, d0[1], d1[1]); }
                    if constexpr (b == 1) {
                        en[0] = d0[0] + sg * d1[0]; en[1] = d0[1] + sg * d1[1];
                        window(st, kk + 1, 2, d0[0], d1[0]); window(st, kk + 1, 3, d0[1], d1[1]);
                    }
                }
                if constexpr (b < 3 || kk < 3) u = un;
                __builtin_amdgcn_sched_barrier(0);
            });
            if constexpr (kk < 3) {
#pragma unroll
                for (int x = 0; x < 4; ++x) e[x] = en[x];
            }
            // (stage (kt + 1) & 1 is free since the barrier that ended step kt - 1)
            if constexpr (kk == 2) { issue(c0 + 32, (kt + 1) & 1, more); __builtin_amdgcn_sched_barrier(0); }
        });
        __syncthreads();                      // DMA of step kt + 1 landed; every read of stage kt & 1 done
    }

    // epilogue operands from memory first: their latency overlaps the exchange of the rows through LDS
    const int q = threadIdx.x & 15, c = n0 + q * 4;
    f32x4 bias = {0.f, 0.f, 0.f, 0.f}, cb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (p.bias) bias[j] = p.bias[c + j];
        if (p.chan_bias) cb[j] = p.chan_bias[(size_t)n * p.chan_bias_stride + c + j];
    }
    f32x4 rv[2][2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int tl = (threadIdx.x >> 4) + 16 * u, tr = R == 1 ? 0 : tl / TPR, tc = tl - tr * TPR;
                rv[u][r][cc] = p.resid.p ? *reinterpret_cast<const f32x4 *>(p.resid.p + p.resid.pix(n, 2 * (ty + tr) + r, 2 * (tx0 + tc) + cc) * Cout + c)
                                         : f32x4{0.f, 0.f, 0.f, 0.f};
            }

    // t[c] = M[a] A[:, c] per (tile, channel) into LDS: tb[a][c][tile][channel]
    float *tb = smem;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tile = (r & 3) + 8 * (r >> 2) + 4 * h, col = ni * 32 + li;
            const float m0 = acc[0][ni][r], m1 = acc[1][ni][r], m2 = acc[2][ni][r], m3 = acc[3][ni][r];
            tb[((a * 2 + 0) * WF_T + tile) * WF_BN + col] = m0 + m1 + m2;
            tb[((a * 2 + 1) * WF_T + tile) * WF_BN + col] = m1 - m2 - m3;
        }
    __syncthreads();

    double s1[2][4], s2[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int tl = (threadIdx.x >> 4) + 16 * u, tr = R == 1 ? 0 : tl / TPR, tc = tl - tr * TPR;
        f32x4 t[4][2];
#pragma unroll
        for (int aa = 0; aa < 4; ++aa)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) t[aa][cc] = *reinterpret_cast<const f32x4 *>(tb + ((aa * 2 + cc) * WF_T + tl) * WF_BN + q * 4);
        f32x4 y[2][2];
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            y[0][cc] = t[0][cc] + t[1][cc] + t[2][cc];
            y[1][cc] = t[1][cc] - t[2][cc] - t[3][cc];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { s1[u][j] = 0.0; s2[u][j] = 0.0; }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int oy = 2 * (ty + tr) + r, ox = 2 * (tx0 + tc) + cc;
                f32x4 add = bias;   // (the direct kernel's epilogue order: bias, residual, FeatureWiseAffine bias)
                if (p.resid.p) add += rv[u][r][cc];
                if (p.chan_bias) add += cb;
                const f32x4 o = y[r][cc] + add;
                *reinterpret_cast<f32x4 *>(p.out.p + p.out.pix(n, oy, ox) * Cout + c) = o;
#pragma unroll
                for (int j = 0; j < 4; ++j) { s1[u][j] += (double)o[j]; s2[u][j] = fma((double)o[j], (double)o[j], s2[u][j]); }
            }
    }
    if (p.stats == nullptr) return;
    __syncthreads();                          // every read of tb done: its space holds the per-tile sums
    double2 *red = reinterpret_cast<double2 *>(smem);     // [tile][channel]
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[((threadIdx.x >> 4) + 16 * u) * WF_BN + q * 4 + j] = make_double2(s1[u][j], s2[u][j]);
    __syncthreads();
    if ((int)threadIdx.x < spb * WF_BN) {
        const int sl = threadIdx.x / WF_BN, col = threadIdx.x % WF_BN, tps = WF_T / spb;
        double sa = 0, sq = 0;
        for (int k = 0; k < tps; ++k) { const double2 t2 = red[(sl * tps + k) * WF_BN + col]; sa += t2.x; sq += t2.y; }
        double *o = p.stats + (((size_t)n * p.stats_slices + si * spb + sl) * Cout + n0 + col) * 2;
        o[0] = sa; o[1] = sq;
    }
}

// ---- Upsample (nearest x2) + conv3x3 as sub-pixel Winograd F(2x2, 2x2) ---------------------------------------------------
// (transforms and indexing: sr3_internal.h at make_up2_wino_weights.) One pass, modelled on wino_fused_kernel:
//   * block = 32 tiles of the phase images (R tile rows x TPR = 32 / R tiles) x WU_BN = 32 output channels x the four
//     phases; wave a owns phase (py, px) = (a >> 1, a & 1). The 3x3 windows of all four phases lie inside the 4x4
//     low-resolution window (padded rows 2ti .. 2ti + 3) of the tile, so a stage is wino_fused_kernel's: the block's
//     2R + 2 distinct padded rows (R = 1: 4), each once, of WX = 2 TPR + 2 padded pixels x 32 channels, by LDS-DMA with
//     the same swizzle (264 | 204 | 180 live pixel rows for R = 1 | 2 | 4: 33 | 26 | 23 instructions, the tail of the
//     last one switched off). Every wave issues 9 | 7 | 6 instructions per stage: the lanes past the live rows (and every
//     lane of a step that has no next stage) go past the end of the descriptor, so no vector memory instruction of the K
//     loop sits behind a branch; a stage has room for all 36 | 28 | 24 slots.
//   * per 8-channel group a lane reads the nine window pixels of its tile (4 channels each), forms B^T d B with
//     differences only, and runs 9 positions x 4 MFMAs against B fragments loaded straight from the fragment-major
//     weights [phase][position][CinPad/8][Cout][8]; each position's fragment is reloaded for the next group right
//     behind its MFMAs, as in wino_fused_kernel.
//   * epilogue: the wave holds all nine M of its phase, so A^T M A is per-lane arithmetic on the accumulators: lane
//     (li, h) holds channel li of 16 tiles and stores 128 contiguous bytes per pixel with its 31 neighbours. Bias and
//     FeatureWiseAffine bias in the direct kernel's order. Statistics: per lane in fp64 over its tiles in register
//     order, then the two lane halves; one slice = one phase of 128 consecutive low-resolution pixels, which is what a
//     wave holds at R = 1 | 2 | 4, or of 64 (where the direct plan's tile is 64 pixels high): the two halves of them, kept
//     apart from the start. At widths of a multiple of 128 with 128-pixel slices the block runs the two strips of a slice
//     pair one after the other and the second adds to what the first stored. No LDS, no atomics, no inter-block waits.
// Registers: 9 positions x 16 accumulators = 144, a ring of six B fragments (24), nine transformed values (36).
constexpr int WU_BN = 32;
constexpr int WU_DMA = 36;                  // LDS-DMA slots per stage (R = 1: nine per wave; R = 2 | 4 use 28 | 24)
constexpr int WU_STAGE = WU_DMA * 256;      // floats per stage
constexpr size_t WU_LDS = (size_t)2 * WU_STAGE * sizeof(float);
static_assert(WU_BN == UP2_WINO_BN && UP2_WINO_TILES == 32, "conv_plan gates wino_up2_kernel on its block shape");

template <int R>
__global__ __launch_bounds__(256, 2) void wino_up2_kernel(const ConvParams p, int smode) {
    const int nst = smode == 1 ? 2 : 1;
    constexpr int TPR = 32 / R, WX = 2 * TPR + 2, PIX = (R == 1 ? 4 : 2 * R + 2) * WX;     // live pixel rows of a stage
    constexpr int NDMA = (PIX + 7) / 8, NPW = (NDMA + 3) / 4;                              // instructions per stage / per wave
    static_assert(4 * NPW <= WU_DMA, "every slot inside a stage");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Cin = p.in0.C, Cout = p.out.C;
    const int Hl = p.in0.H, Wl = p.in0.W, th = Hl >> 1, tw = Wl >> 1;     // tiles of a phase image
    const int bpr = (tw / TPR) / nst;                    // blocks per group of R tile rows
    const int bpi = (th / R) * bpr;                      // blocks per image
    const int nbl = Cout / WU_BN;
    int bid = blockIdx.x;
    {   // XCD-aware remap (as wino_fused_kernel): the channel blocks of one strip share an L2
        const int nwg = gridDim.x;
        const int xcd = bid & 7, loc = bid >> 3;
        const int qq = nwg >> 3, rr = nwg & 7;
        bid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + loc;
    }
    const int nb = bid % nbl, blk = bid / nbl;
    const int n = blk / bpi, bi = blk - n * bpi;
    const int tg = bi / bpr, sj = bi - tg * bpr;
    const int ti0 = tg * R;
    const int n0 = nb * WU_BN;
    const int a = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int py = a >> 1, px = a & 1;
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int Wp = p.in0.Wp();
    const int phase_slices = p.stats_slices >> 2;

    // B fragments of position pos, 8-channel group c8: lane (li, h) loads channels 8 c8 + 4h .. + 3 of output channel
    // n0 + li from w_up_wino[phase a][pos][c8][n0 + li][4h ..] (a wave-uniform descriptor over the phase's nine planes)
    const unsigned wlane = ((unsigned)(n0 + li) * 8u + 4u * h) * 4u;
    const size_t plane = (size_t)Cout * Cin;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w_up_wino + (size_t)(9 * a) * plane), 0, -1, 0x00020000);
    auto loadB = [&](f32x4 &bfb, int pos, int c8) {
        const int soff = (int)((unsigned)pos * (unsigned)plane + (unsigned)c8 * (unsigned)Cout * 8u) * 4;
        bfb = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)wlane, soff, 0));
    };

    // the lane's tile and its window: pixel (py + i, px + j) of the tile's 4x4 window, i, j = 0..2
    // (float offset wbase + (i WX + j) * 32 in a stage, 16-B chunk c of column j at c ^ wsw[j])
    const int ltr = li / TPR, ltc = li - ltr * TPR;
    const int wbase = ((ltr * 2 + py) * WX + 2 * ltc + px) * 32;       // (tile row ltr: stage rows 2 ltr + 0..3)
    int wsw[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) wsw[j] = (ltc + ((px + j) >> 1)) & 7;

    const int co = n0 + li;
    float add = p.bias ? p.bias[co] : 0.f;               // (the direct kernel's epilogue order: bias, FeatureWiseAffine bias)
    if (p.chan_bias) add += p.chan_bias[(size_t)n * p.chan_bias_stride + co];

    // LDS-DMA: wave a issues instructions i = a + 4m, m = 0..NPW - 1; lane -> pixel row 8i + (lane >> 3) of the stage
    // (stage row, column x: padded row 2 ti0 + stage row), stored chunk lane & 7. The lane's byte offsets depend on lane, i, Wp and Cin
    // only (strip and channel step go into the descriptor's base), so they are computed once for all strips and K-steps
    // and held (dvoff, pinned in issue() as in wino_fused_kernel). A live descriptor ends at 2^31 - 1 bytes and a live
    // offset stays below it (conv_plan: (10 Wp + 70) * Cin * 4 < 2^31; stage row 2R + 1 <= 9 is the last); a lane past
    // the live rows (q >= PIX, fixed per wave, m and lane) holds an offset with bit 31 set, and a step with no next stage (on == false,
    // wave-uniform) takes a descriptor with num_records = 0: either way the load is out of range and makes no memory
    // request.
    unsigned dvoff[NPW];
    {
        const unsigned cs4 = (unsigned)Cin * 4u;
#pragma unroll
        for (int m = 0; m < NPW; ++m) {
            const int i = a + 4 * m;
            const int q = 8 * i + (lane >> 3);
            const int wr = q / WX, x = q - wr * WX;
            const int row = R == 1 ? 2 * (wr >> 2) + (wr & 3) : wr;      // (R = 1: wr itself in every live lane)
            const unsigned voff = (unsigned)(row * Wp + x) * cs4 + (unsigned)(((lane & 7) ^ ((x >> 1) & 7)) * 16);
            dvoff[m] = (R == 1 ? i < NDMA : q < PIX) ? voff : 0x80000000u;
        }
    }

    const int nk = Cin / 32;
    for (int ss = 0; ss < nst; ++ss) {
        const int tj0 = (sj * nst + ss) * TPR;
        const size_t pix0 = ((size_t)n * p.in0.Hp() + 2 * ti0) * Wp + 2 * tj0;      // window origin of the block's first tile
        const char *src0 = reinterpret_cast<const char *>(p.in0.p + pix0 * Cin);

        auto issue = [&](int c0, int stage, bool on) {
            const __amdgpu_buffer_rsrc_t rsrc =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(src0 + (size_t)c0 * 4), 0, on ? 0x7fffffff : 0, 0x00020000);
            float *dst = smem + stage * WU_STAGE;
            wf_static_for<NPW>([&](auto mc) {
                constexpr int m = decltype(mc)::value;
                asm volatile("" : "+v"(dvoff[m]));   // (held, not recomputed: as in wino_fused_kernel)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(dst + (a + 4 * m) * 256),
                                                         16, (int)dvoff[m], 0, 0, 0);
            });
        };

        // window pixel (py + i, px + j) of the lane's tile, channels 8 kk + 4h .. + 3
        auto rd = [&](const float *st, int kk, int i, int j) {
            return *reinterpret_cast<const f32x4 *>(st + wbase + (i * WX + j) * 32 + (((2 * kk + h) ^ wsw[j]) << 2));
        };

        f32x16 acc[9];
#pragma unroll
        for (int ps = 0; ps < 9; ++ps)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ps][r] = 0.f;

        // K loop. The 36 (group, position) products of a step take their B fragments from a ring of six: slot t % 6 for
        // product t = 9 kk + position, refilled right behind its MFMAs with the fragment of product t + 6 (20 MFMAs of this
        // wave ahead of its use; past kk = 3 the next step's first group, past the last step the same addresses again,
        // never used).
        f32x4 bf[6];
        issue(0, 0, true);
#pragma unroll
        for (int t = 0; t < 6; ++t) loadB(bf[t], t, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMA landed; the barrier publishes everybody's
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int c0 = kt * 32;
            const bool more = kt + 1 < nk;
            const int c8n = more ? c0 / 8 + 4 : c0 / 8;
            const float *st = smem + (kt & 1) * WU_STAGE;
            f32x4 dn0[3], dn1[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) { dn0[j] = rd(st, 0, 0, j); dn1[j] = rd(st, 0, 1, j); }
            wf_static_for<4>([&](auto kc) {
                constexpr int kk = decltype(kc)::value;
                // B^T d B: rows (d0 - d1, d1, d1 - d2), then the same over the columns. Rows 0 and 1 of the window were
                // read under the previous group's last positions (a step's first group: after the barrier); row 2 is
                // read behind position 2 and folded in behind position 5; the next group's rows 0 and 1 follow position 6.
                f32x4 u[9];
                {
                    f32x4 e0[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) e0[j] = dn0[j] - dn1[j];
                    u[0] = e0[0] - e0[1]; u[1] = e0[1]; u[2] = e0[1] - e0[2];
                    u[3] = dn1[0] - dn1[1]; u[4] = dn1[1]; u[5] = dn1[1] - dn1[2];
                }
                f32x4 d1[3], d2[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) d1[j] = dn1[j];
                __builtin_amdgcn_sched_barrier(0);
                wf_static_for<9>([&](auto pc) {
                    constexpr int ps = decltype(pc)::value;
                    constexpr int t = 9 * kk + ps, slot = t % 6;
                    constexpr int tn = t + 6, psn = tn % 9, kkn = tn / 9;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[ps] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[ps][j], bf[slot][j], acc[ps], 0, 0, 0);
                    loadB(bf[slot], psn, kkn < 4 ? c0 / 8 + kkn : c8n);
                    if constexpr (ps == 2) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) d2[j] = rd(st, kk, 2, j);
                    }
                    if constexpr (ps == 5) {
                        f32x4 e2[3];
#pragma unroll
                        for (int j = 0; j < 3; ++j) e2[j] = d1[j] - d2[j];
                        u[6] = e2[0] - e2[1]; u[7] = e2[1]; u[8] = e2[1] - e2[2];
                    }
                    if constexpr (ps == 6 && kk < 3) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) { dn0[j] = rd(st, kk + 1, 0, j); dn1[j] = rd(st, kk + 1, 1, j); }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
                // (stage (kt + 1) & 1 is free since the barrier that ended step kt - 1)
                if constexpr (kk == 2) { issue(c0 + 32, (kt + 1) & 1, more); __builtin_amdgcn_sched_barrier(0); }
            });
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                      // DMA of step kt + 1 landed; every read of stage kt & 1 done
        }

        // A^T M A per tile in the accumulator layout (register r of lane half h = tile (r & 3) + 8 (r >> 2) + 4h)
        // (4h is less than the distance to the next multiple of 8, so the tile row is the same in both halves and the
        // half only shifts the lane by 4 tiles = 16 output pixels along the row: every other term of the address is
        // wave-uniform)
        // statistics of the two 64-pixel halves of the wave's 128 low-resolution pixels (row-major): the tiles' pixel rows
        // 0 | 1 at R = 1, the tile rows 0 | 1 at R = 2, 0-1 | 2-3 at R = 4
        double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0};
        const int Wpo = p.out.Wp();
        float *const ob = p.out.p + p.out.pix(n, 4 * ti0 + py, 4 * tj0 + px) * Cout;
        const unsigned lo = (unsigned)(16 * h * Cout + co);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tl = (r & 3) + 8 * (r >> 2), tr = tl / TPR, tc = tl - tr * TPR;
            const float t00 = acc[0][r] + acc[3][r], t01 = acc[1][r] + acc[4][r], t02 = acc[2][r] + acc[5][r];
            const float t10 = acc[3][r] - acc[6][r], t11 = acc[4][r] - acc[7][r], t12 = acc[5][r] - acc[8][r];
            const float y[2][2] = {{t00 + t01, t01 - t02}, {t10 + t11, t11 - t12}};
#pragma unroll
            for (int ya = 0; ya < 2; ++ya)
#pragma unroll
                for (int xb = 0; xb < 2; ++xb) {
                    const float o = y[ya][xb] + add;
                    (ob + (size_t)((4 * tr + 2 * ya) * Wpo + 4 * tc + 2 * xb) * Cout)[lo] = o;
                    const int g = R == 1 ? ya : R == 2 ? tr : tr >> 1;
                    s1[g] += (double)o;
                    s2[g] = fma((double)o, (double)o, s2[g]);
                }
        }
        if (p.stats != nullptr) {
            // the two lane halves hold different tiles of the same channel; half 0 writes. The second strip of a slice
            // pair adds to what the same lane stored after the first (its own store: no other thread touches the word)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                s1[g] += __shfl_xor(s1[g], 32);
                s2[g] += __shfl_xor(s2[g], 32);
            }
            if (h == 0) {
                if (smode == 0) {           // one 128-pixel slice per wave
                    double *o = p.stats + (((size_t)n * p.stats_slices + a * phase_slices + bi) * Cout + co) * 2;
                    o[0] = s1[0] + s1[1]; o[1] = s2[0] + s2[1];
                } else {
#pragma unroll
                    for (int g = 0; g < 2; ++g) {
                        // smode 1 (R = 1): pixel row g of the tile row, 128 columns = this block's two strips;
                        // smode 2: the 64-pixel slices (R = 1: one strip's part of pixel row g)
                        const int slice = a * phase_slices + (smode == 1 ? (2 * ti0 + g) * (Wl / 128) + sj
                                                              : R == 1 ? (2 * ti0 + g) * (Wl / 64) + sj : 2 * bi + g);
                        double *o = p.stats + (((size_t)n * p.stats_slices + slice) * Cout + co) * 2;
                        if (ss == 0) { o[0] = s1[g]; o[1] = s2[g]; }
                        else { o[0] += s1[g]; o[1] += s2[g]; }
                    }
                }
            }
        }
    }
}

// ---- second form of the three-pass plan: the 16 position GEMMs and the output transform in ONE kernel ----------------
// U -> wino_gemm_out_kernel -> output: M never goes through memory (it is four times the conv's output), and one block
// runs ONE K loop of 16 * Cin / 32 steps instead of 16 blocks with Cin / 32 steps, a pipeline fill and an M-tile store each.
// Block = WG_BT consecutive tiles (global tile index of U, so A rows are contiguous in every position plane) x BN output
// channels; 2 x BN/32 consumer waves with ONE 32x32 accumulator tile each, 4 producer waves (conv_igemm_dma_f32's
// pipeline, swizzle and v_mfma_f32_32x32x2_f32 fragment mapping; the K loop runs over (position, 32-channel step)).
// Bit-identical to launch_wino_gemm + wino_output_kernel:
//   * every position's chain starts from zero and adds its K-steps in ascending order (kk = 0..3, elements x, y, z, w):
//     the bits of M[pos] as conv_igemm_dma_f32 leaves them, whatever its tile;
//   * the positions are walked column-major (pos = 4a + b, b outer) and folded with per-lane adds in the accumulator
//     layout, in wino_output_kernel's left-to-right order: u0 = (M0b + M1b) + M2b, u1 = (M1b - M2b) - M3b,
//     y.0 = (u.[0] + u.[1]) + u.[2], y.1 = (u.[1] - u.[2]) - u.[3]: 7 accumulator sets (t, u0, u1, four y) x 16 registers;
//   * the epilogue order is the direct kernel's (bias, residual, FeatureWiseAffine bias);
//   * the statistics of a slice of tps = 16 | 32 tiles are added as wino_output_kernel does (tile lane k mod 16: its
//     tiles in order, four pixels each; then the lanes in order): a lane holds whole tiles, tiles k and k + 16 of a
//     32-tile slice are accumulator registers r and r + 8 of the same lane, and the running sum over the 16 tile lanes
//     alternates between the two lane halves (rows 0-3 | 4-7 | 8-11 | 12-15) through three exchanges. No LDS, no atomics.
// Whole channel blocks (Cout % BN == 0); rows past the last tile are clamped (min(t, tiles - 1)) and never stored.
constexpr int WG_BT = 64;                   // 2x2 output tiles per block
constexpr int WG_NS = 3;                    // LDS pipeline stages (4 stages, or two K-steps per stage and barrier: measured the same)

template <int N>
__device__ __forceinline__ void wg_producer_sync() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
    __builtin_amdgcn_s_barrier();
}

// keeps a value (and the adds that made it) where the program has it
__device__ __forceinline__ void wg_pin(f32x16 &x) { asm volatile("" : "+v"(x)); }

template <int BN>
__global__ __launch_bounds__((2 * (BN / 32) + 4) * 64) void wino_gemm_out_kernel(const ConvParams p, const float *__restrict__ U,
                                                                                  int Cin, int tps) {
#pragma clang fp contract(off)
    constexpr int BT = WG_BT, NS = WG_NS;
    constexpr int WGN = BN / 32, NC = 2 * WGN;          // consumer waves: 2 (tiles) x WGN (channels)
    constexpr int AR = BT / 32, BR = BN / 32;           // DMA instructions per producer wave and K-step
    constexpr int STAGE = (BT + BN) * 32;               // floats per pipeline stage
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int *rowpix = reinterpret_cast<int *>(smem + NS * STAGE);   // [BT] padded output pixel of the tile's (0, 0)
    int *rowimg = rowpix + BT;                                  // [BT] image

    const int Cout = p.out.C, th = p.Hout >> 1, tw = p.Wout >> 1, tpi = th * tw;
    const int tiles = p.B * tpi;
    const int tilesN = Cout / BN;
    int bid = blockIdx.x;                   // XCD-aware remap (conv_igemm_dma_f32): the channel blocks of a tile range share an L2
    {
        const int nwg = gridDim.x;
        const int xcd = bid & 7, loc = bid >> 3;
        const int qq = nwg >> 3, rr = nwg & 7;
        bid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + loc;
    }
    const int t0 = (bid / tilesN) * BT;
    const int n0 = (bid % tilesN) * BN;
    const int nc = Cin >> 5;                // K-steps per position
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;

    if (wid >= NC) {
        // ------------------------------- producer waves -------------------------------------
        const int w = wid - NC;
        const int tid = threadIdx.x - NC * 64;
        if (tid < BT) {
            const int t = min(t0 + tid, tiles - 1);
            const int n = t / tpi, rem = t - n * tpi;
            const int ty = rem / tw, tx = rem - ty * tw;
            rowpix[tid] = (int)p.out.pix(n, 2 * ty, 2 * tx);
            rowimg[tid] = n;
        }
        // DMA instruction i of this wave fills rows (4i + w) * 8 + (lane >> 3); uniform 64-bit base per position and
        // K-step, per-lane 32-bit byte offsets constant over the whole K loop (conv_igemm_dma_f32)
        const int rsub = lane >> 3;
        const unsigned schunk16 = (unsigned)(((lane & 7) ^ ((((w & 1) << 2) | (lane >> 4)) & 7)) * 16);
        unsigned vA[AR], vB[BR];
        wf_static_for<AR>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const int t = min(t0 + (4 * i + w) * 8 + rsub, tiles - 1);
            vA[i] = (unsigned)t * (unsigned)Cin * 4u + schunk16;
        });
        wf_static_for<BR>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const int n = n0 + (4 * i + w) * 8 + rsub;
            vB[i] = (unsigned)n * (unsigned)Cin * 4u + schunk16;
        });
        const size_t uplane = (size_t)tiles * Cin, wplane = (size_t)Cout * Cin;
        int k = 0, stage = 0;
        for (int b = 0; b < 4; ++b)
            for (int a = 0; a < 4; ++a) {
                const int ps = 4 * a + b;
                const float *ub = U + (size_t)ps * uplane, *wb = p.w_wino + (size_t)ps * wplane;
                for (int c0 = 0; c0 < Cin; c0 += 32) {
                    float *Ad = smem + stage * STAGE + w * 256;
                    float *Bd = Ad + BT * 32;
                    const char *ab = reinterpret_cast<const char *>(ub + c0);
                    const char *bb = reinterpret_cast<const char *>(wb + c0);
                    wf_static_for<AR>([&](auto ic) {
                        constexpr int i = decltype(ic)::value;
                        wf_dma16(ab, vA[i], Ad + i * 1024);
                    });
                    wf_static_for<BR>([&](auto ic) {
                        constexpr int i = decltype(ic)::value;
                        wf_dma16(bb, vB[i], Bd + i * 1024);
                    });
                    if (k >= NS - 2) wg_producer_sync<(NS - 2) * (AR + BR)>();
                    ++k;
                    stage = stage + 1 == NS ? 0 : stage + 1;
                }
            }
        wf_static_for<NS - 2>([&](auto rc) {          // drain: the last NS-2 tiles are still in flight
            constexpr int r = NS - 3 - decltype(rc)::value;
            wg_producer_sync<r * (AR + BR)>();
        });
        __syncthreads();
        return;
    }

    // ----------------------------------- consumer waves -----------------------------------------
    const int li = lane & 31, lh = lane >> 5;
    const int wm = wid / WGN, wn = wid % WGN;
    const int swz = (li >> 1) & 7;
    const float *Abase = smem + (wm * 32 + li) * 32;
    const float *Bbase = smem + BT * 32 + (wn * 32 + li) * 32;
    int koff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) koff[kk] = (((2 * kk + lh) ^ swz) & 7) * 4;
    f32x4 fa[4], fb[4];
#define WG_FRAG_READ(SET, CUR, KK)                                                              \
    {                                                                                           \
        fa[SET] = *reinterpret_cast<const f32x4 *>(Abase + (CUR) * STAGE + koff[KK]);           \
        fb[SET] = *reinterpret_cast<const f32x4 *>(Bbase + (CUR) * STAGE + koff[KK]);           \
    }
#define WG_FRAG_MMA(SET)                                                                        \
    {                                                                                           \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET].x, fb[SET].x, acc, 0, 0, 0);         \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET].y, fb[SET].y, acc, 0, 0, 0);         \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET].z, fb[SET].z, acc, 0, 0, 0);         \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET].w, fb[SET].w, acc, 0, 0, 0);         \
    }
    int cur = 0;
    // M[pos] of this wave's 32 tiles x 32 channels: nc K-steps from zero
    auto chain = [&](f32x16 &acc) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int c = 0; c < nc; ++c) {
            const int nxt = cur + 1 == NS ? 0 : cur + 1;
            // Group kk has its own register set; every read is issued one MFMA group (256 cycles) before the wait that
            // covers it. Scheduling barriers: left alone, the scheduler reuses one set and waits right behind each read.
            WG_FRAG_MMA(0)
            __builtin_amdgcn_sched_barrier(0);
            WG_FRAG_READ(2, cur, 2)
            __builtin_amdgcn_sched_barrier(0);
            WG_FRAG_MMA(1)
            __builtin_amdgcn_sched_barrier(0);
            WG_FRAG_READ(3, cur, 3)
            __builtin_amdgcn_sched_barrier(0);
            WG_FRAG_MMA(2)
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();                   // every read of this stage has been issued and waited
            WG_FRAG_READ(0, nxt, 0)            // next K-step, whichever position it belongs to (stale data after the
            WG_FRAG_READ(1, nxt, 1)            // last one: unused)
            __builtin_amdgcn_sched_barrier(0);
            WG_FRAG_MMA(3)
            __builtin_amdgcn_sched_barrier(0);
            cur = nxt;
        }
    };
    f32x16 t, u0, u1, y[2][2];
    __syncthreads();
    WG_FRAG_READ(0, 0, 0)
    WG_FRAG_READ(1, 0, 1)
    wf_static_for<4>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        // (the folds are pinned where they stand: left to the optimiser they sink to the epilogue and all 16 M tiles
        // stay live, 256 registers)
        chain(u0);                              // a = 0
        chain(u1);                              // a = 1
        u0 += u1;
        wg_pin(u0);
        chain(t);                               // a = 2
        u0 += t;
        u1 -= t;
        wg_pin(u0); wg_pin(u1);
        chain(t);                               // a = 3
        u1 -= t;
        wg_pin(u1);
        if constexpr (b == 0) { y[0][0] = u0; y[1][0] = u1; }
        if constexpr (b == 1) { y[0][0] += u0; y[1][0] += u1; y[0][1] = u0; y[1][1] = u1; }
        if constexpr (b == 2) { y[0][0] += u0; y[1][0] += u1; y[0][1] -= u0; y[1][1] -= u1; }
        if constexpr (b == 3) { y[0][1] -= u0; y[1][1] -= u1; }
        wg_pin(y[0][0]); wg_pin(y[0][1]); wg_pin(y[1][0]); wg_pin(y[1][1]);
    });
#undef WG_FRAG_READ
#undef WG_FRAG_MMA

    // epilogue: lane (li, lh) holds channel col of tiles wm * 32 + (r & 3) + 8 (r >> 2) + 4 lh, r = 0..15
    const unsigned col = (unsigned)(n0 + wn * 32 + li);
    const float bs = p.bias ? p.bias[col] : 0.f;
    const unsigned Wp = (unsigned)p.out.Wp(), uC = (unsigned)Cout;
    const bool want_stats = p.stats != nullptr;
    const bool pair = tps == 32;               // a slice is the wave's 32 tiles (else its rows 0-15 and 16-31 are two slices)
    double run[2][2] = {{0, 0}, {0, 0}};       // [slice of the wave: rows 0-15 | 16-31][sum, sum of squares]
#pragma unroll
    for (int g = 0; g < 2; ++g) {              // tile lanes 8g .. 8g+7: registers 4g .. 4g+3 of both lane halves
        double s1[2][4], s2[2][4];             // partials of tile lane (r & 3) + 8g + 4 lh in the two slices
#pragma unroll
        for (int h = 0; h < 2; ++h)            // h = 1: registers r + 8 (tiles + 16)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 8 * h + 4 * g + j;
                const int row = wm * 32 + 16 * h + 8 * g + 4 * lh + j;
                const unsigned pix = (unsigned)rowpix[row];
                const bool ok = t0 + row < tiles;
                const float cb = p.chan_bias ? p.chan_bias[(size_t)rowimg[row] * p.chan_bias_stride + col] : 0.f;
                double a1 = (h == 1 && pair) ? s1[0][j] : 0.0, a2 = (h == 1 && pair) ? s2[0][j] : 0.0;
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                    for (int cc = 0; cc < 2; ++cc) {
                        const unsigned off = (pix + rr * Wp + cc) * uC + col;
                        float add = bs;        // (the direct kernel's epilogue order: bias, residual, FeatureWiseAffine bias)
                        if (p.resid.p) add += p.resid.p[off];
                        if (p.chan_bias) add += cb;
                        const float o = y[rr][cc][r] + add;
                        if (ok) p.out.p[off] = o;
                        if (want_stats) { a1 += (double)o; a2 = fma((double)o, (double)o, a2); }
                    }
                s1[h][j] = a1; s2[h][j] = a2;
                __builtin_amdgcn_sched_barrier(0);      // one tile's four pixels in flight at a time: bounds the registers
            }
        if (want_stats) {
            // the lanes of half 0 add their four tile lanes, hand the sum to half 1, which adds its four
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    // slice 0 of a 32-tile slice carries the chained partials in s.[1]; two 16-tile slices carry s.[sl]
                    double a = run[sl][0], q = run[sl][1];
                    if (g + hh > 0) { a = __shfl_xor(a, 32); q = __shfl_xor(q, 32); }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        a += (pair ? s1[1][j] : s1[sl][j]);
                        q += (pair ? s2[1][j] : s2[sl][j]);
                    }
                    run[sl][0] = a; run[sl][1] = q;
                }
            }
        }
    }
    if (want_stats && lh == 1) {
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            if (pair && sl == 1) break;
            const int first = t0 + wm * 32 + 16 * sl;           // first tile of the slice
            if (first < tiles) {
                double *o = p.stats + ((size_t)(first / tps) * Cout + col) * 2;
                o[0] = run[sl][0]; o[1] = run[sl][1];
            }
        }
    }
}

template <int BN>
void launch_wino_gemm_out(const ConvParams &o, const float *U, int Cin, hipStream_t s) {
    static bool attr_set = false;           // (more than 64 KiB of dynamic LDS at BN = 128)
    constexpr size_t lds = ((size_t)WG_NS * (WG_BT + BN) * 32 + 2 * WG_BT) * sizeof(float);
    auto kern = wino_gemm_out_kernel<BN>;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    const int tpi = (o.Hout / 2) * (o.Wout / 2), tiles = o.B * tpi;
    const int tps = o.stats ? tpi / o.stats_slices : 0;
    const unsigned blocks = (unsigned)((tiles + WG_BT - 1) / WG_BT) * (unsigned)(o.out.C / BN);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3((2 * (BN / 32) + 4) * 64), lds, s, o, U, Cin, tps);
}

int out_slices(const ConvParams &p) {
    const int tiles = (p.Hout >> 1) * (p.Wout >> 1);
    if (p.stats) return p.stats_slices;
    return (tiles % 16) == 0 ? tiles / 16 : 1;
}

} // namespace

static_assert(WF_T == WINO_FUSED_TILES && WF_BN == WINO_FUSED_BN, "conv_plan gates the one-pass kernel on its block shape");

void make_wino_weights(const float *w9, int Cout, int CinPad, float *dst) {
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const size_t plane = (size_t)Cout * CinPad;
    for (size_t i = 0; i < plane; ++i) {
        double g[3][3];
        for (int t = 0; t < 9; ++t) g[t / 3][t % 3] = (double)w9[(size_t)t * plane + i];
        for (int a = 0; a < 4; ++a) {
            double gg[3];     // (G g)[a][:]
            for (int x = 0; x < 3; ++x) gg[x] = G[a][0] * g[0][x] + G[a][1] * g[1][x] + G[a][2] * g[2][x];
            for (int b = 0; b < 4; ++b)
                dst[(size_t)(a * 4 + b) * plane + i] = (float)(gg[0] * G[b][0] + gg[1] * G[b][1] + gg[2] * G[b][2]);
        }
    }
}

void make_wino_weights_frag(const float *wino, int Cout, int CinPad, float *dst) {
    const int groups = CinPad / 8;
    for (int ps = 0; ps < 16; ++ps)
        for (int g = 0; g < groups; ++g)
            for (int n = 0; n < Cout; ++n)
                for (int j = 0; j < 8; ++j)
                    dst[(((size_t)ps * groups + g) * Cout + n) * 8 + j] = wino[((size_t)ps * Cout + n) * CinPad + 8 * g + j];
}

namespace {
// the same permutation on the device: one thread per 8-float group (two 16-B loads, two 16-B stores)
__global__ __launch_bounds__(256) void wino_frag_kernel(const float *__restrict__ wino, int Cout, int CinPad, float *__restrict__ dst) {
    const int groups = CinPad / 8;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // destination group ((ps, g), n)
    if (i >= (size_t)16 * groups * Cout) return;
    const size_t n = i % (size_t)Cout, pg = i / (size_t)Cout;
    const size_t ps = pg / (size_t)groups, g = pg - ps * groups;
    const f32x4 *s = reinterpret_cast<const f32x4 *>(wino + (ps * Cout + n) * CinPad + 8 * g);
    f32x4 *d = reinterpret_cast<f32x4 *>(dst + i * 8);
    d[0] = s[0];
    d[1] = s[1];
}
} // namespace

void launch_wino_frag(const float *wino, int Cout, int CinPad, float *dst, hipStream_t s) {
    const size_t n = (size_t)16 * (CinPad / 8) * Cout;
    hipLaunchKernelGGL(wino_frag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, wino, Cout, CinPad, dst);
}

void launch_conv_wino(const ConvParams &p, const ConvPlan &plan, hipStream_t s) {
    const ConvKernel form = plan.kernel;
    const int H = p.Hout, W = p.Wout, Cout = p.out.C;
    const int Cin = p.in0.C + (p.in1.p ? p.in1.C : 0);
    ConvParams o = p;
    if (p.in2.p && p.res_ready) {
        // (block1's GroupNorm pass left the 1x1 term in the output: launch_gn_res1x1)
        o.resid = p.out;
    } else if (p.in2.p) {
        // fused 1x1 term: a 1x1 conv over in2 || in2b (+ the residual) into the output, added back as the residual
        ConvParams r;
        r.in0 = p.in2; r.in1 = p.in2b;
        r.B = p.B; r.Hout = H; r.Wout = W;
        r.ks = 1; r.prec = 0;
        r.w = p.w2;
        r.resid = p.resid;
        r.out = p.out;
        r.ovf = p.ovf;
        launch_conv(r, s);
        o.resid = p.out;
    }
    if (form == CK_WINO_ONE_PASS || plan.wino_fused_rows) {
        // (the second case: a form of the three-pass plan; U and M, the whole workspace, stay unused)
        const int spi = (H / 2) * (W / 2) / WF_T;          // blocks of 32 tiles per image
        const int spb = o.stats ? o.stats_slices / spi : 1;
        const unsigned blocks = (unsigned)((size_t)p.B * spi * (Cout / WF_BN));
        static bool attr_set = false;          // (more than 64 KiB of dynamic LDS)
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wino_fused_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)WfGeom<1>::LDS);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wino_fused_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)WfGeom<2>::LDS);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wino_fused_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)WfGeom<4>::LDS);
            attr_set = true;
        }
        if (form == CK_WINO_ONE_PASS) hipLaunchKernelGGL(wino_fused_kernel<1>, dim3(blocks), dim3(256), WfGeom<1>::LDS, s, o, spb);
        else if (plan.wino_fused_rows == 2) hipLaunchKernelGGL(wino_fused_kernel<2>, dim3(blocks), dim3(256), WfGeom<2>::LDS, s, o, spb);
        else hipLaunchKernelGGL(wino_fused_kernel<4>, dim3(blocks), dim3(256), WfGeom<4>::LDS, s, o, spb);
        return;
    }

    const size_t tiles = (size_t)p.B * (H / 2) * (W / 2);
    float *U = p.wino_ws, *Mw = p.wino_ws + 16 * tiles * Cin;
    const size_t items = tiles * (Cin / 4);
    if (!p.u_ready)
        hipLaunchKernelGGL(wino_input_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p.in0, p.in1, p.B, U);

    if (plan.wino_gemm_out) {
        // second form: position GEMMs + output transform in one kernel (the M half of the workspace stays unused)
        if (plan.wino_gemm_out == 128) launch_wino_gemm_out<128>(o, U, Cin, s);
        else launch_wino_gemm_out<64>(o, U, Cin, s);
        return;
    }

    ConvParams g;
    g.in0.p = U; g.in0.C = Cin; g.in0.H = H / 2; g.in0.W = W / 2; g.in0.pad = 0;
    g.B = p.B; g.Hout = H / 2; g.Wout = W / 2;
    g.ks = 1; g.prec = 0;
    g.w = p.w_wino;
    g.out.p = Mw; g.out.C = Cout; g.out.H = H / 2; g.out.W = W / 2; g.out.pad = 0;
    g.zbatch = 16;
    g.phase_w_stride = (size_t)Cout * Cin;
    g.batch_in_stride = tiles * Cin;
    g.batch_out_stride = tiles * Cout;
    launch_wino_gemm(g, s);

    const int sl = out_slices(o);
    hipLaunchKernelGGL(wino_output_kernel, dim3(Cout / 64, sl, p.B), dim3(256), 0, s, o, Mw, sl);
}

void launch_conv_up2_wino(const ConvParams &p, const ConvPlan &plan, hipStream_t s) {
    const int R = plan.up2_wino, Hl = p.in0.H, Wl = p.in0.W;
    // statistics: 0 = one 128-pixel slice per wave, 1 = 128-pixel slices over the two strips a block then runs (conv_plan:
    // Wl % 128 == 0), 2 = 64-pixel slices (the direct plan's tile of 64 pixels)
    const int smode = !p.stats ? 0 : p.stats_slices == 4 * (Hl * Wl / 64) ? 2 : Wl > 64 ? 1 : 0;
    const int nst = smode == 1 ? 2 : 1;
    const unsigned blocks = (unsigned)((size_t)p.B * ((size_t)Hl * Wl / (4 * UP2_WINO_TILES) / nst) * (p.out.C / WU_BN));
    static bool attr_set = false;          // (more than 64 KiB of dynamic LDS)
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wino_up2_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)WU_LDS);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wino_up2_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)WU_LDS);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wino_up2_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)WU_LDS);
        attr_set = true;
    }
    if (R == 1) hipLaunchKernelGGL(wino_up2_kernel<1>, dim3(blocks), dim3(256), WU_LDS, s, p, smode);
    else if (R == 2) hipLaunchKernelGGL(wino_up2_kernel<2>, dim3(blocks), dim3(256), WU_LDS, s, p, smode);
    else hipLaunchKernelGGL(wino_up2_kernel<4>, dim3(blocks), dim3(256), WU_LDS, s, p, smode);
}

} // namespace sr3
