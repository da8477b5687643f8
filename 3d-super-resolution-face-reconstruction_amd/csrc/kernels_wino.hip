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
// Registers: 4 positions x 2 N-fragments x 16 accumulators = 128, plus two sets of B fragments (64): 2 waves per SIMD.
// A 64-tile or 128-channel block doubles the accumulators (256: 1 wave per SIMD, nothing left for operands).
// One input tensor only (conv_plan): the engine writes x || skip as one tensor in the GroupNorm apply pass.
constexpr int WF_T = 32;                    // 2x2 output tiles per block (one strip of a tile row)
constexpr int WF_BN = 64;                   // output channels per block
constexpr int WF_WX = 2 * WF_T + 2;         // padded input columns of a strip's windows
constexpr int WF_ROWS = 4 * WF_WX;          // pixel rows of 32 floats per LDS stage
constexpr int WF_STAGE = WF_ROWS * 32;      // floats per stage
constexpr int WF_DMA = WF_ROWS / 8;         // LDS-DMA instructions per stage (64 lanes x 16 B each)
constexpr int WF_DMA_PER_WAVE = (WF_DMA + 3) / 4;
static_assert(WF_ROWS % 8 == 0, "whole DMA instructions per stage");
constexpr size_t WF_LDS = (size_t)2 * WF_STAGE * sizeof(float);
static_assert(WF_LDS >= (size_t)4 * 2 * WF_T * WF_BN * sizeof(float), "epilogue exchange fits in the stages");

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

__global__ __launch_bounds__(256, 2) void wino_fused_kernel(const ConvParams p, int spb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Cin = p.in0.C;                             // (one input tensor: conv_wino_taken)
    const int Cout = p.out.C, th = p.Hout >> 1, tw = p.Wout >> 1;
    const int spr = tw / WF_T, spi = th * spr;           // strips per tile row / per image
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
    const int ty = si / spr, tx0 = (si - ty * spr) * WF_T;
    const int n0 = nb * WF_BN;
    const int a = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int Wp = p.in0.Wp();
    const size_t pix0 = ((size_t)n * p.in0.Hp() + 2 * ty) * Wp + 2 * tx0;     // window origin of the strip
    const char *src0 = reinterpret_cast<const char *>(p.in0.p + pix0 * Cin);

    // LDS-DMA: wave a issues instructions i = a + 4m; lane -> pixel row 8i + (lane >> 3) (window row r, column x),
    // stored chunk lane & 7 (offsets recomputed per K-step: a few VALU operations, no registers held across the loop)
    auto issue = [&](int c0, int stage) {
        const char *sb = src0 + (size_t)c0 * 4;
        const unsigned cs4 = (unsigned)Cin * 4u;
        float *dst = smem + stage * WF_STAGE;
        wf_static_for<WF_DMA_PER_WAVE>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            if (a + 4 * m < WF_DMA) {
                int q = 8 * (a + 4 * m) + (lane >> 3);
                asm volatile("" : "+v"(q));      // (kept in the loop: hoisted, the per-instruction offsets would be held in registers)
                const int r = q / WF_WX, x = q - r * WF_WX;
                const unsigned voff = (unsigned)(r * Wp + x) * cs4 + (unsigned)(((lane & 7) ^ ((x >> 1) & 7)) * 16);
                wf_dma16(sb, voff, dst + (a + 4 * m) * 256);
            }
        });
    };

    // B fragments: lane (li, h) loads channels c0 + 8kk + 4h .. +3 of output channel n0 + 32ni + li, position 4a + b,
    // from w_wino_f[4a + b][(c0 + 8kk) / 8][n0 + 32ni + li][4h .. 4h + 3]
    // (buffer loads: a wave-uniform descriptor over the wave's 4 position planes, the uniform part of the offset in
    // soffset, the lane part in one VGPR — no 64-bit address arithmetic per load)
    const unsigned wlane = ((unsigned)(n0 + li) * 8u + 4u * h) * 4u;
    const size_t plane = (size_t)Cout * Cin;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w_wino_f + (size_t)(4 * a) * plane), 0, -1, 0x00020000);
    auto loadB = [&](f32x4 (&bf)[4][2], int c0, int kk) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int soff = (int)(((size_t)b * plane + ((size_t)(c0 / 8 + kk) * Cout + (size_t)ni * 32) * 8) * 4);
                bf[b][ni] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)wlane, soff, 0));
            }
    };

    // rows of the 4x4 window that (B^T d)[a] combines: e = d[ra] + sg * d[rb]
    const int ra = a == 0 ? 0 : (a == 2 ? 2 : 1);
    const int rb = a == 0 ? 2 : (a == 1 ? 2 : (a == 2 ? 1 : 3));
    const float sg = a == 1 ? 1.f : -1.f;
    int aoff[2][4];          // float offsets of the lane's window pixels (rows ra, rb; columns 0..3) in a stage
    int asw[4];              // swizzle of those columns
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        aoff[0][x] = (ra * WF_WX + 2 * li + x) * 32;
        aoff[1][x] = (rb * WF_WX + 2 * li + x) * 32;
        asw[x] = (li + (x >> 1)) & 7;
    }

    f32x16 acc[4][2];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][ni][r] = 0.f;

    const int nk = Cin / 32;
    f32x4 bf[2][4][2];
    issue(0, 0);
    loadB(bf[0], 0, 0);
    __syncthreads();                          // (waits for this wave's DMA; the barrier publishes everybody's)
    for (int kt = 0; kt < nk; ++kt) {
        const int c0 = kt * 32;
        if (kt + 1 < nk) issue(c0 + 32, (kt + 1) & 1);   // stage free since the barrier that ended step kt - 1
        const float *st = smem + (kt & 1) * WF_STAGE;
        wf_static_for<4>([&](auto kc) {
            constexpr int kk = decltype(kc)::value;
            if constexpr (kk < 3) loadB(bf[(kk + 1) & 1], c0, kk + 1);
            else if (kt + 1 < nk) loadB(bf[0], c0 + 32, 0);
            const int ch = 2 * kk + h;
            f32x4 e[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const f32x4 d0 = *reinterpret_cast<const f32x4 *>(st + aoff[0][x] + ((ch ^ asw[x]) << 2));
                const f32x4 d1 = *reinterpret_cast<const f32x4 *>(st + aoff[1][x] + ((ch ^ asw[x]) << 2));
                e[x] = d0 + sg * d1;
            }
            f32x4 u[4];
            u[0] = e[0] - e[2];
            u[1] = e[1] + e[2];
            u[2] = e[2] - e[1];
            u[3] = e[1] - e[3];
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[b][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[b][j], bf[kk & 1][b][ni][j], acc[b][ni], 0, 0, 0);
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
                const int tl = (threadIdx.x >> 4) + 16 * u;
                rv[u][r][cc] = p.resid.p ? *reinterpret_cast<const f32x4 *>(p.resid.p + p.resid.pix(n, 2 * ty + r, 2 * (tx0 + tl) + cc) * Cout + c)
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
        const int tl = (threadIdx.x >> 4) + 16 * u;
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
                const int oy = 2 * ty + r, ox = 2 * (tx0 + tl) + cc;
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

void launch_conv_wino(const ConvParams &p, ConvKernel form, hipStream_t s) {
    const int H = p.Hout, W = p.Wout, Cout = p.out.C;
    const int Cin = p.in0.C + (p.in1.p ? p.in1.C : 0);
    ConvParams o = p;
    if (p.in2.p) {
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
    if (form == CK_WINO_ONE_PASS) {
        const int spi = (H / 2) * (W / (2 * WF_T));
        const int spb = o.stats ? o.stats_slices / spi : 1;
        const unsigned blocks = (unsigned)((size_t)p.B * spi * (Cout / WF_BN));
        static bool attr_set = false;          // (more than 64 KiB of dynamic LDS)
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wino_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)WF_LDS);
            attr_set = true;
        }
        hipLaunchKernelGGL(wino_fused_kernel, dim3(blocks), dim3(256), WF_LDS, s, o, spb);
        return;
    }

    const size_t tiles = (size_t)p.B * (H / 2) * (W / 2);
    float *U = p.wino_ws, *Mw = p.wino_ws + 16 * tiles * Cin;
    const size_t items = tiles * (Cin / 4);
    if (!p.u_ready)
        hipLaunchKernelGGL(wino_input_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p.in0, p.in1, p.B, U);

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

} // namespace sr3
