// GroupNorm + Swish apply pass of ResnetBlock.block1 AND the block's 1x1 res_conv in ONE pass over the raw x ‖ skip
// (exact f32; reference unet.py:84-87 and :102-110).
//
// Before this kernel the raw concatenation was streamed from memory twice: by the apply pass (gn_apply_rows_kernel,
// HBM-bound, no MFMA) and, a few hundred microseconds later, by the 1x1 side launch of conv2's Winograd plan
// (conv_igemm_dma_f32<.., KS = 1, PREC = 0>, whose matrix pipe is half idle at the 128x128 level). Here the K loop of that
// 1x1 GEMM stages the raw A tile of every K-step (BM pixels x 32 channels) in LDS anyway; the waves that do not
// multiply read it from there, apply fmaf + swish_fast and store the activated values:
//   act = swish_fast(fmaf(x, scale, shift))   at the interior pixels of the zero-bordered activated tensor — the bits
//                                             gn_apply_rows_kernel<2, 0, ..> / gn_apply_kernel<2, 0> write;
//   res = W2 . raw                            into the block's output — the bits the side launch writes: one
//                                             v_mfma_f32_32x32x2_f32 chain per element, ascending K over in0 then in1,
//                                             no bias, no statistics. conv2 then takes it as its residual
//                                             (ConvParams::res_ready).
// Structure (kernels_conv.hip, the KS = 1 / PREC = 0 / NS = 2 form of conv_igemm_dma_f32): 512 threads = 4 consumer waves
// (ds_read_b128 + MFMA only) + 4 producer waves; LDS-DMA A and B tiles with the chunk swizzle c ^ ((row >> 1) & 7) on the
// source address and on the fragment read; two stages; the XCD block remap.
// What the producer waves do per K-step k:
//   s_waitcnt vmcnt(0) + s_barrier   tile k has landed (and this wave's stores of step k-1 have been acknowledged)
//   DMA of tile k+1                  into the stage every wave finished reading before that barrier
//   activation of tile k             each lane reads back the 16 B it DMA'd itself (lane-linear, conflict-free), so the
//                                    channel quad of a lane is the same in every K-step and row; scale / shift of the
//                                    tile's image come from a table staged into LDS once per block
// The wait is vmcnt(0), never a partial count: DMA loads and global stores share the counter and their completion
// order relative to each other is not defined, so no count between 0 and "everything" names a set of finished loads.
// The LDS reads of the activation are inline assembly: through the compiler they would be waited for with vmcnt(0)
// (a DMA in flight is a pending LDS write to it), i.e. tile k+1 would have to land before tile k is activated.
// A pixel tile with several Cout tiles (Cout / BN > 1): K-step k's activation is written by the block whose N-tile index
// is k % tilesN — every act element is written exactly once and the work is spread. No border pixel is ever written.
// Preconditions (gn_res1x1_shape_ok): C0 % 32 == 0, C1 % 32 == 0, Cout % 64 == 0, H * W % 128 == 0 (a tile lies in one
// image); every tensor below 4 GiB (32-bit byte offsets).
#include "sr3_internal.h"
#include <type_traits>

namespace sr3 {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32;            // channels per K-step
constexpr int ROWF = 32;          // floats per LDS row (128 B, unpadded)
constexpr int GR_BM = 128;        // pixels per tile

template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// every vector memory operation of this wave has completed, every LDS operation has returned; then the workgroup barrier
// (raw: __syncthreads() is the same wait here, but this keeps the count in the source)
__device__ __forceinline__ void producer_sync0() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

// 64 lanes x 16 B -> 1 KiB at lds_wave_base (wave-uniform) + lane * 16, from a wave-uniform base + a per-lane 32-bit byte
// offset: a resource descriptor in scalar registers, the offset goes into the instruction as it is (no vector arithmetic)
__device__ __forceinline__ void dma16b(const char *sbase, unsigned voff, float *lds_wave_base) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(sbase), 0, -1, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)lds_wave_base, 16, (int)voff, 0, 0, 0);
}

__device__ __forceinline__ unsigned lds_byte_addr(const float *p) {
    return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) float *)p;
}

// 16 B from LDS, invisible to the compiler's wait insertion (see the head of the file); the caller waits lgkmcnt(0)
__device__ __forceinline__ f32x4 lds_read16(unsigned byte_addr) {
    f32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(byte_addr));
    return v;
}

#pragma clang fp contract(off)      // (the activation is fmaf, then swish_fast: nothing else may fuse)
__device__ __forceinline__ float swish_fast(float x) {
    // x * sigmoid(x), as kernels_misc.hip
    return x * __frcp_rn(1.0f + __expf(-x));
}

struct GnResArgs {
    TDesc in0, in1;             // raw x, skip (in1.p == nullptr: none); zero-bordered or not
    const float *scale, *shift; // [B][C0 + C1]
    TDesc act;                  // activated, zero-bordered tensor of C0 + C1 channels
    const float *w2;            // [Cout][C0 + C1]
    TDesc out;                  // the block's output, C = Cout
    int B;
};

// (BN = 64: three blocks per CU, as the side launch's 128x64 tile has; the 128-wide tile holds two)
template <int BN>
__global__ __launch_bounds__(512, BN == 64 ? 6 : 4) void gn_res1x1_kernel(const GnResArgs p) {
    constexpr int BM = GR_BM, WGM = 2, WGN = 2, NS = 2;
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int MI = WM / 32, NI = WN / 32;
    constexpr int AR = BM / 32, BR = BN / 32;     // DMA instructions per producer wave and K-step
    constexpr int STAGE = (BM + BN) * ROWF;       // floats per pipeline stage
    static_assert(MI >= 1 && NI >= 1, "wave tile");

    // ONE LDS object: [2 stages][A: BM rows | B: BN rows][32 floats] | rowpix [BM] | scale [Cin] | shift [Cin]
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int *rowpix = reinterpret_cast<int *>(smem + NS * STAGE);   // [BM] output pixel index
    float *tab = smem + NS * STAGE + BM;                        // scale | shift of this tile's image

    const int C0 = p.in0.C, C1 = p.in1.p ? p.in1.C : 0;
    const int Cin = C0 + C1;
    const int Cout = p.out.C;
    const int HW = p.out.H * p.out.W, W = p.out.W;
    const int tilesN = Cout / BN;
    // XCD-aware block remap (bijective): the n-tiles of one m-tile share one L2 (kernels_conv.hip)
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x;
        const int xcd = bid & 7, loc = bid >> 3;
        const int qq = nwg >> 3, rr = nwg & 7;
        bid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + loc;
    }
    const int tn = bid % tilesN;
    const int m0 = (bid / tilesN) * BM;
    const int n0 = tn * BN;
    const int img = m0 / HW;                      // (HW % BM == 0: the tile lies in one image)
    const int nk = Cin / BK;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;

    if (wid >= 4) {
        // ------------------------------- producer waves -------------------------------------
        const int w = wid - 4;
        const int tid = threadIdx.x - 256;
        if (tid < BM) {
            const int rem = m0 + tid - img * HW;
            const int oy = rem / W;
            rowpix[tid] = (int)p.out.pix(img, oy, rem - oy * W);
        }
        // (ordinary loads: before the first DMA is issued, so that no wait for them drains a DMA)
        for (int c = tid; c < Cin; c += 256) {
            tab[c] = p.scale[(size_t)img * Cin + c];
            tab[Cin + c] = p.shift[(size_t)img * Cin + c];
        }
        // DMA instruction i of this wave fills tile rows (4i + w) * 8 + (lane >> 3); lane & 7 is the 16-B position inside
        // the row, which holds source chunk (lane & 7) ^ ((row >> 1) & 7) = sq — the same for every i.
        const int rsub = lane >> 3;
        const unsigned sq = (unsigned)((lane & 7) ^ ((((w & 1) << 2) | (lane >> 4)) & 7));
        const unsigned schunk16 = sq * 16u;
        unsigned vA0[AR], vA1[AR], vAct[AR], vB[BR];
        static_for<AR>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const int rem = m0 + (4 * i + w) * 8 + rsub - img * HW;
            const int oy = rem / W, ox = rem - oy * W;
            vA0[i] = (unsigned)p.in0.pix(img, oy, ox) * (unsigned)C0 * 4u + schunk16;
            vA1[i] = C1 ? (unsigned)p.in1.pix(img, oy, ox) * (unsigned)C1 * 4u + schunk16 : 0u;
            vAct[i] = (unsigned)p.act.pix(img, oy, ox) * (unsigned)Cin * 4u + schunk16;
        });
        static_for<BR>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            vB[i] = (unsigned)(n0 + (4 * i + w) * 8 + rsub) * (unsigned)Cin * 4u + schunk16;
        });
        const unsigned a_lds = lds_byte_addr(smem + w * 256) + (unsigned)lane * 16u;    // this lane's 16 B of DMA 0, stage 0
        const unsigned tab_lds = lds_byte_addr(tab) + schunk16;

        auto issue = [&](int k) {
            const int c0 = k * BK;
            float *Ad = smem + (k & 1) * STAGE + w * 256;
            float *Bd = Ad + BM * ROWF;
            const bool first = c0 < C0;
            const char *ab = reinterpret_cast<const char *>(first ? p.in0.p + c0 : p.in1.p + (c0 - C0));
            const char *wb = reinterpret_cast<const char *>(p.w2 + c0);
            if (first) {
                static_for<AR>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    dma16b(ab, vA0[i], Ad + i * 1024);
                });
            } else {
                static_for<AR>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    dma16b(ab, vA1[i], Ad + i * 1024);
                });
            }
            static_for<BR>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                dma16b(wb, vB[i], Bd + i * 1024);
            });
        };

        issue(0);
        int turn = 0;                        // k % tilesN
        for (int k = 0; k < nk; ++k) {
            producer_sync0();                // barrier #k: tile k is in LDS, stage (k+1)&1 is free
            if (k + 1 < nk) issue(k + 1);
            if (turn == tn) {
                const int c0 = k * BK;
                const unsigned ad = a_lds + (unsigned)((k & 1) * STAGE * 4);
                const unsigned td = tab_lds + (unsigned)c0 * 4u;
                f32x4 x[AR];
                const f32x4 sc = lds_read16(td), sh = lds_read16(td + (unsigned)Cin * 4u);
                static_for<AR>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    x[i] = lds_read16(ad + i * 4096u);
                });
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                char *ob = reinterpret_cast<char *>(p.act.p + c0);
                static_for<AR>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = swish_fast(fmaf(x[i][j], sc[j], sh[j]));
                    *reinterpret_cast<f32x4 *>(ob + vAct[i]) = v;
                });
            }
            turn = turn + 1 == tilesN ? 0 : turn + 1;
        }
        producer_sync0();                    // the consumers' barrier behind their last tile
        return;
    }

    // ----------------------------------- consumer waves -----------------------------------------
    const int li = lane & 31, lh = lane >> 5;
    const int wm = wid / WGN, wn = wid % WGN;

    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    const int swz = (li >> 1) & 7;          // == ((row >> 1) & 7) for every row this lane reads
    const float *Abase = smem + (wm * WM + li) * ROWF;
    const float *Bbase = smem + BM * ROWF + (wn * WN + li) * ROWF;
    // Fragment reads run one 8-k group ahead of the MFMAs (two register sets); the reads of the next tile's first group
    // are issued right after the barrier and land under the last group's MFMAs (kernels_conv.hip).
    int koff[BK / 8];                   // float offset of chunk (2kk + lh) after swizzling
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) koff[kk] = (((2 * kk + lh) ^ swz) & 7) * 4;
    f32x4 fa[2][MI], fb[2][NI];
#define SR3_FRAG_READ(SET, CUR, KK)                                                                \
    {                                                                                              \
        _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) fa[SET][mi] =                            \
            *reinterpret_cast<const f32x4 *>(Abase + (CUR) * STAGE + mi * 32 * ROWF + koff[KK]);   \
        _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) fb[SET][ni] =                            \
            *reinterpret_cast<const f32x4 *>(Bbase + (CUR) * STAGE + ni * 32 * ROWF + koff[KK]);   \
    }
#define SR3_FRAG_MMA(SET)                                                                          \
    {                                                                                              \
        _Pragma("unroll") for (int mi = 0; mi < MI; ++mi)                                          \
        _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) {                                        \
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET][mi].x, fb[SET][ni].x, acc[mi][ni], 0, 0, 0); \
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET][mi].y, fb[SET][ni].y, acc[mi][ni], 0, 0, 0); \
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET][mi].z, fb[SET][ni].z, acc[mi][ni], 0, 0, 0); \
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[SET][mi].w, fb[SET][ni].w, acc[mi][ni], 0, 0, 0); \
        }                                                                                          \
    }
    __syncthreads();                        // barrier #0
    SR3_FRAG_READ(0, 0, 0)
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1, nxt = cur ^ 1;
        SR3_FRAG_READ(1, cur, 1)
        SR3_FRAG_MMA(0)
        SR3_FRAG_READ(0, cur, 2)
        SR3_FRAG_MMA(1)
        SR3_FRAG_READ(1, cur, 3)
        SR3_FRAG_MMA(0)
        __syncthreads();                    // every read of this stage has been issued and waited
        SR3_FRAG_READ(0, nxt, 0)            // next tile (stale data after the last one: unused)
        SR3_FRAG_MMA(1)
    }
#undef SR3_FRAG_READ
#undef SR3_FRAG_MMA

    // epilogue: the accumulators as they are (whole tiles in M and N: nothing is masked).
    // C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const unsigned n = (unsigned)(n0 + wn * WN + ni * 32 + li);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * WM + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                p.out.p[(unsigned)rowpix[row] * (unsigned)Cout + n] = acc[mi][ni][r];
            }
    }
}

template <int BN>
void launch_inst(const GnResArgs &a, hipStream_t s) {
    static bool attr_set = false;
    const int Cin = a.in0.C + (a.in1.p ? a.in1.C : 0);
    // (the attribute is set for the widest table any caller may bring: gn_res1x1_shape_ok bounds Cin)
    constexpr size_t lds_max = ((size_t)2 * (GR_BM + BN) * ROWF + GR_BM + 2 * GN_RES1X1_MAX_CIN) * sizeof(float);
    const size_t lds = ((size_t)2 * (GR_BM + BN) * ROWF + GR_BM + 2 * (size_t)Cin) * sizeof(float);
    auto kern = gn_res1x1_kernel<BN>;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
        attr_set = true;
    }
    const long M = (long)a.B * a.out.H * a.out.W;
    hipLaunchKernelGGL(kern, dim3((unsigned)((M / GR_BM) * (a.out.C / BN))), dim3(512), lds, s, a);
}

} // namespace

bool gn_res1x1_shape_ok(int H, int W, int C0, int C1, int Cout) {
    const long HW = (long)H * W;
    return H > 0 && W > 0 && C0 > 0 && C1 >= 0 && Cout > 0 && (C0 % 32) == 0 && (C1 % 32) == 0 && C0 + C1 <= GN_RES1X1_MAX_CIN &&
           (Cout % 64) == 0 && (HW % GR_BM) == 0;
}

// output channels per block: 128 where that still leaves two resident blocks per CU on 256 CUs (conv_tile_choice's rule)
int gn_res1x1_bn(int B, int H, int W, int Cout) {
    const long M = plan_b(B) * H * W;
    return ((Cout % 128) == 0 && (M / GR_BM) * (Cout / 128) >= 512) ? 128 : 64;
}

void launch_gn_res1x1(const TDesc &in0, const TDesc &in1, int B, const float *scale, const float *shift, const TDesc &act,
                      const float *w2, const TDesc &out, hipStream_t s) {
    GnResArgs a;
    a.in0 = in0; a.in1 = in1; a.scale = scale; a.shift = shift; a.act = act; a.w2 = w2; a.out = out; a.B = B;
    if (gn_res1x1_bn(B, out.H, out.W, out.C) == 128) launch_inst<128>(a, s);
    else launch_inst<64>(a, s);
}

} // namespace sr3
