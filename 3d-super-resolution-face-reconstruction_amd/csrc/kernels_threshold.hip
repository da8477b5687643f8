// Dynamic thresholding of the sampler's x0 prediction (Imagen, Saharia et al. 2022, §2.3). Per image,
// s = the `ratio`-quantile of |x0| over its n = C*H*W values (linear interpolation between two order statistics),
// raised to 1 and capped at max_value; x0 <- clamp(x0, -s, s) / s. With s = 1 that is the reference's
// x_recon.clamp_(-1., 1.) (model/sr/sr3_modules/diffusion.py:175-176) bit for bit.
//
// The order statistics are exact: a radix select over the keys (bit patterns of |x0| as unsigned integers, a total
// order with NaN above inf) in four passes of 8 bits, most significant first. A pass counts, per image, the keys that
// carry the prefix selected so far by their next digit: 256 integer bins in LDS per block (a wave whose lanes agree on
// the digit — the rule in the exponent passes — adds its popcount once), merged into the image's global bins with
// integer atomics, so several blocks share one image and the counts do not depend on their order. The digit of rank k is
// where the running sum of the bins passes k; every block of the next pass and the final kernel redo that 256-wide scan
// from the global bins instead of waiting for one another. Rank k + 1 rides along: while its prefix equals rank k's it
// reads the same bins, and once they part a key can carry only one of the two prefixes, so it is still counted once, in
// a second set of bins. No floating-point atomics, no sampling: two calls return the same bits.
#include "sr3_internal.h"
#include <algorithm>
#include <math.h>

namespace sr3 {

namespace {

constexpr int THR_THREADS = 256;                // = bins of a pass: thread d owns digit d in the scans and merges
constexpr int THR_UNROLL = 4;                   // loads in flight per thread
constexpr long THR_CHUNK = 16384;               // keys per block at which an image gets another block
constexpr int THR_MAX_BLOCKS = 1024;            // blocks per image (the blocks stride over the image beyond that)

// rank state of the select: the key bits fixed so far and the rank left among the keys that carry them
struct ThrRank { unsigned prefix, rank; };

// The states of ranks k and k2 after `passes` passes, from the image's global bins [THR_PASSES][2][256]. Every thread of
// the block (256) takes part and returns the same values. sc [256] and win [2]: LDS.
__device__ __forceinline__ void thr_resolve(const unsigned *__restrict__ bins, int passes, unsigned k, unsigned k2, unsigned *sc,
                                            unsigned *win, ThrRank &A, ThrRank &B) {
    const int tid = threadIdx.x;
    A.prefix = 0u; A.rank = k; B.prefix = 0u; B.rank = k2;
    for (int p = 0; p < passes; ++p) {
        const int shift = 24 - THR_DIGIT_BITS * p;
        const bool same = A.prefix == B.prefix;         // (the prefixes the counting pass p saw)
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const unsigned *h = bins + (size_t)(p * 2 + ((w && !same) ? 1 : 0)) * THR_BINS;
            const unsigned r = w ? B.rank : A.rank;
            const unsigned v = h[tid];
            sc[tid] = v;
            __syncthreads();
            for (int off = 1; off < THR_BINS; off <<= 1) {          // inclusive scan
                const unsigned t = tid >= off ? sc[tid - off] : 0u;
                __syncthreads();
                sc[tid] += t;
                __syncthreads();
            }
            const unsigned incl = sc[tid], excl = incl - v;
            if (tid == 0) { win[0] = THR_BINS - 1; win[1] = sc[THR_BINS - 2]; }   // (a rank past the count: the last digit)
            __syncthreads();
            if (r >= excl && r < incl) { win[0] = (unsigned)tid; win[1] = excl; }  // one thread at most: empty bins never win
            __syncthreads();
            const unsigned d = win[0], below = win[1];
            if (w) { B.prefix |= d << shift; B.rank = r - below; }
            else { A.prefix |= d << shift; A.rank = r - below; }
            __syncthreads();
        }
    }
}

// pass `pass` over image blockIdx.y: bins[pass][0][d] += keys with rank k's prefix and next digit d; [pass][1][d] the
// same for rank k2's prefix once it differs
__global__ __launch_bounds__(THR_THREADS) void thr_count_kernel(const float *__restrict__ x, long n, unsigned *__restrict__ bins_all,
                                                                int pass, unsigned k, unsigned k2) {
    __shared__ unsigned h[2 * THR_BINS];
    __shared__ unsigned sc[THR_BINS];
    __shared__ unsigned win[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const float *xi = x + (size_t)blockIdx.y * (size_t)n;
    unsigned *bins = bins_all + (size_t)blockIdx.y * THR_BINS_PER_IMAGE;
    ThrRank A, B;
    thr_resolve(bins, pass, k, k2, sc, win, A, B);
    h[tid] = 0u; h[THR_BINS + tid] = 0u;
    __syncthreads();
    const int shift = 24 - THR_DIGIT_BITS * pass;
    const unsigned pmask = pass == 0 ? 0u : ~0u << (shift + THR_DIGIT_BITS);
    const long step = (long)gridDim.x * THR_THREADS * THR_UNROLL;
    for (long base = (long)blockIdx.x * THR_THREADS * THR_UNROLL; base < n; base += step) {     // (uniform over the block)
        unsigned key[THR_UNROLL];
#pragma unroll
        for (int u = 0; u < THR_UNROLL; ++u) {
            const long i = base + (long)u * THR_THREADS + tid;
            key[u] = i < n ? (__float_as_uint(xi[i]) & 0x7FFFFFFFu) : 0xFFFFFFFFu;      // (no key has the top bit: matches no prefix)
        }
#pragma unroll
        for (int u = 0; u < THR_UNROLL; ++u) {
            const unsigned hp = key[u] & pmask;
            const bool tail = (base + (long)u * THR_THREADS + tid) < n;
            const bool inA = tail && hp == A.prefix;
            const bool inB = tail && !inA && hp == B.prefix;
            const bool valid = inA || inB;
            const unsigned d = ((key[u] >> shift) & (THR_BINS - 1)) | (inB ? THR_BINS : 0);
            const unsigned long long vm = __ballot(valid);
            if (vm == 0ull) continue;                                   // (wave-uniform)
            const int leader = __ffsll((long long)vm) - 1;
            const unsigned d0 = __shfl(d, leader);
            const unsigned long long eq = __ballot(valid && d == d0);
            if (lane == leader) atomicAdd(&h[d0], (unsigned)__popcll(eq));
            else if (valid && d != d0) atomicAdd(&h[d], 1u);
        }
    }
    __syncthreads();
    unsigned *out = bins + (size_t)pass * 2 * THR_BINS;
    if (h[tid]) atomicAdd(&out[tid], h[tid]);
    if (h[THR_BINS + tid]) atomicAdd(&out[THR_BINS + tid], h[THR_BINS + tid]);
}

// one block per image: the two keys, and s = min(max(lo + frac * (hi - lo), 1), max_value) (a NaN sum gives 1)
__global__ __launch_bounds__(THR_THREADS) void thr_final_kernel(const unsigned *__restrict__ bins_all, unsigned k, unsigned k2, float frac,
                                                                float max_value, float *__restrict__ lo_out, float *__restrict__ hi_out,
                                                                float *__restrict__ s_out) {
    __shared__ unsigned sc[THR_BINS];
    __shared__ unsigned win[2];
    ThrRank A, B;
    thr_resolve(bins_all + (size_t)blockIdx.x * THR_BINS_PER_IMAGE, THR_PASSES, k, k2, sc, win, A, B);
    if (threadIdx.x != 0) return;
    const float lo = __uint_as_float(A.prefix), hi = __uint_as_float(B.prefix);
    const float s_raw = __fadd_rn(lo, __fmul_rn(frac, __fsub_rn(hi, lo)));
    if (lo_out) lo_out[blockIdx.x] = lo;
    if (hi_out) hi_out[blockIdx.x] = hi;
    if (s_out) s_out[blockIdx.x] = fminf(fmaxf(s_raw, 1.0f), max_value);
}

// the counts back to zero, as a kernel: a captured step holds kernel nodes only. With a hipMemsetAsync here (a memset node
// of the captured step) a thresholded call repeated on a workspace that replaced an older one ran with s = 1 in every step
// when replayed from its graph, and an armed thresholded rows step gave other images replayed than run eagerly
// (tests/test_gpu_engine_history.py fails on such a build)
__global__ void thr_zero_kernel(unsigned *__restrict__ bins, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) bins[i] = 0u;
}

__global__ void thr_apply_kernel(float *__restrict__ x, long n, size_t total, const float *__restrict__ s_all) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float s = s_all[i / (size_t)n];
    x[i] = __fdiv_rn(fminf(fmaxf(x[i], -s), s), s);
}

// measurement switch (read once): the blocks that share one image, 0 = by size
int thr_blocks_override() {
    static const int v = std::max(0, env_int("SR3_THRESHOLD_BLOCKS", 0));
    return v;
}

} // namespace

ThrPlan threshold_plan(float ratio, int64_t n) {
    ThrPlan p;
    const double pos = (double)ratio * (double)(n - 1);
    const double fl = floor(pos);
    const int64_t k = std::min<int64_t>((int64_t)fl, n - 1);
    p.k = (unsigned)k;
    p.k2 = (unsigned)std::min<int64_t>(k + 1, n - 1);
    p.frac = (float)(pos - (double)k);
    const int ov = thr_blocks_override();
    p.blocks = ov ? std::min(ov, THR_MAX_BLOCKS) : (int)std::min<int64_t>((n + THR_CHUNK - 1) / THR_CHUNK, THR_MAX_BLOCKS);
    return p;
}

void launch_abs_quantile(const float *x, int B, int64_t n, const ThrPlan &p, float max_value, unsigned *bins, float *lo, float *hi,
                         float *s, hipStream_t st) {
    const size_t total = (size_t)B * THR_BINS_PER_IMAGE;
    hipLaunchKernelGGL(thr_zero_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, bins, total);
    for (int pass = 0; pass < THR_PASSES; ++pass)
        hipLaunchKernelGGL(thr_count_kernel, dim3(p.blocks, B), dim3(THR_THREADS), 0, st, x, (long)n, bins, pass, p.k, p.k2);
    hipLaunchKernelGGL(thr_final_kernel, dim3(B), dim3(THR_THREADS), 0, st, (const unsigned *)bins, p.k, p.k2, p.frac, max_value, lo, hi, s);
}

void launch_threshold_apply(float *x, int B, int64_t n, const float *s, hipStream_t st) {
    const size_t total = (size_t)B * (size_t)n;
    hipLaunchKernelGGL(thr_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, (long)n, total, s);
}

} // namespace sr3
