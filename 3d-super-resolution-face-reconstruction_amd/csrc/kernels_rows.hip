// The update half of a rolling-batch step: every batch row sits at its own position of the schedule, so
// the per-step values that ddpm_update_kernel reads once from StepArgs come per row from a RowArgs table instead. The three
// kernels below are ddpm_update_kernel (kernels_misc.hip), x0_predict_kernel and update_from_x0_kernel
// (kernels_consist.hip) statement for statement — the same __fmul_rn / __fsub_rn / __fadd_rn sequence, clamp, history
// read-before-write, packed split-f16 twin store and range detection — with `rows[n]` in the place of `*u.args`: a row
// stepped here carries the bits the uniform sampler gives it, whatever its slot and its neighbours.
// A row with live == 0 is neither read nor written: not the state, not the packed copy, not the history.
// Element-wise, no matrix work: bound by the Philox / Box-Muller arithmetic like the kernels they mirror.
#include "sr3_internal.h"

#include <algorithm>

namespace sr3 {

namespace {

inline unsigned nblk(size_t n) { return (unsigned)((n + 255) / 256); }

// (image, channel, pixel) of flat NCHW index i
struct Elem { int n, c, pp, y, x, HW; };
__device__ __forceinline__ Elem elem_of(const RowsUpdateParams &u, size_t i) {
    Elem e;
    e.HW = u.state.H * u.state.W;
    e.pp = (int)(i % e.HW);
    const size_t nc = i / e.HW;
    e.n = (int)(nc / u.C);
    e.c = (int)(nc - (size_t)e.n * u.C);
    e.y = e.pp / u.state.W;
    e.x = e.pp - e.y * u.state.W;
    return e;
}

// the tail both update kernels share from `v = c1*x0 + c2*x` on (ddpm_update_kernel's, with the row's arguments)
__device__ __forceinline__ void finish_update(const RowsUpdateParams &u, const RowArgs &ra, const Elem &e, size_t i, size_t pix,
                                              size_t si, float x, float x0) {
    float v = __fadd_rn(__fmul_rn(ra.c1, x0), __fmul_rn(ra.c2, x));
    if (ra.hist) {
        if (ra.hist == 2) v = __fadd_rn(v, __fmul_rn(ra.c3, u.hist[i]));
        u.hist[i] = x0;                 // (same element, same thread: read before the overwrite)
    }
    if (ra.sigma != 0.f) {
        // the row's own slab [C][HW] | the stream of its global image id
        const float z = ra.noise ? ra.noise[(size_t)e.c * e.HW + e.pp]
                                 : philox_normal(ra.seed, ra.image, ra.draw, (uint32_t)(e.c * e.HW + e.pp));
        v = __fadd_rn(v, __fmul_rn(z, ra.sigma));
    }
    u.state.p[si] = v;
    if (u.packed != nullptr) {
        _Float16 *pk = reinterpret_cast<_Float16 *>(u.packed) + pix * 16 + u.xoff + e.c;
        const _Float16 hi = (_Float16)v;
        pk[0] = hi;
        pk[8] = (_Float16)(v - (float)hi);
        if (u.ovf != nullptr && ((unsigned)__builtin_bit_cast(unsigned short, hi) & 0x7C00u) == 0x7C00u) *u.ovf = 1;
    }
    if (ra.frame) ra.frame[(size_t)e.c * e.HW + e.pp] = v;     // (the row's own [C][HW] frame of this step)
}

__global__ void rows_update_kernel(const RowsUpdateParams u, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over B*C*HW, NCHW order
    if (i >= total) return;
    const Elem e = elem_of(u, i);
    const RowArgs ra = u.rows[e.n];
    if (!ra.live) return;
    const size_t pix = u.state.pix(e.n, e.y, e.x);
    const size_t si = pix * u.state.C + u.xoff + e.c;
    const float x = u.state.p[si];
    const float ep = u.eps.p[u.eps.pix(e.n, e.y, e.x) * u.eps.C + e.c];
    float x0 = __fsub_rn(__fmul_rn(ra.a, x), __fmul_rn(ra.b, ep));
    x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    finish_update(u, ra, e, i, pix, si, x, x0);
}

// CLAMP false: the prediction as it is, for the dynamic threshold. An idle row's slab of x0hat is written as zeros: the
// threshold kernels behind this one run over all B rows, and zeros give them s = 1 and nothing to do.
template <bool CLAMP>
__global__ void rows_x0_predict_kernel(const RowsUpdateParams u, float *__restrict__ x0hat, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const Elem e = elem_of(u, i);
    const RowArgs ra = u.rows[e.n];
    if (!ra.live) { x0hat[i] = 0.f; return; }
    const float x = u.state.p[u.state.pix(e.n, e.y, e.x) * u.state.C + u.xoff + e.c];
    const float ep = u.eps.p[u.eps.pix(e.n, e.y, e.x) * u.eps.C + e.c];
    const float x0 = __fsub_rn(__fmul_rn(ra.a, x), __fmul_rn(ra.b, ep));
    x0hat[i] = CLAMP ? fminf(fmaxf(x0, -1.0f), 1.0f) : x0;
}

__global__ void rows_update_from_x0_kernel(const RowsUpdateParams u, const float *__restrict__ x0hat, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const Elem e = elem_of(u, i);
    const RowArgs ra = u.rows[e.n];
    if (!ra.live) return;
    const size_t pix = u.state.pix(e.n, e.y, e.x);
    const size_t si = pix * u.state.C + u.xoff + e.c;
    finish_update(u, ra, e, i, pix, si, u.state.p[si], x0hat[i]);
}

// sr3_rows_move (live rows only): a pure copy, bound by memory traffic (about 3 MB at 128x128: the
// 2.2 MB state slab read, written and zeroed dominates). blockIdx.y picks the segment, blockIdx.x strides over its
// 16-byte units (VEC) or its floats; each element is read, stored to the destination and, for the state and the packed
// copy, overwritten with zero at the source by the same thread.
__global__ void rows_move_kernel(const RowsMoveParams p) {
    const RowsMoveSeg sg = p.seg[blockIdx.y];
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool vec = (sg.n % 4) == 0 && ((reinterpret_cast<uintptr_t>(sg.src) | reinterpret_cast<uintptr_t>(sg.dst)) & 15) == 0;
    if (vec) {
        float4 *src = reinterpret_cast<float4 *>(sg.src);
        float4 *dst = reinterpret_cast<float4 *>(sg.dst);
        const size_t n4 = sg.n / 4;
        for (size_t i = i0; i < n4; i += stride) {
            dst[i] = src[i];
            if (sg.zero) src[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        for (size_t i = i0; i < sg.n; i += stride) {
            sg.dst[i] = sg.src[i];
            if (sg.zero) sg.src[i] = 0.f;
        }
    }
}

} // namespace

void launch_rows_move(const RowsMoveParams &p, hipStream_t s) {
    if (p.nseg < 1) return;
    size_t most = 0;
    for (int i = 0; i < p.nseg; ++i) most = std::max(most, (p.seg[i].n + 3) / 4);
    // memory-bound: one 16-byte unit per thread up to 2048 blocks, the rest in the grid-stride loop
    const unsigned gx = (unsigned)std::min<size_t>(std::max<size_t>(nblk(most), 1), 2048);
    hipLaunchKernelGGL(rows_move_kernel, dim3(gx, (unsigned)p.nseg), dim3(256), 0, s, p);
}

void launch_rows_update(const RowsUpdateParams &p, int B, hipStream_t s) {
    const size_t total = (size_t)B * p.C * p.state.H * p.state.W;
    hipLaunchKernelGGL(rows_update_kernel, dim3(nblk(total)), dim3(256), 0, s, p, total);
}
void launch_rows_x0_predict(const RowsUpdateParams &p, float *x0hat, int B, hipStream_t s, bool clamp) {
    const size_t total = (size_t)B * p.C * p.state.H * p.state.W;
    if (clamp) hipLaunchKernelGGL(rows_x0_predict_kernel<true>, dim3(nblk(total)), dim3(256), 0, s, p, x0hat, total);
    else hipLaunchKernelGGL(rows_x0_predict_kernel<false>, dim3(nblk(total)), dim3(256), 0, s, p, x0hat, total);
}
void launch_rows_update_from_x0(const RowsUpdateParams &p, const float *x0hat, int B, hipStream_t s) {
    const size_t total = (size_t)B * p.C * p.state.H * p.state.W;
    hipLaunchKernelGGL(rows_update_from_x0_kernel, dim3(nblk(total)), dim3(256), 0, s, p, x0hat, total);
}

} // namespace sr3
