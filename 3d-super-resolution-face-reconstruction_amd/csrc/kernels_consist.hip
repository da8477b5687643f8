// Low-resolution consistency of the sampler. The reference's degradation model — Pillow's antialiased
// bicubic resample r -> l (datasets/tool/prepare_data.py:37-47) — is, in real arithmetic, the separable linear operator
// A = A_v (x) A_h with A_v [lh][H], A_h [lw][W] the weights of precompute_coeffs before their fixed-point rounding.
// With P = A^T (A A^T)^-1, projecting the predicted x0 of a step onto {x : A x = y},
//     X <- X + lambda * P_v (Y - A_v X A_h^T) P_h^T          per (image, channel) plane,
// is the range / null-space correction of DDNM (Wang et al. 2022): the LR image fixes what it can see, the network
// keeps the rest. This file: the operators (host, float64), the projection in two forms (one block per plane with the
// intermediates in LDS; four launches over global scratch), the residual score, and the DDPM update split in two around
// the projection. All fp32, no atomics.
#include "sr3_internal.h"
#include <math.h>
#include <vector>

namespace sr3 {

// ---- operators (host) ----------------------------------------------------------------------------------------------
namespace {

double bicubic_weight(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

} // namespace

// A [l][r]: row i = the normalised real weights of output pixel i of the r -> l resample (bounds [l][2] = first input and
// count, may be null); P [r][l] = A^T (A A^T)^-1 through a Cholesky factorisation of the l x l Gram matrix (symmetric
// positive definite, condition number ~2). false: the Gram matrix was not positive definite.
bool lr_operators(int l, int r, double *A, double *P, int *bounds) {
    const double scale = (double)r / l;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale, ss = 1.0 / filterscale;
    std::fill(A, A + (size_t)l * r, 0.0);
    for (int i = 0; i < l; ++i) {
        const double center = (i + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > r) xmax = r;
        double *row = A + (size_t)i * r;
        double ww = 0.0;
        for (int x = xmin; x < xmax; ++x) {
            row[x] = bicubic_weight((x - center + 0.5) * ss);
            ww += row[x];
        }
        if (ww != 0.0)
            for (int x = xmin; x < xmax; ++x) row[x] /= ww;
        if (bounds) { bounds[2 * i] = xmin; bounds[2 * i + 1] = xmax - xmin; }
    }
    // G = A A^T = L L^T (lower triangle of G overwritten by L)
    std::vector<double> G((size_t)l * l);
    for (int i = 0; i < l; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int x = 0; x < r; ++x) s += A[(size_t)i * r + x] * A[(size_t)j * r + x];
            G[(size_t)i * l + j] = s;
        }
    for (int j = 0; j < l; ++j) {
        double d = G[(size_t)j * l + j];
        for (int k = 0; k < j; ++k) d -= G[(size_t)j * l + k] * G[(size_t)j * l + k];
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        G[(size_t)j * l + j] = d;
        for (int i = j + 1; i < l; ++i) {
            double s = G[(size_t)i * l + j];
            for (int k = 0; k < j; ++k) s -= G[(size_t)i * l + k] * G[(size_t)j * l + k];
            G[(size_t)i * l + j] = s / d;
        }
    }
    // column x of Z = G^-1 A is row x of P (G is symmetric): forward, then backward substitution
    std::vector<double> z(l);
    for (int x = 0; x < r; ++x) {
        for (int i = 0; i < l; ++i) {
            double s = A[(size_t)i * r + x];
            for (int k = 0; k < i; ++k) s -= G[(size_t)i * l + k] * z[k];
            z[i] = s / G[(size_t)i * l + i];
        }
        for (int i = l - 1; i >= 0; --i) {
            double s = z[i];
            for (int k = i + 1; k < l; ++k) s -= G[(size_t)k * l + i] * z[k];
            z[i] = s / G[(size_t)i * l + i];
        }
        for (int i = 0; i < l; ++i) P[(size_t)x * l + i] = z[i];
    }
    return true;
}

// ---- the four stages, one element each (shared by both forms: they agree bit for bit) ---------------------------------
namespace {

// T[y][j] = sum_x X[y][x] A_h[j][x] over the band of row j
__device__ __forceinline__ float stage_t(const float *__restrict__ xrow, const LrOps &o, int j) {
    const int x0 = o.bh[2 * j], n = o.bh[2 * j + 1];
    const float *a = o.Ah + (size_t)j * o.W + x0;
    const float *x = xrow + x0;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s = fmaf(x[k], a[k], s);
    return s;
}
// R[i][j] = Y[i][j] - sum_y A_v[i][y] T[y][j] over the band of row i (T row stride lw)
__device__ __forceinline__ float stage_r(const float *T, float yv, const LrOps &o, int i, int j) {
    const int y0 = o.bv[2 * i], n = o.bv[2 * i + 1];
    const float *a = o.Av + (size_t)i * o.H + y0;
    const float *t = T + (size_t)y0 * o.lw + j;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s = fmaf(a[k], t[(size_t)k * o.lw], s);
    return __fsub_rn(yv, s);
}
// U[y][j] = sum_i P_v[y][i] R[i][j]
__device__ __forceinline__ float stage_u(const float *R, const LrOps &o, int y, int j) {
    const float *p = o.Pv + (size_t)y * o.lh;
    float s = 0.f;
    for (int i = 0; i < o.lh; ++i) s = fmaf(p[i], R[i * o.lw + j], s);
    return s;
}
// X[y][x] + lambda * sum_j U[y][j] P_h[x][j]   (P_h stored transposed, [lw][W]: consecutive x are consecutive floats)
__device__ __forceinline__ float stage_x(float xv, const float *urow, const LrOps &o, int x, float lambda) {
    float s = 0.f;
    for (int j = 0; j < o.lw; ++j) s = fmaf(urow[j], o.PhT[(size_t)j * o.W + x], s);
    return fmaf(lambda, s, xv);
}

__device__ __forceinline__ const float *lr_plane(const LrArgs &a, const LrOps &o, int plane, int C) {
    const int b = plane / C, c = plane - b * C;
    const uint64_t n = (a.row_offset + (uint64_t)b) % (uint64_t)a.N;
    return a.lr + ((size_t)n * C + c) * o.lh * o.lw;
}

// one block per plane; LDS: T [H][lw] (reused for U) | R [lh][lw]. B*C planes are fewer blocks than the device has compute
// units at the sampler's batch sizes, so a plane of 64 x 64 or more takes 1024 threads (the stages are latency-bound
// chains of loads and fmaf: at B = 64, 16 -> 128, 82 us with 256 threads, 67 us with 1024; profiles/README.md finding 87).
// the four stages of one plane xp [H][W] against Y [lh][lw], by the whole block (both LDS kernels: the same statements)
__device__ __forceinline__ void lr_project_plane_lds(float *__restrict__ xp, const float *__restrict__ Y, const LrOps &o,
                                                     float strength, float *lds) {
    float *T = lds, *R = lds + (size_t)o.H * o.lw;
    const int nT = o.H * o.lw, nR = o.lh * o.lw, nX = o.H * o.W;
    for (int e = threadIdx.x; e < nT; e += blockDim.x) {
        const int y = e / o.lw, j = e - y * o.lw;
        T[e] = stage_t(xp + (size_t)y * o.W, o, j);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nR; e += blockDim.x) {
        const int i = e / o.lw, j = e - i * o.lw;
        R[e] = stage_r(T, Y[e], o, i, j);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nT; e += blockDim.x) {
        const int y = e / o.lw, j = e - y * o.lw;
        T[e] = stage_u(R, o, y, j);         // (T is dead: U takes its place)
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nX; e += blockDim.x) {
        const int y = e / o.W, x = e - y * o.W;
        xp[e] = stage_x(xp[e], T + (size_t)y * o.lw, o, x, strength);
    }
}

__global__ void __launch_bounds__(1024) lr_project_lds_kernel(float *__restrict__ X, int C, const LrOps o, const LrArgs val,
                                                             const LrArgs *dyn) {
    extern __shared__ float lds[];
    const LrArgs a = dyn ? *dyn : val;
    const int plane = blockIdx.x;
    lr_project_plane_lds(X + (size_t)plane * o.H * o.W, lr_plane(a, o, plane, C), o, a.strength, lds);
}

// ---- the rows form (rolling batch): the LR image and the strength of a plane come from its row's slot ---------------
// strength of the row a plane belongs to; 0: the plane is not touched (idle slot, or a row admitted without an LR image)
__device__ __forceinline__ float row_strength(const RowArgs *__restrict__ rows, int b) {
    return rows[b].live ? rows[b].lr_strength : 0.f;
}

// (the test is uniform over the block: all of it leaves before the first barrier, or none)
__global__ void __launch_bounds__(1024) lr_project_lds_rows_kernel(float *__restrict__ X, int C, const LrOps o,
                                                                  const float *__restrict__ lr_rows,
                                                                  const RowArgs *__restrict__ rows) {
    extern __shared__ float lds[];
    const int plane = blockIdx.x;
    const float strength = row_strength(rows, plane / C);
    if (strength == 0.f) return;
    lr_project_plane_lds(X + (size_t)plane * o.H * o.W, lr_rows + (size_t)plane * o.lh * o.lw, o, strength, lds);
}

__global__ void lr_rows_stage_t_kernel(const float *__restrict__ X, int C, const LrOps o, const RowArgs *__restrict__ rows,
                                       float *__restrict__ T, size_t total) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over planes*H*lw
    if (e >= total) return;
    const int j = (int)(e % o.lw);
    const size_t row = e / o.lw;                                        // plane*H + y
    if (row_strength(rows, (int)(row / o.H / C)) == 0.f) return;
    T[e] = stage_t(X + row * o.W, o, j);
}
__global__ void lr_rows_stage_r_kernel(const float *__restrict__ T, int C, const LrOps o, const float *__restrict__ lr_rows,
                                       const RowArgs *__restrict__ rows, float *__restrict__ R, size_t total) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over planes*lh*lw
    if (e >= total) return;
    const int nR = o.lh * o.lw;
    const int plane = (int)(e / nR), r = (int)(e - (size_t)plane * nR);
    if (row_strength(rows, plane / C) == 0.f) return;
    const int i = r / o.lw, j = r - i * o.lw;
    R[e] = stage_r(T + (size_t)plane * o.H * o.lw, lr_rows[e], o, i, j);
}
__global__ void lr_rows_stage_u_kernel(const float *__restrict__ R, int C, const LrOps o, const RowArgs *__restrict__ rows,
                                       float *__restrict__ U, size_t total) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over planes*H*lw
    if (e >= total) return;
    const int j = (int)(e % o.lw);
    const size_t row = e / o.lw;
    const size_t plane = row / o.H;
    if (row_strength(rows, (int)(plane / C)) == 0.f) return;
    U[e] = stage_u(R + plane * o.lh * o.lw, o, (int)(row - plane * o.H), j);
}
__global__ void lr_rows_stage_x_kernel(float *__restrict__ X, const float *__restrict__ U, int C, const LrOps o,
                                       const RowArgs *__restrict__ rows, size_t total) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over planes*H*W
    if (e >= total) return;
    const int x = (int)(e % o.W);
    const size_t row = e / o.W;
    const float lambda = row_strength(rows, (int)(row / o.H / C));
    if (lambda == 0.f) return;
    X[e] = stage_x(X[e], U + row * o.lw, o, x, lambda);
}

// the same stages as four launches over global scratch: T [planes][H][lw] | U [planes][H][lw] | R [planes][lh][lw]
__global__ void lr_stage_t_kernel(const float *__restrict__ X, const LrOps o, float *__restrict__ T, size_t total) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over planes*H*lw
    if (e >= total) return;
    const int j = (int)(e % o.lw);
    const size_t row = e / o.lw;                                        // plane*H + y
    T[e] = stage_t(X + row * o.W, o, j);
}
__global__ void lr_stage_r_kernel(const float *__restrict__ T, int C, const LrOps o, const LrArgs val, const LrArgs *dyn,
                                  float *__restrict__ R, size_t total) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over planes*lh*lw
    if (e >= total) return;
    const LrArgs a = dyn ? *dyn : val;
    const int nR = o.lh * o.lw;
    const int plane = (int)(e / nR), r = (int)(e - (size_t)plane * nR);
    const int i = r / o.lw, j = r - i * o.lw;
    R[e] = stage_r(T + (size_t)plane * o.H * o.lw, lr_plane(a, o, plane, C)[r], o, i, j);
}
__global__ void lr_stage_u_kernel(const float *__restrict__ R, const LrOps o, float *__restrict__ U, size_t total) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over planes*H*lw
    if (e >= total) return;
    const int j = (int)(e % o.lw);
    const size_t row = e / o.lw;
    const size_t plane = row / o.H;
    U[e] = stage_u(R + plane * o.lh * o.lw, o, (int)(row - plane * o.H), j);
}
__global__ void lr_stage_x_kernel(float *__restrict__ X, const float *__restrict__ U, const LrOps o, const LrArgs val,
                                  const LrArgs *dyn, size_t total) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // over planes*H*W
    if (e >= total) return;
    const float lambda = dyn ? dyn->strength : val.strength;
    const int x = (int)(e % o.W);
    const size_t row = e / o.W;
    X[e] = stage_x(X[e], U + row * o.lw, o, x, lambda);
}

// one block per image over its C residual planes R [C][lh][lw]: sum of squares in fp64, max |.|; wave64 shuffles, then
// one LDS slot per wave, added in wave order (bitwise reproducible)
__global__ void __launch_bounds__(256) lr_residual_reduce_kernel(const float *__restrict__ R, int per_image, double *sumsq,
                                                                 float *maxabs) {
    __shared__ double ws[4];
    __shared__ float wm[4];
    const float *r = R + (size_t)blockIdx.x * per_image;
    double s = 0.0;
    float m = 0.f;
    for (int e = threadIdx.x; e < per_image; e += blockDim.x) {
        const float v = r[e];
        s += (double)v * (double)v;
        m = fmaxf(m, fabsf(v));
    }
    for (int d = 32; d > 0; d >>= 1) {
        s += __shfl_down(s, d, 64);
        m = fmaxf(m, __shfl_down(m, d, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { ws[wave] = s; wm[wave] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sumsq[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
        maxabs[blockIdx.x] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    }
}

inline unsigned nblk(size_t n) { return (unsigned)((n + 255) / 256); }

} // namespace

size_t lr_lds_bytes(const LrOps &o) { return ((size_t)o.H * o.lw + (size_t)o.lh * o.lw) * sizeof(float); }
bool lr_lds_fits(const LrOps &o) { return lr_lds_bytes(o) <= LR_LDS_MAX_BYTES; }
size_t lr_scratch_floats(int planes, const LrOps &o) { return (size_t)planes * (2 * (size_t)o.H * o.lw + (size_t)o.lh * o.lw); }

void launch_lr_project(float *x, int planes, int C, const LrOps &o, const LrArgs &val, const LrArgs *dyn, bool lds_form,
                       float *scratch, hipStream_t s) {
    if (planes <= 0) return;
    if (lds_form) {
        const int threads = (size_t)o.H * o.W >= 4096 ? 1024 : 256;
        hipLaunchKernelGGL(lr_project_lds_kernel, dim3(planes), dim3(threads), lr_lds_bytes(o), s, x, C, o, val, dyn);
        return;
    }
    const size_t nT = (size_t)planes * o.H * o.lw, nR = (size_t)planes * o.lh * o.lw, nX = (size_t)planes * o.H * o.W;
    float *T = scratch, *U = scratch + nT, *R = scratch + 2 * nT;
    hipLaunchKernelGGL(lr_stage_t_kernel, dim3(nblk(nT)), dim3(256), 0, s, x, o, T, nT);
    hipLaunchKernelGGL(lr_stage_r_kernel, dim3(nblk(nR)), dim3(256), 0, s, T, C, o, val, dyn, R, nR);
    hipLaunchKernelGGL(lr_stage_u_kernel, dim3(nblk(nT)), dim3(256), 0, s, R, o, U, nT);
    hipLaunchKernelGGL(lr_stage_x_kernel, dim3(nblk(nX)), dim3(256), 0, s, x, U, o, val, dyn, nX);
}

void launch_lr_project_rows(float *x, int B, int C, const LrOps &o, const float *lr_rows, const RowArgs *rows, bool lds_form,
                            float *scratch, hipStream_t s) {
    const int planes = B * C;
    if (planes <= 0) return;
    if (lds_form) {
        const int threads = (size_t)o.H * o.W >= 4096 ? 1024 : 256;
        hipLaunchKernelGGL(lr_project_lds_rows_kernel, dim3(planes), dim3(threads), lr_lds_bytes(o), s, x, C, o, lr_rows, rows);
        return;
    }
    const size_t nT = (size_t)planes * o.H * o.lw, nR = (size_t)planes * o.lh * o.lw, nX = (size_t)planes * o.H * o.W;
    float *T = scratch, *U = scratch + nT, *R = scratch + 2 * nT;
    hipLaunchKernelGGL(lr_rows_stage_t_kernel, dim3(nblk(nT)), dim3(256), 0, s, x, C, o, rows, T, nT);
    hipLaunchKernelGGL(lr_rows_stage_r_kernel, dim3(nblk(nR)), dim3(256), 0, s, T, C, o, lr_rows, rows, R, nR);
    hipLaunchKernelGGL(lr_rows_stage_u_kernel, dim3(nblk(nT)), dim3(256), 0, s, R, C, o, rows, U, nT);
    hipLaunchKernelGGL(lr_rows_stage_x_kernel, dim3(nblk(nX)), dim3(256), 0, s, x, U, C, o, rows, nX);
}

void launch_lr_residual(const float *img, int B, int C, const LrOps &o, const LrArgs &val, float *scratch, double *sumsq,
                        float *maxabs, hipStream_t s) {
    if (B <= 0) return;
    const int planes = B * C;
    const size_t nT = (size_t)planes * o.H * o.lw, nR = (size_t)planes * o.lh * o.lw;
    float *T = scratch, *R = scratch + 2 * nT;
    hipLaunchKernelGGL(lr_stage_t_kernel, dim3(nblk(nT)), dim3(256), 0, s, img, o, T, nT);
    hipLaunchKernelGGL(lr_stage_r_kernel, dim3(nblk(nR)), dim3(256), 0, s, T, C, o, val, (const LrArgs *)nullptr, R, nR);
    hipLaunchKernelGGL(lr_residual_reduce_kernel, dim3(B), dim3(256), 0, s, R, C * o.lh * o.lw, sumsq, maxabs);
}

// ---- the DDPM update in two halves around the projection --------------------------------------------------------------
namespace {

// x0 = clamp(a*x - b*eps, -1, 1), the head of ddpm_update_kernel in its operation order, into x0hat NCHW [B][C][H][W].
// CLAMP false: the prediction as it is, for the dynamic threshold that takes the clamp's place (kernels_threshold.hip)
template <bool CLAMP>
__global__ void x0_predict_kernel(const UpdateParams u, float *__restrict__ x0hat, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over B*C*HW, NCHW order
    if (i >= total) return;
    const StepArgs sa = *u.args;
    const int HW = u.state.H * u.state.W;
    const int pp = (int)(i % HW);
    const size_t nc = i / HW;
    const int n = (int)(nc / u.C);
    const int c = (int)(nc - (size_t)n * u.C);
    const int y = pp / u.state.W, xx = pp - y * u.state.W;
    const float x = u.state.p[u.state.pix(n, y, xx) * u.state.C + u.xoff + c];
    const float e = u.eps.p[u.eps.pix(n, y, xx) * u.eps.C + c];
    const float x0 = __fsub_rn(__fmul_rn(sa.a, x), __fmul_rn(sa.b, e));
    x0hat[i] = CLAMP ? fminf(fmaxf(x0, -1.0f), 1.0f) : x0;
}

// the tail of ddpm_update_kernel, statement for statement, with x0 read from x0hat (the projected prediction: nothing
// is clamped again, and the history of the multistep samplers keeps the projected value)
__global__ void update_from_x0_kernel(const UpdateParams u, const float *__restrict__ x0hat, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // over B*C*HW, NCHW order
    if (i >= total) return;
    const StepArgs sa = *u.args;
    const int HW = u.state.H * u.state.W;
    const int pp = (int)(i % HW);
    const size_t nc = i / HW;
    const int n = (int)(nc / u.C);
    const int c = (int)(nc - (size_t)n * u.C);
    const int y = pp / u.state.W, xx = pp - y * u.state.W;
    const size_t pix = u.state.pix(n, y, xx);
    const size_t si = pix * u.state.C + u.xoff + c;
    const float x = u.state.p[si];
    const float x0 = x0hat[i];
    float v = __fadd_rn(__fmul_rn(sa.c1, x0), __fmul_rn(sa.c2, x));
    if (sa.hist) {
        if (sa.hist == 2) v = __fadd_rn(v, __fmul_rn(sa.c3, u.hist[i]));
        u.hist[i] = x0;
    }
    if (sa.sigma != 0.f) {
        const float z = sa.noise ? sa.noise[i]
                                 : philox_normal(sa.seed, sa.image_offset + n, sa.draw, (uint32_t)(c * HW + pp));
        v = __fadd_rn(v, __fmul_rn(z, sa.sigma));
    }
    u.state.p[si] = v;
    if (u.packed != nullptr) {
        _Float16 *pk = reinterpret_cast<_Float16 *>(u.packed) + pix * 16 + u.xoff + c;
        const _Float16 hi = (_Float16)v;
        pk[0] = hi;
        pk[8] = (_Float16)(v - (float)hi);
        if (u.ovf != nullptr && ((unsigned)__builtin_bit_cast(unsigned short, hi) & 0x7C00u) == 0x7C00u) *u.ovf = 1;
    }
    if (sa.frame) sa.frame[i] = v;
}

} // namespace

void launch_x0_predict(const UpdateParams &p, float *x0hat, int B, hipStream_t s, bool clamp) {
    const size_t total = (size_t)B * p.C * p.state.H * p.state.W;
    if (clamp) hipLaunchKernelGGL(x0_predict_kernel<true>, dim3(nblk(total)), dim3(256), 0, s, p, x0hat, total);
    else hipLaunchKernelGGL(x0_predict_kernel<false>, dim3(nblk(total)), dim3(256), 0, s, p, x0hat, total);
}
void launch_update_from_x0(const UpdateParams &p, const float *x0hat, int B, hipStream_t s) {
    const size_t total = (size_t)B * p.C * p.state.H * p.state.W;
    hipLaunchKernelGGL(update_from_x0_kernel, dim3(nblk(total)), dim3(256), 0, s, p, x0hat, total);
}

} // namespace sr3
