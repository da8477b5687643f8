// The SR3 denoising loss on the device (GaussianDiffusion.p_losses): what the reference wraps around one
// UNet forward when it evaluates its training objective (model/sr/sr3_modules/diffusion.py),
//   q_sample   :275-282  x_noisy = a * x_start + sqrt(1 - a^2) * noise, a = one continuous noise level per image
//   cat        :305-306  torch.cat([x_in['SR'], x_noisy], dim=1), then the layout change and the split-f16 packing
//   loss       :85-91, 312  L1Loss / MSELoss(reduction='sum') of the noise against the UNet's prediction
// as two memory-bound passes, one on each side of the forward. q_sample_state_kernel reads the images once and leaves the
// UNet's input state (and its packed split-f16 twin) as launch_nchw_to_nhwc + launch_pack_state would; the loss kernels
// read eps once, regenerate the Philox noise instead of storing it, and can emit eps as NCHW in the same pass.
// No matrix work; latency / bandwidth bound like kernels_metrics.hip, whose reduction pattern this follows: one fp64
// partial per block, added in block order by a second kernel (no floating-point atomics: two calls are bitwise equal).
#include "sr3_internal.h"

// torch rounds every product and every sum of q_sample and of the loss' difference / square. The arithmetic below is
// written with plain operators under this pragma: the __fmul_rn / __fadd_rn wrappers are inline functions of a header
// compiled with contraction allowed, and a product and a sum inlined from there can still meet in one v_fma_f32.
#pragma clang fp contract(off)

namespace sr3 {

namespace {
constexpr int THREADS = 256;
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

struct QSampleParams {
    const float *hr, *cond;     // NCHW [N][C][HW], [N][nc][HW] (null: nc == 0)
    const float *a, *s;         // [B]
    NoiseRef nz;
    TDesc state;                // p == nullptr: no state written (sr3_op_q_sample)
    _Float16 *packed;           // 16 halfs per padded pixel (8 hi | 8 lo) or null
    int *ovf;
    float *xn_out;              // NCHW [B][C][HW] or null
    int N, row_offset, C, nc, HW, W, bpi;
};

// G consecutive values of one NCHW plane. G == 4: HW % 4 == 0 and the tensor starts on 16 bytes (the launcher checks)
template <int G>
__device__ __forceinline__ void load_run(const float *p, float v[G]) {
    if constexpr (G == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int G>
__device__ __forceinline__ void store_run(float *p, const float v[G]) {
    if constexpr (G == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
// noise values [elem, elem + G) of row j (elem = c * HW + pixel; G == 4: elem % 4 == 0, one Philox counter)
template <int G>
__device__ __forceinline__ void noise_run(const NoiseRef &nz, size_t j, int C, int HW, int c, int pp, float v[G]) {
    if (nz.noise) {
        load_run<G>(nz.noise + (j * C + c) * (size_t)HW + pp, v);
    } else if constexpr (G == 4) {
        philox_normal4(nz.seed, nz.image_offset + j, 0u, (uint32_t)(c * HW + pp) >> 2, v);
    } else {
        v[0] = philox_normal(nz.seed, nz.image_offset + j, 0u, (uint32_t)(c * HW + pp));
    }
}

// One thread per run of G pixels of one batch row (flat pixel index: a run may cross the end of an image row). The 8
// leading channels of the state are built in registers — cond, x_noisy, zeros — so that the fp32 state takes whole
// 16-byte stores and the packed twin is made from the same registers (pack_state_kernel reads the state back instead).
// The zeros stored behind in_channel equal what the workspace holds there (its pad channels are zero from creation).
template <int G>
__global__ __launch_bounds__(THREADS) void q_sample_state_kernel(const QSampleParams p) {
    const int b = (int)(blockIdx.x / (unsigned)p.bpi);
    const int g = (int)(blockIdx.x % (unsigned)p.bpi) * THREADS + threadIdx.x;
    const int pp0 = g * G;
    if (pp0 >= p.HW) return;
    const size_t n = (size_t)(((long long)p.row_offset + b) % p.N);
    const size_t j = p.nz.per_source ? n : (size_t)b;
    const float av = p.a[b], sv = p.s[b];
    float v[8][G];
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
#pragma unroll
        for (int e = 0; e < G; ++e) v[ch][e] = 0.f;
        if (ch < p.nc) {
            load_run<G>(p.cond + (n * p.nc + ch) * (size_t)p.HW + pp0, v[ch]);
        } else if (ch < p.nc + p.C) {
            const int c = ch - p.nc;
            float x[G], z[G];
            load_run<G>(p.hr + (n * p.C + c) * (size_t)p.HW + pp0, x);
            noise_run<G>(p.nz, j, p.C, p.HW, c, pp0, z);
#pragma unroll
            for (int e = 0; e < G; ++e) v[ch][e] = av * x[e] + sv * z[e];
            if (p.xn_out) store_run<G>(p.xn_out + ((size_t)b * p.C + c) * p.HW + pp0, v[ch]);
        }
    }
    if (p.state.p == nullptr) return;
    bool over = false;
#pragma unroll
    for (int e = 0; e < G; ++e) {
        const int pp = pp0 + e, y = pp / p.W, x = pp - y * p.W;
        const size_t pix = p.state.pix(b, y, x);
        float *d = p.state.p + pix * p.state.C;
        *reinterpret_cast<float4 *>(d) = make_float4(v[0][e], v[1][e], v[2][e], v[3][e]);
        if (p.nc + p.C > 4) *reinterpret_cast<float4 *>(d + 4) = make_float4(v[4][e], v[5][e], v[6][e], v[7][e]);
        if (p.packed != nullptr) {
            h16x8 hi, lo;
            float absmax = 0.f;
#pragma unroll
            for (int ch = 0; ch < 8; ++ch) {
                absmax = fmaxf(absmax, fabsf(v[ch][e]));
                hi[ch] = (_Float16)v[ch][e];
                lo[ch] = (_Float16)(v[ch][e] - (float)hi[ch]);
            }
            *reinterpret_cast<h16x8 *>(p.packed + pix * 16) = hi;
            *reinterpret_cast<h16x8 *>(p.packed + pix * 16 + 8) = lo;
            over = over || absmax > SPLIT_F16_MAX;
        }
    }
    if (p.ovf != nullptr && over) *p.ovf = 1;
}

struct LossParams {
    const float *eps;           // unpadded NHWC [B][HW][C]
    NoiseRef nz;
    double *part;               // [B][bpi]
    float *eps_out;             // NCHW [B][C][HW] or null
    int N, row_offset, C, HW, bpi, l2;
};

// One thread per run of G pixels; G == 4 takes C == 3 (the 12 floats of the run are three 16-byte loads of eps).
template <int G>
__global__ __launch_bounds__(THREADS) void loss_partial_kernel(const LossParams p) {
    __shared__ double red[THREADS / 64];
    const int C = G == 4 ? 3 : p.C;
    const int b = (int)(blockIdx.x / (unsigned)p.bpi);
    const int g = (int)(blockIdx.x % (unsigned)p.bpi) * THREADS + threadIdx.x;
    const int pp0 = g * G;
    double sum = 0.0;
    if (pp0 < p.HW) {
        const size_t n = (size_t)(((long long)p.row_offset + b) % p.N);
        const size_t j = p.nz.per_source ? n : (size_t)b;
        const float *src = p.eps + ((size_t)b * p.HW + pp0) * C;
        float t[G == 4 ? 12 : 1];
        if constexpr (G == 4) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4 q = reinterpret_cast<const float4 *>(src)[k];
                t[4 * k] = q.x; t[4 * k + 1] = q.y; t[4 * k + 2] = q.z; t[4 * k + 3] = q.w;
            }
        }
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            float z[G], e[G];
            noise_run<G>(p.nz, j, C, p.HW, c, pp0, z);
            if constexpr (G == 4) {
                // (c is a loop variable: select instead of indexing the register array)
#pragma unroll
                for (int i = 0; i < G; ++i) e[i] = c == 0 ? t[3 * i] : c == 1 ? t[3 * i + 1] : t[3 * i + 2];
            } else {
                e[0] = src[c];
            }
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const float d = z[i] - e[i];
                sum = sum + (double)(p.l2 ? d * d : fabsf(d));
            }
            if (p.eps_out) store_run<G>(p.eps_out + ((size_t)b * C + c) * p.HW + pp0, e);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum = sum + __shfl_down(sum, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) p.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// part [B][bpi] -> per_image [B]: the partials of an image in block order
__global__ void loss_final_kernel(const double *__restrict__ part, int B, int bpi, double *__restrict__ per_image) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int k = 0; k < bpi; ++k) s = s + part[(size_t)b * bpi + k];
    per_image[b] = s;
}

// a[b] = av, s[b] = sv: the per-row coefficients of a q_sample whose rows share one level (the sampler's warm start)
__global__ void fill_pair_kernel(float *__restrict__ a, float *__restrict__ s, float av, float sv, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    a[b] = av;
    s[b] = sv;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int blocks_of(int HW, int G) { return ((HW + G - 1) / G + THREADS - 1) / THREADS; }
} // namespace

void launch_q_sample_state(const float *hr, const float *cond, int N, int row_offset, const float *a, const float *s,
                           const NoiseRef &nz, int B, int C, int nc, const TDesc &state, float *packed, int *ovf,
                           float *x_noisy_out, hipStream_t st) {
    QSampleParams p;
    p.hr = hr; p.cond = cond; p.a = a; p.s = s; p.nz = nz; p.state = state;
    p.packed = reinterpret_cast<_Float16 *>(packed); p.ovf = ovf; p.xn_out = x_noisy_out;
    p.N = N; p.row_offset = row_offset; p.C = C; p.nc = cond ? nc : 0;
    p.W = state.W; p.HW = state.H * state.W;
    const bool vec = p.HW % 4 == 0 && aligned16(hr) && aligned16(cond) && aligned16(nz.noise) && aligned16(x_noisy_out);
    p.bpi = blocks_of(p.HW, vec ? 4 : 1);
    const dim3 grid((unsigned)((size_t)B * p.bpi)), block(THREADS);
    if (vec) hipLaunchKernelGGL(q_sample_state_kernel<4>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(q_sample_state_kernel<1>, grid, block, 0, st, p);
}

void launch_fill_pair(float *a, float *s, float av, float sv, int B, hipStream_t st) {
    if (B <= 0) return;
    hipLaunchKernelGGL(fill_pair_kernel, dim3((B + 63) / 64), dim3(64), 0, st, a, s, av, sv, B);
}

int loss_blocks(int H, int W) { return blocks_of(H * W, 1); }     // the scalar form: the most blocks

void launch_denoise_loss(const TDesc &eps, const NoiseRef &nz, int N, int row_offset, int B, int C, int loss_type, double *ws,
                         double *per_image, float *eps_out, hipStream_t st) {
    LossParams p;
    p.eps = eps.p; p.nz = nz; p.part = ws; p.eps_out = eps_out;
    p.N = N; p.row_offset = row_offset; p.C = C; p.HW = eps.H * eps.W; p.l2 = loss_type;
    const bool vec = C == 3 && p.HW % 4 == 0 && aligned16(eps.p) && aligned16(nz.noise) && aligned16(eps_out);
    p.bpi = blocks_of(p.HW, vec ? 4 : 1);
    const dim3 grid((unsigned)((size_t)B * p.bpi)), block(THREADS);
    if (vec) hipLaunchKernelGGL(loss_partial_kernel<4>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(loss_partial_kernel<1>, grid, block, 0, st, p);
    hipLaunchKernelGGL(loss_final_kernel, dim3((B + 63) / 64), dim3(64), 0, st, ws, B, p.bpi, per_image);
}

} // namespace sr3
