// Weight layouts built on the device from fp32 tensors in the reference layout (Conv2d OIHW, Linear [out,in]) — the
// device twin of the host helpers pack_conv_weight, make_up2_phase_weights, make_up2_wino_weights, make_wino_weights and split_conv_weight_k,
// byte for byte: the same operations in the same order in the same precision (the Winograd and phase sums in fp64,
// rounded once). Everything here is a permutation or an elementwise pass, so the only concerns are that every tensor is
// read once, that every layout is written once, and that the 64 lanes of a wave touch consecutive addresses:
//   weight_pack_kernel    one thread per (o, i), consecutive lanes on consecutive i. A lane reads its KS*KS contiguous taps
//                         (a wave: one contiguous 64 * 36-byte run of the source) and writes one float into each plane of
//                         every k-independent layout — packed, phase or Winograd planes, 256 contiguous bytes per wave and
//                         plane — and the block's max|w| into the parameter's slot of the context's table (one atomic
//                         per block; |w| as its bit pattern, which orders like the value for non-negative floats).
//   weight_split_kernel   one thread per 4 channels of a 32-channel chunk: 16-B load, two 8-B stores.
// The split needs the exponent k of the WHOLE tensor (and of its fused partner), so it is a second pass over the packed
// copy, launched once the host has read the maxima.
#include "sr3_internal.h"

namespace sr3 {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// max over the block of a non-negative value -> atomicMax into *slot
__device__ __forceinline__ void block_absmax(float m, unsigned *slot) {
    __shared__ float red[4];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (m > 0.f) atomicMax(slot, __float_as_uint(m));
    }
}

// UP: the 16 phase planes of an Upsample conv instead of the 9 tap planes. wino: G g G^T planes or null.
template <int KS, bool UP>
__global__ __launch_bounds__(256) void weight_pack_kernel(const float *__restrict__ oihw, int Cout, int Cin, int CinPad,
                                                          float *__restrict__ packed, float *__restrict__ wino,
                                                          unsigned *__restrict__ wmax, float *__restrict__ up_wino) {
#pragma clang fp contract(off)
    constexpr int TAPS = KS * KS;
    const size_t plane = (size_t)Cout * CinPad;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    float m = 0.f;
    if (t < plane) {
        const size_t o = t / (size_t)CinPad;
        const int i = (int)(t - o * CinPad);
        float w[TAPS];
        if (i < Cin) {
            const float *src = oihw + (o * Cin + i) * TAPS;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) w[k] = src[k];
        } else {
#pragma unroll
            for (int k = 0; k < TAPS; ++k) w[k] = 0.f;
        }
        if constexpr (UP) {
            // make_up2_phase_weights: taps in dy, dx order, summed in fp64 from 0.0
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int px = 0; px < 2; ++px)
#pragma unroll
                    for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
                        for (int c2 = 0; c2 < 2; ++c2) {
                            double acc = 0.0;
#pragma unroll
                            for (int dy = 0; dy < 3; ++dy) {
                                if (((py + dy + 1) >> 1) != py + r2) continue;
#pragma unroll
                                for (int dx = 0; dx < 3; ++dx)
                                    if (((px + dx + 1) >> 1) == px + c2) acc += (double)w[dy * 3 + dx];
                            }
                            const float v = (float)acc;
                            packed[(size_t)((py * 2 + px) * 4 + r2 * 2 + c2) * plane + t] = v;
                            m = fmaxf(m, fabsf(v));
                        }
            if (up_wino) {
                // make_up2_wino_weights: position (i, j) of phase (py, px) adds the taps lo <= d <= hi of both axes, in
                // (dy, dx) order, in fp64 from 0.0; fragment-major [phase][position][CinPad/8][Cout][8]
                const int lo[2][3] = {{0, 0, 1}, {0, 0, 2}}, hi[2][3] = {{0, 2, 2}, {1, 2, 2}};
                const size_t at = ((size_t)(i >> 3) * Cout + o) * 8 + (i & 7);
#pragma unroll
                for (int py = 0; py < 2; ++py)
#pragma unroll
                    for (int px = 0; px < 2; ++px)
#pragma unroll
                        for (int a = 0; a < 3; ++a)
#pragma unroll
                            for (int b = 0; b < 3; ++b) {
                                double acc = 0.0;
#pragma unroll
                                for (int dy = 0; dy < 3; ++dy) {
                                    if (dy < lo[py][a] || dy > hi[py][a]) continue;
#pragma unroll
                                    for (int dx = 0; dx < 3; ++dx)
                                        if (dx >= lo[px][b] && dx <= hi[px][b]) acc += (double)w[dy * 3 + dx];
                                }
                                up_wino[(size_t)((py * 2 + px) * 9 + a * 3 + b) * plane + at] = (float)acc;
                            }
            }
        } else {
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                packed[(size_t)k * plane + t] = w[k];
                m = fmaxf(m, fabsf(w[k]));          // (fmaxf drops a NaN operand, as on the host)
            }
            if constexpr (KS == 3) {
                if (wino) {
                    // make_wino_weights: every term is kept, also those whose coefficient is 0 (0 * w carries w's sign
                    // into the sum of zeros)
                    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
                    double g[3][3];
#pragma unroll
                    for (int k = 0; k < 9; ++k) g[k / 3][k % 3] = (double)w[k];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        double gg[3];
#pragma unroll
                        for (int x = 0; x < 3; ++x) gg[x] = G[a][0] * g[0][x] + G[a][1] * g[1][x] + G[a][2] * g[2][x];
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            wino[(size_t)(a * 4 + b) * plane + t] = (float)(gg[0] * G[b][0] + gg[1] * G[b][1] + gg[2] * G[b][2]);
                    }
                }
            }
        }
    }
    block_absmax(m, wmax);
}

// max|w| of a tensor that already is in its packed form (the partner of a refreshed tensor in a fused launch)
__global__ __launch_bounds__(256) void weight_absmax_kernel(const float *__restrict__ w, size_t n4, unsigned *__restrict__ wmax) {
    float m = 0.f;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n4; t += (size_t)gridDim.x * 256) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(w)[t];
        m = fmaxf(fmaxf(m, fabsf(v[0])), fmaxf(fabsf(v[1]), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
    block_absmax(m, wmax);
}

// split_conv_weight_k: per 32-channel chunk 32 hi halfs | 32 lo halfs of w * 2^k
__global__ __launch_bounds__(256) void weight_split_kernel(const float *__restrict__ packed, size_t chunks, float sc,
                                                           float *__restrict__ dst) {
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= chunks * 8) return;
    const size_t ch = t >> 3;
    const int j = (int)(t & 7) * 4;
    const f32x4 w = *reinterpret_cast<const f32x4 *>(packed + ch * 32 + j);
    alignas(8) _Float16 hi[4], lo[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float v = w[u] * sc;
        hi[u] = (_Float16)v;
        lo[u] = (_Float16)(v - (float)hi[u]);
    }
    _Float16 *o = reinterpret_cast<_Float16 *>(dst + ch * 32);
    *reinterpret_cast<uint2 *>(o + j) = *reinterpret_cast<const uint2 *>(hi);
    *reinterpret_cast<uint2 *>(o + 32 + j) = *reinterpret_cast<const uint2 *>(lo);
}

__global__ __launch_bounds__(256) void weight_bias_sum_kernel(const float *__restrict__ a, const float *__restrict__ b, int n,
                                                              float *__restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = a[i] + b[i];
}

// ResBlock::ident_w: split-f16 [C][C], row o holds `half_bits` at hi position o of its chunk, zero elsewhere. One thread
// per float (= two halfs) of the matrix.
__global__ __launch_bounds__(256) void weight_ident_kernel(int C, unsigned half_bits, unsigned *__restrict__ dst) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= C * C) return;
    const int o = e / C;
    const int at = (o & ~31) + ((o & 31) >> 1);       // float column that holds half (o & ~31) * 2 + (o & 31) of row o
    dst[e] = (e - o * C == at) ? half_bits << (16 * (o & 1)) : 0u;
}

} // namespace

void launch_weight_pack(const float *oihw, int Cout, int Cin, int ks, int CinPad, bool up_phase, float *packed, float *wino,
                        unsigned *wmax, hipStream_t s, float *up_wino) {
    const size_t plane = (size_t)Cout * CinPad;
    const dim3 grid((unsigned)((plane + 255) / 256)), block(256);
    if (ks == 1) hipLaunchKernelGGL((weight_pack_kernel<1, false>), grid, block, 0, s, oihw, Cout, Cin, CinPad, packed, wino, wmax, up_wino);
    else if (up_phase) hipLaunchKernelGGL((weight_pack_kernel<3, true>), grid, block, 0, s, oihw, Cout, Cin, CinPad, packed, wino, wmax, up_wino);
    else hipLaunchKernelGGL((weight_pack_kernel<3, false>), grid, block, 0, s, oihw, Cout, Cin, CinPad, packed, wino, wmax, up_wino);
}

void launch_weight_absmax(const float *packed, size_t n, unsigned *wmax, hipStream_t s) {
    const size_t n4 = n / 4;                           // (packed tensors are multiples of 32 floats)
    const size_t blocks = (n4 + 255) / 256;
    hipLaunchKernelGGL(weight_absmax_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, packed, n4, wmax);
}

void launch_weight_split(const float *packed, size_t floats, int k, float *dst, hipStream_t s) {
    const size_t chunks = floats / 32;
    hipLaunchKernelGGL(weight_split_kernel, dim3((unsigned)((chunks * 8 + 255) / 256)), dim3(256), 0, s, packed, chunks,
                       ldexpf(1.0f, k), dst);
}

void launch_weight_bias_sum(const float *a, const float *b, int n, float *dst, hipStream_t s) {
    hipLaunchKernelGGL(weight_bias_sum_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, b, n, dst);
}

void launch_weight_ident(int C, float v, float *dst, hipStream_t s) {
    const _Float16 h = (_Float16)v;
    unsigned short bits;
    __builtin_memcpy(&bits, &h, 2);
    hipLaunchKernelGGL(weight_ident_kernel, dim3((C * C + 255) / 256), dim3(256), 0, s, C, (unsigned)bits,
                       reinterpret_cast<unsigned *>(dst));
}

} // namespace sr3
