// Validation metrics on the device: the PSNR / SSIM scoring the reference runs on the host one
// image at a time after every validation chain (lib/trainer_temp.py:441-446 -> core/metrics.py), for a whole batch of
// sampler outputs that never leave HBM. Latency-bound byte work like kernels_post.hip; no MFMA.
//   quantisation  Metrics.tensor2img (core/metrics.py:16-42) for both images: to_u8 (sr3_internal.h)
//   PSNR          calculate_psnr (core/metrics.py:74-81): the kernel returns the exact integer sum of squared uint8
//                 differences per row; the host applies 20*log10(255/sqrt(sum/n)) (validation.scores_from_sums)
//   SSIM          ssim / calculate_ssim (core/metrics.py:84-125): 11x11 Gaussian (sigma 1.5), 'valid' region, fp64,
//                 mean of the map per channel, mean of the three channels
// Arithmetic follows validation.py:28-46 operation by operation (separable filter, horizontal pass first, taps in
// ascending order, no fused multiply-add), so the SSIM map itself matches the host's; only the order of the final
// mean differs. No floating-point atomics: the per-block partial sums are added in a fixed order, so two calls return
// bitwise equal scores.
#include "sr3_internal.h"

// the host formula rounds every product and every sum (numpy): keep the compiler from contracting them into fma
#pragma clang fp contract(off)

namespace sr3 {

namespace {
constexpr int WIN = 11;                    // window side
constexpr int TILE = 32;                   // output tile side
constexpr int HALO = TILE + WIN - 1;       // 42: input tile side
constexpr int LROW = 44;                   // LDS row stride in bytes (whole 4-pixel groups)
constexpr int THREADS = 256;
constexpr int PER_THREAD = TILE * TILE / THREADS;   // 4 output pixels per thread

struct Taps { double k[WIN]; };

__device__ __forceinline__ unsigned pack_u8x4(float4 v) {
    return (unsigned)to_u8(v.x) | ((unsigned)to_u8(v.y) << 8) | ((unsigned)to_u8(v.z) << 16) | ((unsigned)to_u8(v.w) << 24);
}

// One block per (row b, channel c, 32x32 output tile). It stages the 42x42 input tile of both quantised images in LDS,
// adds the squared differences of the pixels it OWNS (every pixel of the image has exactly one owner: the tile whose
// 32x32 square holds it, the last tile of a row / column of tiles also owning the 10-pixel rim behind its square) into
// ssd[b], filters the five planes a, b, a*a, a*b, b*b one after the other (horizontal pass into LDS, vertical pass into
// registers), forms the SSIM map and writes the sum of its valid entries to part[block].
// VEC: W % 4 == 0 and both tensors 16-byte aligned -> the tile is fetched as float4.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void ssim_tile_kernel(const float *__restrict__ sr, const float *__restrict__ hr,
                                                            int N, int row_offset, int H, int W, int tilesX, int tilesY,
                                                            Taps taps, double C1, double C2,
                                                            unsigned long long *__restrict__ ssd, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) uint8_t sa[HALO * LROW];
    __shared__ __attribute__((aligned(16))) uint8_t sb[HALO * LROW];
    __shared__ double sh[HALO * TILE];
    __shared__ double red_d[THREADS / 64];
    __shared__ unsigned red_u[THREADS / 64];

    const int tid = threadIdx.x;
    const int tiles = tilesX * tilesY;
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const unsigned bc = blockIdx.x / (unsigned)tiles;
    const int c = (int)(bc % 3u), b = (int)(bc / 3u);
    const int ty = tile / tilesX, tx = tile - ty * tilesX;
    const int y0 = ty * TILE, x0 = tx * TILE;
    const bool lastY = ty == tilesY - 1, lastX = tx == tilesX - 1;
    const int n = (int)(((long long)row_offset + b) % N);
    const size_t HW = (size_t)H * W;
    const float *pa = sr + ((size_t)b * 3 + c) * HW;
    const float *pb = hr + ((size_t)n * 3 + c) * HW;

    // ---- stage + squared differences of the owned pixels (<= 42*42*255^2 per block: fits 32 bits) ----
    unsigned sq = 0;
    if (VEC) {
        for (int i = tid; i < HALO * (LROW / 4); i += THREADS) {
            const int ly = i / (LROW / 4), lx = (i - ly * (LROW / 4)) * 4;
            const int y = y0 + ly, x = x0 + lx;
            unsigned wa = 0, wb = 0;
            if (y < H && x < W) {                          // W % 4 == 0: the group is inside or outside as a whole
                wa = pack_u8x4(*reinterpret_cast<const float4 *>(pa + (size_t)y * W + x));
                wb = pack_u8x4(*reinterpret_cast<const float4 *>(pb + (size_t)y * W + x));
                if (ly < TILE || lastY) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int d = (int)((wa >> (8 * e)) & 255u) - (int)((wb >> (8 * e)) & 255u);
                        if (lx + e < TILE || lastX) sq += (unsigned)(d * d);
                    }
                }
            }
            *reinterpret_cast<unsigned *>(sa + ly * LROW + lx) = wa;
            *reinterpret_cast<unsigned *>(sb + ly * LROW + lx) = wb;
        }
    } else {
        for (int i = tid; i < HALO * LROW; i += THREADS) {
            const int ly = i / LROW, lx = i - ly * LROW;
            const int y = y0 + ly, x = x0 + lx;
            uint8_t va = 0, vb = 0;
            if (y < H && x < W) {
                va = to_u8(pa[(size_t)y * W + x]);
                vb = to_u8(pb[(size_t)y * W + x]);
                const int d = (int)va - (int)vb;
                if ((ly < TILE || lastY) && (lx < TILE || lastX)) sq += (unsigned)(d * d);
            }
            sa[i] = va;
            sb[i] = vb;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_down(sq, o, 64);
    if ((tid & 63) == 0) red_u[tid >> 6] = sq;

    // ---- the five filtered planes of this thread's output pixels (ox, oy0 + 8 i) ----
    const int ox = tid & (TILE - 1), oy0 = tid >> 5;
    double f[5][PER_THREAD];
#pragma unroll
    for (int p = 0; p < 5; ++p) {
        __syncthreads();                                   // tile staged / previous plane's vertical pass done
#pragma unroll 1
        for (int i = tid; i < HALO * TILE; i += THREADS) {
            const int r = i >> 5, col = i & (TILE - 1);
            const uint8_t *ra = sa + r * LROW + col, *rb = sb + r * LROW + col;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < WIN; ++j) {
                const int a = ra[j], bq = rb[j];
                const int v = p == 0 ? a : p == 1 ? bq : p == 2 ? a * a : p == 3 ? a * bq : bq * bq;
                s = s + taps.k[j] * (double)v;
            }
            sh[i] = s;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) {
            const double *col = sh + (oy0 + 8 * i) * TILE + ox;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < WIN; ++j) s = s + taps.k[j] * col[j * TILE];
            // finish the sum here (empty asm: the value must exist at this point): left alone, the compiler sinks the
            // arithmetic to the SSIM map below and keeps every plane's 35 loaded rows alive until then (256 VGPRs +
            // 48 AGPRs, one block per CU)
            asm volatile("" : "+v"(s));
            f[p][i] = s;
        }
    }

    // ---- SSIM map (core/metrics.py:95-104) and its sum over the valid entries of the tile ----
    const int Ho = H - (WIN - 1), Wo = W - (WIN - 1);
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < PER_THREAD; ++i) {
        const double mu1 = f[0][i], mu2 = f[1][i];
        const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const double s1 = f[2][i] - mu1_sq, s2 = f[4][i] - mu2_sq, s12 = f[3][i] - mu1_mu2;
        const double m = ((2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
        if (y0 + oy0 + 8 * i < Ho && x0 + ox < Wo) sum = sum + m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum = sum + __shfl_down(sum, o, 64);
    if ((tid & 63) == 0) red_d[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        part[blockIdx.x] = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];
        atomicAdd(ssd + b, (unsigned long long)red_u[0] + red_u[1] + red_u[2] + red_u[3]);   // integer: order-free
    }
}

// part [B][3][tiles] -> ssim [B]: mean of the map per channel (tiles added in tile order), then the mean of the channels
__global__ void ssim_finalize_kernel(const double *__restrict__ part, int B, int tiles, double count, double *__restrict__ ssim) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double acc = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double *p = part + ((size_t)b * 3 + c) * tiles;
        double s = 0.0;
        for (int t = 0; t < tiles; ++t) s = s + p[t];
        acc = acc + s / count;
    }
    ssim[b] = acc / 3.0;
}

inline int tiles_of(int n) { return (n - (WIN - 1) + TILE - 1) / TILE; }
} // namespace

long long metrics_blocks(int B, int H, int W) { return (long long)B * 3 * tiles_of(H) * tiles_of(W); }

void launch_metrics(const float *sr, const float *hr, int B, int N, int row_offset, int H, int W, const double *taps,
                    double *ws, int64_t *ssd, double *ssim, hipStream_t s) {
    const int tilesY = tiles_of(H), tilesX = tiles_of(W);
    Taps k;
    for (int j = 0; j < WIN; ++j) k.k[j] = taps[j];
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);      // core/metrics.py:85-86
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(ssd);
    const dim3 grid((unsigned)metrics_blocks(B, H, W)), block(THREADS);
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(sr) | reinterpret_cast<uintptr_t>(hr)) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(ssim_tile_kernel<true>, grid, block, 0, s, sr, hr, N, row_offset, H, W, tilesX, tilesY, k, C1, C2, acc, ws);
    else
        hipLaunchKernelGGL(ssim_tile_kernel<false>, grid, block, 0, s, sr, hr, N, row_offset, H, W, tilesX, tilesY, k, C1, C2, acc, ws);
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, s, ws, B, tilesX * tilesY,
                       (double)(H - (WIN - 1)) * (double)(W - (WIN - 1)), ssim);
}

} // namespace sr3
