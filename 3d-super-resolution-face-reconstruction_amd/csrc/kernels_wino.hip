// Winograd F(2x2, 3x3) for the exact-f32 3x3 / stride-1 convs of the deep UNet levels (prec 0).
//
//   Y = A^T [ (G g G^T) . (B^T d B) ] A          per 2x2 output tile, 4x4 input window d
//
//   B^T = | 1  0 -1  0 |     G = | 1    0    0  |     A^T = | 1  1  1  0 |
//         | 0  1  1  0 |         | 1/2  1/2  1/2|           | 0  1 -1 -1 |
//         | 0 -1  1  0 |         | 1/2 -1/2  1/2|
//         | 0  1  0 -1 |         | 0    0    1  |
//
// Three passes per conv, all on one stream:
//   1. wino_input_kernel: U[pos][tile][Cin] = (B^T d B)[pos] over the zero-bordered input (window origins (2ty, 2tx)
//      in padded coordinates, so the borders are already zero and nothing is masked); in0 || in1 concatenated here.
//   2. launch_wino_gemm: M[pos] = U[pos] x V[pos] for the 16 positions, on the f32 implicit-GEMM kernel
//      (conv_igemm_dma_f32 as a 1x1 conv, blockIdx.z = position): fixed K order, no atomics.
//   3. wino_output_kernel: A^T M A per tile + bias + FeatureWiseAffine bias + residual into the zero-bordered output,
//      and the fused GroupNorm statistics (ConvParams::stats layout) in a fixed order.
// The fused 1x1 term (res_conv, ConvParams::in2 / in2b / w2) runs as a 1x1 conv on the direct kernel into the output
// first (with the conv's residual); the output transform then adds it as the residual.
// The operands and the accumulation stay fp32; the data transforms use only +-1, the weight transform (1/2) runs in fp64.
#include "sr3_internal.h"

namespace sr3 {

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

int out_slices(const ConvParams &p) {
    const int tiles = (p.Hout >> 1) * (p.Wout >> 1);
    if (p.stats) return p.stats_slices;
    return (tiles % 16) == 0 ? tiles / 16 : 1;
}

} // namespace

bool conv_wino_supported(int B, int H, int W, int Cin, int Cout) {
    static const bool off = env_int("SR3_NO_WINOGRAD", 0) != 0;    // product switch (read once)
    if (off || B <= 0 || (H & 1) || (W & 1) || H * W > 1024 || Cin < WINO_MIN_CIN || (Cin % 32) || (Cout % 64)) return false;
    // few tiles (a single 128x128 image: 256 at its 32x32 level): the three dependent passes cost more latency than the
    // MACs they save (B = 1 step 1.99 -> 2.27 ms with every level in Winograd form); B = 64 at 8x8 is 1024 tiles and gains
    const uint64_t tiles = (uint64_t)B * (H / 2) * (W / 2);
    if (tiles < WINO_MIN_TILES) return false;
    // the LDS-DMA and epilogue addressing of the position GEMMs uses 32-bit byte offsets inside one position's plane
    return tiles * (uint64_t)(Cin > Cout ? Cin : Cout) * 4 < (1ull << 32);
}

size_t conv_wino_ws_floats(int B, int H, int W, int Cin, int Cout) {
    return (size_t)16 * B * (H / 2) * (W / 2) * (Cin + Cout);
}

bool conv_wino_taken(const ConvParams &p) {
    if (!p.w_wino || !p.wino_ws || p.prec != 0 || p.ks != 3 || p.stride != 1 || p.up2 || p.phases != 1 || p.in_fm || p.f8)
        return false;
    if (p.gnf_gamma || p.out_split.p || !p.out_f32 || p.resid_split) return false;
    if (p.in0.pad != 1 || p.in0.H != p.Hout || p.in0.W != p.Wout) return false;
    if (p.in1.p && (p.in1.pad != 1 || p.in1.H != p.Hout || p.in1.W != p.Wout)) return false;
    if (p.in2.p && !p.w2) return false;
    if (!conv_wino_supported(p.B, p.Hout, p.Wout, p.in0.C + (p.in1.p ? p.in1.C : 0), p.out.C)) return false;
    const int tiles = (p.Hout >> 1) * (p.Wout >> 1);
    return p.stats == nullptr || (p.stats_slices > 0 && (tiles % p.stats_slices) == 0);
}

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

void launch_conv_wino(const ConvParams &p, hipStream_t s) {
    const int H = p.Hout, W = p.Wout, Cout = p.out.C;
    const int Cin = p.in0.C + (p.in1.p ? p.in1.C : 0);
    const size_t tiles = (size_t)p.B * (H / 2) * (W / 2);
    float *U = p.wino_ws, *Mw = p.wino_ws + 16 * tiles * Cin;
    const size_t items = tiles * (Cin / 4);
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
    const int sl = out_slices(o);
    hipLaunchKernelGGL(wino_output_kernel, dim3(Cout / 64, sl, p.B), dim3(256), 0, s, o, Mw, sl);
}

} // namespace sr3
