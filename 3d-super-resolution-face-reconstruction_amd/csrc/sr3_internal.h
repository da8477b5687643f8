// Internal declarations shared by the HIP translation units of libsr3hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>

namespace sr3 {

// ---- environment switches ---------------------------------------------------------------------------
// Everything the library reads from the environment (INTEGRATION.md lists the same names, tests/test_switches_host.py
// compares; each is read on its first use in a process and then baked into captured graphs). All but the last are
// entries of ONE table, read through env_switch / form_switch (conv_plan.h):
//   SR3_NO_GRAPH=1          every kernel launched individually, no hipGraph replay (hosts that cannot capture); the one
//                           switch read again by every sr3_create
//   SR3_NO_HALO=1           generic implicit-GEMM kernel instead of the x-halo kernels (safety switch; slower)
//   SR3_HALO_SPLITS=0|2|4   in-place split-K of deep-K convs on 128x128 x-halo tiles: off / forced
//   SR3_NO_INPLACE_SPLIT=1  split-K always as conv + reduce kernel
//   SR3_NO_WINOGRAD=1       exact-f32 3x3 convs always on the direct implicit-GEMM kernel (conv_plan)
//   SR3_NO_GN_WINO=1        three-pass Winograd convs always behind gn_apply + wino_input_kernel: the GroupNorm apply
//                           pass never writes the transformed input itself (no conv-plan switch: every plan stays)
//   SR3_NO_WINO_GEMM_OUT=1  three-pass Winograd convs always as position GEMMs + wino_output_kernel (M through memory);
//                           same bits
//   SR3_WINO_GEMM_OUT_FORCE=1  that one-kernel form wherever its preconditions hold, whatever the block count and Cin
//                           (tests, per-shape timing)
//   SR3_NO_UP2_WINO=1       exact-f32 Upsample convs always as four sub-pixel 2x2 phase convs on the direct kernel (the
//                           bits of the library before wino_up2_kernel)
//   SR3_UP2_WINO_FORCE=1    the sub-pixel Winograd form wherever its preconditions hold, whatever the block count
//                           (tests, per-shape timing)
//   SR3_NO_WINO_FUSED_ROWS=1  three-pass Winograd convs never on the one-pass kernel's tile-row instantiations
//                           (ConvPlan::wino_fused_rows): the launches of the library before them, same bits
//   SR3_WINO_FUSED_ROWS_FORCE=1  that form wherever its preconditions hold, whatever the block count and Cin (tests,
//                           per-shape timing)
//   SR3_NO_GN_RES1X1=1      block1's GroupNorm apply pass and the 1x1 res_conv side launch of a Winograd conv2 always as
//                           two launches (the library before gn_res1x1_kernel; same bits)
//   SR3_GN_RES1X1_FORCE=1   that kernel wherever its preconditions hold, whatever the level and block count (tests,
//                           per-shape timing)
//   SR3_NO_CONV_IN_F32=1    the exact-f32 first conv always on the generic implicit-GEMM kernel over the 32 padded input
//                           channels (the launch of the library before conv_in_f32_kernel; another summation order,
//                           so not the same bits). No _FORCE twin: the form has no tuned gate
//   SR3_THRESHOLD_BLOCKS=N  blocks that share one image in the selection of the dynamic threshold instead of one per
//                           16384 keys (per-shape timing; same bits); read where kernels_threshold.hip plans a selection
inline int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }

// ---- batch-invariant mode (sr3_set_batch_invariant) ---------------------------------------------------
// The planning batch P of the calling thread, 0 = off (conv_plan.hip). While it is set, every host decision that picks
// an arithmetic from the amount of work (a tile, a split-K count, a Winograd form, the statistics slices, the attention
// block) counts P images instead of the call's B, so the bytes of one image do not depend on its batch. The C-ABI entry
// points set it from their context for the time of the call (sr3_api.hip: PlanScope); set_plan_batch returns the old value.
int plan_batch();
int set_plan_batch(int P);
inline long plan_b(long B) { const int P = plan_batch(); return P > 0 ? (long)P : B; }

// Activation tensor: NHWC fp32 with an optional 1-pixel zero border ("pad") stored around every
// image, so a 3x3 window never needs a bounds check: pixel (n, y, x) lives at
//   p + (((n * (H + 2*pad)) + y + pad) * (W + 2*pad) + x + pad) * C.
// Borders are zeroed once when the workspace is created and never written again.
struct TDesc {
    float *p = nullptr;
    int C = 0, H = 0, W = 0, pad = 0;
    __host__ __device__ int Hp() const { return H + 2 * pad; }
    __host__ __device__ int Wp() const { return W + 2 * pad; }
    __host__ __device__ size_t pix(int n, int y, int x) const {
        return ((size_t)n * Hp() + y + pad) * Wp() + x + pad;
    }
    size_t floats(int B) const { return (size_t)B * Hp() * Wp() * C; }
};

// ---- conv as implicit GEMM (kernels_conv.hip) -------------------------------------------------
// Input = channel concatenation in0 ‖ in1 (reference unet.py:261), already activated where the
// reference applies GroupNorm+Swish first (launch_gn_apply), seen through an optional nearest x2
// upsample (unet.py:61). 3x3 convs require pad == 1 on the inputs.
struct ConvParams {
    TDesc in0, in1;         // in1.p == nullptr if none; same H, W, pad as in0; C multiples of 32
    int B = 0;
    int Hout = 0, Wout = 0;
    int ks = 3, stride = 1, up2 = 0;   // ks 1 | 2 | 3; ks == 2 (stride 1) reads the window (oy+org_y+{0,1}, ox+org_x+{0,1})
    // sub-pixel phases of the upsample conv (launch_conv, up2): window origin shift in padded
    // coordinates, and the output pixel written for window (oy, ox) is (oy*out_step + out_oy, ...)
    int org_y = 0, org_x = 0;
    int out_step = 1, out_oy = 0, out_ox = 0;
    int stats_slice0 = 0;              // first statistics slice of this launch
    // log2(Hout*Wout) / log2(Wout) when they are powers of two (set by launch_conv, -1 otherwise): the
    // per-lane address set-up of a tile then uses shifts instead of integer divisions
    int hw_shift = -1, w_shift = -1;
    // phases > 1 (= 4): one launch runs the four sub-pixel phases of an upsample conv on blockIdx.z
    // (grid.y of the split-K reduce): phase ph = (py, px) sets org_* = out_o* = (py, px) and advances
    // w by ph * phase_w_stride floats, stats_slice0 by ph * phase_slices, part by ph * phase_part_stride
    int phases = 1, phase_slices = 0;
    size_t phase_w_stride = 0, phase_part_stride = 0;
    const float *w = nullptr;          // packed [ks*ks][Cout][Cin]
    // optional fused 1x1 term (ResnetBlock.res_conv, unet.py:102-103,110): out += in2 (*) w2, read at
    // the output pixel; same precision format and (for prec 1) the same weight scale as w
    TDesc in2;                         // p == nullptr if none; same H, W as the output
    TDesc in2b;                        // optional second part: the 1x1 input is in2 ‖ in2b (x ‖ skip, unet.py:261)
    const float *w2 = nullptr;         // packed [Cout][in2.C + in2b.C]
    const float *bias = nullptr;       // [Cout] or null
    const float *chan_bias = nullptr;  // [B][chan_bias_stride] (+ offset applied by caller) or null
    int chan_bias_stride = 0;
    // optional fused GroupNorm statistics of the OUTPUT: per (image, M-tile-in-image, channel)
    // {sum, sum of squares} in fp64 at stats[((n * stats_slices + slice) * Cout + c) * 2]; requires
    // Hout*Wout % BM == 0 for the tile the launcher picks; stats_slices as ConvPlan::stats_slices tells
    double *stats = nullptr;
    int stats_slices = 0;
    TDesc resid;            // p == nullptr if none; same geometry as out
    int resid_split = 0;    // 1: resid is stored in the split-f16 format (hi + lo), not fp32
    TDesc out;              // C = Cout
    // optional twin of the output in the split-f16 input format (same geometry as out): lets the
    // next conv read this tensor directly (Down/Upsample input, fused res_conv operand)
    TDesc out_split;
    int out_f32 = 1;        // 0: only out_split is written (out.p then only provides the geometry)
    // prec 0: exact f32 MFMA; inputs / weights are fp32.
    // prec 1: split-f16 ("f16x3"): every 32-channel chunk of the inputs and of the packed weights is
    //         stored as 32 hi halfs | 32 lo halfs (x = hi + lo to ~2^-22), the product is
    //         hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation; weights are
    //         pre-scaled by 2^k (w_unscale = 2^-k is applied to the accumulator in the epilogue).
    int prec = 0;
    // f8 = 1 (prec 1 only; "f16f8" mode, conv_f8_supported() tells for which shapes): in0 / in1 and w are in the F8C
    // variant of the split format — per 32-channel chunk 32 hi halfs | 32 x e4m3(lo * 2^SR3_F8_XL) | 32 x e4m3(hi * 2^SR3_F8_XH)
    // for activations, 32 hi halfs | 32 x e4m3(hi * 2^SR3_F8_WH) | 32 x e4m3(lo * 2^SR3_F8_WL) for weights — and the two
    // correction products xl*wh + xh*wl run as ONE v_mfma_scale_f32_32x32x64_f8f6f4 per 32x32 tile and K-step (half the
    // cycles of the four f16 MFMAs they replace; ~6e-5 instead of ~4e-6 from the reference over a sampler run).
    // in2 / in2b / w2 (fused 1x1 term) stay in the plain split format.
    int f8 = 0;
    float w_unscale = 1.0f;
    // split-K for small problems (few tiles, deep K): `splits` blocks share one output tile, each
    // reducing a contiguous range of 32-channel chunks into part[split][M][Cout]; a second kernel
    // adds the partials and applies the epilogue. splits <= 1: single pass. Set by launch_conv from its plan (a caller's
    // value is ignored); part: ConvPlan::part_floats floats, nullptr: never split
    int splits = 1;
    float *part = nullptr;
    // in-place split-K (ConvPlan::split tells when launch_conv uses it): CONV_TILE_COUNTERS counters, one zero-initialised counter per
    // output tile and sub-pixel phase; the last block to arrive at a tile adds the partials and runs the
    // epilogue itself (no reduce kernel; fused statistics in the unsplit layout: one slice per M-tile).
    // nullptr: always the two-kernel form.
    unsigned *tile_cnt = nullptr;
    // 1: never the in-place split-K of the 128x128 x-halo tile (CS_INPLACE_HALO) — set for the rest of a context's
    // life once one of its bounded inter-block waits gave up (SR3_FLAG_WAIT_TIMEOUT): the conv then runs unsplit on the
    // generic 64x64 tile, whose blocks never wait for each other
    int no_halo_split = 0;
    // split-f16 range check: any value stored in the split format (out_split) with |v| > 65504 (or
    // non-finite) sets *ovf = 1; the API call that ran the launch then fails (never a silent clamp)
    int *ovf = nullptr;
    // Winograd F(2x2, 3x3) form of this conv (prec 0 only; conv_plan takes it where the shape gains and the conv uses
    // nothing the Winograd path does not handle): transformed weights [16][Cout][CinPad] (make_wino_weights) and a
    // workspace of ConvPlan::wino_ws_floats floats; either null: direct kernel
    const float *w_wino = nullptr;
    float *wino_ws = nullptr;
    // the one-pass kernel's copy of w_wino in fragment-major order [16][CinPad/8][Cout][8] (make_wino_weights_frag);
    // null: a conv of the one-pass shapes runs on the direct kernel
    const float *w_wino_f = nullptr;
    // Upsample convs (up2, prec 0): the sub-pixel Winograd F(2x2, 2x2) weights [4 phases][9][CinPad/8][Cout][8]
    // (make_up2_wino_weights); null: the four phase convs on the direct kernel
    const float *w_up_wino = nullptr;
    // 1 (CK_WINO_THREE_PASS only): U of in0 || in1 is already at the head of wino_ws (launch_gn_wino_input wrote it);
    // launch_conv_wino then skips wino_input_kernel and does nothing else differently. No input of conv_plan.
    int u_ready = 0;
    // 1 (Winograd plans with the fused 1x1 term only): out already holds w2 . (in2 || in2b) — launch_gn_res1x1 wrote it in
    // block1's GroupNorm pass (conv_plan.hip: gn_res1x1_gate) — so launch_conv_wino skips its 1x1 side launch and takes out
    // as the residual, and does nothing else differently. No input of conv_plan.
    int res_ready = 0;
    // GEMM batch (launch_wino_gemm only): blockIdx.z = z multiplies in0.p + z * batch_in_stride by
    // w + z * phase_w_stride into out.p + z * batch_out_stride
    int zbatch = 1;
    size_t batch_in_stride = 0, batch_out_stride = 0;
};
// bit raised in *ConvParams::ovf when the bounded inter-block wait of the in-place split-K on x-halo tiles gives up (the
// only such wait in the library): the launch's result is invalid; the API replays the work with
// ConvParams::no_halo_split set (sr3_api.hip: range_read)
constexpr int SR3_FLAG_WAIT_TIMEOUT = 2;
// bound of that wait in ticks of s_memrealtime (constant 100 MHz on gfx950, MI355X_MICROARCH.md): 2^19 = 5.2 ms — the
// blocks of one tile are dispatched back to back and the whole conv takes < 0.1 ms on an idle chip
constexpr long long SR3_WAIT_TICKS = 1ll << 19;
// largest magnitude the split-f16 format (hi + lo, both fp16) can hold
constexpr float SPLIT_F16_MAX = 65504.0f;

// ---- split-f16 twin stores from MFMA accumulators (conv epilogues) -----------------------------------
// Two lanes that hold neighbouring channels (lane ^ 1) exchange halfs so that each lane stores ONE 4-byte
// word: the even lane both hi halfs, the odd lane both lo halfs. own = hi | lo << 16, oth = the partner's
// (DPP quad_perm [1,0,3,2]); v_perm_b32 picks {own.hi16?..} by a per-lane selector:
//   even: [own.b0, own.b1, oth.b0, oth.b1]   odd: [oth.b2, oth.b3, own.b2, own.b3]
// (v_perm_b32 D = bytes of {src0 = oth : bytes 4..7, src1 = own : bytes 0..3}).
// range: running unsigned max of (hi bits & 0x7C00) — 0x7C00 at the end means some hi half was inf / nan,
// i.e. |value| beyond what hi + lo can hold (>= 65520) or not finite: two VALU operations per value.
__device__ __forceinline__ unsigned split_pair_selector(bool odd) { return odd ? 0x03020706u : 0x05040100u; }
__device__ __forceinline__ unsigned split_pair_word(float v, unsigned selector, unsigned &range) {
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    const unsigned own = (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
    const unsigned e = own & 0x7C00u;
    range = e > range ? e : range;
    const unsigned oth = (unsigned)__builtin_amdgcn_mov_dpp((int)own, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    return __builtin_amdgcn_perm(oth, own, selector);
}
__device__ __forceinline__ bool split_range_overflow(unsigned range) { return range == 0x7C00u; }
// F8C operand scaling (powers of two; activations beyond e4m3's 448 raise the range flag). The CPU emulation of these
// formats (tests/emulate_operand_formats.py) gives the same sampler error for activation exponents 0, 2 and 4.
constexpr int SR3_F8_XH = 0, SR3_F8_XL = 11;      // xh8 = e4m3(xh), xl8 = e4m3(xl * 2048)   (|xl| <= 2^-11 |xh|: <= 256 at the limit)
constexpr int SR3_F8_WH = -3, SR3_F8_WL = 9;      // weights are pre-scaled into [1024, 2048): wh8 < 256, |wl| <= 0.5 -> wl8 <= 256
constexpr float SPLIT_F8_MAX = 448.0f;
// true when launch_conv runs this 3x3 / stride-1 split-f16 conv with the fp8 correction products if ConvParams::f8 is set
// (the caller then writes the conv's input with split format 2 and passes the F8C weights): conv_plan's answer
bool conv_f8_supported(int B, int H, int W, int Cout, int Cin);
// split weights [chunks][32 hi | 32 lo] -> F8C weights [chunks][32 hi | 32 wh8 | 32 wl8] (device to device)
void launch_make_f8_weights(const float *split, float *dst, size_t chunks, hipStream_t s);
// ---- the dispatch plan: which kernel, which split-K form, which buffers — decided in ONE place (conv_plan) ----------
enum ConvKernel {
    CK_WINO_ONE_PASS, CK_WINO_THREE_PASS,                        // exact-f32 Winograd F(2x2, 3x3) (kernels_wino.hip)
    CK_HALO_F8C, CK_HALO_128x128_SEG32, CK_HALO_128x128_SEG8, CK_HALO_128x64,     // x-halo kernels (split-f16)
    CK_GENERIC_128x32, CK_GENERIC_128x64, CK_GENERIC_64x64, CK_GENERIC_128x128,   // implicit GEMM over LDS-DMA rings
    CK_COUNT
};
const char *conv_kernel_name(ConvKernel k);
enum ConvSplit { CS_NONE, CS_REDUCE, CS_INPLACE, CS_INPLACE_HALO };   // conv + reduce kernel | in place, 64x64 tile | in place, x-halo tile
constexpr int CONV_TILE_COUNTERS = 8192;    // capacity of ConvParams::tile_cnt (tiles x phases of one launch)
struct ConvPlan {
    ConvKernel kernel = CK_GENERIC_128x128;
    int tile_m = 128, tile_n = 128;    // output tile of the main kernel (Winograd: of the direct kernel the shape would take)
    ConvSplit split = CS_NONE;
    int splits = 1;                    // K-splits (1 = none)
    int phases = 1;                    // 4: the sub-pixel phases of an upsample conv in one launch
    size_t part_floats = 0;            // ConvParams::part as this launch uses it (all phases), 0 = none
    bool needs_counters = false;       // ConvParams::tile_cnt is used (in-place split-K)
    // slices per image the fused statistics of the output come in for this shape (what the caller passes as
    // ConvParams::stats_slices with ConvParams::stats), 0 = no fused statistics: the caller's statistics kernel runs
    int stats_slices = 0;
    size_t wino_ws_floats = 0;         // ConvParams::wino_ws: U [16][B*H*W/4][Cin] + M [16][B*H*W/4][Cout] (three-pass form)
    bool needs_wino_frag = false;      // reads ConvParams::w_wino_f (one-pass form)
    // CK_WINO_THREE_PASS only: 0 = position GEMMs + wino_output_kernel; 64 | 128 = wino_gemm_out_kernel with that many
    // output channels per block (the M half of wino_ws then stays unused). Not part of the exported plan.
    int wino_gemm_out = 0;
    // CK_WINO_THREE_PASS only: 0 = one of the forms above; 2 | 4 = the one-pass kernel with that many tile rows per block
    // (wino_fused_kernel<R>, kernels_wino.hip), reading ConvParams::w_wino_f: neither U nor M exists, the whole of
    // wino_ws stays unused and the conv reads its zero-bordered activated input, as the one-pass plan does. Wins over
    // wino_gemm_out. Not part of the exported plan: kernel, stats_slices, wino_ws_floats and needs_wino_frag stay the
    // three-pass plan's, and the statistics come in the same slices.
    int wino_fused_rows = 0;
    // Upsample convs only: 0 = the four phase convs on `kernel`; 1 | 2 | 4 = wino_up2_kernel (kernels_wino.hip) with that
    // many tile rows per block, reading ConvParams::w_up_wino instead of w. Not part of the exported plan: kernel, phases,
    // split and stats_slices stay the direct plan's, and the statistics come in the same slices.
    int up2_wino = 0;
    // Batch-invariant mode only: the largest batch this plan holds for (a limit on the real batch — arrival counters,
    // 32-bit offsets inside one Winograd plane — never changes the form there; a launch past it fails), 0 = none.
    long batch_limit = 0;
    const char *error = nullptr;      // a request no kernel honours (ConvParams::f8 on a shape outside the F8C kernel)
};
// reads p as launch_conv does: a null part / tile_cnt / w_wino / w_wino_f / wino_ws / stats means "not offered", and the
// plan degrades (no split-K, two-kernel split, direct kernel); p.up2: p describes the conv at the OUTPUT resolution
ConvPlan conv_plan(const ConvParams &p);
// the plan of a conv shape with every buffer offered (fused statistics, in the layout the plan names, only with
// `stats`) — for callers that size buffers before they exist. H, W: input size; f8: the F8C request (prec 1)
ConvPlan conv_plan_offered(int B, int H, int W, int Cin, int Cout, int ks, int stride, int up2, int prec, bool f8, bool stats);
// computes the plan and launches it. Upsample (nearest x2) + conv3x3 (unet.py:58-65, p.up2) runs as four sub-pixel
// phases in one launch: output pixels of parity (py, px) see only a 2x2 window of the low-resolution input, with the
// 3x3 taps that land on the same source pixel pre-added (make_up2_phase_weights) — 16 instead of 36 MACs per
// low-resolution pixel, channel pair and 2x2 output block. p then describes the conv at the OUTPUT resolution (Hout,
// Wout = 2H, 2W; in0 = low-resolution input), p.w = phase weights [4 phases][4 taps][Cout][CinPad].
void launch_conv(const ConvParams &p, hipStream_t s);
// launch_conv never aborts the process: a request it cannot honour (a caller / library bug) launches nothing and leaves
// a message here; returns it once (nullptr if none) — the C-ABI entry points fail the call with it
const char *conv_take_error();
// packed [9][Cout][CinPad] -> [py*2+px][dy2*2+dx2][Cout][CinPad]
void make_up2_phase_weights(const float *packed9, int Cout, int CinPad, float *dst);
// ---- Upsample conv as sub-pixel Winograd F(2x2, 2x2) (kernels_wino.hip, wino_up2_kernel) --------------------------------
// Each phase (py, px) is a stride-1 2x2 conv over the zero-bordered low-resolution image, so 2x2 outputs of a phase come
// from a 3x3 window with 9 products instead of 16:
//   Y = A^T [ (G g G^T) . (B^T d B) ] A,  G = [[1,0],[1,1],[0,1]],  B^T = [[1,-1,0],[0,1,0],[0,1,-1]],  A^T = [[1,1,0],[0,1,-1]]
//   d = padded low-resolution rows 2ti + py .. 2ti + py + 2, columns 2tj + px .. + 2; outputs at (2(2ti + a) + py, 2(2tj + b) + px).
// The transforms hold 0 and +-1 only; G g G^T is a sum of original 3x3 taps (1-D: py = 0 -> {w0}, {w0, w1, w2}, {w1, w2};
// py = 1 -> {w0, w1}, {w0, w1, w2}, {w2}), added in fp64 from 0.0 in (dy, dx) order and rounded once.
// One block = 32 tiles (R tile rows of 32 / R tiles: R = 1 | 2 | 4 for low-resolution widths 64k | 32 | 16) x 32 output
// channels x the four phases, one phase per wave. Taken from UP2_WINO_MIN_BLOCKS blocks on (two resident per CU).
constexpr int UP2_WINO_TILES = 32, UP2_WINO_BN = 32;
constexpr int UP2_WINO_MIN_BLOCKS = 512;
// host helper: packed [9][Cout][CinPad] -> [py*2+px][3i+j][CinPad/8][Cout][8]; up2_wino_floats: its size
inline size_t up2_wino_floats(int Cout, int CinPad) { return (size_t)36 * Cout * CinPad; }
void make_up2_wino_weights(const float *packed9, int Cout, int CinPad, float *dst);
// the form ConvPlan::up2_wino names; p as launch_conv takes it (up2 = 1, at the output resolution)
void launch_conv_up2_wino(const ConvParams &p, const ConvPlan &plan, hipStream_t s);
// ---- Winograd F(2x2, 3x3) for the exact-f32 3x3 convs of the deep levels (kernels_wino.hip) ----------------------
// Y = A^T [ (G g G^T) . (B^T d B) ] A per 2x2 output tile: the 16 positions of the transformed 4x4 window are 16
// independent GEMMs [B*H/2*W/2][Cin] x [Cin][Cout] on the f32 implicit-GEMM kernel (4 instead of 9 MACs per output
// pixel and channel pair); the input transform and the output transform (+ bias, FeatureWiseAffine bias, residual,
// fused 1x1 term, fused GroupNorm statistics) are separate passes.
constexpr int WINO_MIN_CIN = 128;      // narrower inputs: the transforms' memory passes cost more than the MACs saved
constexpr int WINO_MIN_TILES = 1024;   // fewer 2x2 output tiles per launch (B * H/2 * W/2): the direct kernel (latency)
// 64x64 pixels and up: ONE kernel per conv (U and M stay on chip; kernels_wino.hip, wino_fused_kernel), taken from this
// many blocks of 32 tiles x 64 output channels (4 per CU) — fewer: the direct kernel
constexpr int WINO_FUSED_CIN = 64;
constexpr int WINO_FUSED_MIN_BLOCKS = 1024;
// the one-pass kernel's block: a strip of WINO_FUSED_TILES 2x2 tiles along a tile row x WINO_FUSED_BN output channels
constexpr int WINO_FUSED_TILES = 32, WINO_FUSED_BN = 64;
// The same kernel at the 32x32 and 16x16 levels (ConvPlan::wino_fused_rows, a form of the three-pass plan): a block's 32
// tiles are R = 2 | 4 tile rows of 16 | 8 tiles, i.e. 32 consecutive tiles of the image. What it saves over the three
// passes is U's trip through memory (four times the activated input, written by the GroupNorm pass and read by the
// GEMMs) and, beyond WINO_GEMM_OUT_MAX_CIN, M's. Taken from WINO_FUSED_ROWS_MIN_BLOCKS blocks on at a width of 32 (the
// smallest count timed: the B = 64 step's 32x32 convs; profiles/README.md finding 91). At a width of 16, from
// WINO_FUSED_ROWS_MIN_BLOCKS_16 blocks on (B = 64, Cout = 512: the only count timed) and up to
// WINO_FUSED_ROWS_MAX_CIN_16 input channels: with each window row staged once, Cin = 256 and 512 run at 0.88 and
// 0.85-0.88 of the three-pass form in both rounds, Cin = 768 and 1024 at 0.92-0.96, over the 0.9 rule (finding 102);
// those stay on the position GEMMs and are reached only under SR3_WINO_FUSED_ROWS_FORCE=1.
// (tests/test_wino_rows16_host.py restates the gate with all three constants: retune them there too)
constexpr int WINO_FUSED_ROWS_MIN_BLOCKS = 2048;
constexpr int WINO_FUSED_ROWS_MIN_BLOCKS_16 = 1024;
constexpr int WINO_FUSED_ROWS_MAX_CIN_16 = 512;
// host helper: packed [9][Cout][CinPad] -> G g G^T as [16][Cout][CinPad] (fp64, rounded once to fp32)
void make_wino_weights(const float *packed9, int Cout, int CinPad, float *dst);
// host helper: [16][Cout][CinPad] (make_wino_weights) -> [16][CinPad/8][Cout][8]; launch_wino_frag: the same on the device
void make_wino_weights_frag(const float *wino, int Cout, int CinPad, float *dst);
void launch_wino_frag(const float *wino, int Cout, int CinPad, float *dst, hipStream_t s);
// the Winograd form conv_plan chose (CK_WINO_ONE_PASS | CK_WINO_THREE_PASS)
void launch_conv_wino(const ConvParams &p, const ConvPlan &plan, hipStream_t s);
// Second form of the three-pass plan (ConvPlan::wino_gemm_out): U -> wino_gemm_out_kernel -> output. One block owns
// WINO_GEMM_OUT_TILES consecutive tiles x 64 | 128 output channels, walks the 16 positions in ONE K loop and folds
// A^T M A in the accumulators, so M is never stored; bit-identical to launch_wino_gemm + wino_output_kernel. Each block
// runs 16 times longer than a position-GEMM block, so the form is taken only from WINO_GEMM_OUT_MIN_BLOCKS blocks on
// (fewer: the position-parallel form, whose 16 x more blocks spread further), and up to WINO_GEMM_OUT_MAX_CIN input
// channels (what it saves is M's traffic, fixed per conv; its K loop is no faster than the position GEMMs').
constexpr int WINO_GEMM_OUT_TILES = 64;
constexpr int WINO_GEMM_OUT_MIN_BLOCKS = 256;
constexpr int WINO_GEMM_OUT_MAX_CIN = 256;
// (tests/test_gpu_wino_gemm_out.py restates the gate with both constants: retune them there too)
// the 16 position GEMMs of one Winograd conv on conv_igemm_dma_f32 (kernels_conv.hip); p as described at zbatch
void launch_wino_gemm(const ConvParams &p, hipStream_t s);
// host helper: OIHW -> [tap][Cout][CinPad] (zero pad input channels up to CinPad)
void pack_conv_weight(const float *oihw, int Cout, int Cin, int ks, int CinPad, float *dst);
// host helper: fp32 packed weights -> split-f16 layout (same byte size), returns the unscale factor
float split_conv_weight(const float *packed, size_t rows, int CinPad, float *dst);

// ---- train-mode Dropout of ResnetBlock.block2 (unet.py:81-91) -----------------------------------------
// What the masked apply passes read from device memory, refreshed like the rest of StepArgs: a captured step keeps its
// launch arguments. The input of block2's conv is keep ? swish(gn(h1)) * s : 0.
struct DropArgs {
    uint64_t seed = 0, image_offset = 0;    // key of the mask stream; global image index = image_offset + n
    const uint8_t *mask = nullptr;          // injected masks (layers concatenated, each NCHW [B][C][H][W], nonzero = keep) or null -> Philox
    uint32_t draw = 0;                      // StepArgs::draw in the sampler, 0 in the forward and the loss
    uint32_t thr = 0;                       // round-half-even(p * 65536): an element is kept iff its 16-bit field >= thr
    float s = 1.0f;                         // float32(1.0 / (1.0 - p)), the division in double
    uint32_t pad_ = 0;
};
// One masked apply pass (a launch argument, constant per workspace): a == null: no dropout
struct DropLayer {
    const DropArgs *a = nullptr;
    uint32_t c1_hi = 0;                     // (layer + 1) << 24, layer = 0-based ordinal of the ResnetBlock (downs, mid, ups)
    uint32_t pad_ = 0;
    uint64_t base = 0;                      // offset of this layer in the injected buffer
};
constexpr int DROP_MAX_LAYERS = 254;        // the top byte of counter word c1 is layer + 1 in [1, 255)
constexpr uint32_t DROP_MAX_DRAW = 1u << 24;

// ---- GroupNorm (kernels_misc.hip) -------------------------------------------------------------
// statistics over the virtual concatenation in0 ‖ in1 -> folded affine scale/shift [B][C]
size_t gn_workspace_floats(int B, int c_max);   // c_max = widest normalised tensor
void launch_groupnorm_affine(const TDesc &in0, const TDesc &in1, int B, int groups, const float *gamma,
                             const float *beta, float eps, float *part, float *scale, float *shift,
                             hipStream_t s);
// statistics already accumulated by the producing convs (ConvParams::stats): only the reduce
struct StatsRef { const double *p = nullptr; int slices = 0; };
void launch_groupnorm_finalize(const StatsRef &s0, int C0, const StatsRef &s1, int C1, int B, int HW, int groups,
                               const float *gamma, const float *beta, float eps, float *scale, float *shift,
                               hipStream_t s);
// out[n,y,x,:] = act(concat(in0,in1)[n,y,x,:] * scale[n,:] + shift[n,:]); mode 0 copy, 1 affine,
// 2 affine + Swish. out.C == in0.C + in1.C; writes the interior only. split = 1 stores every
// 32-channel chunk as 32 hi halfs | 32 lo halfs (the conv's prec 1 input format), split = 2 as
// 32 hi halfs | 32 x e4m3(lo * 2^SR3_F8_XL) | 32 x e4m3(hi * 2^SR3_F8_XH) (ConvParams::f8; `raw` stays format 1).
// raw (optional, p != nullptr): additionally stores the un-normalised concatenation in the same
// format (the input of a fused res_conv).
// in_split: bit 0 / bit 1 = in0 / in1 is itself stored in the split-f16 format (split-only tensors)
// ovf: range-check flag of the split format (see ConvParams::ovf), may be null
// drop (drop.a != null; mode 2 only): the Dropout mask of ResnetBlock.block2 multiplies the activated values in registers
// in front of the store, whatever the format (the range check sees the scaled value); `raw` is never masked
void launch_gn_apply(const TDesc &in0, const TDesc &in1, int B, const float *scale, const float *shift,
                     int mode, int split, const TDesc &out, hipStream_t s, const TDesc &raw = TDesc(),
                     int in_split = 0, int *ovf = nullptr, const DropLayer &drop = DropLayer());
// streaming form of the apply pass for large tensors (one item per thread; scale / shift from memory)
void launch_gn_apply_rows(const TDesc &in0, const TDesc &in1, int B, const float *scale, const float *shift,
                          int mode, int split, const TDesc &out, hipStream_t s, const TDesc &raw = TDesc(),
                          int in_split = 0, int *ovf = nullptr, const DropLayer &drop = DropLayer());
// GroupNorm finalize folded into the apply pass (one launch per normalised tensor): s0 / s1 are the fp64
// partial statistics of in0 / in1 (ConvParams::stats layout; from conv epilogues or
// launch_groupnorm_partials, which returns the virtual concatenation as one source: pass it as s0
// with s1 empty)
void launch_gn_fold_apply(const TDesc &in0, const TDesc &in1, int B, const StatsRef &s0, const StatsRef &s1, int groups,
                          const float *gamma, const float *beta, float eps, int mode, int split, const TDesc &out,
                          hipStream_t s, const TDesc &raw = TDesc(), int in_split = 0, int *ovf = nullptr,
                          const DropLayer &drop = DropLayer());
// The apply pass in front of a three-pass Winograd conv (exact f32, unsplit inputs): activates in0 || in1 as
// launch_gn_apply / launch_gn_fold_apply do and writes, instead of the zero-bordered tensor, its Winograd input
// transform U [16][B*H/2*W/2][C] — bit for bit what wino_input_kernel makes of that tensor (ConvParams::u_ready).
// in0 / in1 padded or not; H, W even; C multiples of 4 on both sides of the concatenation.
void launch_gn_wino_input(const TDesc &in0, const TDesc &in1, int B, const float *scale, const float *shift, int mode,
                          float *U, hipStream_t s);
void launch_gn_fold_wino_input(const TDesc &in0, const TDesc &in1, int B, const StatsRef &s0, const StatsRef &s1, int groups,
                               const float *gamma, const float *beta, float eps, int mode, float *U, hipStream_t s);
StatsRef launch_groupnorm_partials(const TDesc &in0, const TDesc &in1, int B, float *part, hipStream_t s);
// ---- block1's apply pass + the block's 1x1 res_conv in one pass over the raw x || skip (kernels_gn_res.hip) -------------
// act (zero-bordered, C0 + C1 channels; interior only) = swish_fast(fmaf(in0 || in1, scale, shift)), bit for bit what
// launch_gn_apply* write in mode 2 / format 0; out (C = Cout) = w2 . (in0 || in1), bit for bit what launch_conv writes for
// the unsplit 1x1 conv without bias (the side launch of launch_conv_wino). scale / shift [B][C0 + C1] from
// launch_groupnorm_finalize. Shapes: gn_res1x1_shape_ok — channels in 32s on both sides of the concatenation, Cout in
// 64s (a whole number of gn_res1x1_bn column tiles), H * W a multiple of the 128-pixel tile, at most GN_RES1X1_MAX_CIN
// input channels (the scale / shift table of a block lives in LDS).
constexpr int GN_RES1X1_MAX_CIN = 1024;
bool gn_res1x1_shape_ok(int H, int W, int C0, int C1, int Cout);
int gn_res1x1_bn(int B, int H, int W, int Cout);
void launch_gn_res1x1(const TDesc &in0, const TDesc &in1, int B, const float *scale, const float *shift, const TDesc &act,
                      const float *w2, const TDesc &out, hipStream_t s);
// common power-of-two scale for several weight tensors: returns k with max|w| * 2^k in [1024, 2048)
int split_scale_exponent(const float *packed, size_t n);
float split_conv_weight_k(const float *packed, size_t rows, int CinPad, int k, float *dst);

// ---- weight layouts made on the device (kernels_weights.hip; sr3_load_weights_dev) -----------------------------------
// The device twins of the host helpers above, bit for bit. launch_weight_pack: fp32 OIHW in device memory -> packed
// [tap][Cout][CinPad] (up_phase: the 16 phase planes), G g G^T planes into `wino` when given (ks 3, not up_phase), and
// max|w| of what it wrote to `packed` (NaN ignored) as a bit pattern into *wmax by atomic max (zero it first).
// up_wino (up_phase only, may be null): the make_up2_wino_weights layout.
void launch_weight_pack(const float *oihw, int Cout, int Cin, int ks, int CinPad, bool up_phase, float *packed, float *wino,
                        unsigned *wmax, hipStream_t s, float *up_wino = nullptr);
// the same maximum of a tensor that is packed already (n a multiple of 4)
void launch_weight_absmax(const float *packed, size_t n, unsigned *wmax, hipStream_t s);
// split_conv_weight_k over `floats` packed values (a multiple of 32)
void launch_weight_split(const float *packed, size_t floats, int k, float *dst, hipStream_t s);
void launch_weight_bias_sum(const float *a, const float *b, int n, float *dst, hipStream_t s);
// ResBlock::ident_w of a C-wide block: (fp16)v on the diagonal of the split-f16 [C][C] matrix, zero elsewhere
void launch_weight_ident(int C, float v, float *dst, hipStream_t s);

// ---- attention core ----------------------------------------------------------------------------
double launch_attention(const float *qkv, int B, int N, int C, float *out, hipStream_t s);
// streaming form (online softmax, any N >= 1, no N x N score tile): same operands and result as launch_attention;
// C a multiple of 32 up to 512 (attention_stream_supported)
bool attention_stream_supported(int C);
double launch_attention_stream(const float *qkv, int B, int N, int C, float *out, hipStream_t s);
// split-f16 form: qkv in the conv's split operand format ([B][N][3C], 32-channel chunks of hi | lo halfs);
// out (fp32 [B][N][C]) and / or out_split (the same tensor in the split format) may be null
bool attention_split_supported(int N, int C);
size_t attention_vt_floats(int B, int N, int C);     // scratch for v^T
// Which core runs self-attention over N tokens of C channels: the split-f16 core where the arithmetic is split-f16 and the
// shape fits it; else the 32 x N score-tile core while that tile fits in LDS; else the streaming core within its channel
// bound. The one decision behind workspace sizing, the batch bound, the UNet's launch and sr3_op_attention.
constexpr int ATTN_TILE_MAX_TOKENS = 1024;
enum AttnCore { ATTN_SPLIT, ATTN_TILE, ATTN_STREAM, ATTN_UNSUPPORTED };
AttnCore attention_core(bool split_f16, long N, int C);
double launch_attention_split(const float *qkv_split, float *vt, int B, int N, int C, float *out, float *out_split,
                              int *ovf, hipStream_t s);

// ---- noise-level embedding ---------------------------------------------------------------------
struct EmbedParams {
    const float *noise_level; // noise_level[n * nl_stride]; stride 0 broadcasts one scalar
    int nl_stride;
    int dim;                  // inner_channel
    const float *w1, *b1;     // [4dim][dim], [4dim]
    const float *w2, *b2;     // [dim][4dim], [dim]
    const float *nfw, *nfb;   // [total][dim], [total]
    int total;
    float *temb;              // [B][dim]
    float *chan_bias;         // [B][total]
};
void launch_noise_embed(const EmbedParams &p, int B, hipStream_t s);

// ---- layout + DDPM update ----------------------------------------------------------------------
// NCHW [B][C][H][W] -> channels [coff, coff+C) of dst (NHWC TDesc)
void launch_nchw_to_nhwc(const float *in, int B, int C, const TDesc &dst, int coff, hipStream_t s);
// channels [coff, coff+C) of src -> NCHW
void launch_nhwc_to_nchw(const TDesc &src, int coff, int B, int C, float *out, hipStream_t s);
// Per-step values live in device memory (written by a tiny async copy before every step), so the
// kernel arguments of a step never change and the whole step can be replayed as one hipGraph.
struct StepArgs {
    float nl;                   // noise level fed to the embedding (diffusion.py:166-167)
    float a, b, c1, c2, sigma;  // recip, recipm1, coef1, coef2, exp(0.5*logvar) (0 at t == 0)
    float c3;                   // weight of the previous step's x0 (multistep samplers, hist == 2)
    uint32_t draw;
    uint32_t hist;              // x0 history: 0 untouched (DDPM / DDIM), 1 store x0, 2 read the previous x0, then store
    uint32_t pad_;
    const float *noise;         // NCHW [B][C][HW] or null -> Philox
    float *frame;               // NCHW [B][C][HW] or null: copy of the updated image
    uint64_t seed, image_offset;
    DropArgs drop;              // read by the block2 apply passes while dropout is live (DropLayer::a points here)
};
struct UpdateParams {
    float *packed = nullptr;   // optional packed split-f16 copy of the state (conv_in_kernel): 16 halfs per padded pixel
    TDesc state;        // x lives in channels [xoff, xoff+C)
    int xoff, C;        // C = image channels (3)
    TDesc eps;          // eps.C >= C
    const StepArgs *args;
    int *ovf = nullptr; // range check of the packed copy (ConvParams::ovf contract)
    float *hist = nullptr;  // NCHW [B][C][H][W] clamped x0 of the previous step (StepArgs::hist)
};
void launch_ddpm_update(const UpdateParams &p, int B, hipStream_t s);
// ---- rolling batch: every row at its own position of the schedule (kernels_rows.hip) ----------------
// What StepArgs holds once per step, once per batch ROW: a table of B entries in device memory at an address that is
// constant per session size, refreshed from a pinned ring before every step (so one captured step serves every mix of
// positions). The host stays authoritative for the positions; the device sees only the values of the step at hand.
struct RowArgs {
    uint32_t live;              // 0: idle slot — the update kernels neither read nor write this row
    float nl;                   // noise level fed to the embedding (EmbedParams::noise_level points here, stride sizeof / 4)
    float a, b, c1, c2, c3, sigma;  // as StepArgs, of this row's step
    uint32_t draw;
    uint32_t hist;              // as StepArgs::hist, of this row
    uint64_t image;             // global image id of the Philox key
    uint64_t seed;
    const float *noise;         // this row's [C][HW] slab of the step, or null -> Philox
    float *frame;               // this row's [C][HW] copy of the updated image for this step, or null (as StepArgs::frame)
    float lr_strength;          // low-resolution consistency of this row (launch_lr_project_rows); 0: the row is not held
    uint32_t pad_;
};
static_assert(sizeof(RowArgs) % sizeof(float) == 0, "RowArgs::nl is read with a stride in floats");
struct RowsUpdateParams {
    float *packed = nullptr;    // as UpdateParams
    TDesc state;
    int xoff = 0, C = 0;
    TDesc eps;
    const RowArgs *rows = nullptr;  // [B]
    int *ovf = nullptr;
    float *hist = nullptr;
};
// launch_ddpm_update / launch_x0_predict / launch_update_from_x0 with the row's arguments; bit for bit the same update
// for a live row, nothing touched for an idle one (launch_rows_x0_predict writes zeros into an idle row's slab of x0hat)
void launch_rows_update(const RowsUpdateParams &p, int B, hipStream_t s);
void launch_rows_x0_predict(const RowsUpdateParams &p, float *x0hat, int B, hipStream_t s, bool clamp = true);
void launch_rows_update_from_x0(const RowsUpdateParams &p, const float *x0hat, int B, hipStream_t s);
// sr3_rows_move: one row's slabs into another slot in ONE launch. Each segment is a contiguous run of n floats (the state
// slab, the packed slab, the history slab, the LR image); zero: the source is left as zeros (state and packed copy, as
// sr3_rows_drop leaves them). Source and destination are different rows and never overlap. A segment whose addresses
// and length allow it moves in 16-byte units.
struct RowsMoveSeg { float *src = nullptr; float *dst = nullptr; size_t n = 0; int zero = 0; };
struct RowsMoveParams { RowsMoveSeg seg[4]; int nseg = 0; };
void launch_rows_move(const RowsMoveParams &p, hipStream_t s);
// x <- noise (NCHW buffer or Philox draw 0) into state channels
void launch_init_state(const TDesc &state, int xoff, int C, const float *noise, uint64_t seed,
                       uint64_t image_offset, int B, hipStream_t s);
void launch_philox_normal(uint64_t seed, uint64_t image, uint32_t draw, int n, float *out,
                          hipStream_t s);
// one image's Philox Dropout mask as uint8 [C][H][W] (1 = keep): the stream the masked apply passes evaluate (C % 8 == 0)
void launch_dropout_mask(uint64_t seed, uint64_t image, uint32_t draw, int layer, uint32_t thr, int C, int H, int W,
                         uint8_t *out, hipStream_t s);

// ---- low-resolution consistency (kernels_consist.hip) --------------------------------------------------
// The operators of one size pair (lh, lw) -> (H, W), fp32 on the device: A_v [lh][H] and A_h [lw][W] dense with the band of
// every row in bv / bh ({first, count} pairs), P_v [H][lh], and P_h transposed, PhT [lw][W].
struct LrOps {
    const float *Av = nullptr, *Ah = nullptr, *Pv = nullptr, *PhT = nullptr;
    const int *bv = nullptr, *bh = nullptr;
    int lh = 0, lw = 0, H = 0, W = 0;
};
// What varies between calls. The sampler's kernels read it from device memory (`dyn`), like StepArgs: a captured step
// keeps its launch arguments. Batch row b is held to lr[(row_offset + b) % N] (NCHW [N][C][lh][lw]).
struct LrArgs {
    const float *lr = nullptr;
    uint64_t row_offset = 0;
    int N = 1;
    float strength = 0.f;
};
// host, float64: A [l][r] (Pillow's real bicubic weights of the r -> l resample, rows normalised), P [r][l] = A^T (A A^T)^-1,
// bounds [l][2] (optional); false if the Gram matrix is not positive definite
bool lr_operators(int l, int r, double *A, double *P, int *bounds);
// X <- X + strength * P_v (Y - A_v X A_h^T) P_h^T in place on `planes` = B*C planes of x (NCHW). lds_form: one block per
// plane with the intermediates in LDS (lr_lds_fits); else four launches over scratch (lr_scratch_floats). Both forms run
// the same arithmetic in the same order. dyn (device) overrides val when not null.
constexpr size_t LR_LDS_MAX_BYTES = 64 * 1024;
size_t lr_lds_bytes(const LrOps &o);
bool lr_lds_fits(const LrOps &o);
size_t lr_scratch_floats(int planes, const LrOps &o);
void launch_lr_project(float *x, int planes, int C, const LrOps &o, const LrArgs &val, const LrArgs *dyn, bool lds_form,
                       float *scratch, hipStream_t s);
// The rows form (rolling batch): the same stages on the planes of x [B][C][H][W] whose row is live and held
// (rows[b].live && rows[b].lr_strength != 0), row b against lr_rows[b] ([B slots][C][lh][lw]) at rows[b].lr_strength. A plane
// of any other row is neither read nor written: its block returns before the first barrier (LDS form), every stage skips
// it (scratch form). A held plane carries the bits launch_lr_project gives it.
void launch_lr_project_rows(float *x, int B, int C, const LrOps &o, const float *lr_rows, const RowArgs *rows, bool lds_form,
                            float *scratch, hipStream_t s);
// per image b: sumsq[b] = sum over its C planes of (A img - y)^2 (fp32 residuals, fp64 sum), maxabs[b] = max |A img - y|;
// scratch as for the projection
void launch_lr_residual(const float *img, int B, int C, const LrOps &o, const LrArgs &val, float *scratch, double *sumsq,
                        float *maxabs, hipStream_t s);
// launch_ddpm_update in two halves: the clamped x0 prediction into x0hat (NCHW [B][C][H][W]), and the rest of the update
// reading x0 from there (between them: launch_lr_project on x0hat)
// clamp false: x0 = a x - b eps as it is (the dynamic threshold below takes the clamp's place)
void launch_x0_predict(const UpdateParams &p, float *x0hat, int B, hipStream_t s, bool clamp = true);
void launch_update_from_x0(const UpdateParams &p, const float *x0hat, int B, hipStream_t s);

// ---- dynamic thresholding of the x0 prediction (kernels_threshold.hip) ----------------------------------
// Exact per-image order statistics of |x| over x [B][n] by a radix select: THR_PASSES passes of THR_DIGIT_BITS key bits,
// integer counts only. bins: [B][THR_PASSES][2][THR_BINS] unsigned of scratch (zeroed by the launch).
constexpr int THR_DIGIT_BITS = 8, THR_BINS = 1 << THR_DIGIT_BITS, THR_PASSES = 4;
constexpr size_t THR_BINS_PER_IMAGE = (size_t)THR_PASSES * 2 * THR_BINS;
inline size_t threshold_bins_bytes(int B) { return (size_t)B * THR_BINS_PER_IMAGE * sizeof(unsigned); }
// What (ratio, n) fix, on the host: pos = (double)ratio * (n - 1), k = min(floor(pos), n - 1), k2 = min(k + 1, n - 1),
// frac = (float)(pos - k); and the blocks that share one image. Launch arguments: constant over a sampling call.
struct ThrPlan {
    unsigned k = 0, k2 = 0;
    float frac = 0.f;
    int blocks = 1;
};
ThrPlan threshold_plan(float ratio, int64_t n);
// per image b: lo[b] / hi[b] = the k-th / k2-th smallest |x| (keys: bit patterns of |x| as unsigned integers),
// s[b] = min(max(lo + frac * (hi - lo), 1), max_value); lo, hi, s may each be null
void launch_abs_quantile(const float *x, int B, int64_t n, const ThrPlan &p, float max_value, unsigned *bins, float *lo, float *hi,
                         float *s, hipStream_t st);
// x[b][i] <- clamp(x[b][i], -s[b], s[b]) / s[b]
void launch_threshold_apply(float *x, int B, int64_t n, const float *s, hipStream_t st);

// ---- Philox normal stream (device functions; the kernels that draw from it: kernels_misc.hip, kernels_loss.hip) ----
// Philox4x32-10 (Salmon et al. 2011). CPU twin: oracle/philox.py.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Standard normal number `elem` of draw `draw` for image `image`: counter = (elem/4, draw,
// image_lo, image_hi), key = seed; Box-Muller on the two 24-bit uniform pairs.
__device__ __forceinline__ float philox_normal(uint64_t seed, uint64_t image, uint32_t draw,
                                               uint32_t elem) {
    uint32_t r[4];
    philox4x32_10(elem >> 2, draw, (uint32_t)image, (uint32_t)(image >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    const int pair = (elem >> 1) & 1;
    const float u1 = ((float)(r[2 * pair] >> 8) + 0.5f) * 5.9604644775390625e-08f;      // 2^-24
    const float u2 = ((float)(r[2 * pair + 1] >> 8) + 0.5f) * 5.9604644775390625e-08f;
    const float rad = sqrtf(-2.0f * logf(u1));
    const float th = 6.283185307179586f * u2;
    return (elem & 1) ? rad * sinf(th) : rad * cosf(th);
}

// The four standard normals of one counter: elements 4*quad .. 4*quad+3 of the same stream, each bit-equal to
// philox_normal(seed, image, draw, 4*quad + j) (one Philox evaluation and two Box-Muller pairs instead of four of each).
__device__ __forceinline__ void philox_normal4(uint64_t seed, uint64_t image, uint32_t draw, uint32_t quad, float out[4]) {
    uint32_t r[4];
    philox4x32_10(quad, draw, (uint32_t)image, (uint32_t)(image >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int pair = 0; pair < 2; ++pair) {
        const float u1 = ((float)(r[2 * pair] >> 8) + 0.5f) * 5.9604644775390625e-08f;
        const float u2 = ((float)(r[2 * pair + 1] >> 8) + 0.5f) * 5.9604644775390625e-08f;
        const float rad = sqrtf(-2.0f * logf(u1));
        const float th = 6.283185307179586f * u2;
        out[2 * pair] = rad * cosf(th);
        out[2 * pair + 1] = rad * sinf(th);
    }
}

// ---- Dropout mask stream (same Philox, disjoint counters: c1's top byte is layer + 1 >= 1, the noise stream's draw < 2^24) ----
// One evaluation serves the 8 consecutive channels c .. c+7 (c a multiple of 8) of pixel (y, x) of a [C][H][W] layer:
// counter = (octet = (y*W + x)*(C/8) + c/8, (layer+1) << 24 | draw, image_lo, image_hi), key = seed; channel c + j takes
// the 16-bit field (r[j>>1] >> 16*(j&1)) & 0xffff and is kept iff field >= thr. CPU twin: tests/dropout_ref.py.
__device__ __forceinline__ void dropout_fields8(uint64_t seed, uint64_t image, uint32_t c1, uint32_t octet, uint32_t field[8]) {
    uint32_t r[4];
    philox4x32_10(octet, c1, (uint32_t)image, (uint32_t)(image >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int j = 0; j < 8; ++j) field[j] = (r[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}
// f[j] <- keep ? f[j] * s : 0 for channels c .. c+7 of pixel (y, x) of batch row n (one fp32 multiply, as torch's Dropout)
__device__ __forceinline__ void dropout_apply8(const DropArgs &a, const DropLayer &L, int n, int y, int x, int c, int C, int H,
                                               int W, float (&f)[8]) {
    if (a.mask != nullptr) {
        const uint8_t *m = a.mask + L.base + (((size_t)n * C + c) * H + y) * W + x;
        const size_t plane = (size_t)H * W;
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = m[j * plane] != 0 ? f[j] * a.s : 0.0f;
    } else {
        uint32_t field[8];
        dropout_fields8(a.seed, a.image_offset + (uint64_t)n, L.c1_hi | a.draw, (uint32_t)(y * W + x) * (uint32_t)(C >> 3) + (uint32_t)(c >> 3), field);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = field[j] >= a.thr ? f[j] * a.s : 0.0f;
    }
}

// ---- edge convolutions (kernels_edge.hip) ----------------------------------------------------------
// final_conv = GroupNorm affine + Swish + Conv3x3(C -> Cout <= 4) in one fp32 VALU kernel: x is the raw
// fp32 zero-bordered tensor, scale / shift [B][C] the folded GroupNorm (gn_finalize), wq the weights as
// [9][C][4] (pack_final_conv_weight), out [B][H][W][Cout] unpadded
bool final_conv_supported(int C, int Cout);
void pack_final_conv_weight(const float *oihw, int Cout, int C, float *dst);
void launch_final_conv(const TDesc &x, int B, const float *scale, const float *shift, const float *wq, const float *bias,
                       const TDesc &out, hipStream_t s);

// the same conv in split-f16 mode as a per-pixel [C] x [27 -> 32] MFMA GEMM + a 9-tap gather (kernels_edge.hip)
bool final_conv_mfma_supported(int C, int Cout);
size_t final_conv_mfma_weight_floats(int C);
float pack_final_conv_mfma_weight(const float *oihw, int C, float *dst_as_float);
void launch_final_conv_mfma(const TDesc &x, int B, const float *scale, const float *shift, const float *wfr, float w_unscale,
                            const float *bias, const TDesc &out, hipStream_t s, int *ovf = nullptr);
// downs.0 (Conv3x3 in_channel <= 8 -> Cout) on the packed split-f16 state: xp = [B][H+2][W+2] pixels of
// 16 halfs (8 channels hi | lo; + 16 floats of slack behind the last pixel), wci from pack_conv_in_weight
bool conv_in_supported(int Cin, int Cout, int H, int W);
float pack_conv_in_weight(const float *oihw, int Cout, int Cin, float *dst_as_float);
size_t conv_in_weight_floats(int Cout);
void launch_pack_state(const TDesc &x, int B, float *xp, hipStream_t s, int *ovf);
void launch_conv_in(const float *xp, const float *wci, const float *bias, float w_unscale, int B, const TDesc &out,
                    const TDesc &out_split, int out_f32, double *stats, int stats_slices, int *ovf, hipStream_t s);
// downs.0 in the exact-f32 arithmetic (conv_in_f32_kernel; the shapes of conv_in_supported): x = the fp32 state tensor
// itself (zero border of 1 pixel, x.C >= 8 channels per pixel, those >= Cin zero), w = the parameter's packed copy
// [tap][Cout][w_cin_pad] (pack_conv_weight), out.C = Cout; stats (optional): one slice per 256 pixels, stats_slices = H*W/256.
// A persistent grid of at most CONV_IN_F32_GRID blocks (2 resident blocks of 4 waves per CU)
constexpr int CONV_IN_F32_GRID = 512;
void launch_conv_in_f32(const TDesc &x, const float *w, int w_cin_pad, const float *bias, int B, const TDesc &out,
                        double *stats, int stats_slices, hipStream_t s);

// ---- pre-processing: PIL-exact 8-bit bicubic resize -> sampler input tensor (kernels_pre.hip) ----
} // namespace sr3
#include <vector>
namespace sr3 {
int bicubic_coeffs(int in_size, int out_size, std::vector<int> &bounds, std::vector<int> &kk);   // returns ksize
void launch_resample_h(const uint8_t *in, int B, int H, int Win, int Wout, const int *bounds, const int *kk,
                       int ksize, uint8_t *out, hipStream_t s);
// bounds == nullptr: no vertical resize (Hin == Hout), only the tensor conversion
void launch_resample_v(const uint8_t *in, int B, int Hin, int Hout, int W, const int *bounds, const int *kk,
                       int ksize, float *out_nchw, uint8_t *out_u8, hipStream_t s);

// ---- tensor2img for one value (core/metrics.py:16-42): clamp(-1,1) -> (v+1)/2 -> *255 -> round half to even -> u8;
// shared by the post-processing chain (kernels_post.hip) and the validation metrics (kernels_metrics.hip)
__device__ __forceinline__ uint8_t to_u8(float v) {
    v = fminf(fmaxf(v, -1.f), 1.f);
    const float t = __fmul_rn(__fdiv_rn(__fadd_rn(v, 1.f), 2.f), 255.f);
    return (uint8_t)(int)rintf(t);
}

// ---- post-processing: tensor2img / cv2-style 8-bit linear resize / ArcFace blob (kernels_post.hip) ----
void cv_linear_coeffs(int in_size, int out_size, bool horizontal, std::vector<int> &ofs, std::vector<int> &ab);
void launch_tensor2img(const float *in_nchw, int B, int H, int W, uint8_t *out_hwc, hipStream_t s);
// tab = xofs[Wd] | xa[Wd][2] | yofs[Hd] | yb[Hd][2]; images (optional) = dst / 255 as [B][3][Hd][Wd]
void launch_resize_linear_u8(const uint8_t *src, int B, int Hs, int Ws, int Hd, int Wd, const int *tab, uint8_t *dst,
                             float *images, hipStream_t s);
// src is f x the blob size (f = 1 | 2); out [B][3][Hb][Wb], channels swapped, (avg - mean) * scale
void launch_blob(const uint8_t *src, int B, int Hb, int Wb, int f, float mean, float scale, float *out, hipStream_t s);
void launch_tensor_blob(const float *in_nchw, int B, int H, int W, int Hb, int Wb, float *out, hipStream_t s);

// ---- validation metrics: PSNR sums and SSIM of uint8-quantised image pairs (kernels_metrics.hip) ----
// row b of sr [B][3][H][W] is scored against hr[(row_offset + b) % N] ([N][3][H][W]); H, W >= 11 (the 11x11 window).
// ssd[b] += sum of squared uint8 differences (exact; the caller zeroes ssd on the stream first), ssim[b] =
// core/metrics.py:84-125 in fp64; taps = the 11 normalised Gaussian weights (host). ws: one double per block. Bitwise
// reproducible (no floating-point atomics).
long long metrics_blocks(int B, int H, int W);           // blocks of the tile kernel (the caller bounds them by INT_MAX)
void launch_metrics(const float *sr, const float *hr, int B, int N, int row_offset, int H, int W, const double *taps,
                    double *ws, int64_t *ssd, double *ssim, hipStream_t s);

// ---- denoising loss: q_sample into the UNet's input state, summed L1 / L2 of noise against eps (kernels_loss.hip) ----
// Batch row b noises source image n = (row_offset + b) % N of hr / cond (NCHW [N][C][H][W] / [N][nc][H][W], cond null:
// unconditional) with coefficients a[b], s[b]. Its noise is row j of the NCHW slab `noise`, or (noise == nullptr) the
// Philox stream (seed, image_offset + j, draw 0) in the sampler's element order c*H*W + y*W + x, where j = b, or j = n
// with per_source (one noise image per SOURCE image, whatever the row's level).
struct NoiseRef {
    const float *noise = nullptr;
    uint64_t seed = 0, image_offset = 0;
    int per_source = 0;
};
// x_noisy = a*x + s*n (product, product, sum: each rounded to fp32) -> channels [nc, nc+C) of the interior of `state`
// (cond in [0, nc)), nc + C <= 8; packed (optional): the split-f16 state of conv_in_kernel with pack_state_kernel's range
// flag; x_noisy_out (optional): NCHW [B][C][H][W]. The border of `state` is not touched; its channels behind nc + C, up to
// the next multiple of four, are stored as the zeros the workspace holds there. The packed twin always takes 8 channels,
// those behind nc + C as register zeros: it equals pack_state_kernel's (which reads them from `state`) only because the
// pad channels of `state` stay zero for the life of the workspace — whoever starts writing them must pack from memory.
void launch_q_sample_state(const float *hr, const float *cond, int N, int row_offset, const float *a, const float *s,
                           const NoiseRef &nz, int B, int C, int nc, const TDesc &state, float *packed, int *ovf,
                           float *x_noisy_out, hipStream_t st);
// a[b] = av, s[b] = sv for b < B: the coefficient arrays of launch_q_sample_state when every row shares one level
// (sr3_sample_begin_from), written on the stream from kernel arguments: no host copy, no synchronisation
void launch_fill_pair(float *a, float *s, float av, float sv, int B, hipStream_t st);
// per_image[b] = sum over the image of |n - eps| (loss_type 0) or (n - eps)^2 (1): difference and square in fp32,
// accumulation in fp64, one partial per block added in block order (no floating-point atomics: bitwise reproducible).
// eps: unpadded NHWC [B][H][W][C]; eps_out (optional): eps as NCHW. ws: loss_blocks(H, W) * B doubles.
int loss_blocks(int H, int W);
void launch_denoise_loss(const TDesc &eps, const NoiseRef &nz, int N, int row_offset, int B, int C, int loss_type, double *ws,
                         double *per_image, float *eps_out, hipStream_t st);

} // namespace sr3
