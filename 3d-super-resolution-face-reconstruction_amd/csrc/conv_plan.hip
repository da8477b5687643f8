// libsr3hip.so — the dispatch decisions (conv_plan.h): which kernel a conv runs on, which split-K form, which buffers; the
// form of the GroupNorm apply pass in front of it; and the environment switches those decisions read. Host arithmetic
// only: no kernel, no HIP runtime call. The launchers are in kernels_conv.hip / kernels_wino.hip / kernels_gn_res.hip.
#include "conv_plan.h"

#include <algorithm>
#include <mutex>

namespace sr3 {

// ---- environment switches: ONE table ----------------------------------------------------------------------------------
// (SR3_THRESHOLD_BLOCKS, the sixteenth, is read by kernels_threshold.hip where it plans a selection)
namespace {
struct SwitchDef { const char *name; int dflt; };
const SwitchDef kSwitches[SW_COUNT] = {
    /* SW_NO_GRAPH */ {"SR3_NO_GRAPH", 0},
    /* SW_NO_HALO */ {"SR3_NO_HALO", 0},
    /* SW_HALO_SPLITS */ {"SR3_HALO_SPLITS", -1},
    /* SW_NO_INPLACE_SPLIT */ {"SR3_NO_INPLACE_SPLIT", 0},
    /* SW_NO_WINOGRAD */ {"SR3_NO_WINOGRAD", 0},
    /* SW_NO_GN_WINO */ {"SR3_NO_GN_WINO", 0},
    /* SW_NO_WINO_GEMM_OUT */ {"SR3_NO_WINO_GEMM_OUT", 0},
    /* SW_WINO_GEMM_OUT_FORCE */ {"SR3_WINO_GEMM_OUT_FORCE", 0},
    /* SW_NO_WINO_FUSED_ROWS */ {"SR3_NO_WINO_FUSED_ROWS", 0},
    /* SW_WINO_FUSED_ROWS_FORCE */ {"SR3_WINO_FUSED_ROWS_FORCE", 0},
    /* SW_NO_UP2_WINO */ {"SR3_NO_UP2_WINO", 0},
    /* SW_UP2_WINO_FORCE */ {"SR3_UP2_WINO_FORCE", 0},
    /* SW_NO_GN_RES1X1 */ {"SR3_NO_GN_RES1X1", 0},
    /* SW_GN_RES1X1_FORCE */ {"SR3_GN_RES1X1_FORCE", 0},
    /* SW_NO_CONV_IN_F32 */ {"SR3_NO_CONV_IN_F32", 0},
};
} // namespace

int env_switch_now(Switch s) { return env_int(kSwitches[s].name, kSwitches[s].dflt); }

int env_switch(Switch s) {
    static std::once_flag once[SW_COUNT];
    static int value[SW_COUNT];
    std::call_once(once[s], [s] { value[s] = env_switch_now(s); });
    return value[s];
}

FormSwitch form_switch(Form f) {
    static const Switch pair[][2] = {{SW_NO_WINO_GEMM_OUT, SW_WINO_GEMM_OUT_FORCE}, {SW_NO_WINO_FUSED_ROWS, SW_WINO_FUSED_ROWS_FORCE},
                                     {SW_NO_UP2_WINO, SW_UP2_WINO_FORCE}, {SW_NO_GN_RES1X1, SW_GN_RES1X1_FORCE}};
    return {env_switch(pair[f][0]) != 0, env_switch(pair[f][1]) != 0};
}

// downs.0 on conv_in_f32_kernel (kernels_edge.hip) instead of the generic kernel: the exact-f32 arithmetic, a shape of
// conv_in_supported, SR3_NO_CONV_IN_F32 unset. Asks nothing of B (the same answer in the batch-invariant mode)
bool conv_in_f32_gate(bool split_arith, int Cin, int Cout, int H, int W) {
    return !split_arith && conv_in_supported(Cin, Cout, H, W) && env_switch(SW_NO_CONV_IN_F32) == 0;
}

// ---- batch-invariant mode: the planning batch of the calling thread ----------------------------------
// Every decision below that asks "is there enough work for this form?" reads plan_b(B) in place of B; every rule that
// says "the kernel can run this shape" is evaluated on one image, so that what holds at B = 1 holds at every B; a limit
// on the real B (tile counters, 32-bit offsets) becomes ConvPlan::batch_limit, the mode's maximum batch.
namespace { thread_local int g_plan_batch = 0; }
int plan_batch() { return g_plan_batch; }
int set_plan_batch(int P) { const int prev = g_plan_batch; g_plan_batch = P > 0 ? P : 0; return prev; }

int splitk_reduce_tp(int HWo) { const int tp = HWo / 64; return tp < 1 ? 1 : tp; }
int splitk_stats_slices(int HWo, int Cout) {
    const int tp = splitk_reduce_tp(HWo);
    return ((HWo % tp) == 0 && Cout <= 1024 && (Cout & 3) == 0) ? HWo / tp : 0;
}

// ---- the dispatch plan ---------------------------------------------------------------------------------------------
Tile conv_tile_choice(long M, int Cout) {
    auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((Cout + bn - 1) / bn); };
    const long want = 512;  // 256 CUs x 2 resident blocks
    const Tile t32 = {CK_GENERIC_128x32, 128, 32}, t64 = {CK_GENERIC_128x64, 128, 64}, t6464 = {CK_GENERIC_64x64, 64, 64};
    if (Cout <= 32) return t32;
    if (Cout <= 64 || (Cout % 128) != 0) return blocks(128, 64) >= want ? t64 : t6464;
    if (blocks(128, 128) >= want) return Tile{CK_GENERIC_128x128, 128, 128};
    return blocks(128, 64) >= want ? t64 : t6464;
}
static long tile_count(const Tile &t, long M, int Cout) { return ((M + t.bm - 1) / t.bm) * ((Cout + t.bn - 1) / t.bn); }

// K-splits of the generic kernel for small problems (1 = none); Cin per tap, multiple of 32
static int conv_splits(long M, int Cout, int Cin) {
    if (Cout & 3) return 1;
    const long tiles = tile_count(conv_tile_choice(M, Cout), M, Cout);
    const int nchunk = Cin / 32;            // K-steps of 32 channels (BK of kernels_conv.hip)
    // (tuned on B = 1 at 128x128 and config 1, with the in-place fix-up: profiles/README.md finding 42)
    constexpr int tmin = 256, target = 256, chmin = 2;
    if (tiles >= tmin || nchunk < 2 * chmin) return 1;
    int s = 2;
    while (s * 2 <= nchunk / chmin && tiles * s * 2 <= target && s < 16) s *= 2;
    return s;
}

// SR3_NO_HALO=1 (product safety switch): no x-halo kernel anywhere — and therefore no F8C path and no halo split-K
static bool halo_off() { return env_switch(SW_NO_HALO) != 0; }

// Deep-K 3x3 / stride-1 split-f16 convs over FEW output tiles (the 8x8 level at B = 64: M = 4096 pixels, 512 channels):
// instead of 64x64 tiles of the generic kernel (LDS traffic per MFMA twice that of a 128x128 tile) they run on the
// 128x128 x-halo tile with the K range split over `return value` blocks per tile, added IN PLACE by the block that
// arrives last (conv3x3_halo_h3, end of the consumer path) — no reduce pass, statistics in the unsplit layout (one
// slice per 128-row tile, or one per image where a tile covers several whole images). 0 or 1: not for this shape.
// Assumes ks 3, stride 1, prec 1, pad 1 (conv_plan checks them).
// M: the pixels the gates count (the planning batch's in the batch-invariant mode, where whole tiles per IMAGE are asked for)
static int conv_halo_splits(long M, int H, int W, int Cout, int Cin) {
    const int force = env_switch(SW_HALO_SPLITS);               // product switch: 0 off, 2 | 4 forced
    if (force == 0 || halo_off()) return 0;
    const int HWo = H * W;
    if (W < 8 || (M % 128) || (Cout % 128) || (Cin % 32)) return 0;
    const int seg = W < 128 ? W : 128;
    if ((W % seg) || (128 % seg)) return 0;
    if (HWo >= 128 ? (HWo % 128) != 0 : ((128 % HWo) != 0 || (HWo % 32) != 0)) return 0;
    if (plan_batch() > 0 && HWo < 128) return 0;        // (a tile over several whole images does not exist at B = 1)
    if (conv_tile_choice(M, Cout).generic != CK_GENERIC_64x64) return 0;   // enough 128-row tiles already: no split needed
    const long tiles = (M / 128) * (Cout / 128);
    const int nchunk = Cin / 32;
    if (tiles < 64 || tiles > CONV_TILE_COUNTERS || nchunk < 8) return 0;
    int sp = 2;
    while (sp * 2 <= nchunk / 4 && tiles * sp * 2 <= 512 && sp < 4) sp *= 2;      // (the reduce-scatter tail handles 2 or 4 splits)
    if (force == 2 || force == 4) sp = force;
    return sp;
}

// preconditions of the x-halo kernel for tile height BM: p after the phase transform, splits = the plan's
static bool halo_ok(const ConvParams &p, int splits, int BM, int segmin, int bn, bool split_ok = false) {
    if (halo_off() || p.prec != 1 || (p.ks != 3 && p.ks != 2) || p.stride != 1 || p.up2 || (splits > 1 && !split_ok) || p.in0.pad != 1) return false;
    const int W = p.Wout;
    if (p.in0.W != W || p.in0.H != p.Hout) return false;
    const int seg = W < BM ? W : BM;
    if (seg < segmin || (W % seg) || (BM % seg)) return false;
    // no masking anywhere in the halo kernels: whole tiles in M (batch-invariant mode: in every image, so that the answer
    // at B = 1 is the answer) and (for the tile width bn the caller picks) in N
    const long M = (long)(plan_batch() > 0 ? 1 : p.B) * p.Hout * W;
    return (M % BM) == 0 && (p.out.C % bn) == 0 && (!p.in2.p || (p.in2.C % 32) == 0) && (!p.in2b.p || (p.in2b.C % 32) == 0);
}

// ---- Winograd gates (the kernels are in kernels_wino.hip) ----
// one-pass kernel: 64x64 pixels and up, whole strips per tile row, whole channel blocks, and enough blocks to fill the
// chip (fewer: the direct kernel, whose smaller tiles spread further)
static bool wino_fused_shape(int B, int H, int W, int Cin, int Cout) {
    if (H * W < 4096 || (H & 1) || (W % (2 * WINO_FUSED_TILES)) || Cin < WINO_FUSED_CIN || (Cin % 32) || (Cout % WINO_FUSED_BN)) return false;
    const uint64_t blocks = (uint64_t)plan_b(B) * (H / 2) * (W / (2 * WINO_FUSED_TILES)) * (Cout / WINO_FUSED_BN);
    return blocks >= WINO_FUSED_MIN_BLOCKS;
}

// shape rule (3x3 / stride 1 / prec 0 convs): false also under SR3_NO_WINOGRAD=1
static bool wino_shape(int B, int H, int W, int Cin, int Cout) {
    if (env_switch(SW_NO_WINOGRAD) != 0 || B <= 0) return false;   // product switch
    if (wino_fused_shape(B, H, W, Cin, Cout)) return true;
    if ((H & 1) || (W & 1) || H * W > 1024 || Cin < WINO_MIN_CIN || (Cin % 32) || (Cout % 64)) return false;
    // few tiles (a single 128x128 image: 256 at its 32x32 level): the three dependent passes cost more latency than the
    // MACs they save (B = 1 step 1.99 -> 2.27 ms with every level in Winograd form); B = 64 at 8x8 is 1024 tiles and gains
    const uint64_t tpi = (uint64_t)(H / 2) * (W / 2);
    if ((uint64_t)plan_b(B) * tpi < WINO_MIN_TILES) return false;
    // the LDS-DMA and epilogue addressing of the position GEMMs uses 32-bit byte offsets inside one position's plane
    // (batch-invariant mode: asked of one image; the real batch's bound is ConvPlan::batch_limit)
    return (plan_batch() > 0 ? 1 : (uint64_t)B) * tpi * (uint64_t)(Cin > Cout ? Cin : Cout) * 4 < (1ull << 32);
}

// the Winograd form this conv runs in, CK_COUNT: none (the direct kernels)
static ConvKernel wino_form(const ConvParams &p) {
    if (p.prec != 0 || p.ks != 3 || p.stride != 1 || p.up2 || p.phases != 1 || p.f8) return CK_COUNT;
    if (p.out_split.p || !p.out_f32 || p.resid_split) return CK_COUNT;
    if (p.in0.pad != 1 || p.in0.H != p.Hout || p.in0.W != p.Wout) return CK_COUNT;
    if (p.in1.p && (p.in1.pad != 1 || p.in1.H != p.Hout || p.in1.W != p.Wout)) return CK_COUNT;
    if (p.in2.p && !p.w2) return CK_COUNT;
    const int Cin = p.in0.C + (p.in1.p ? p.in1.C : 0);
    if (!wino_shape(p.B, p.Hout, p.Wout, Cin, p.out.C)) return CK_COUNT;
    if (wino_fused_shape(p.B, p.Hout, p.Wout, Cin, p.out.C)) {
        // one input tensor: the engine concatenates x || skip in the GroupNorm apply pass that writes the conv's input,
        // so no caller hands these convs a second tensor (one that does gets the direct kernel)
        if (!p.w_wino_f || p.in1.p) return CK_COUNT;
        // the statistics slices must be whole strips or 2 | 4 equal parts of one
        const int spi = (p.Hout / 2) * (p.Wout / (2 * WINO_FUSED_TILES));
        if (p.stats == nullptr) return CK_WINO_ONE_PASS;
        if (p.stats_slices <= 0 || (p.stats_slices % spi)) return CK_COUNT;
        const int spb = p.stats_slices / spi;
        return (spb == 1 || spb == 2 || spb == 4) ? CK_WINO_ONE_PASS : CK_COUNT;
    }
    if (!p.w_wino || !p.wino_ws) return CK_COUNT;
    const int tiles = (p.Hout >> 1) * (p.Wout >> 1);
    return (p.stats == nullptr || (p.stats_slices > 0 && (tiles % p.stats_slices) == 0)) ? CK_WINO_THREE_PASS : CK_COUNT;
}

// second form of the three-pass plan (kernels_wino.hip, wino_gemm_out_kernel): output channels per block, 0 = the
// position GEMMs + wino_output_kernel. Preconditions: whole channel blocks (wino_shape: Cout % 64 == 0), statistics
// slices of 16 | 32 tiles (what a block's waves hold whole). Tuning (profiles/README.md finding 86): enough blocks of
// 64 tiles to fill the chip, as each runs all 16 positions, and Cin small enough for M's traffic to matter
static int wino_gemm_out_bn(const ConvParams &p, int Cin) {
    const FormSwitch sw = form_switch(FORM_WINO_GEMM_OUT);
    if (sw.off) return 0;
    const int tpi = (p.Hout >> 1) * (p.Wout >> 1), Cout = p.out.C;
    if (p.stats) {
        const int tps = tpi / p.stats_slices;
        if (tps != 16 && tps != 32) return 0;
    }
    // the epilogue addresses the zero-bordered output (and the residual, same geometry) with 32-bit byte offsets
    // (batch-invariant mode: every activation tensor of a call within the mode's maximum batch is below 4 GiB)
    if ((uint64_t)p.out.floats(plan_batch() > 0 ? 1 : p.B) * 4 >= (1ull << 32)) return 0;
    const int bn = (Cout % 128) == 0 ? 128 : 64;
    if (sw.force) return bn;
    const long blocks = ((plan_b(p.B) * tpi + WINO_GEMM_OUT_TILES - 1) / WINO_GEMM_OUT_TILES) * (Cout / bn);
    return (blocks >= WINO_GEMM_OUT_MIN_BLOCKS && Cin <= WINO_GEMM_OUT_MAX_CIN) ? bn : 0;
}

// third form of the three-pass plan: the one-pass kernel with R = 2 | 4 tile rows per block (kernels_wino.hip,
// wino_fused_kernel<R>), 0 = not taken. Preconditions: one input tensor (the engine's GroupNorm pass concatenates) and
// the fragment-major weights; a width of 32 | 16 (R = 2 | 4: a block's 32 tiles are R whole tile rows) and whole blocks
// (H % 2R == 0); whole 32-channel K-steps and 64-channel blocks; statistics slices that are a whole block or 2 | 4
// equal parts of one; 32-bit offsets of the input DMA (bit 31 of a lane's offset switches an instruction off) and of
// the weight loads (the four planes of a wave). Tuning: WINO_FUSED_ROWS_MIN_BLOCKS (per level) and, at a width of 16,
// WINO_FUSED_ROWS_MAX_CIN_16.
static int wino_fused_rows(const ConvParams &p, int Cin) {
    const FormSwitch sw = form_switch(FORM_WINO_FUSED_ROWS);
    if (sw.off || p.in1.p || !p.w_wino_f) return 0;
    const int H = p.Hout, W = p.Wout, Cout = p.out.C;
    const int R = W == 32 ? 2 : W == 16 ? 4 : 0;
    if (R == 0 || (H % (2 * R)) || (Cin % 32) || (Cout % WINO_FUSED_BN)) return 0;
    const int bpi = (H / 2) * (W / 2) / WINO_FUSED_TILES;                    // blocks per image
    if (p.stats) {
        if (p.stats_slices <= 0 || (p.stats_slices % bpi)) return 0;
        const int spb = p.stats_slices / bpi;
        if (spb != 1 && spb != 2 && spb != 4) return 0;
    }
    if (((uint64_t)(2 * R + 1) * (W + 2) + W + 1) * (uint64_t)Cin * 4 + 128 >= (1ull << 31) || (uint64_t)4 * Cout * Cin * 4 >= (1ull << 31)) return 0;
    if (sw.force) return R;
    const int min_blocks = R == 2 ? WINO_FUSED_ROWS_MIN_BLOCKS : WINO_FUSED_ROWS_MIN_BLOCKS_16;
    if (R == 4 && Cin > WINO_FUSED_ROWS_MAX_CIN_16) return 0;       // (deeper K: the position GEMMs are within 0.9)
    const uint64_t blocks = (uint64_t)plan_b(p.B) * bpi * (Cout / WINO_FUSED_BN);
    return (min_blocks > 0 && blocks >= (uint64_t)min_blocks) ? R : 0;
}

ConvParams phase_form(const ConvParams &p_in) {
    ConvParams p = p_in;
    if (!p.up2) return p;
    p.ks = 2; p.stride = 1; p.up2 = 0;
    p.Hout = p_in.Hout / 2; p.Wout = p_in.Wout / 2;
    p.out_step = 2;
    p.phases = 4;
    p.phase_w_stride = (size_t)4 * p.out.C * (p.in0.C + (p.in1.p ? p.in1.C : 0));
    return p;
}

const char *conv_kernel_name(ConvKernel k) {
    static const char *const names[CK_COUNT] = {"wino_one_pass", "wino_three_pass", "halo_f8c", "halo_128x128_seg32", "halo_128x128_seg8",
                                                "halo_128x64", "generic_128x32", "generic_128x64", "generic_64x64", "generic_128x128"};
    return (unsigned)k < (unsigned)CK_COUNT ? names[k] : "?";
}

// Upsample convs (prec 0): tile rows per block of wino_up2_kernel (kernels_wino.hip), 0 = the four phase convs of `direct`.
// Preconditions: one f32 input with its zero border, f32 output only, nothing fused but the biases; whole 32-channel
// blocks on both sides; a low-resolution width of 16, 32 or a multiple of 64 and whole blocks of 32 tiles; an unsplit
// direct plan; statistics absent or in the direct plan's slices of 128 pixels (one phase of a block: widths 16, 32, 64; two
// strips of a tile row, run by one block: multiples of 128) or of 64 (half of that; few-tile shapes); 32-bit offsets of the input DMA (as wino_fused_kernel: bit
// 31 of a lane's offset switches an instruction off) and of the weight loads (the nine planes of a phase).
// Tuning: UP2_WINO_MIN_BLOCKS.
static int up2_wino_rows(const ConvParams &p, const ConvPlan &direct) {
    const FormSwitch sw = form_switch(FORM_UP2_WINO);
    if (sw.off || !p.up2 || p.prec != 0 || p.f8 || p.ks != 3 || p.stride != 1 || !p.w_up_wino) return 0;
    if (p.in1.p || p.in2.p || p.resid.p || p.out_split.p || !p.out_f32 || p.in0.pad != 1) return 0;
    const int Hl = p.in0.H, Wl = p.in0.W, Cin = p.in0.C, Cout = p.out.C;
    if (p.B <= 0 || 2 * Hl != p.Hout || 2 * Wl != p.Wout || (Cin % 32) || (Cout % UP2_WINO_BN)) return 0;
    const int R = Wl == 16 ? 4 : Wl == 32 ? 2 : (Wl % 64) == 0 ? 1 : 0;
    if (R == 0 || (Hl % (2 * R))) return 0;
    if (direct.split != CS_NONE || direct.error) return 0;
    if (p.stats) {
        if ((direct.tile_m != 128 && direct.tile_m != 64) || p.stats_slices != 4 * (Hl * Wl / direct.tile_m)) return 0;
        if (direct.tile_m == 128 && Wl > 64 && (Wl % 128)) return 0;
    }
    if (((uint64_t)10 * (Wl + 2) + 70) * (uint64_t)Cin * 4 >= (1ull << 31) || (uint64_t)9 * Cout * Cin * 4 >= (1ull << 31)) return 0;
    const uint64_t blocks = (uint64_t)plan_b(p.B) * ((uint64_t)Hl * Wl / (4 * UP2_WINO_TILES)) * (Cout / UP2_WINO_BN);
    return (sw.force || blocks >= (uint64_t)UP2_WINO_MIN_BLOCKS) ? R : 0;
}

static ConvPlan conv_plan_direct(const ConvParams &p_in);
ConvPlan conv_plan(const ConvParams &p_in) {
    ConvPlan plan = conv_plan_direct(p_in);
    plan.up2_wino = up2_wino_rows(p_in, plan);
    return plan;
}

static ConvPlan conv_plan_direct(const ConvParams &p_in) {
    const ConvParams p = phase_form(p_in);
    const int Cout = p.out.C, Cin = p.in0.C + (p.in1.p ? p.in1.C : 0);
    const int HWo = p.Hout * p.Wout;                 // pixels of one image (and phase)
    const long M = (long)p.B * HWo;
    // what the performance gates count: the planning batch's pixels in the batch-invariant mode, else the call's
    const bool inv = plan_batch() > 0;
    const long Mp = plan_b(p.B) * HWo;
    const Tile t = conv_tile_choice(Mp, Cout);
    ConvPlan plan;
    // batch-invariant mode: a limit on the real batch never changes the form, it bounds the batch (and fails a launch past it)
    auto limit = [&](uint64_t b) {
        if (!inv) return;
        const long l = (long)std::min<uint64_t>(b, 1u << 30);
        if (plan.batch_limit == 0 || l < plan.batch_limit) plan.batch_limit = l;
        if (p.B > l) plan.error = "batch-invariant mode: the batch exceeds the mode's maximum (sr3_max_batch)";
    };
    plan.phases = p.phases;
    plan.tile_m = t.bm; plan.tile_n = t.bn;
    // split-K of the generic kernel: in place on the 64x64 tile where every tile has a counter, whole tiles per image (the
    // statistics slices are per M-tile of an image) and in N (nothing is masked in the fix-up); else conv + reduce kernel
    const int no_inplace = env_switch(SW_NO_INPLACE_SPLIT);
    const int gs = p.part ? conv_splits(Mp, Cout, Cin) : 1;
    const bool inplace = gs > 1 && p.tile_cnt && !no_inplace && t.generic == CK_GENERIC_64x64 && (HWo % t.bm) == 0 && (Cout % t.bn) == 0 &&
                         tile_count(t, inv ? Mp : M, Cout) * p.phases <= CONV_TILE_COUNTERS;
    // fused statistics: one slice per M-tile of an image (an in-place split conv leaves the same slices as an unsplit
    // one; every kernel of one output shape uses the same tile height), a two-kernel split one slice per reduce block
    plan.stats_slices = p.phases * ((gs > 1 && !inplace) ? splitk_stats_slices(HWo, Cout) : (HWo % t.bm) == 0 ? HWo / t.bm : 0);

    const ConvKernel wino = wino_form(p);
    if (wino != CK_COUNT) {
        plan.kernel = wino;
        if (wino == CK_WINO_THREE_PASS)
            limit(((1ull << 32) - 1) / ((uint64_t)(p.Hout / 2) * (p.Wout / 2) * (uint64_t)std::max(Cin, Cout) * 4));
        plan.needs_wino_frag = wino == CK_WINO_ONE_PASS;       // (U and M never leave the CU)
        if (wino == CK_WINO_THREE_PASS) {
            plan.wino_ws_floats = (size_t)16 * p.B * (p.Hout / 2) * (p.Wout / 2) * (Cin + Cout);
            plan.wino_fused_rows = wino_fused_rows(p, Cin);
            plan.wino_gemm_out = plan.wino_fused_rows ? 0 : wino_gemm_out_bn(p, Cin);
        }
        return plan;
    }
    auto split = [&](ConvSplit kind, int splits) {
        plan.split = kind; plan.splits = splits;
        plan.part_floats = (size_t)p.phases * splits * M * Cout;
        plan.needs_counters = kind != CS_REDUCE;
    };
    if (p.prec == 1 && p.ks == 3 && p.stride == 1 && p.phases == 1 && p.part != nullptr && p.tile_cnt != nullptr && p.in0.pad == 1 &&
        p.in0.W == p.Wout && p.in0.H == p.Hout && !p.no_halo_split) {
        const int hs = conv_halo_splits(Mp, p.Hout, p.Wout, Cout, Cin);
        const bool stats_ok = p.stats == nullptr || p.stats_slices == (HWo >= 128 ? HWo / 128 : 1);
        const bool seg32 = halo_ok(p, hs, 128, 32, 128, true);
        if (hs > 1 && stats_ok && (seg32 || halo_ok(p, hs, 128, 8, 128, true))) {
            plan.kernel = seg32 ? CK_HALO_128x128_SEG32 : CK_HALO_128x128_SEG8;
            plan.tile_m = plan.tile_n = 128;
            split(CS_INPLACE_HALO, hs);
            if (inv) limit((uint64_t)CONV_TILE_COUNTERS / ((uint64_t)(HWo / 128) * (Cout / 128)));     // (HWo >= 128 there)
            return plan;
        }
    }
    if (gs > 1) split(inplace ? CS_INPLACE : CS_REDUCE, gs);
    if (gs > 1 && inplace) limit((uint64_t)CONV_TILE_COUNTERS / ((uint64_t)tile_count(t, HWo, Cout) * p.phases));
    if (p.f8) {
        // the caller asked conv_f8_supported() first and wrote the input / passes the weights in the F8C format
        // (conv_f8_supported is this plan's answer; a mismatch is a library bug, reported through the API's error
        // path — nothing is launched, the process is never aborted)
        if (!(p.prec == 1 && p.ks == 3 && p.phases == 1 && gs <= 1 && halo_ok(p, gs, 128, 8, 128)))
            plan.error = "internal: fp8 correction products requested for a conv the F8C kernel does not support";
        plan.kernel = CK_HALO_F8C;
        plan.tile_m = plan.tile_n = 128;
        return plan;
    }
    plan.kernel = t.generic;
    if (t.generic == CK_GENERIC_128x64 && halo_ok(p, gs, 128, 32, 64)) plan.kernel = CK_HALO_128x64;
    else if (t.generic == CK_GENERIC_128x128 && halo_ok(p, gs, 128, 32, 128)) plan.kernel = CK_HALO_128x128_SEG32;   // rows of 32+ pixels: one row segment per wave (ONESEG)
    else if (t.generic == CK_GENERIC_128x128 && halo_ok(p, gs, 128, 8, 128)) plan.kernel = CK_HALO_128x128_SEG8;
    return plan;
}

ConvPlan conv_plan_offered(int B, int H, int W, int Cin, int Cout, int ks, int stride, int up2, int prec, bool f8, bool stats) {
    static float buf;                    // (never dereferenced: a plan only asks whether a buffer is offered)
    static unsigned cnt;
    static double st;
    const int pad = ks / 2, Hv = H << up2, Wv = W << up2;
    ConvParams p;
    p.in0.p = &buf; p.in0.C = Cin; p.in0.H = H; p.in0.W = W; p.in0.pad = 1;
    p.B = B; p.ks = ks; p.stride = stride; p.up2 = up2; p.prec = prec; p.f8 = f8 ? 1 : 0;
    p.Hout = (Hv + 2 * pad - ks) / stride + 1; p.Wout = (Wv + 2 * pad - ks) / stride + 1;
    p.out.p = &buf; p.out.C = Cout; p.out.H = p.Hout; p.out.W = p.Wout;
    p.w = p.w_wino = p.w_wino_f = p.w_up_wino = &buf;
    p.part = p.wino_ws = &buf;
    p.tile_cnt = &cnt;
    if (stats) {
        p.stats_slices = conv_plan(p).stats_slices;       // (the layout does not depend on what is offered beyond part / tile_cnt)
        if (p.stats_slices) p.stats = &st;
    }
    return conv_plan(p);
}

// F8C ("f16f8" mode): 3x3 / stride-1 split-f16 convs that run on the 128x128 x-halo tile without split-K at the 32x32- and
// 16x16-pixel levels — the MFMA-bound shapes, where the 32x32 consumers with the corrections on the fp8 path measured
// 14-20 % faster than the f16x3 kernel (profiles/README.md finding 64); the 64x64- and 128x128-pixel levels are bound by
// operand movement and gain nothing. Callers format the conv's input accordingly.
bool conv_f8_supported(int B, int H, int W, int Cout, int Cin) {
    constexpr int maxhw = 1024;         // pixels of one image: the 32x32 level and below
    const int HWo = H * W;
    if ((Cin % 32) || HWo > maxhw || HWo < 128 || (HWo % 128)) return false;
    // where the f16x3 plan runs the conv unsplit on a 128x128 x-halo tile, the F8C kernel can take its place
    const ConvPlan f16 = conv_plan_offered(B, H, W, Cin, Cout, 3, 1, 0, 1, false, false);
    return f16.split == CS_NONE && (f16.kernel == CK_HALO_128x128_SEG32 || f16.kernel == CK_HALO_128x128_SEG8);
}

// ---- the GroupNorm apply pass in front of a conv ---------------------------------------------------------------------
GnRoute gn_route(const TDesc &a, const TDesc &b, int B, const StatsRef &sa, const StatsRef &sb) {
    if (!gn_stats_fused(b, sa, sb)) return GN_FOLDED;
    // bytes the pass moves (read + write, 4 B per element each way): above ~200 MB the one-item-per-thread
    // streaming kernel behind a separate finalize launch is faster than the folded form (A/B on one box,
    // profiles/README.md); below it the launch saved and the shorter critical path win
    const long Bp = plan_b(B);           // (batch-invariant mode: the planning batch's pass)
    const double pass_bytes = 8.0 * Bp * a.H * a.W * (a.C + (b.p ? b.C : 0));
    constexpr double fold_max = 200.0 * 1e6;
    // few images with many statistics slices (a single 128x128 image on 64x64 tiles leaves 256): the folded form's
    // prologue walks them in 12-16 dependent round trips in EVERY block (12-23 us per apply at B = 1); the
    // per-(image, group) finalize launch takes one round trip
    const bool many_slices = Bp * 4 < 128 && std::max(sa.slices, b.p ? sb.slices : 0) >= 64;
    return (pass_bytes > fold_max || many_slices) ? GN_FINALIZE_ROWS : GN_FOLDED;
}

bool gn_pass_writes_u(bool split_arith, const ConvPlan &pl, bool raw_wanted, int in_split) {
    return !gn_wino_off() && !split_arith && !raw_wanted && !in_split && pl.kernel == CK_WINO_THREE_PASS && !pl.wino_fused_rows;
}

bool GnResGate::takes() const {
    if (!valid) return false;
    const FormSwitch sw = form_switch(FORM_GN_RES1X1);
    return (tuned || sw.force) && !sw.off;
}

constexpr int GN_RES1X1_MIN_HW = 32 * 32;      // pixels of one image: the 32x32 level and above
constexpr long GN_RES1X1_MIN_BLOCKS = 1024;
GnResGate gn_res1x1_gate(int prec, bool has_res, bool direct, bool raw_wanted, int in_split, int mode, bool conv1_reads_u,
                         int conv1_fused_rows, const ConvPlan &pl2, int B, int H, int W, int C0, int C1, int Cout) {
    GnResGate g;
    const bool wino2 = pl2.kernel == CK_WINO_ONE_PASS || pl2.kernel == CK_WINO_THREE_PASS;
    // (conv1 on wino_fused_kernel<4>: the kernel has not been run behind that form)
    g.valid = prec == 0 && has_res && direct && !raw_wanted && !in_split && mode == 2 && !conv1_reads_u && conv1_fused_rows != 4 &&
              wino2 && gn_res1x1_shape_ok(H, W, C0, C1, Cout);
    if (g.valid) {
        const long blocks = (plan_b(B) * H * W / 128) * (Cout / gn_res1x1_bn(B, H, W, Cout));
        g.tuned = (long)H * W >= GN_RES1X1_MIN_HW && blocks >= GN_RES1X1_MIN_BLOCKS;
    }
    return g;
}

// the engine's gate with everything that is no property of a single op granted: a res_conv over unsplit x / skip, mode 2,
// conv1 reading the plain activated tensor and a Winograd plan for conv2 (a made-up one: the op has no conv2)
GnResGate gn_res1x1_gate_op(int prec, int B, int H, int W, int C0, int C1, int Cout) {
    ConvPlan wino;
    wino.kernel = CK_WINO_ONE_PASS;
    return gn_res1x1_gate(prec, true, true, false, 0, 2, false, 0, wino, B, H, W, C0, C1, Cout);
}

} // namespace sr3

