// libsr3hip.so — C-ABI (include/sr3hip.h), context, UNet graph builder and the DDPM sampler loop.
//
// The graph builder restates UNet.__init__ (reference model/sr/sr3_modules/unet.py:161-233) so the
// parameter names are the reference's state_dict keys; forward() restates UNet.forward (:235-265)
// and ResnetBlock/SelfAttention.forward (:105-110, :123-142) as a sequence of HIP launches.
#include "../../include/sr3hip.h"
#include "sr3_internal.h"
#include "conv_plan.h"

#include <limits.h>
#include <math.h>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <string>
#include <tuple>
#include <vector>

using namespace sr3;

namespace {

thread_local std::string g_err;
thread_local std::string g_warn;

int fail(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

#define HIP_OK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return fail("%s: %s", #expr, hipGetErrorString(e_));          \
    } while (0)

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

enum ParamKind { P_CONV, P_PLAIN };

struct Param {
    std::string name;
    std::vector<int64_t> shape;
    ParamKind kind = P_PLAIN;
    int cout = 0, cin = 0, ks = 0, cin_pad = 0;  // P_CONV
    float *dev = nullptr;                        // device storage (kernel layout)
    float *dev_split = nullptr;                  // P_CONV: split-f16 copy (prec 1), same size
    float *dev_f8 = nullptr;                     // P_CONV 3x3: F8C copy of dev_split ("f16f8" mode; made on demand)
    float *dev_wino = nullptr;                   // P_CONV 3x3 (wino_weights): G g G^T [16][cout][cin_pad] for prec 0
    float *dev_wino_f = nullptr;                 // the same in fragment-major order [16][cin_pad/8][cout][8] for the
                                                 // one-pass kernel: made when a workspace plan runs the conv there
    float *dev_up_wino = nullptr;                // Upsample convs (up2_wino_weights): sub-pixel Winograd F(2x2, 2x2) weights
                                                 // [4][9][cin_pad/8][cout][8] for prec 0 (make_up2_wino_weights)
    float w_unscale = 1.0f;
    bool keep_host = false;                      // part of a fused (conv2 + res_conv) launch
    bool up_phase = false;                       // Upsample conv: stored as 4 sub-pixel phases x 2x2 taps
    std::vector<float> host;                     // packed fp32 weights / bias kept for re-scaling; empty after a device
                                                 // refresh (sr3_load_weights_dev): fused_host fetches dev again on demand
    size_t dev_floats = 0;
    bool owns = true;                            // false: a view into a concatenated buffer
    bool loaded = false;
};

struct GNRef { int gamma = -1, beta = -1, C = 0; };
struct ConvRef { int w = -1, b = -1, cin = 0, cout = 0, ks = 0, cin_pad = 0; };

struct ResBlock {
    int cin = 0, cout = 0;
    GNRef gn1, gn2, agn;
    ConvRef c1, c2, res, qkv, aout;
    int nf_off = 0;  // offset into the concatenated FeatureWiseAffine output
    bool has_res = false, attn = false;
    float *fused_bias = nullptr;   // has_res: conv2 bias + res_conv bias (the fused launch adds both)
    // identity skip (dim == dim_out) of a narrow block in split-f16 mode: `h + x` runs as cout / 32 extra
    // K-steps of conv2 over the raw x twin with the matrix 2^k * I (exact: 2^k is a half, x = hi + lo),
    // instead of a per-element gather of x in the epilogue — the K loop of these 64/128-channel layers
    // is short and the gather cost more than the two or four extra K-steps
    float *ident_w = nullptr;      // split-f16 [cout][cout], rebuilt whenever conv2's scale changes
};

enum ModKind { M_CONV_IN, M_RES, M_DOWN, M_UP };
struct Module {
    ModKind kind;
    ResBlock rb;
    ConvRef conv;
    // workspace (set by ensure_workspace)
    TDesc out;      // module output (zero-bordered)
    bool so_now = false;   // this forward: out was written ONLY as out_s (prec 1, split-only mode)
    TDesc out_s;    // split-f16 twin of out, written by the producing conv's epilogue in prec 1 when a
                    // later conv reads this tensor raw (Down/Upsample input, fused res_conv operand); p == null: none
    TDesc rb_out;   // ResBlock output before attention (== out if no attention)
    TDesc act1, act2, h1;   // activated conv inputs and the block1 output (per-shape buffers)
    TDesc up_in;            // M_UP / M_DOWN: split-f16 copy of the raw input (prec 1)
    int slices_default = 0; // st_out.slices when the generic conv produces the statistics (conv_in_kernel: HW / 256)
    TDesc raw1;             // has_res: un-normalised x ‖ skip in the conv input format (fused res_conv)
    // fused GroupNorm statistics written by the conv that produces out / rb_out / h1 (p == null:
    // the tile does not divide the image, fall back to the statistics kernel)
    StatsRef st_out, st_rb, st_h1;
    int oc = 0, oh = 0, ow = 0;     // output channels and resolution
    int ih = 0, iw = 0;             // input resolution
};

// exact f32 MFMA | split-f16, three f16 products (f16x3) | split-f16 with two fp8 correction products (f16f8): the values
// of sr3_set_precision, and the order of the range policy's ladder (step_down)
enum Arith { A_F32 = 0, A_F16X3 = 1, A_F16F8 = 2 };

enum Family { F_CONV = 0, F_GN = 1, F_ATTN = 2, F_EMBED = 3, F_MISC = 4 };

struct ProfRec { int fam; hipEvent_t a, b; double flops; std::string tag; };
struct ProfAgg { double ms = 0, flops = 0; int64_t n = 0; };

// What a captured p_sample step is valid for (step_key builds it from the live context, once per step). The rule: a launch
// argument that a capture bakes in and that can change without a new workspace or new weights is a member. Equal keys then
// mean a valid graph, whatever was freed, reallocated or set in between (an address that comes back after a free holds
// what the step expects again). The members of a feature that is off stay zero: "off" is one value. Everything else a
// step bakes in (arena addresses, weight pointers and unscale scalars, the choice of kernels) is constant until
// drop_graphs.
struct StepKey {
    int mode = 0;                   // Arith
    int depth = 0;                  // feature cache: levels a shallow step keeps fresh, 0 = the whole step
    bool lr = false, dyn = false;   // form of the update: plain | projection | dynamic threshold | both
    float *x0hat = nullptr;         // lr || dyn
    LrOps lr_ops;                   // lr
    bool lr_lds = false;
    float *lr_scratch = nullptr;    // lr && !lr_lds (the LDS form takes no scratch)
    int64_t dyn_n = 0;              // dyn
    ThrPlan dyn_plan;
    float dyn_max = 0.f;
    float *dyn_s = nullptr;
    unsigned *dyn_bins = nullptr;
    RowArgs *rows = nullptr;        // rolling batch (sr3_rows_step): the per-row argument table; null: the uniform step
    const float *rows_lr = nullptr; // rows && lr (a session armed by sr3_rows_lr_consistency): the per-slot LR images
    int batch = 0;                  // rows: the slots [0, batch) the step covers (sr3_rows_step_batch); 0: the whole workspace

    // one graph is kept per (arithmetic, whole | shallow, form): 24 at the most, and per (arithmetic, plain | dynamic
    // threshold, unarmed | armed for the projection) of the rows form (always whole): 12 more, 36 in all while no step is
    // elastic. Each of the 12 rows forms keeps up to kRowsBatchGraphs (16) more, one per batch value below the slot count
    // (launch_step evicts the least recently used): 12 * 17 + 24 = 228 at the most. A rows step and a uniform one never
    // share a slot, nor do the steps of an armed and of an unarmed session, nor those of two batch values.
    bool same_form(const StepKey &o) const {
        return mode == o.mode && (depth > 0) == (o.depth > 0) && lr == o.lr && dyn == o.dyn && (rows != nullptr) == (o.rows != nullptr);
    }
    bool same_slot(const StepKey &o) const { return same_form(o) && batch == o.batch; }
    auto tie() const {
        return std::tie(mode, depth, lr, dyn, rows, rows_lr, batch, x0hat, lr_ops.Av, lr_ops.Ah, lr_ops.Pv, lr_ops.PhT, lr_ops.bv, lr_ops.bh, lr_ops.lh,
                        lr_ops.lw, lr_ops.H, lr_ops.W, lr_lds, lr_scratch, dyn_n, dyn_plan.k, dyn_plan.k2, dyn_plan.frac,
                        dyn_plan.blocks, dyn_max, dyn_s, dyn_bins);
    }
    bool operator==(const StepKey &o) const { return tie() == o.tie(); }
};
// warm: steps run eagerly under this key (the first sets one-time function attributes; the second is captured)
// used: launch_step's clock at the last launch (the eviction order of the elastic rows graphs)
struct StepGraph { StepKey key; hipGraphExec_t exec = nullptr; int warm = 0; uint64_t used = 0; };

} // namespace

struct sr3_ctx {
    sr3_unet_cfg cfg;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t order_ev = nullptr;      // sr3_wait_for_stream / sr3_stream_wait_for_ctx
    std::vector<Param> params;
    std::vector<Module> mods;   // downs ‖ mid ‖ ups
    int n_downs = 0, n_mid = 0;
    GNRef final_gn;
    ConvRef final_conv;
    int mlp_w1 = -1, mlp_b1 = -1, mlp_w2 = -1, mlp_b2 = -1;
    float *final_wq = nullptr;             // final_conv weights as [9][C][4] for the fused VALU kernel (kernels_edge.hip)
    float *final_wm = nullptr;             // final_conv weights as MFMA fragments (split-f16 mode, final_conv_mfma_kernel)
    float final_unscale = 1.0f;
    float *ci_w = nullptr;                 // downs.0 weights as MFMA fragments for conv_in_kernel (split-f16 mode)
    float ci_unscale = 1.0f;
    float *nfw = nullptr, *nfb = nullptr;  // concatenated FeatureWiseAffine linears
    int nf_total = 0;
    int in_pad = 0;     // in_channel padded to 32
    int c_max = 0;      // widest GroupNorm input
    uint64_t weight_bytes = 0;
    // The arithmetic of the 3x3 / activated-input convs (sr3_set_precision). Assigned by sr3_set_precision, step_down
    // and ModeScope only; everything else asks the three questions below (step_key and the feature cache record it).
    Arith mode = A_F32;
    // Batch-invariant mode (sr3_set_batch_invariant): the planning batch every dispatch decision of this
    // context counts in place of the call's B, 0 = off. Installed for the calling thread by PlanScope in every entry point that plans or launches.
    int plan_batch = 0;
    bool split() const { return mode != A_F32; }        // split-f16 operands (f16x3 or f16f8)
    // "f16f8": the two correction products of eligible convs run on the fp8 matrix path (ConvParams::f8, conv_f8_supported)
    bool f8() const { return mode == A_F16F8; }
    // split format of an activated conv input (launch_gn_apply's `split`): 0 fp32, 1 split-f16, 2 F8C when the consumer
    // conv takes the fp8 operands (f8_conv() said so)
    int act_format(bool f8_operand) const { return split() ? (f8_operand ? 2 : 1) : 0; }
    bool f8_dirty = true;      // dev_f8 copies are stale (weights loaded / re-split since they were made)
    bool fused_dirty = true;   // fused bias / common weight scales need (re)building
    bool all_fused = false;        // every GroupNorm of the current workspace gets its statistics from a conv epilogue
    // split-f16 range check: kernels set *d_ovf when a value stored in the split format exceeds the
    // fp16 range (|v| > 65504); sr3_unet_forward / sr3_sample_end / sr3_range_check read it and fail
    int *d_ovf = nullptr, *h_ovf = nullptr;
    // Range policy of the split-f16 mode (sr3_set_range_policy). strict: a call whose activations leave the fp16
    // range FAILS (round-2 behaviour). Default (not strict): the call is FINISHED in the exact-f32 arithmetic —
    // the reference computes in fp32 and has no such limit (unet.py:235-265) — and returns SR3_OK_F32_FALLBACK.
    bool strict_range = false;
    int fallback_calls = 0;             // calls finished by the f32 fallback since sr3_create
    int gn_wino_passes = 0;             // GroupNorm apply passes launched as launch_gn_wino_input / _fold_ since sr3_create
    int up2_wino_launches = 0;          // Upsample convs launched on wino_up2_kernel (ConvPlan::up2_wino) since sr3_create
    int wino_fused_rows_launches = 0;   // three-pass Winograd convs launched on the one-pass kernel's tile-row form (ConvPlan::wino_fused_rows) since sr3_create
    int conv_in_f32_launches = 0;       // forwards whose first conv ran on conv_in_f32_kernel (conv_in_f32_gate) since sr3_create
    int wino_gemm_out_launches = 0;    // three-pass Winograd convs launched in the one-kernel form (ConvPlan::wino_gemm_out) since sr3_create
    int gn_res1x1_launches = 0;         // block1 apply passes launched together with the block's 1x1 res_conv (launch_gn_res1x1) since sr3_create
    float *ckpt = nullptr;              // sr3_sample: NCHW copy of the sampler state at the last clean checkpoint
    size_t ckpt_floats = 0;
    double *metrics_ws = nullptr;       // sr3_metrics_psnr_ssim / sr3_denoise_loss: per-block fp64 partial sums (grows on demand)
    size_t metrics_ws_n = 0;
    // sr3_load_weights_dev: max|w| per parameter (bit patterns, reduced on the device) and the pinned staging area of its
    // one device-to-host copy: the maxima, the OIHW sources of the edge convs, and their packed forms on the way back
    unsigned *d_wmax = nullptr;
    float *h_stage = nullptr;
    unsigned *tile_cnt = nullptr;       // ConvParams::tile_cnt: arrival counters of the in-place split-K convs (zero between launches)
    // Set (for the rest of the context's life) when a bounded inter-block wait of the in-place split-K on x-halo tiles
    // gave up — a co-tenant kernel held the CU slots its sibling blocks needed (range_read): every conv then runs on a
    // path whose blocks never wait for each other. Captured step graphs are rebuilt.
    bool halo_split_off = false;
    int replay_calls = 0;               // calls (or segments) replayed for that reason since sr3_create

    // Train-mode Dropout of every ResnetBlock.block2 (unet.py:81-91; sr3_set_dropout). Off by default; p is
    // latched from cfg.dropout by the setter. drop_live(): the block2 apply passes launch their masked instantiations.
    bool drop_on = false;
    uint64_t drop_seed = 0, drop_offset = 0;    // drop_offset: image offset of sr3_unet_forward (the other entry points take one)
    uint32_t drop_thr = 0;                      // round-half-even(p * 65536)
    float drop_s = 1.0f;                        // float32(1.0 / (1.0 - p))
    const uint8_t *drop_masks = nullptr;        // injected masks (sr3_set_dropout_masks) or null -> Philox
    uint64_t drop_mask_bytes = 0;
    int n_res = 0;                              // ResnetBlocks = Dropout layers (build_graph)
    int drop_layer = 0;                         // run_unet_body's cursor: ordinal of the next ResnetBlock ...
    uint64_t drop_base = 0;                     // ... and its offset in the injected buffer
    bool drop_live() const { return drop_on && drop_thr > 0; }

    // Low-resolution consistency (sr3_set_lr_consistency). Off by default: a step then launches exactly
    // the kernels it always did. lr: the host copy of what d_lr holds; lr_cur / lr_cur_lds: the operators and the form of
    // the current sampling call (sr3_sample_begin), launch arguments of the captured steps (StepKey).
    struct LrDev { float *buf = nullptr; int *bounds = nullptr; LrOps ops; };
    std::map<std::tuple<int, int, int, int>, LrDev> lr_ops;     // per (lh, lw, H, W), built on first use
    LrArgs lr;
    int lr_lh = 0, lr_lw = 0;
    LrArgs *d_lr = nullptr, *h_lr = nullptr;    // device copy <- pinned host ring (as StepArgs: the copy is asynchronous)
    static constexpr int kLrRing = 64;
    uint64_t lr_count = 0;
    float *x0hat = nullptr;             // NCHW [B][out_channel][H][W]: the predicted x0 between the two halves of the update
    size_t x0hat_floats = 0;
    float *lr_scratch = nullptr;        // T | U | R of the multi-launch projection and of the residual score
    size_t lr_scratch_n = 0;
    LrOps lr_cur;
    bool lr_cur_lds = false;
    bool lr_on() const { return lr.lr != nullptr && lr.strength != 0.f; }

    // Dynamic thresholding of the x0 prediction (sr3_set_dynamic_threshold). Off by default (dyn_ratio 0):
    // a step then launches exactly the kernels it always did. dyn_plan: rank, weight and blocks of the current sampling
    // call's n = out_channel * H * W (sr3_sample_begin), launch arguments of the captured steps like dyn_max (StepKey).
    float dyn_ratio = 0.f, dyn_max = INFINITY;
    ThrPlan dyn_plan;
    int64_t dyn_n = 0;
    float *dyn_s = nullptr;             // [dyn_rows]: s of every image of the step
    unsigned *dyn_bins = nullptr;       // [dyn_rows][THR_BINS_PER_IMAGE]: the select's counts
    int dyn_rows = 0;
    int dyn_steps = 0;                  // sampler steps issued in the thresholded form since sr3_create
    bool dyn_on() const { return dyn_ratio > 0.f; }
    unsigned *thr_op_bins = nullptr;    // sr3_op_abs_quantile / sr3_op_dynamic_threshold: counts, then thr_op_rows floats of s
    int thr_op_rows = 0;

    // Feature cache (sr3_set_feature_cache; DeepCache, Ma, Fang, Wang 2023). Off by default (fc_interval
    // <= 1): every step is then the whole forward it always was. On: step fc_k of a call is whole when fc_k % fc_interval
    // == 0 or the cache is not valid, else it runs the fc_depth top levels on what the last whole step left in the
    // workspace. The cache IS the workspace: fc_mode is the arithmetic of the last whole run_unet_body on it (-1: none
    // since the workspace was built, a weight changed or sr3_set_precision was called), fc_call says that forward was a
    // step of the live sampling call (any other run_unet_body clears it).
    int fc_interval = 0, fc_depth = 1;
    int fc_k = 0;                       // steps since sr3_sample_begin*
    int fc_mode = -1;
    bool fc_call = false;
    int fc_whole = 0, fc_shallow = 0;   // steps of the last call, replayed ones included (sr3_feature_cache_steps)
    bool fc_on() const { return fc_interval > 1; }
    void fc_invalidate() { fc_mode = -1; fc_call = false; }
    int fc_max_depth() const { return cfg.n_mults - 1; }

    // workspace for one (B, H, W)
    int wB = 0, wH = 0, wW = 0;
    char *arena = nullptr;
    // what ensure_workspace carved of the buffers every conv / attention / GroupNorm shares, in floats, and the statistics
    // slices per image of every conv in the order it asked (rows_batch_fits holds a smaller batch against them)
    uint64_t cap_part = 0, cap_wino = 0, cap_vt = 0, cap_gpart = 0;
    std::vector<int> conv_slices;
    uint64_t arena_bytes = 0;
    TDesc x0;                   // [B][H+2][W+2][in_pad]: cond ‖ x ‖ zero pad (UNet input = sampler state)
    TDesc x0s;                  // split-f16 copy of x0 for the first conv (prec 1)
    float *x0p = nullptr;       // packed split-f16 state for conv_in_kernel (null: shape not supported); kept in
                                // step with x0 by launch_pack_state / the DDPM update
    TDesc eps;                  // [B][H][W][out_channel]
    float *xhist = nullptr;     // NCHW [B][out_channel][H][W]: x0 history of the multistep samplers (UpdateParams::hist)
    TDesc final_act;            // activated input of final_conv
    float *qkvb = nullptr, *aob = nullptr, *vtb = nullptr;   // attention: qkv, core output, v^T scratch (split-f16 core)
    float *part = nullptr;      // split-K partial sums (small-M convs)
    float *wino_ws = nullptr;   // transformed input and products of the Winograd convs (ConvPlan::wino_ws_floats)
    float *gscale = nullptr, *gshift = nullptr, *gpart = nullptr;
    float *temb = nullptr, *cbias = nullptr;
    int cb_stride = 0;          // row stride of cbias: nf_total, or 0 when one noise level serves the whole batch (sampler steps)

    // sampler schedule (sr3_set_schedule: the reference's DDPM loop; sr3_set_sampler_schedule: S of its levels)
    int T = 0;              // steps of one call: T of the DDPM schedule, or S
    std::vector<float> s_nl, s_a, s_b, s_c1, s_c2, s_c3, s_sig;   // s_nl [T+1], the others [T], indexed by step t
    bool uses_hist = false; // the update keeps the clamped x0 of the previous step (xhist)
    bool hist_valid = false;// xhist holds the x0 of an earlier step of the current call (reset by sr3_sample_begin)
    float *d_nl = nullptr;  // [T+1]
    // Warm start (sr3_sample_begin_from). d_start: a[B] | s[B], the per-row q_sample coefficients of the
    // start state (grown on demand). fold_first: the call was begun there with a multistep sampler, so its first step
    // (no x0 history yet) takes c1 + c3 as its c1; sr3_sample_begin clears it.
    float *d_start = nullptr;
    int start_rows = 0;
    bool fold_first = false;

    // sampler state
    uint64_t seed = 0, image_offset = 0;
    bool sampling = false;
    // Rolling batch (sr3_rows_begin): a session of wB slots, each idle or at its own position. The host
    // is authoritative: rows[r].pos steps are left for slot r (its next step is t = pos - 1). d_rows: the table the
    // kernels read, rows_cap entries (grown on demand: its address is a member of the StepKey); h_rows: the pinned ring
    // it is refreshed from, kRowRing slots of rows_cap entries.
    // Per row as well: lr_strength (0: not held to an LR image) and frames (null, or where the row writes the frames of
    // a uniform call from `start`; frames_n of them written so far).
    struct RowState {
        bool live = false, hist_valid = false, fold = false;
        int pos = 0, start = 0;
        uint64_t image = 0;
        float lr_strength = 0.f;
        float *frames = nullptr;
        int frames_n = 0, frames_cap = 0;   // (frames_cap: the count sr3_rows_frames checked; never written past)
    };
    bool rows_on = false;
    // sr3_rows_lr_consistency: the session is armed — its steps run the projection's rows form between the halves of the
    // update. rows_lr_ops / rows_lr_lds: operators and form, launch arguments of the captured steps (StepKey) like
    // rows_lr_buf, the LR image of every slot [rows_lr_slots][out_channel][lh][lw] (grown on demand, kept between sessions).
    bool rows_lr = false, rows_lr_lds = false;
    bool rows_admitted = false;         // a row was admitted since sr3_rows_begin
    LrOps rows_lr_ops;
    float *rows_lr_buf = nullptr;
    size_t rows_lr_floats = 0;
    std::vector<RowState> rows;
    RowArgs *d_rows = nullptr, *h_rows = nullptr;
    int rows_cap = 0;
    static constexpr int kRowRing = 256;        // as kRing: the host synchronises every 128 steps
    uint64_t rows_count = 0;
    // Elastic steps (sr3_rows_step_batch): rows_run sums the batch of every row-session step launched; rows_batch_ok holds
    // the batch values below wB whose plans were checked against what ensure_workspace carved (rows_batch_fits; emptied
    // with every new workspace and every change of the planning batch).
    uint64_t rows_run = 0;
    std::vector<int> rows_batch_ok;
    static constexpr int kRowsBatchGraphs = 16;
    uint64_t graph_clock = 0;
    float *d_row_start = nullptr;       // a[rows_cap] | s[rows_cap]: q_sample coefficients of the rows admitted noised
    // per-step arguments: pinned host ring -> device struct (async copy before every step)
    static constexpr int kRing = 256;
    StepArgs *h_ring = nullptr, *d_step = nullptr;
    uint64_t step_count = 0;
    // p_sample steps captured as hipGraphs, each with the key it is valid for: step_impl looks its step's key up, and
    // replaces the graph of the same slot (StepKey::same_slot) when the key differs. drop_graphs empties it: the workspace,
    // the weights or the choice of kernels changed.
    std::vector<StepGraph> step_graphs;
    int step_graph_captures = 0;        // graphs instantiated by step_impl since sr3_create
    bool no_graph = false;

    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> ev_pool;
    double acc_ms[SR3_N_FAMILIES] = {0}, acc_flops[SR3_N_FAMILIES] = {0};
    int64_t acc_n[SR3_N_FAMILIES] = {0};
    std::map<std::string, ProfAgg> by_tag;   // per distinct launch shape

    hipEvent_t get_event() {
        if (!ev_pool.empty()) { hipEvent_t e = ev_pool.back(); ev_pool.pop_back(); return e; }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    }
    void pbegin(int fam) {
        if (!prof) return;
        ProfRec r{fam, get_event(), get_event(), 0.0, std::string()};
        (void)hipEventRecord(r.a, stream);
        recs.push_back(r);
    }
    void pend(double flops = 0.0, const char *tag = nullptr) {
        if (!prof) return;
        recs.back().flops = flops;
        if (tag) recs.back().tag = tag;
        (void)hipEventRecord(recs.back().b, stream);
    }
    void pflush() {
        if (recs.empty()) return;
        (void)hipStreamSynchronize(stream);
        for (auto &r : recs) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, r.a, r.b);
            acc_ms[r.fam] += ms;
            acc_flops[r.fam] += r.flops;
            acc_n[r.fam] += 1;
            if (!r.tag.empty()) {
                ProfAgg &g = by_tag[r.tag];
                g.ms += ms; g.flops += r.flops; g.n += 1;
            }
            ev_pool.push_back(r.a);
            ev_pool.push_back(r.b);
        }
        recs.clear();
    }
};

namespace {

// ---------------------------------------------------------------------------------------------
// graph construction (unet.py:161-233)
// ---------------------------------------------------------------------------------------------
int add_param(sr3_ctx *c, const std::string &name, std::vector<int64_t> shape, ParamKind kind = P_PLAIN) {
    Param p;
    p.name = name;
    p.shape = std::move(shape);
    p.kind = kind;
    c->params.push_back(p);
    return (int)c->params.size() - 1;
}

ConvRef add_conv(sr3_ctx *c, const std::string &prefix, int cin, int cout, int ks, bool bias) {
    ConvRef r;
    r.cin = cin; r.cout = cout; r.ks = ks; r.cin_pad = round_up(cin, 32);
    r.w = add_param(c, prefix + ".weight", {cout, cin, ks, ks}, P_CONV);
    Param &p = c->params[r.w];
    p.cout = cout; p.cin = cin; p.ks = ks; p.cin_pad = r.cin_pad;
    if (bias) r.b = add_param(c, prefix + ".bias", {cout});
    return r;
}

GNRef add_gn(sr3_ctx *c, const std::string &prefix, int C) {
    GNRef g;
    g.C = C;
    g.gamma = add_param(c, prefix + ".weight", {C});
    g.beta = add_param(c, prefix + ".bias", {C});
    if (C > c->c_max) c->c_max = C;
    return g;
}

// identity skip as extra K-steps of conv2 (ResBlock::ident_w): narrow blocks that keep their width
bool ident_eligible(const ResBlock &rb) { return !rb.has_res && rb.cout <= 128 && (rb.cout % 32) == 0; }

Module make_res(sr3_ctx *c, const std::string &prefix, int cin, int cout, bool attn) {
    Module m;
    m.kind = M_RES;
    ++c->n_res;
    ResBlock &rb = m.rb;
    rb.cin = cin; rb.cout = cout; rb.attn = attn;
    const int inner = c->cfg.inner_channel;
    const std::string rp = prefix + ".res_block";
    // registration order of the reference: noise_func, block1, block2, res_conv (unet.py:97-103)
    int nfw = add_param(c, rp + ".noise_func.noise_func.0.weight", {cout, inner});
    int nfb = add_param(c, rp + ".noise_func.noise_func.0.bias", {cout});
    c->params[nfw].owns = false;
    c->params[nfb].owns = false;
    rb.nf_off = c->nf_total;
    c->nf_total += cout;
    rb.gn1 = add_gn(c, rp + ".block1.block.0", cin);
    rb.c1 = add_conv(c, rp + ".block1.block.3", cin, cout, 3, true);
    rb.gn2 = add_gn(c, rp + ".block2.block.0", cout);
    rb.c2 = add_conv(c, rp + ".block2.block.3", cout, cout, 3, true);
    rb.has_res = (cin != cout);
    if (rb.has_res) {
        rb.res = add_conv(c, rp + ".res_conv", cin, cout, 1, true);
        for (int idx : {rb.c2.w, rb.c2.b, rb.res.w, rb.res.b}) c->params[idx].keep_host = true;
    } else if (ident_eligible(rb)) {
        c->params[rb.c2.w].keep_host = true;     // prepare_fused may re-split conv2 with a capped scale
    }
    if (attn) {
        rb.agn = add_gn(c, prefix + ".attn.norm", cout);
        rb.qkv = add_conv(c, prefix + ".attn.qkv", cout, 3 * cout, 1, false);
        rb.aout = add_conv(c, prefix + ".attn.out", cout, cout, 1, true);
    }
    return m;
}

bool in_list(const int *v, int n, int x) {
    for (int i = 0; i < n; ++i)
        if (v[i] == x) return true;
    return false;
}

int build_graph(sr3_ctx *c) {
    const sr3_unet_cfg &g = c->cfg;
    const int inner = g.inner_channel;
    // noise_level_mlp is registered first (unet.py:177-184)
    c->mlp_w1 = add_param(c, "noise_level_mlp.1.weight", {4 * inner, inner});
    c->mlp_b1 = add_param(c, "noise_level_mlp.1.bias", {4 * inner});
    c->mlp_w2 = add_param(c, "noise_level_mlp.3.weight", {inner, 4 * inner});
    c->mlp_b2 = add_param(c, "noise_level_mlp.3.bias", {inner});

    int pre = inner, now_res = g.image_size, idx = 0;
    std::vector<int> feat{pre};
    {
        Module m;
        m.kind = M_CONV_IN;
        m.conv = add_conv(c, "downs.0", g.in_channel, inner, 3, true);
        c->mods.push_back(m);
        idx = 1;
    }
    for (int ind = 0; ind < g.n_mults; ++ind) {
        const bool last = ind == g.n_mults - 1;
        const bool attn = in_list(g.attn_res, g.n_attn_res, now_res);
        const int ch = inner * g.channel_mults[ind];
        for (int k = 0; k < g.res_blocks; ++k) {
            c->mods.push_back(make_res(c, "downs." + std::to_string(idx++), pre, ch, attn));
            feat.push_back(ch);
            pre = ch;
        }
        if (!last) {
            Module m;
            m.kind = M_DOWN;
            m.conv = add_conv(c, "downs." + std::to_string(idx++) + ".conv", pre, pre, 3, true);
            c->mods.push_back(m);
            feat.push_back(pre);
            now_res /= 2;
        }
    }
    c->n_downs = (int)c->mods.size();
    c->mods.push_back(make_res(c, "mid.0", pre, pre, true));
    c->mods.push_back(make_res(c, "mid.1", pre, pre, false));
    c->n_mid = 2;
    idx = 0;
    for (int ind = g.n_mults - 1; ind >= 0; --ind) {
        const bool last = ind < 1;
        const bool attn = in_list(g.attn_res, g.n_attn_res, now_res);
        const int ch = inner * g.channel_mults[ind];
        for (int k = 0; k < g.res_blocks + 1; ++k) {
            const int skip = feat.back();
            feat.pop_back();
            if (pre + skip == ch)
                return fail("up-path ResnetBlock with cin == cout (identity skip over a concatenation) is not supported");
            c->mods.push_back(make_res(c, "ups." + std::to_string(idx++), pre + skip, ch, attn));
            pre = ch;
        }
        if (!last) {
            Module m;
            m.kind = M_UP;
            m.conv = add_conv(c, "ups." + std::to_string(idx++) + ".conv", pre, pre, 3, true);
            c->params[m.conv.w].up_phase = true;
            c->mods.push_back(m);
            now_res *= 2;
        }
    }
    c->final_gn = add_gn(c, "final_conv.block.0", pre);
    c->final_conv = add_conv(c, "final_conv.block.3", pre, g.out_channel, 3, true);
    c->in_pad = round_up(g.in_channel, 32);
    return 0;
}

// 3x3 conv weights that may run in Winograd form (conv_plan: the batch and resolution decide per launch).
// The parameter does not know its level: a conv with 64 <= Cin < 128 gets the transformed copy (16/9 of its 3x3
// weights) even where it only ever runs at 32x32 or below, where only Cin >= 128 is taken (none in the yml UNet).
bool wino_weights(const Param &p) {
    return p.kind == P_CONV && p.ks == 3 && !p.up_phase && p.cin_pad >= std::min(WINO_MIN_CIN, WINO_FUSED_CIN) && (p.cin_pad % 32) == 0 &&
           (p.cout % 64) == 0;
}

// Upsample conv weights that may run as sub-pixel Winograd F(2x2, 2x2) (conv_plan decides per launch). The layout is made
// with the phase planes at every load, by either route: it adds original 3x3 taps, which the engine does not keep, so
// unlike dev_wino_f it cannot be made later from what is on the device.
bool up2_wino_weights(const Param &p) {
    return p.kind == P_CONV && p.ks == 3 && p.up_phase && (p.cin_pad % 32) == 0 && (p.cout % UP2_WINO_BN) == 0;
}

// the one-pass Winograd kernel's fragment-major copy of a parameter's transformed weights, made from dev_wino on the
// device the first time a workspace plan runs the conv at a one-pass shape or in the tile-row form of the three-pass plan
// (ConvPlan::wino_fused_rows) (a parameter does not know its level; only the convs of the 64x64 and 128x128 levels, and
// of the 32x32 level from WINO_FUSED_ROWS_MIN_BLOCKS blocks on, get one). sr3_load_weight refreshes it with dev_wino.
int ensure_wino_frag(sr3_ctx *c, Param &p) {
    if (p.dev_wino_f) return 0;
    const size_t n = (size_t)16 * p.cout * p.cin_pad;
    HIP_OK(hipMalloc(&p.dev_wino_f, n * sizeof(float)));
    c->weight_bytes += n * sizeof(float);
    launch_wino_frag(p.dev_wino, p.cout, p.cin_pad, p.dev_wino_f, c->stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

int alloc_weights(sr3_ctx *c) {
    const int inner = c->cfg.inner_channel;
    HIP_OK(hipMalloc(&c->nfw, (size_t)c->nf_total * inner * sizeof(float)));
    HIP_OK(hipMalloc(&c->nfb, (size_t)c->nf_total * sizeof(float)));
    c->weight_bytes += (uint64_t)c->nf_total * (inner + 1) * sizeof(float);
    if (final_conv_supported(c->final_conv.cin, c->final_conv.cout)) {
        HIP_OK(hipMalloc(&c->final_wq, (size_t)9 * c->final_conv.cin * 4 * sizeof(float)));
        c->weight_bytes += (uint64_t)9 * c->final_conv.cin * 4 * sizeof(float);
    }
    if (final_conv_mfma_supported(c->final_conv.cin, c->final_conv.cout)) {
        HIP_OK(hipMalloc(&c->final_wm, final_conv_mfma_weight_floats(c->final_conv.cin) * sizeof(float)));
        c->weight_bytes += final_conv_mfma_weight_floats(c->final_conv.cin) * sizeof(float);
    }
    if (c->cfg.in_channel <= 8 && (c->cfg.inner_channel % 32) == 0 && c->cfg.inner_channel <= 64) {
        HIP_OK(hipMalloc(&c->ci_w, conv_in_weight_floats(c->cfg.inner_channel) * sizeof(float)));
        c->weight_bytes += conv_in_weight_floats(c->cfg.inner_channel) * sizeof(float);
    }
    int nf_off = 0;
    for (auto &p : c->params) {
        if (!p.owns) {
            // FeatureWiseAffine weight/bias pairs are registered back to back in module order
            if (p.shape.size() == 2) {
                p.dev = c->nfw + (size_t)nf_off * inner;
                p.dev_floats = (size_t)p.shape[0] * inner;
            } else {
                p.dev = c->nfb + nf_off;
                p.dev_floats = (size_t)p.shape[0];
                nf_off += (int)p.shape[0];
            }
            continue;
        }
        size_t n = 1;
        if (p.kind == P_CONV) n = (size_t)(p.up_phase ? 16 : p.ks * p.ks) * p.cout * p.cin_pad;
        else for (auto d : p.shape) n *= (size_t)d;
        p.dev_floats = n;
        HIP_OK(hipMalloc(&p.dev, n * sizeof(float)));
        c->weight_bytes += n * sizeof(float);
        if (p.kind == P_CONV) {
            HIP_OK(hipMalloc(&p.dev_split, n * sizeof(float)));
            c->weight_bytes += n * sizeof(float);
        }
        if (wino_weights(p)) {
            HIP_OK(hipMalloc(&p.dev_wino, (size_t)16 * p.cout * p.cin_pad * sizeof(float)));
            c->weight_bytes += (size_t)16 * p.cout * p.cin_pad * sizeof(float);
        }
        if (up2_wino_weights(p)) {
            HIP_OK(hipMalloc(&p.dev_up_wino, up2_wino_floats(p.cout, p.cin_pad) * sizeof(float)));
            c->weight_bytes += up2_wino_floats(p.cout, p.cin_pad) * sizeof(float);
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------
struct Carver {
    uint64_t off = 0;
    uint64_t take(uint64_t floats) {
        const uint64_t o = off;
        off += (floats * sizeof(float) + 255) / 256 * 256;
        return o;
    }
};

// per-shape buffer pool: tensors of one (C, H, W) that are never live at the same time share a
// buffer; because the shape is fixed per buffer its zero border is never overwritten
struct ShapePool {
    std::map<std::tuple<int, int, int>, uint64_t> off;
    uint64_t get(Carver &cv, int B, int C, int H, int W) {
        auto key = std::make_tuple(C, H, W);
        auto it = off.find(key);
        if (it != off.end()) return it->second;
        const uint64_t o = cv.take((uint64_t)B * (H + 2) * (W + 2) * C);
        off[key] = o;
        return o;
    }
};

void drop_graphs(sr3_ctx *c);
int prepare_f8(sr3_ctx *c);

// installs the context's planning batch (batch-invariant mode; 0 = off) for the decisions of one entry point. The rule:
// every extern "C" function that reaches conv_plan / conv_plan_offered / gn_route / gn_res1x1_gate / max_batch or a
// launcher that reads plan_b (launch_conv, launch_wino_gemm, the GroupNorm launchers, launch_gn_res1x1,
// launch_attention_split) opens one first. ensure_workspace refuses to size a workspace for a context in the mode
// without one, so an entry point of the UNet that forgets it fails instead of planning by B.
struct PlanScope {
    const int was;
    explicit PlanScope(const sr3_ctx *c) : was(set_plan_batch(c ? c->plan_batch : 0)) {}
    PlanScope(const PlanScope &) = delete;
    ~PlanScope() { set_plan_batch(was); }
};

// largest batch one call can take at H x W: every activation tensor must stay below 4 GiB (32-bit byte offsets of the
// conv's LDS-DMA addressing) and the padded pixel count below 2^31. Batch-invariant mode: also what the plans of the
// UNet's convs hold for (ConvPlan::batch_limit, either arithmetic, with and without fused statistics) and 65535, the
// grid rows of the launches that take one image per row — past the bound a call fails, it never changes its arithmetic.
int max_batch(const sr3_ctx *c, int H, int W) {
    const int div = 1 << (c->cfg.n_mults - 1);
    if (H <= 0 || W <= 0 || (H % div) || (W % div)) return 0;
    uint64_t per = (uint64_t)(H + 2) * (W + 2) * c->in_pad;          // floats per image of the widest tensor
    int h = H, w = W;
    for (const Module &m : c->mods) {
        if (m.kind == M_DOWN) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
        else if (m.kind == M_UP) { h *= 2; w *= 2; }
        uint64_t ch = m.kind == M_RES ? (uint64_t)m.rb.cout : (uint64_t)m.conv.cout;
        if (m.kind == M_RES) ch = std::max<uint64_t>(ch, std::max<uint64_t>(m.rb.attn ? 3ull * m.rb.cout : 0ull, (uint64_t)m.rb.cin));
        // (no core for this token count and width: ensure_workspace says which; both arithmetics share the bound)
        if (m.kind == M_RES && m.rb.attn && attention_core(false, (long)h * w, m.rb.cout) == ATTN_UNSUPPORTED) return -1;
        per = std::max(per, (uint64_t)(h + 2) * (w + 2) * ch);
    }
    const uint64_t by_bytes = ((1ull << 32) - 1) / (per * sizeof(float));
    const uint64_t by_pix = ((1ull << 31) - 1) / ((uint64_t)(H + 2) * (W + 2));
    uint64_t bound = std::min<uint64_t>(std::min(by_bytes, by_pix), 1u << 20);
    if (c->plan_batch > 0) {
        PlanScope plan(c);
        bound = std::min<uint64_t>(bound, 65535);
        auto conv = [&](const ConvRef &cr, int ih, int iw, int stride, int up2) {
            for (int v = 0; v < 4; ++v) {
                const ConvPlan pl = conv_plan_offered(1, ih, iw, cr.cin_pad, cr.cout, cr.ks, stride, up2, v & 1, false, (v & 2) != 0);
                if (pl.batch_limit > 0) bound = std::min<uint64_t>(bound, (uint64_t)pl.batch_limit);
            }
        };
        h = H; w = W;
        for (const Module &m : c->mods) {
            const int ih = h, iw = w;
            if (m.kind == M_DOWN) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
            else if (m.kind == M_UP) { h *= 2; w *= 2; }
            if (m.kind == M_RES) {
                conv(m.rb.c1, h, w, 1, 0);
                conv(m.rb.c2, h, w, 1, 0);
                if (m.rb.attn) { conv(m.rb.qkv, h, w, 1, 0); conv(m.rb.aout, h, w, 1, 0); }
            } else {
                conv(m.conv, ih, iw, m.kind == M_DOWN ? 2 : 1, m.kind == M_UP ? 1 : 0);
            }
        }
    }
    return (int)bound;
}

int ensure_workspace(sr3_ctx *c, int B, int H, int W) {
    if (plan_batch() != c->plan_batch) return fail("internal: an entry point reached the workspace without the context's planning batch (PlanScope)");
    if (c->arena && c->wB == B && c->wH == H && c->wW == W) return 0;
    const sr3_unet_cfg &g = c->cfg;
    const int div = 1 << (g.n_mults - 1);
    if (B <= 0 || H <= 0 || W <= 0 || (H % div) || (W % div))
        return fail("unsupported shape B=%d H=%d W=%d: H and W must be multiples of %d", B, H, W, div);
    if (c->arena) {
        HIP_OK(hipStreamSynchronize(c->stream));
        HIP_OK(hipFree(c->arena));
        c->arena = nullptr;
    }
    drop_graphs(c);
    c->fc_invalidate();
    // Feature cache: every module below gets an output (out_off), twin (tw_off) and statistics slices
    // (so_off / sr_off / sh_off) of its own, which only the module's own convs write; acts, h1s and raws are
    // block-internal. A shallow forward therefore leaves the outputs of the modules it skips as the last whole forward
    // wrote them.
    // dry run over the graph for sizes
    Carver cv;
    ShapePool acts, h1s, raws;
    const size_t nm = c->mods.size();
    std::vector<uint64_t> out_off(nm), rb_off(nm), a1_off(nm), a2_off(nm), h1_off(nm), raw_off(nm);
    std::vector<uint64_t> so_off(nm), sr_off(nm), sh_off(nm), tw_off(nm);
    std::vector<char> twin(nm, 0);
    for (size_t i = 0; i < nm; ++i) {
        const bool skip = (int)i < c->n_downs;                       // consumed raw by an up-path res_conv
        const Module *nx = i + 1 < nm ? &c->mods[i + 1] : nullptr;
        twin[i] = skip || (nx && (nx->kind == M_DOWN || nx->kind == M_UP || (nx->kind == M_RES && nx->rb.has_res)));
    }
    std::vector<int> s_slices(nm, 0), s_out(nm, 0), s_h1(nm, 0);
    uint64_t max_qkv = 0, max_ao = 0, max_part = 0, max_vt = 0, max_wino = 0;
    int h = H, w = W;
    std::vector<int> feat_c;
    // What one conv asks of the shared buffers: its plan with everything offered, in either arithmetic (the exact-f32
    // repeat of the range check runs on the same workspace) and with or without fused statistics (a shape that has none
    // runs without). Returns the statistics slices per image of its output (the same in all four plans).
    bool frag_ok = true;
    c->conv_slices.clear();
    c->rows_batch_ok.clear();
    auto want = [&](const ConvRef &cr, int ih, int iw, int stride, int up2) {
        int slices = 0;
        for (int v = 0; v < 4; ++v) {
            const ConvPlan pl = conv_plan_offered(B, ih, iw, cr.cin_pad, cr.cout, cr.ks, stride, up2, v & 1, false, (v & 2) != 0);
            max_part = std::max<uint64_t>(max_part, pl.part_floats);
            slices = pl.stats_slices;
            if (!wino_weights(c->params[cr.w])) continue;
            max_wino = std::max<uint64_t>(max_wino, pl.wino_ws_floats);
            if ((pl.needs_wino_frag || pl.wino_fused_rows) && ensure_wino_frag(c, c->params[cr.w])) frag_ok = false;
        }
        c->conv_slices.push_back(slices);
        return slices;
    };
    for (size_t i = 0; i < nm; ++i) {
        Module &m = c->mods[i];
        const int ih = h, iw = w;                 // the module's input resolution
        int oc;
        if (m.kind == M_CONV_IN) { oc = m.conv.cout; }
        else if (m.kind == M_DOWN) { oc = m.conv.cout; a1_off[i] = acts.get(cv, B, m.conv.cin, h, w); h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
        else if (m.kind == M_UP) { oc = m.conv.cout; a1_off[i] = acts.get(cv, B, m.conv.cin, h, w); h *= 2; w *= 2; }
        else {
            oc = m.rb.cout;
            a1_off[i] = acts.get(cv, B, m.rb.cin, h, w);
            a2_off[i] = acts.get(cv, B, oc, h, w);
            h1_off[i] = h1s.get(cv, B, oc, h, w);
            if (m.rb.has_res) raw_off[i] = raws.get(cv, B, m.rb.cin, h, w);
            if (m.rb.attn) {
                const uint64_t nu = (uint64_t)B * h * w * oc;
                if (3 * nu > max_qkv) max_qkv = 3 * nu;
                if (nu > max_ao) max_ao = nu;
                for (const bool split : {false, true}) {       // (either arithmetic runs on this workspace)
                    const AttnCore core = attention_core(split, (long)h * w, oc);
                    if (core == ATTN_UNSUPPORTED)
                        return fail("attention over %d tokens at %d channels: the streaming core takes at most 512 channels", h * w, oc);
                    if (core == ATTN_SPLIT) max_vt = std::max<uint64_t>(max_vt, attention_vt_floats(B, h * w, oc));
                }
            }
        }
        m.oc = oc; m.oh = h; m.ow = w; m.ih = ih; m.iw = iw;
        // split-K partials, Winograd workspace and fused statistics: a conv writing an [oc, h, w] tensor leaves one slice
        // per M-tile of an image (every such conv uses the same tile height), a split-K conv one per block of its reduce pass
        if (m.kind == M_RES) {
            s_h1[i] = want(m.rb.c1, h, w, 1, 0);
            s_out[i] = want(m.rb.c2, h, w, 1, 0);
            if (m.rb.attn) { want(m.rb.qkv, h, w, 1, 0); want(m.rb.aout, h, w, 1, 0); }
        } else {
            s_out[i] = want(m.conv, ih, iw, m.kind == M_DOWN ? 2 : 1, m.kind == M_UP ? 1 : 0);
        }
        if (!frag_ok) return -1;
        s_slices[i] = std::max(s_out[i], s_h1[i]);
        if (s_slices[i]) {
            const uint64_t sf = (uint64_t)B * s_slices[i] * oc * 4;   // 2 doubles per channel
            so_off[i] = cv.take(sf);
            sr_off[i] = cv.take(sf);
            sh_off[i] = cv.take(sf);
        }
        const uint64_t n = (uint64_t)B * (h + 2) * (w + 2) * oc;
        out_off[i] = cv.take(n);
        if (twin[i]) tw_off[i] = cv.take(n);
        rb_off[i] = (m.kind == M_RES && m.rb.attn) ? cv.take(n) : out_off[i];
    }
    if (h != H || w != W) return fail("internal: UNet does not return to the input resolution");
    {   // the conv's LDS-DMA addressing uses 32-bit byte offsets inside one tensor
        const int bmax = max_batch(c, H, W);
        if (B > bmax)
            return fail("batch %d at %dx%d makes an activation tensor of 4 GiB or more (32-bit DMA offsets inside one tensor); "
                        "run at most %d images per call (sr3_max_batch; the Python facade chunks larger batches by itself)",
                        B, H, W, bmax);
    }
    const uint64_t o_fa = acts.get(cv, B, c->final_gn.C, H, W);
    const uint64_t HW = (uint64_t)H * W;
    const uint64_t o_x0 = cv.take((uint64_t)B * (H + 2) * (W + 2) * c->in_pad);
    const uint64_t o_x0s = cv.take((uint64_t)B * (H + 2) * (W + 2) * c->in_pad);
    const bool ci_ok = c->ci_w && conv_in_supported(g.in_channel, c->mods[0].conv.cout, H, W);
    const uint64_t o_x0p = ci_ok ? cv.take((uint64_t)B * (H + 2) * (W + 2) * 8 + 16) : 0;   // + slack: the last A fragment reads one pixel on
    const uint64_t o_qkv = cv.take(max_qkv), o_ao = cv.take(max_ao), o_vt = cv.take(max_vt);
    const uint64_t o_part = cv.take(max_part);
    const uint64_t o_wino = cv.take(max_wino);
    const uint64_t o_gs = cv.take((uint64_t)B * c->c_max), o_gh = cv.take((uint64_t)B * c->c_max);
    const uint64_t o_gp = cv.take(gn_workspace_floats(B, c->c_max));
    const uint64_t o_te = cv.take((uint64_t)B * g.inner_channel);
    const uint64_t o_cb = cv.take((uint64_t)B * c->nf_total);
    const uint64_t o_eps = cv.take((uint64_t)B * HW * g.out_channel);
    const uint64_t o_hist = cv.take((uint64_t)B * HW * g.out_channel);
    HIP_OK(hipMalloc(&c->arena, cv.off));
    c->arena_bytes = cv.off;
    // zero everything once: the 1-pixel borders and the pad channels of x0 stay zero for the
    // lifetime of the workspace (kernels only ever write interiors)
    HIP_OK(hipMemsetAsync(c->arena, 0, cv.off, c->stream));
    auto at = [&](uint64_t o) { return reinterpret_cast<float *>(c->arena + o); };
    auto desc = [&](uint64_t o, int C, int hh, int ww, int pad) {
        TDesc d; d.p = at(o); d.C = C; d.H = hh; d.W = ww; d.pad = pad; return d;
    };
    bool all_fused = true;
    for (size_t i = 0; i < nm; ++i) {
        Module &m = c->mods[i];
        m.out = desc(out_off[i], m.oc, m.oh, m.ow, 1);
        m.rb_out = desc(rb_off[i], m.oc, m.oh, m.ow, 1);
        m.out_s = twin[i] ? desc(tw_off[i], m.oc, m.oh, m.ow, 1) : TDesc();
        m.st_out = m.st_rb = m.st_h1 = StatsRef();
        if (s_slices[i]) {
            m.st_out.p = reinterpret_cast<double *>(c->arena + so_off[i]);
            m.st_rb.p = reinterpret_cast<double *>(c->arena + sr_off[i]);
            m.st_h1.p = reinterpret_cast<double *>(c->arena + sh_off[i]);
            m.st_out.slices = m.st_rb.slices = s_out[i];
            m.st_h1.slices = s_h1[i];
            m.slices_default = s_out[i];
            if (!s_out[i]) m.st_out = m.st_rb = StatsRef();      // shape without fused statistics: the statistics kernel runs
            if (!s_h1[i]) m.st_h1 = StatsRef();
            if (!(m.kind == M_RES && m.rb.attn)) m.st_rb = m.st_out;   // rb_out aliases out
        }
        if (!m.st_out.p || (m.kind == M_RES && (!m.st_h1.p || !m.st_rb.p))) all_fused = false;
        if (m.kind == M_UP || m.kind == M_DOWN) m.up_in = desc(a1_off[i], m.conv.cin, m.ih, m.iw, 1);
        if (m.kind == M_RES) {
            m.act1 = desc(a1_off[i], m.rb.cin, m.oh, m.ow, 1);
            m.act2 = desc(a2_off[i], m.oc, m.oh, m.ow, 1);
            m.h1 = desc(h1_off[i], m.oc, m.oh, m.ow, 1);
            if (m.rb.has_res) m.raw1 = desc(raw_off[i], m.rb.cin, m.oh, m.ow, 1);
        }
    }
    c->x0 = desc(o_x0, c->in_pad, H, W, 1);
    c->x0s = desc(o_x0s, c->in_pad, H, W, 1);
    c->x0p = ci_ok ? at(o_x0p) : nullptr;
    c->eps = desc(o_eps, g.out_channel, H, W, 0);
    c->xhist = at(o_hist);
    c->final_act = desc(o_fa, c->final_gn.C, H, W, 1);
    c->qkvb = at(o_qkv); c->aob = at(o_ao); c->vtb = at(o_vt);
    c->part = max_part ? at(o_part) : nullptr;
    c->wino_ws = max_wino ? at(o_wino) : nullptr;
    c->gscale = at(o_gs); c->gshift = at(o_gh); c->gpart = at(o_gp);
    c->temb = at(o_te); c->cbias = at(o_cb);
    c->all_fused = all_fused;
    c->cap_part = max_part; c->cap_wino = max_wino; c->cap_vt = max_vt; c->cap_gpart = gn_workspace_floats(B, c->c_max);
    c->wB = B; c->wH = H; c->wW = W;
    return 0;
}

// Elastic row steps (sr3_rows_step_batch): does a step over `b` < wB images fit the workspace carved for wB? The same
// questions ensure_workspace asked at wB, asked at b: split-K partials, Winograd workspace, v^T scratch and GroupNorm
// partials must not exceed what was carved, the statistics slices per image must be the ones the buffers were laid out
// for, and a plan must not want a weight layout nobody made. In batch-invariant mode all of it follows from the plans
// being those of the planning batch (part_floats = phases * splits * M * Cout with splits a function of P: monotone in
// the batch); this check is what keeps a later change of a plan from launching past a buffer. 0, or -1 with the error set.
int rows_batch_fits(sr3_ctx *c, int b) {
    size_t at = 0;
    int bad = 0;
    auto ask = [&](const ConvRef &cr, int ih, int iw, int stride, int up2) {
        const int slices = at < c->conv_slices.size() ? c->conv_slices[at] : -1;
        ++at;
        for (int v = 0; v < 4 && !bad; ++v) {
            const ConvPlan pl = conv_plan_offered(b, ih, iw, cr.cin_pad, cr.cout, cr.ks, stride, up2, v & 1, false, (v & 2) != 0);
            if (pl.part_floats > c->cap_part)
                bad = fail("internal: a step over %d of %d rows wants %llu floats of split-K partials (conv %d -> %d at %dx%d), the workspace holds %llu",
                           b, c->wB, (unsigned long long)pl.part_floats, cr.cin, cr.cout, ih, iw, (unsigned long long)c->cap_part);
            else if (pl.stats_slices != slices)
                bad = fail("internal: a step over %d of %d rows leaves %d statistics slices per image (conv %d -> %d at %dx%d), the workspace was laid out for %d",
                           b, c->wB, pl.stats_slices, cr.cin, cr.cout, ih, iw, slices);
            else if (wino_weights(c->params[cr.w])) {
                if (pl.wino_ws_floats > c->cap_wino)
                    bad = fail("internal: a step over %d of %d rows wants %llu floats of Winograd workspace (conv %d -> %d at %dx%d), the workspace holds %llu",
                               b, c->wB, (unsigned long long)pl.wino_ws_floats, cr.cin, cr.cout, ih, iw, (unsigned long long)c->cap_wino);
                else if ((pl.needs_wino_frag || pl.wino_fused_rows) && !c->params[cr.w].dev_wino_f)
                    bad = fail("internal: a step over %d of %d rows wants fragment-major Winograd weights (conv %d -> %d at %dx%d) that the plans of the workspace never asked for",
                               b, c->wB, cr.cin, cr.cout, ih, iw);
            }
        }
    };
    for (const Module &m : c->mods) {
        if (bad) break;
        if (m.kind == M_RES) {
            ask(m.rb.c1, m.oh, m.ow, 1, 0);
            ask(m.rb.c2, m.oh, m.ow, 1, 0);
            if (m.rb.attn) {
                ask(m.rb.qkv, m.oh, m.ow, 1, 0);
                ask(m.rb.aout, m.oh, m.ow, 1, 0);
                for (const bool split : {false, true})
                    if (!bad && attention_core(split, (long)m.oh * m.ow, m.oc) == ATTN_SPLIT &&
                        attention_vt_floats(b, m.oh * m.ow, m.oc) > c->cap_vt)
                        bad = fail("internal: a step over %d of %d rows wants more attention scratch than the workspace holds", b, c->wB);
            }
        } else {
            ask(m.conv, m.ih, m.iw, m.kind == M_DOWN ? 2 : 1, m.kind == M_UP ? 1 : 0);
        }
    }
    if (!bad && at != c->conv_slices.size()) bad = fail("internal: the workspace recorded %zu convs, its modules hold %zu", c->conv_slices.size(), at);
    if (!bad && gn_workspace_floats(b, c->c_max) > c->cap_gpart)
        bad = fail("internal: a step over %d of %d rows wants more GroupNorm partials than the workspace holds", b, c->wB);
    return bad;
}

// ---------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------
const TDesc kNone{};

// scratch of an apply pass: scale / shift [B][C] of the finalize launch, partials of the statistics kernel (gn_workspace_floats)
struct GnScratch { float *scale = nullptr, *shift = nullptr, *part = nullptr; };

// the second output of an apply pass that also multiplies the block's 1x1 res_conv (launch_gn_res1x1)
struct GnRes1x1 { const float *w2 = nullptr; TDesc out; };

// the launches of one apply pass on `route`; statistics the producers did not fuse come from the streaming statistics
// kernel over the (fp32) tensors, whose partials describe the virtual concatenation as one source of a.C + b.C channels
void launch_gn_act(GnRoute route, const TDesc &a, const TDesc &b, int B, int groups, const float *gamma, const float *beta, int mode,
                   int fmt, const TDesc &act, const StatsRef &sa, const StatsRef &sb, const GnScratch &ws, const TDesc &raw, int in_split,
                   float *U, int *ovf, const DropLayer &drop, hipStream_t s, const GnRes1x1 *res = nullptr) {
    StatsRef s0 = sa, s1 = sb;
    int C0 = a.C, C1 = b.p ? b.C : 0;
    if (!gn_stats_fused(b, sa, sb)) {
        s0 = launch_groupnorm_partials(a, b, B, ws.part, s);
        s1 = StatsRef();
        C0 += C1; C1 = 0;
    }
    if (res) {
        // block1's pass together with the block's 1x1 res_conv (gn_res1x1_gate said so): always behind a finalize launch
        launch_groupnorm_finalize(s0, C0, s1, C1, B, a.H * a.W, groups, gamma, beta, 1e-5f, ws.scale, ws.shift, s);
        launch_gn_res1x1(a, b, B, ws.scale, ws.shift, act, res->w2, res->out, s);
        return;
    }
    if (route == GN_FINALIZE_ROWS) {
        launch_groupnorm_finalize(s0, C0, s1, C1, B, a.H * a.W, groups, gamma, beta, 1e-5f, ws.scale, ws.shift, s);
        if (U) launch_gn_wino_input(a, b, B, ws.scale, ws.shift, mode, U, s);
        else launch_gn_apply_rows(a, b, B, ws.scale, ws.shift, mode, fmt, act, s, raw, in_split, ovf, drop);
    } else {
        // statistics as partials: finalize + apply are ONE launch
        if (U) launch_gn_fold_wino_input(a, b, B, s0, s1, groups, gamma, beta, 1e-5f, mode, U, s);
        else launch_gn_fold_apply(a, b, B, s0, s1, groups, gamma, beta, 1e-5f, mode, fmt, act, s, raw, in_split, ovf, drop);
    }
}

// GroupNorm statistics + apply (+Swish) (+concat) -> activated, zero-bordered conv input
// f8: the consumer conv takes the F8C operand format (f8_conv() said so)
// U != null (gn_writes_u() said so): the consumer is a three-pass Winograd conv and the pass writes its transformed
// input there instead of `act` (the conv then runs with ConvParams::u_ready); the choice between the folded form and
// finalize + streaming form is the same either way, so no pass gains or loses a finalize launch
void run_gn_act(sr3_ctx *c, const TDesc &a, const TDesc &b, const GNRef &g, int B, int mode, const TDesc &act,
                const StatsRef &sa, const StatsRef &sb, const TDesc &raw = TDesc(), int in_split = 0, bool f8 = false,
                float *U = nullptr, const DropLayer &drop = DropLayer(), const GnRes1x1 *res = nullptr) {
    const int fmt = c->act_format(f8);
    if (U) ++c->gn_wino_passes;
    if (res) ++c->gn_res1x1_launches;
    // (with `res` the pass is bracketed in the conv family: most of its time is the 1x1 product, whose FLOPs conv2's
    // record counts as before)
    c->pbegin(res ? F_CONV : F_GN);
    GnScratch ws;
    ws.scale = c->gscale; ws.shift = c->gshift; ws.part = c->gpart;
    launch_gn_act(gn_route(a, b, B, sa, sb), a, b, B, c->cfg.norm_groups, c->params[g.gamma].dev, c->params[g.beta].dev, mode, fmt,
                  act, sa, sb, ws, raw, in_split, U, c->d_ovf, drop, c->stream, res);
    if (res && c->prof) c->pend(0.0, "gn_res1x1");
    else c->pend();
}

// One conv of the engine, by name (defaults = what most convs want)
struct ConvCall {
    TDesc in;                           // (a concatenation x ‖ skip is written as one tensor by the GroupNorm pass)
    const ConvRef *conv = nullptr;
    int B = 0, stride = 1, up2 = 0;
    bool activated = false;             // the input was written by launch_gn_apply and is in the context's precision format
    bool f8 = false;                    // ... in the F8C operand format (f8_conv() said so)
    const float *chan_bias = nullptr;   // FeatureWiseAffine bias rows
    const float *bias_override = nullptr;
    TDesc resid;                        // added to the output
    bool resid_split = false;           // ... which is stored in the split-f16 format
    TDesc out;
    StatsRef stats;                     // fused GroupNorm statistics of the output
    TDesc out_split;                    // split-f16 twin of the output (prec 1)
    bool out_f32 = true;                // false: only the twin is written (where there is one)
    // fused 1x1 term over in2 ‖ in2b: a res_conv, or (ident_w, prec 1) the identity skip as extra K-steps (ResBlock::ident_w)
    TDesc in2, in2b;
    const ConvRef *fused1x1 = nullptr;
    const float *ident_w = nullptr;
    bool u_ready = false;               // the GroupNorm pass wrote the Winograd input transform (gn_writes_u), `in` holds nothing
    bool res_ready = false;             // block1's GroupNorm pass left the fused 1x1 term in `out` (gn_res1x1_gate)
};

// the ConvParams of a ConvCall: what run_conv launches and what conv_plan is asked about before the conv's input exists
ConvParams conv_params(const sr3_ctx *c, const ConvCall &k) {
    const ConvRef &cv = *k.conv;
    const TDesc &a = k.in, &out = k.out;
    const int B = k.B;
    ConvParams p;
    p.in0 = a; p.B = B; p.Hout = out.H; p.Wout = out.W;
    p.ks = cv.ks; p.stride = k.stride; p.up2 = k.up2;
    p.prec = (k.activated && c->split()) ? 1 : 0;
    p.w = p.prec ? c->params[cv.w].dev_split : c->params[cv.w].dev;
    if (!p.prec && cv.cin_pad == a.C) {
        p.w_wino = c->params[cv.w].dev_wino; p.w_wino_f = c->params[cv.w].dev_wino_f; p.wino_ws = c->wino_ws;
        p.w_up_wino = c->params[cv.w].dev_up_wino;
    }
    if (k.f8 && p.prec) { p.f8 = 1; p.w = c->params[cv.w].dev_f8; }
    p.w_unscale = c->params[cv.w].w_unscale;
    p.bias = k.bias_override ? k.bias_override : (cv.b >= 0 ? c->params[cv.b].dev : nullptr);
    p.chan_bias = k.chan_bias; p.chan_bias_stride = c->cb_stride;
    p.resid = k.resid; p.out = out;
    if (c->split()) p.out_split = k.out_split;
    p.out_f32 = (k.out_f32 || !p.out_split.p) ? 1 : 0;
    p.resid_split = k.resid_split ? 1 : 0;
    if (k.stats.p) { p.stats = const_cast<double *>(k.stats.p); p.stats_slices = k.stats.slices; }
    p.part = c->part;
    p.tile_cnt = c->tile_cnt;
    p.no_halo_split = c->halo_split_off ? 1 : 0;
    p.ovf = c->d_ovf;
    if (k.fused1x1) {
        p.in2 = k.in2; p.in2b = k.in2b;
        p.w2 = p.prec ? c->params[k.fused1x1->w].dev_split : c->params[k.fused1x1->w].dev;
    } else if (k.ident_w && p.prec) {
        p.in2 = k.in2;
        p.w2 = k.ident_w;
    }
    p.u_ready = k.u_ready ? 1 : 0;
    p.res_ready = k.res_ready ? 1 : 0;
    return p;
}

// Does the GroupNorm apply pass in front of conv k write the conv's Winograd input transform (into c->wino_ws) instead
// of k.in? gn_pass_writes_u's answer for the conv's plan, asked before the conv's input exists
bool gn_writes_u(const sr3_ctx *c, const ConvCall &k, bool raw_wanted, int in_split) {
    return gn_pass_writes_u(c->split(), conv_plan(conv_params(c, k)), raw_wanted, in_split);
}

// launch_conv on the context's stream; counts the convs whose plan takes the one-kernel form of the three-pass Winograd
// plan or its tile-row form on the one-pass kernel, and the Upsample convs whose plan takes the sub-pixel Winograd form
static void ctx_launch_conv(sr3_ctx *c, const ConvParams &p) {
    const ConvPlan pl = conv_plan(p);
    if (pl.wino_gemm_out) ++c->wino_gemm_out_launches;
    if (pl.wino_fused_rows) ++c->wino_fused_rows_launches;
    if (pl.up2_wino) ++c->up2_wino_launches;
    launch_conv(p, c->stream);
}

void run_conv(sr3_ctx *c, const ConvCall &k) {
    const ConvRef &cv = *k.conv;
    const TDesc &a = k.in, &out = k.out;
    const int B = k.B;
    const ConvParams p = conv_params(c, k);
    c->pbegin(F_CONV);
    ctx_launch_conv(c, p);
    if (c->prof) {
        char tag[160];
        const int cin2 = k.fused1x1 ? k.fused1x1->cin : 0;
        snprintf(tag, sizeof tag, "conv k%d s%d u%d %dx%d cin%d(%d+%d) cout%d res%d fused1x1:%d prec%d%s", cv.ks, k.stride,
                 k.up2, out.H, out.W, cv.cin, a.C, 0, cv.cout, k.resid.p ? 1 : 0, cin2, p.prec, p.f8 ? " f8c" : "");
        c->pend(2.0 * (double)B * out.H * out.W * cv.cout * ((double)(cv.ks * cv.ks) * cv.cin + cin2), tag);
    }
}

// "f16f8" mode: does this ResnetBlock conv (3x3, stride 1, activated input of cin channels) take the F8C operand format?
bool f8_conv(const sr3_ctx *c, const ConvRef &cv, int B, int H, int W) {
    return c->f8() && cv.ks == 3 && c->params[cv.w].dev_f8 != nullptr && conv_f8_supported(B, H, W, cv.cout, cv.cin);
}

TDesc unpadded(float *p, int C, int H, int W) {
    TDesc d; d.p = p; d.C = C; d.H = H; d.W = W; d.pad = 0; return d;
}

// ResnetBlock.forward (unet.py:105-110) + SelfAttention.forward (unet.py:123-142)
// sx / ss: fused statistics of x / skip (written by the convs that produced them)
// xr / skr: what the fused res_conv reads as x / skip — the fp32 tensors themselves in prec 0, their
// split twins in prec 1; xr.p == null: no twin, the GroupNorm pass stores the raw concatenation
// x_so / sk_so: x / skip exist ONLY as their split twins xr / skr this forward; out_so: write this
// block's output only as its twin
void run_res(sr3_ctx *c, Module &m, const TDesc &x, const StatsRef &sx, const TDesc &skip, const StatsRef &ss, int B,
             const TDesc &xr, const TDesc &skr, bool x_so = false, bool sk_so = false, bool out_so = false) {
    const ResBlock &rb = m.rb;
    const int h = m.oh, w = m.ow;
    // block1: GN+Swish(x ‖ skip) -> conv3x3 + bias + FeatureWiseAffine bias; the same pass stores
    // the raw concatenation for the fused res_conv
    const bool direct = rb.has_res && xr.p && (!skip.p || skr.p);
    // (conv2's fused 1x1 K-steps read x / skip — or the raw concatenation — in 32-channel chunks of the plain split format)
    const bool fused_ok = !rb.has_res || (direct ? ((xr.C % 32) == 0 && (!skip.p || (skr.C % 32) == 0)) : (rb.cin % 32) == 0);
    const bool f8a = f8_conv(c, rb.c1, B, h, w), f8b = fused_ok && f8_conv(c, rb.c2, B, h, w);
    // (each conv's plan is asked before its GroupNorm pass runs: the pass writes U for a three-pass Winograd conv)
    ConvCall k1;
    k1.in = m.act1; k1.conv = &rb.c1; k1.B = B; k1.activated = true; k1.f8 = f8a;
    k1.chan_bias = c->cbias + rb.nf_off;
    k1.out = m.h1; k1.stats = m.st_h1;
    const bool raw1 = rb.has_res && !direct;
    const int in_split1 = (x_so ? 1 : 0) | (skip.p && sk_so ? 2 : 0);
    const ConvPlan pl1 = conv_plan(conv_params(c, k1));
    k1.u_ready = gn_pass_writes_u(c->split(), pl1, raw1, in_split1);
    // the same pass multiplies the res_conv into the block's output where conv2 would run it as a side launch
    ConvCall q2;                         // (what conv2's plan depends on)
    q2.in = m.act2; q2.conv = &rb.c2; q2.B = B; q2.activated = true; q2.f8 = f8b; q2.out = m.rb_out; q2.stats = m.st_rb;
    GnRes1x1 res1;
    ConvPlan pl2;                        // (asked only where the rest of the gate can say yes)
    if (!c->split() && rb.has_res && direct) pl2 = conv_plan(conv_params(c, q2));
    const bool res_pass = gn_res1x1_gate(c->split() ? 1 : 0, rb.has_res, direct, raw1, in_split1, 2, k1.u_ready, pl1.wino_fused_rows,
                                         pl2, B, h, w, x.C, skip.p ? skip.C : 0, rb.cout).takes();
    if (res_pass) { res1.w2 = c->params[rb.res.w].dev; res1.out = m.rb_out; }
    run_gn_act(c, x_so ? xr : x, (skip.p && sk_so) ? skr : skip, rb.gn1, B, 2, m.act1, sx, ss, raw1 ? m.raw1 : kNone, in_split1,
               f8a, k1.u_ready ? c->wino_ws : nullptr, DropLayer(), res_pass ? &res1 : nullptr);
    // block1's conv + FeatureWiseAffine bias writes the fp32 h1, then block2's GroupNorm + Swish as the apply pass over it
    run_conv(c, k1);
    // block2 + skip path in one launch: conv3x3(act2) [+ res_conv 1x1 (raw x ‖ skip) as extra
    // K-steps | + x as residual when the block keeps its width]
    ConvCall k2;
    k2.in = m.act2; k2.conv = &rb.c2; k2.B = B; k2.activated = true; k2.f8 = f8b;
    k2.out = m.rb_out; k2.stats = m.st_rb; k2.out_f32 = !out_so;
    k2.out_split = rb.attn ? kNone : m.out_s;      // with attention the out-projection writes the module output
    if (rb.has_res) {
        k2.in2 = direct ? xr : m.raw1; k2.in2b = direct && skip.p ? skr : kNone;
        k2.fused1x1 = &rb.res; k2.bias_override = rb.fused_bias;
        k2.res_ready = res_pass;
    } else if (c->split() && rb.ident_w && xr.p) {
        k2.in2 = xr; k2.ident_w = rb.ident_w;
    } else {
        k2.resid = x_so ? xr : x; k2.resid_split = x_so;
    }
    // train-mode Dropout (unet.py:81-91: after block2's Swish, i.e. this pass's output): the masked instantiation of the
    // apply pass. A three-pass Winograd conv then runs behind the masked two-pass apply (gn_wino_input_kernel sees every
    // window pixel in up to four tiles and knows no mask): gn_writes_u answers no. block1, the attention norm and the
    // res_conv operand are never masked.
    DropLayer drop;
    if (c->drop_live()) {
        drop.a = &c->d_step->drop;
        drop.c1_hi = (uint32_t)(c->drop_layer + 1) << 24;
        drop.base = c->drop_base;
    }
    ++c->drop_layer;
    c->drop_base += (uint64_t)B * rb.cout * h * w;
    k2.u_ready = gn_writes_u(c, k2, drop.a != nullptr, 0);
    run_gn_act(c, m.h1, kNone, rb.gn2, B, 2, m.act2, m.st_h1, StatsRef(), TDesc(), 0, f8b, k2.u_ready ? c->wino_ws : nullptr,
               drop);
    run_conv(c, k2);
    if (rb.attn) {
        run_gn_act(c, m.rb_out, kNone, rb.agn, B, 1, m.act2, m.st_rb, StatsRef());
        const AttnCore core = attention_core(c->split(), (long)h * w, rb.cout);
        const bool split_attn = core == ATTN_SPLIT;
        ConvCall kq, ko;
        kq.in = m.act2; kq.conv = &rb.qkv; kq.B = B; kq.activated = true;
        kq.out = unpadded(c->qkvb, 3 * rb.cout, h, w);
        ko.in = unpadded(c->aob, rb.cout, h, w); ko.conv = &rb.aout; ko.B = B; ko.activated = split_attn;
        ko.resid = m.rb_out; ko.out = m.out; ko.stats = m.st_out; ko.out_split = m.out_s;
        if (split_attn) {
            // split-f16 mode: the qkv projection writes ONLY the split twin of its output, the attention core
            // multiplies hi/lo halfs (3 x v_mfma_f32_16x16x32_f16 per product) and hands its result to the out
            // projection in the same format
            kq.out_split = kq.out; kq.out_f32 = false;
            run_conv(c, kq);
            c->pbegin(F_ATTN);
            const double fl = launch_attention_split(c->qkvb, c->vtb, B, h * w, rb.cout, nullptr, c->aob, c->d_ovf, c->stream);
            c->pend(fl);
        } else {
            run_conv(c, kq);
            c->pbegin(F_ATTN);
            const double fl = core == ATTN_STREAM ? launch_attention_stream(c->qkvb, B, h * w, rb.cout, c->aob, c->stream)
                                                  : launch_attention(c->qkvb, B, h * w, rb.cout, c->aob, c->stream);
            c->pend(fl);
        }
        run_conv(c, ko);
    }
}

// The modules a shallow forward of `depth` runs: conv_in and the next depth * res_blocks + (depth - 1)
// down modules — everything in front of the Downsample that leaves level depth - 1 — are [0, down_end); the last
// depth * (res_blocks + 1) + (depth - 1) up modules are [up_begin, mods.size()). mods[up_begin - 1] is the Upsample that
// returns to level depth - 1: its output, as the last whole forward left it, is the cached feature.
struct ShallowSplit { int down_end, up_begin; };
ShallowSplit shallow_split(const sr3_ctx *c, int depth) {
    const int rb = c->cfg.res_blocks;
    return {1 + depth * rb + (depth - 1), (int)c->mods.size() - (depth * (rb + 1) + (depth - 1))};
}

// UNet.forward body (unet.py:240-265): consumes c->x0 and c->cbias, leaves eps NHWC in c->eps.
// depth > 0: the shallow forward (shallow_split); the caller has checked that the workspace holds a whole forward in the
// current arithmetic.
void run_unet_body(sr3_ctx *c, int B, int H, int W, int depth = 0) {
    std::vector<int> feats;
    c->drop_layer = 0; c->drop_base = 0;      // (run_res numbers the Dropout layers in execution order)
    const ShallowSplit sh = depth > 0 ? shallow_split(c, depth) : ShallowSplit{0, 0};
    TDesc cur = c->x0, cur_s;         // cur_s: split twin of cur (prec 1), null if none
    bool cur_so = false;              // cur exists only as cur_s
    StatsRef scur;
    // split-only mode: a module output that has a twin is written ONLY as the twin (4 instead of 8
    // bytes per element); GroupNorm apply and residual adds read hi + lo. Needs every GroupNorm to get
    // its statistics from a conv epilogue (the fallback statistics kernel reads fp32 tensors).
    const bool so_mode = c->split() && c->all_fused;
    const int n_pre = c->n_downs + c->n_mid;
    for (int i = 0; i < (int)c->mods.size(); ++i) {
        if (depth > 0 && i == sh.down_end) {
            // The jump of the shallow forward. The Dropout cursor advances over the skipped ResnetBlocks, so a fresh up
            // block draws the masks it draws in a whole forward; the traversal continues from the cached Upsample's
            // output, twin and statistics (so_now of an Upsample is a function of the arithmetic, which is the cache's).
            for (int j = i; j < sh.up_begin; ++j) {
                const Module &s = c->mods[j];
                if (s.kind != M_RES) continue;
                ++c->drop_layer;
                c->drop_base += (uint64_t)B * s.rb.cout * s.oh * s.ow;
            }
            const Module &cm = c->mods[sh.up_begin - 1];
            cur = cm.out; cur_s = cm.out_s; cur_so = so_mode && cm.out_s.p; scur = cm.st_out;
            i = sh.up_begin;
        }
        Module &m = c->mods[i];
        const bool is_up_path = i >= n_pre;
        ConvCall k;                       // the module's own conv (conv_in, Downsample, Upsample)
        k.conv = &m.conv; k.B = B; k.out = m.out; k.stats = m.st_out; k.out_split = m.out_s;     // (the twin: prec 1 only)
        switch (m.kind) {
        case M_CONV_IN:
            m.st_out.slices = m.slices_default;
            k.stats = m.st_out;
            if (c->split() && c->x0p) {
                // downs.0 on the packed split-f16 state (kernels_edge.hip): 3 K-steps of 24 live k-values instead
                // of 9 K-steps of 32 mostly-zero channels, no split copy of the state tensor
                if (m.st_out.p) m.st_out.slices = H * W / 256;       // one statistics slice per 256-pixel block
                c->pbegin(F_CONV);
                launch_conv_in(c->x0p, c->ci_w, m.conv.b >= 0 ? c->params[m.conv.b].dev : nullptr, c->ci_unscale, B, m.out,
                               m.out_s, !(so_mode && m.out_s.p), const_cast<double *>(m.st_out.p),
                               m.st_out.slices, c->d_ovf, c->stream);
                if (c->prof) {
                    char tag[160];
                    snprintf(tag, sizeof tag, "conv_in k3 %dx%d cin%d cout%d packed-state mfma16", H, W, m.conv.cin, m.conv.cout);
                    c->pend(2.0 * (double)B * H * W * m.conv.cout * 9.0 * m.conv.cin, tag);
                }
            } else if (c->split()) {   // the 6 (of 32 padded) input channels in split-f16 form: the first conv then runs
                                // on the fast path too instead of 9 mostly-zero K-steps of f32 MFMA
                c->pbegin(F_GN);
                launch_gn_apply_rows(cur, kNone, B, nullptr, nullptr, 0, 1, c->x0s, c->stream, TDesc(), 0, c->d_ovf);
                c->pend();
                k.in = c->x0s; k.activated = true; k.out_f32 = !(so_mode && m.out_s.p);
                run_conv(c, k);
            } else if (conv_in_f32_gate(c->split(), c->cfg.in_channel, m.conv.cout, H, W) && cur.pad == 1 && cur.C >= 8 &&
                       (!m.st_out.p || H * W / 256 <= m.slices_default)) {
                // downs.0 in exact f32 on the state tensor itself (kernels_edge.hip): 72 k-values per output instead of
                // the generic kernel's 9 K-steps of 32 mostly-zero channels; weights: the parameter's packed copy
                if (m.st_out.p) m.st_out.slices = H * W / 256;       // one statistics slice per 256-pixel block
                c->pbegin(F_CONV);
                launch_conv_in_f32(cur, c->params[m.conv.w].dev, m.conv.cin_pad, m.conv.b >= 0 ? c->params[m.conv.b].dev : nullptr,
                                   B, m.out, const_cast<double *>(m.st_out.p), m.st_out.slices, c->stream);
                ++c->conv_in_f32_launches;
                if (c->prof) {
                    char tag[160];
                    snprintf(tag, sizeof tag, "conv_in k3 %dx%d cin%d cout%d f32 mfma", H, W, m.conv.cin, m.conv.cout);
                    c->pend(2.0 * (double)B * H * W * m.conv.cout * 9.0 * m.conv.cin, tag);
                }
            } else {
                k.in = cur;
                run_conv(c, k);
            }
            break;
        case M_DOWN:
        case M_UP: {
            k.stride = m.kind == M_DOWN ? 2 : 1; k.up2 = m.kind == M_UP ? 1 : 0;
            if (c->split() && cur_s.p) {        // the producer left a split-f16 twin: read it directly
                k.in = cur_s; k.activated = true; k.out_f32 = !(so_mode && m.out_s.p);
            } else if (c->split()) {            // no twin: re-store the raw input in split-f16 form first
                c->pbegin(F_GN);
                launch_gn_apply(cur, kNone, B, nullptr, nullptr, 0, 1, m.up_in, c->stream, TDesc(), 0, c->d_ovf);
                c->pend();
                k.in = m.up_in; k.activated = true;
            } else {
                k.in = cur;
            }
            run_conv(c, k);
            break;
        }
        case M_RES:
            if (is_up_path) {
                Module &sk = c->mods[feats.back()];
                feats.pop_back();
                if (c->split()) run_res(c, m, cur, scur, sk.out, sk.st_out, B, cur_s, sk.out_s, cur_so, sk.so_now,
                                     so_mode && m.out_s.p && !m.rb.attn);
                else run_res(c, m, cur, scur, sk.out, sk.st_out, B, cur, sk.out);
            } else {
                if (c->split()) run_res(c, m, cur, scur, kNone, StatsRef(), B, cur_s, kNone, cur_so, false,
                                     so_mode && m.out_s.p && !m.rb.attn);
                else run_res(c, m, cur, scur, kNone, StatsRef(), B, cur, kNone);
            }
            break;
        }
        m.so_now = so_mode && m.out_s.p && !(m.kind == M_RES && m.rb.attn);
        cur = m.out;
        cur_s = m.out_s;
        cur_so = m.so_now;
        scur = m.st_out;
        if (i < c->n_downs) feats.push_back(i);
    }
    if (c->final_wq && !cur_so) {
        // final_conv (unet.py:229,263): GroupNorm + Swish + Conv3x3(C -> 3) as ONE fp32 VALU kernel behind the
        // statistics finalize — no activated copy of the 128x128 tensor, no MFMA tile that is 29/32 padding
        const GNRef &g = c->final_gn;
        c->pbegin(F_GN);
        if (scur.p)
            launch_groupnorm_finalize(scur, cur.C, StatsRef(), 0, B, cur.H * cur.W, c->cfg.norm_groups, c->params[g.gamma].dev,
                                      c->params[g.beta].dev, 1e-5f, c->gscale, c->gshift, c->stream);
        else
            launch_groupnorm_affine(cur, kNone, B, c->cfg.norm_groups, c->params[g.gamma].dev, c->params[g.beta].dev, 1e-5f,
                                    c->gpart, c->gscale, c->gshift, c->stream);
        c->pend();
        c->pbegin(F_CONV);
        const bool mfma = c->split() && c->final_wm;
        if (mfma)
            launch_final_conv_mfma(cur, B, c->gscale, c->gshift, c->final_wm, c->final_unscale, c->params[c->final_conv.b].dev,
                                   c->eps, c->stream, c->d_ovf);
        else
            launch_final_conv(cur, B, c->gscale, c->gshift, c->final_wq, c->params[c->final_conv.b].dev, c->eps, c->stream);
        if (c->prof) {
            char tag[160];
            snprintf(tag, sizeof tag, "final_conv gn+swish+k3 %dx%d cin%d cout%d %s", H, W, cur.C, c->final_conv.cout,
                     mfma ? "per-pixel-mfma16+gather" : "fp32-valu");
            c->pend(2.0 * (double)B * H * W * c->final_conv.cout * 9.0 * cur.C, tag);
        }
        return;
    }
    run_gn_act(c, cur, kNone, c->final_gn, B, 2, c->final_act, scur, StatsRef());
    ConvCall k;
    k.in = c->final_act; k.conv = &c->final_conv; k.B = B; k.activated = true; k.out = c->eps;
    run_conv(c, k);
}

// the noise-level MLP and the concatenated FeatureWiseAffine linears of this context, writing temb / chan_bias
EmbedParams embed_params(const sr3_ctx *c, const float *nl, int stride, float *temb, float *chan_bias) {
    EmbedParams e;
    e.noise_level = nl; e.nl_stride = stride; e.dim = c->cfg.inner_channel;
    e.w1 = c->params[c->mlp_w1].dev; e.b1 = c->params[c->mlp_b1].dev;
    e.w2 = c->params[c->mlp_w2].dev; e.b2 = c->params[c->mlp_b2].dev;
    e.nfw = c->nfw; e.nfb = c->nfb; e.total = c->nf_total;
    e.temb = temb; e.chan_bias = chan_bias;
    return e;
}

void run_embed(sr3_ctx *c, const float *nl, int stride, int B) {
    const EmbedParams e = embed_params(c, nl, stride, c->temb, c->cbias);
    // sampler steps: the noise level is the same for every image (diffusion.py:166-167 repeats one scalar), so the
    // embedding and the FeatureWiseAffine biases are computed ONCE and every conv reads row 0 (stride 0)
    const bool uniform = stride == 0;
    c->cb_stride = uniform ? 0 : c->nf_total;
    c->pbegin(F_EMBED);
    launch_noise_embed(e, uniform ? 1 : B, c->stream);
    c->pend();
}

// ResnetBlocks with a res_conv run conv2 and the 1x1 res_conv as ONE launch (extra K-steps): the
// two biases are pre-added and, for the split-f16 weights, both tensors get the same 2^k scale.
// the host copy prepare_fused re-splits from: what sr3_load_weight kept, or, after a device refresh dropped it, the
// parameter's current device copy (the same values: the packed weights / the bias)
int fused_host(Param &p) {
    if (!p.host.empty()) return 0;
    p.host.resize(p.dev_floats);
    HIP_OK(hipMemcpy(p.host.data(), p.dev, p.dev_floats * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// The identity skip of a narrow block as extra K-steps of conv2 (ResBlock::ident_w): the split-f16 [cout][cout] matrix
// with 2^k of conv2's split weights on the diagonal, for conv2's packed weights w ([9][cout][cin_pad], n floats, currently
// split with w_unscale = 2^-k). The matrix holds 2^k as an fp16 number, so k <= 15 (2^16 is +inf in fp16 and the extra
// K-steps would compute x * inf: NaN). conv2 tensors with max|w| < 2^-5 (k >= 16; e.g. PyTorch's default init of a
// 128 -> 128 conv, bound 1/sqrt(1152)) are re-split with k = 15 into `resplit` (left empty otherwise): hi + lo then
// still carries the weight to 2^-24 absolute in scaled units (fp16 subnormal spacing), far below the 2^-22 relative
// accuracy of the format. Returns conv2's w_unscale to use from now on.
float ident_skip_weights(const float *w, size_t n, int cout, int cin_pad, float w_unscale, std::vector<float> &resplit,
                         std::vector<float> &ident) {
    resplit.clear();
    if (split_scale_exponent(w, n) > 15) {
        resplit.resize(n);
        w_unscale = split_conv_weight_k(w, (size_t)9 * cout, cin_pad, 15, resplit.data());
    }
    ident.assign((size_t)cout * cout, 0.f);
    _Float16 *h = reinterpret_cast<_Float16 *>(ident.data());
    const float v = 1.0f / w_unscale;                               // 2^k of conv2's split weights (k <= 15)
    for (int o = 0; o < cout; ++o) h[((size_t)o * cout + (o & ~31)) * 2 + (o & 31)] = (_Float16)v;
    return w_unscale;
}

int prepare_fused(sr3_ctx *c) {
    if (!c->fused_dirty) return 0;
    HIP_OK(hipStreamSynchronize(c->stream));
    for (auto &m : c->mods) {
        if (m.kind != M_RES) continue;
        if (m.rb.has_res) {
            for (int idx : {m.rb.c2.w, m.rb.c2.b, m.rb.res.w, m.rb.res.b})
                if (fused_host(c->params[idx])) return -1;
        } else if (ident_eligible(m.rb) && fused_host(c->params[m.rb.c2.w])) return -1;
    }
    for (auto &m : c->mods) {
        if (m.kind != M_RES || !ident_eligible(m.rb)) continue;
        ResBlock &rb = m.rb;
        const size_t n = (size_t)rb.cout * rb.cout;
        Param &w2 = c->params[rb.c2.w];
        std::vector<float> buf, sp;
        w2.w_unscale = ident_skip_weights(w2.host.data(), w2.host.size(), w2.cout, w2.cin_pad, w2.w_unscale, sp, buf);
        if (!sp.empty()) HIP_OK(hipMemcpy(w2.dev_split, sp.data(), w2.dev_floats * sizeof(float), hipMemcpyHostToDevice));
        if (!rb.ident_w) HIP_OK(hipMalloc(&rb.ident_w, n * sizeof(float)));
        HIP_OK(hipMemcpy(rb.ident_w, buf.data(), n * sizeof(float), hipMemcpyHostToDevice));
    }
    for (auto &m : c->mods) {
        if (m.kind != M_RES || !m.rb.has_res) continue;
        ResBlock &rb = m.rb;
        Param &w2 = c->params[rb.c2.w], &wr = c->params[rb.res.w];
        const Param &b2 = c->params[rb.c2.b], &br = c->params[rb.res.b];
        std::vector<float> bsum(rb.cout);
        for (int i = 0; i < rb.cout; ++i) bsum[i] = b2.host[i] + br.host[i];
        if (!rb.fused_bias) HIP_OK(hipMalloc(&rb.fused_bias, (size_t)rb.cout * sizeof(float)));
        HIP_OK(hipMemcpy(rb.fused_bias, bsum.data(), bsum.size() * sizeof(float), hipMemcpyHostToDevice));
        const int k = std::min(split_scale_exponent(w2.host.data(), w2.host.size()),
                               split_scale_exponent(wr.host.data(), wr.host.size()));
        std::vector<float> sp(std::max(w2.host.size(), wr.host.size()));
        w2.w_unscale = split_conv_weight_k(w2.host.data(), (size_t)9 * w2.cout, w2.cin_pad, k, sp.data());
        HIP_OK(hipMemcpy(w2.dev_split, sp.data(), w2.dev_floats * sizeof(float), hipMemcpyHostToDevice));
        wr.w_unscale = split_conv_weight_k(wr.host.data(), (size_t)wr.cout, wr.cin_pad, k, sp.data());
        HIP_OK(hipMemcpy(wr.dev_split, sp.data(), wr.dev_floats * sizeof(float), hipMemcpyHostToDevice));
    }
    c->fused_dirty = false;
    c->f8_dirty = true;          // conv2 / res_conv tensors were re-split with a common scale
    return 0;
}

// "f16f8" mode: F8C copies of the 3x3 conv weights (made on the device from the split-f16 copies; same byte size)
int prepare_f8(sr3_ctx *c) {
    if (!c->f8() || !c->f8_dirty) return 0;
    for (auto &p : c->params) {
        if (p.kind != P_CONV || p.ks != 3 || p.up_phase || (p.cin_pad % 32) != 0 || !p.dev_split) continue;
        if (!p.dev_f8) {
            HIP_OK(hipMalloc(&p.dev_f8, p.dev_floats * sizeof(float)));
            c->weight_bytes += p.dev_floats * sizeof(float);
        }
        launch_make_f8_weights(p.dev_split, p.dev_f8, p.dev_floats / 32, c->stream);
    }
    HIP_OK(hipGetLastError());
    c->f8_dirty = false;
    drop_graphs(c);              // (captured steps hold weight pointers; the copies may be new allocations)
    return 0;
}

// clears the range-check flag (stream-ordered; never inside a captured step)
int range_reset(sr3_ctx *c) {
    HIP_OK(hipMemsetAsync(c->d_ovf, 0, sizeof(int), c->stream));
    return 0;
}

// Synchronises the stream and fails if any kernel since the last reset stored a value beyond the
// fp16 range in the split-f16 format (such a value would otherwise corrupt the residual stream
// silently). The flag is cleared either way.
// synchronises, reads and clears the flag: 0 in range, 1 overflow, -1 HIP error, and
// 2: a bounded inter-block wait of the in-place split-K on x-halo tiles gave up (SR3_FLAG_WAIT_TIMEOUT) — some other kernel
//    held the CU slots the tile's sibling blocks needed. Everything computed since the last reset is invalid (the flag may
//    carry a bogus overflow bit from the incomplete sums as well). The context is switched to the conv path whose blocks
//    never wait for each other (halo_split_off; captured graphs dropped) and the CALLER REPLAYS the work: the call still
//    finishes with a correct result, it never hangs and never fails for this reason.
int range_read(sr3_ctx *c) {
    HIP_OK(hipMemcpyAsync(c->h_ovf, c->d_ovf, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (*c->h_ovf == 0) return 0;
    const int v = *c->h_ovf;
    HIP_OK(hipMemsetAsync(c->d_ovf, 0, sizeof(int), c->stream));
    if (v & SR3_FLAG_WAIT_TIMEOUT) {
        c->halo_split_off = true;
        drop_graphs(c);
        // (every block still counts its arrival and departure, so the counters return to zero by themselves; the stream
        // is idle here, so clearing them is free insurance)
        HIP_OK(hipMemsetAsync(c->tile_cnt, 0, CONV_TILE_COUNTERS * sizeof(unsigned), c->stream));
        return 2;
    }
    return 1;
}

// the call was finished after replaying work whose in-place split-K wait had timed out (range_read == 2)
int warn_replay(sr3_ctx *c, const char *what, const char *redo) {
    char buf[640];
    snprintf(buf, sizeof buf, "%s: another kernel held the compute units that the blocks of an in-place split-K conv tile "
             "wait for each other on, and the bounded wait (5 ms) gave up; %s was recomputed on the conv path without "
             "inter-block waits, which this context uses from now on (slightly slower at the 8x8 level). The result is "
             "complete and valid. SR3_HALO_SPLITS=0 selects that path from the start.", what, redo);
    g_warn = buf;
    ++c->replay_calls;
    return SR3_OK_REPLAYED;
}

// to_f16x3: only the fp8 operand range of the "f16f8" mode was exceeded and the plain split-f16 arithmetic held the rest
int warn_fallback(sr3_ctx *c, const char *what, const char *redo, bool to_f16x3 = false) {
    char buf[640];
    if (to_f16x3)
        snprintf(buf, sizeof buf, "%s: an activation exceeded the fp8 operand range (|v| > %g) of the f16f8 arithmetic; %s was "
                 "recomputed with all three products on the f16 matrix path (f16x3). sr3_set_range_policy(ctx, 1) makes "
                 "this an error instead; sr3_set_precision(ctx, 1) avoids the retry.", what, (double)SPLIT_F8_MAX, redo);
    else
    snprintf(buf, sizeof buf, "%s: an activation exceeded the fp16 range (|v| > 65504) of the split-f16 format; %s was "
             "recomputed in the exact f32 arithmetic (the reference computes in fp32 and has no such limit). "
             "sr3_set_range_policy(ctx, 1) makes this an error instead; sr3_set_precision(ctx, 0) avoids the retry.",
             what, redo);
    g_warn = buf;
    ++c->fallback_calls;
    return SR3_OK_F32_FALLBACK;
}

int range_fail(sr3_ctx *c, const char *what) {
    if (c->f8())
        return fail("%s: an activation exceeded the operand range of the f16f8 arithmetic — the fp8 range (|v| > %g) in a "
                    "conv on the fp8 correction path, or the fp16 range (|v| > 65504) of the split-f16 format elsewhere; "
                    "the result is invalid — run this model in f16x3 (sr3_set_precision(ctx, 1): no fp8 operands) or, if "
                    "that overflows too, with the exact f32 arithmetic (sr3_set_precision(ctx, 0))", what, (double)SPLIT_F8_MAX);
    return fail("%s: an activation exceeded the fp16 range (|v| > 65504) of the split-f16 format; the result is "
                "invalid — run this model with the exact f32 arithmetic (sr3_set_precision(ctx, 0))", what);
}

// step API / single ops: the caller owns the inputs, the library cannot replay — fail, naming the remedy
int range_check(sr3_ctx *c, const char *what) {
    const int r = range_read(c);
    if (r <= 0) return r;
    if (r == 2)
        return fail("%s: another kernel held the compute units an in-place split-K conv waits on and its bounded wait gave "
                    "up: this result is invalid; the context now uses the conv path without inter-block waits — repeat the "
                    "call (sr3_sample / sr3_unet_forward replay by themselves)", what);
    return range_fail(c, what);
}

// ---- the range policy of the split-f16 modes -----------------------------------------------------------------------
// One rung down the ladder f16f8 -> f16x3 (the fp8 operands have the narrower range) -> exact f32 (to_f32: straight to
// the bottom); returns the rung landed on.
Arith step_down(sr3_ctx *c, bool to_f32 = false) {
    c->mode = (to_f32 || c->mode == A_F16X3) ? A_F32 : A_F16X3;
    return c->mode;
}

// puts the context's arithmetic back on every exit path of a call that may step down
struct ModeScope {
    sr3_ctx *c;
    const Arith was;
    explicit ModeScope(sr3_ctx *ctx) : c(ctx), was(ctx->mode) {}
    ModeScope(const ModeScope &) = delete;
    ~ModeScope() { c->mode = was; }
};

// The range policy for an entry point that OWNS ITS INPUTS, so that repeating the work is the same evaluation again.
// `once` enqueues one evaluation in the context's current arithmetic (0, or -1 with the error set); `what` names the
// entry point and `redo` what was recomputed in the warnings. Clean flag: done. A split-K wait that gave up
// (range_read == 2): again on the non-waiting path, same arithmetic. Out of range: the call fails under the strict
// policy (and where may_step_down is false: a single op keeps the arithmetic it was asked for), else it is evaluated one
// arithmetic down (step_down) until a rung is clean or f32, which has no range limit, is reached.
template <class Once>
int guarded_eval(sr3_ctx *c, const char *what, const char *redo, bool may_step_down, Once &&once) {
    if (range_reset(c) || once()) return -1;
    if (!c->split()) return 0;
    int r = range_read(c);
    bool replayed = false;
    if (r == 2) {
        replayed = true;
        if (range_reset(c) || once()) return -1;
        r = range_read(c);
        if (r == 2) return fail("internal: inter-block wait flag raised with the in-place split-K disabled");
    }
    if (r < 0) return -1;
    if (r == 0) return replayed ? warn_replay(c, what, redo) : 0;
    if (c->strict_range || !may_step_down) return range_fail(c, what);
    ModeScope scope(c);
    while (step_down(c) != A_F32) {
        if (range_reset(c) || once()) return -1;
        const int r16 = range_read(c);
        if (r16 < 0) return -1;
        if (r16 == 0) return warn_fallback(c, what, redo, true);
    }
    if (range_reset(c) || once()) return -1;
    return warn_fallback(c, what, redo);
}

int check_ready(sr3_ctx *c) {
    if (!c) return fail("null context");
    HIP_OK(hipSetDevice(c->device));
    for (auto &p : c->params)
        if (!p.loaded) return fail("weight '%s' was never loaded (sr3_load_weight)", p.name.c_str());
    if (prepare_fused(c)) return -1;
    return prepare_f8(c);
}

// every captured step: what the UNet body bakes in changed (StepKey covers the update half by itself)
void drop_graphs(sr3_ctx *c) {
    for (StepGraph &g : c->step_graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    c->step_graphs.clear();
}

// The per-call arguments kernels read from device memory (StepArgs): a pinned host ring slot, filled by the caller and
// copied to c->d_step by push_step_args. next_step_slot: null with the error set.
StepArgs *next_step_slot(sr3_ctx *c) {
    if (!c->h_ring) {
        if (hipHostMalloc(reinterpret_cast<void **>(&c->h_ring), sizeof(StepArgs) * sr3_ctx::kRing, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(&c->d_step, sizeof(StepArgs)) != hipSuccess) {
            fail("allocating the step arguments failed");
            return nullptr;
        }
    }
    // the host may run far ahead of the GPU: never reuse a ring slot that may still be pending
    if (c->step_count && (c->step_count % (sr3_ctx::kRing / 2)) == 0 && hipStreamSynchronize(c->stream) != hipSuccess) {
        fail("hipStreamSynchronize failed");
        return nullptr;
    }
    StepArgs *sa = &c->h_ring[c->step_count % sr3_ctx::kRing];
    ++c->step_count;
    *sa = StepArgs();
    return sa;
}
int push_step_args(sr3_ctx *c, const StepArgs *sa) {
    HIP_OK(hipMemcpyAsync(c->d_step, sa, sizeof(StepArgs), hipMemcpyHostToDevice, c->stream));
    return 0;
}

// Dropout layers of the UNet at H x W, in execution order (= the order of the reference's nn.Dropout modules): chw[3*l..]
// = {C, H, W} of layer l's block2 input (chw may be null); returns the bytes of one image's masks over all layers
uint64_t dropout_layers(const sr3_ctx *c, int H, int W, int *chw) {
    uint64_t per_image = 0;
    int h = H, w = W, l = 0;
    for (const Module &m : c->mods) {
        if (m.kind == M_DOWN) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
        else if (m.kind == M_UP) { h *= 2; w *= 2; }
        if (m.kind != M_RES) continue;
        if (chw) { chw[3 * l] = m.rb.cout; chw[3 * l + 1] = h; chw[3 * l + 2] = w; }
        ++l;
        per_image += (uint64_t)m.rb.cout * h * w;
    }
    return per_image;
}

// the mask stream's arguments of one call (draw: StepArgs::draw in the sampler, 0 elsewhere); the injected buffer must
// hold exactly the layers of the current workspace
int fill_drop_args(sr3_ctx *c, const char *what, DropArgs &d, uint32_t draw, uint64_t image_offset) {
    if (draw >= DROP_MAX_DRAW) return fail("%s: dropout draw index %u does not fit the mask stream's 24 bits", what, draw);
    if (c->drop_masks) {
        const uint64_t need = (uint64_t)c->wB * dropout_layers(c, c->wH, c->wW, nullptr);
        if (c->drop_mask_bytes != need)
            return fail("%s: the injected dropout masks hold %llu bytes, B=%d H=%d W=%d needs %llu (sr3_dropout_mask_bytes)", what,
                        (unsigned long long)c->drop_mask_bytes, c->wB, c->wH, c->wW, (unsigned long long)need);
    }
    d.seed = c->drop_seed; d.image_offset = image_offset; d.mask = c->drop_masks;
    d.draw = draw; d.thr = c->drop_thr; d.s = c->drop_s; d.pad_ = 0;
    return 0;
}
// sr3_unet_forward / sr3_denoise_loss with dropout live: the arguments go to the device once, in front of guarded_eval
// (every repeat of the evaluation reads the same ones)
int push_drop_args(sr3_ctx *c, const char *what, uint64_t image_offset) {
    if (!c->drop_live()) return 0;
    StepArgs *sa = next_step_slot(c);
    if (!sa || fill_drop_args(c, what, sa->drop, 0, image_offset)) return -1;
    return push_step_args(c, sa);
}

// ---- low-resolution consistency: operators and buffers ---------------------------------------------------------------
int check_lr_shape(const char *what, int C, int H, int W, int N, int lh, int lw) {
    if (C <= 0 || N <= 0 || lh <= 0 || lw <= 0 || H <= lh || W <= lw)
        return fail("%s: needs C, N > 0 and an LR size below the image size on both axes (got C=%d N=%d, %dx%d -> %dx%d)", what, C,
                    N, lh, lw, H, W);
    return 0;
}

// the device operators of (lh, lw) -> (H, W), built on first use and kept for the life of the context (captured steps
// hold their addresses)
int get_lr_ops(sr3_ctx *c, int lh, int lw, int H, int W, LrOps *out) {
    const auto key = std::make_tuple(lh, lw, H, W);
    auto it = c->lr_ops.find(key);
    if (it != c->lr_ops.end()) { *out = it->second.ops; return 0; }
    std::vector<double> Av((size_t)lh * H), Pv((size_t)H * lh), Ah((size_t)lw * W), Ph((size_t)W * lw);
    std::vector<int> bnd((size_t)2 * (lh + lw));
    if (!lr_operators(lh, H, Av.data(), Pv.data(), bnd.data()) || !lr_operators(lw, W, Ah.data(), Ph.data(), bnd.data() + 2 * lh))
        return fail("low-resolution operators %dx%d -> %dx%d: the Gram matrix is not positive definite", lh, lw, H, W);
    // A_v | A_h | P_v | P_h^T
    const size_t nAv = Av.size(), nAh = Ah.size(), nPv = Pv.size(), nPh = Ph.size();
    std::vector<float> h(nAv + nAh + nPv + nPh);
    for (size_t i = 0; i < nAv; ++i) h[i] = (float)Av[i];
    for (size_t i = 0; i < nAh; ++i) h[nAv + i] = (float)Ah[i];
    for (size_t i = 0; i < nPv; ++i) h[nAv + nAh + i] = (float)Pv[i];
    for (int x = 0; x < W; ++x)
        for (int j = 0; j < lw; ++j) h[nAv + nAh + nPv + (size_t)j * W + x] = (float)Ph[(size_t)x * lw + j];
    sr3_ctx::LrDev d;
    HIP_OK(hipMalloc(&d.buf, h.size() * sizeof(float)));
    if (hipMalloc(&d.bounds, bnd.size() * sizeof(int)) != hipSuccess) { (void)hipFree(d.buf); return fail("allocating the LR operators failed"); }
    if (hipMemcpy(d.buf, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d.bounds, bnd.data(), bnd.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d.buf); (void)hipFree(d.bounds);
        return fail("uploading the LR operators failed");
    }
    d.ops.Av = d.buf; d.ops.Ah = d.buf + nAv; d.ops.Pv = d.buf + nAv + nAh; d.ops.PhT = d.buf + nAv + nAh + nPv;
    d.ops.bv = d.bounds; d.ops.bh = d.bounds + 2 * lh;
    d.ops.lh = lh; d.ops.lw = lw; d.ops.H = H; d.ops.W = W;
    c->lr_ops[key] = d;
    *out = d.ops;
    return 0;
}

// scratch of the multi-launch form / the residual score (a member of the StepKey of the steps that take it)
int ensure_lr_scratch(sr3_ctx *c, size_t floats) {
    if (c->lr_scratch_n >= floats) return 0;
    HIP_OK(hipStreamSynchronize(c->stream));
    if (c->lr_scratch) HIP_OK(hipFree(c->lr_scratch));
    c->lr_scratch = nullptr; c->lr_scratch_n = 0;
    HIP_OK(hipMalloc(&c->lr_scratch, floats * sizeof(float)));
    c->lr_scratch_n = floats;
    return 0;
}

// the x0 prediction between the halves of the update (projection and dynamic threshold share it; a member of the StepKey)
int ensure_x0hat(sr3_ctx *c, size_t need) {
    if (c->x0hat_floats >= need) return 0;
    HIP_OK(hipStreamSynchronize(c->stream));
    if (c->x0hat) HIP_OK(hipFree(c->x0hat));
    c->x0hat = nullptr; c->x0hat_floats = 0;
    HIP_OK(hipMalloc(&c->x0hat, need * sizeof(float)));
    c->x0hat_floats = need;
    return 0;
}

// sr3_sample_begin with the feature on: operators, form, x0 buffer and scratch of this call's shape
int prepare_lr_step(sr3_ctx *c, int B, int H, int W) {
    const int C = c->cfg.out_channel;
    if (check_lr_shape("sr3_sample_begin (low-resolution consistency)", C, H, W, c->lr.N, c->lr_lh, c->lr_lw)) return -1;
    if (get_lr_ops(c, c->lr_lh, c->lr_lw, H, W, &c->lr_cur)) return -1;
    c->lr_cur_lds = lr_lds_fits(c->lr_cur);
    if (ensure_x0hat(c, (size_t)B * C * H * W)) return -1;
    return c->lr_cur_lds ? 0 : ensure_lr_scratch(c, lr_scratch_floats(B * C, c->lr_cur));
}

// sr3_sample_begin with the dynamic threshold on: x0 buffer, s and the select's counts for B images of n values (all
// of them members of the StepKey)
int prepare_dyn_step(sr3_ctx *c, int B, int H, int W) {
    c->dyn_n = (int64_t)c->cfg.out_channel * H * W;
    c->dyn_plan = threshold_plan(c->dyn_ratio, c->dyn_n);
    if (ensure_x0hat(c, (size_t)B * c->dyn_n)) return -1;
    if (c->dyn_rows < B) {
        HIP_OK(hipStreamSynchronize(c->stream));
        if (c->dyn_s) HIP_OK(hipFree(c->dyn_s));
        if (c->dyn_bins) HIP_OK(hipFree(c->dyn_bins));
        c->dyn_s = nullptr; c->dyn_bins = nullptr; c->dyn_rows = 0;
        HIP_OK(hipMalloc(&c->dyn_s, (size_t)B * sizeof(float)));
        HIP_OK(hipMalloc(&c->dyn_bins, threshold_bins_bytes(B)));
        c->dyn_rows = B;
    }
    return 0;
}

// the key of a step of `depth` as the context stands (StepKey: the members of a feature that is off stay zero)
StepKey step_key(const sr3_ctx *c, int depth) {
    StepKey k;
    k.mode = (int)c->mode; k.depth = depth; k.lr = c->lr_on(); k.dyn = c->dyn_on();
    if (k.lr || k.dyn) k.x0hat = c->x0hat;
    if (k.lr) {
        k.lr_ops = c->lr_cur; k.lr_lds = c->lr_cur_lds;
        if (!k.lr_lds) k.lr_scratch = c->lr_scratch;
    }
    if (k.dyn) { k.dyn_n = c->dyn_n; k.dyn_plan = c->dyn_plan; k.dyn_max = c->dyn_max; k.dyn_s = c->dyn_s; k.dyn_bins = c->dyn_bins; }
    return k;
}

// The update half of a step. Launch arguments come from the workspace (u: constant until drop_graphs), from c->d_step
// and c->d_lr (device memory written before every step / by the setter, at addresses that never change) and from the
// key, NOT from the live context: what a capture bakes in is then what its key says. (c->lr travels as launch_lr_project's
// `val`, which no kernel reads when `dyn` is given.)
void enqueue_rows_update(sr3_ctx *c, const StepKey &k) {
    const int B = k.batch ? k.batch : c->wB;        // (every launch below covers rows [0, B) and no other)
    RowsUpdateParams u;
    u.state = c->x0; u.C = c->cfg.out_channel;
    u.packed = c->x0p;
    u.xoff = c->cfg.in_channel - c->cfg.out_channel;
    u.eps = c->eps;
    u.rows = k.rows;
    u.ovf = k.mode != A_F32 ? c->d_ovf : nullptr;
    u.hist = c->xhist;
    c->pbegin(F_MISC);
    if (!k.dyn && !k.lr) {
        launch_rows_update(u, B, c->stream);
    } else {
        // as enqueue_update: prediction | threshold | projection | the rest of the update, each in its rows form
        launch_rows_x0_predict(u, k.x0hat, B, c->stream, !k.dyn);
        if (k.dyn) {
            // (the threshold kernels run over all B rows of the step: an idle row's slab of x0hat is zeros, s = 1, and is never used)
            launch_abs_quantile(k.x0hat, B, k.dyn_n, k.dyn_plan, k.dyn_max, k.dyn_bins, nullptr, nullptr, k.dyn_s, c->stream);
            launch_threshold_apply(k.x0hat, B, k.dyn_n, k.dyn_s, c->stream);
        }
        // (only the planes of live rows admitted with an LR image: the others keep the prediction as it is)
        if (k.lr) launch_lr_project_rows(k.x0hat, B, u.C, k.lr_ops, k.rows_lr, k.rows, k.lr_lds, k.lr_scratch, c->stream);
        launch_rows_update_from_x0(u, k.x0hat, B, c->stream);
    }
    c->pend();
}

void enqueue_update(sr3_ctx *c, const StepKey &k) {
    if (k.rows) { enqueue_rows_update(c, k); return; }
    const int B = c->wB;
    UpdateParams u;
    u.state = c->x0; u.C = c->cfg.out_channel;
    u.packed = c->x0p;          // kept current in both arithmetic modes (the mode may change between steps)
    u.xoff = c->cfg.in_channel - c->cfg.out_channel;
    u.eps = c->eps;
    u.args = c->d_step;
    u.ovf = k.mode != A_F32 ? c->d_ovf : nullptr;   // (the packed copy is only read in split-f16 mode)
    u.hist = c->xhist;                          // constant per workspace: the captured graph stays valid
    c->pbegin(F_MISC);
    if (!k.lr && !k.dyn) {
        launch_ddpm_update(u, B, c->stream);
    } else {
        // x0 prediction, unclamped under the dynamic threshold | per-image s and clamp(x0, -s, s) / s |
        // projection onto {x : A x = y} | the rest of the update
        launch_x0_predict(u, k.x0hat, B, c->stream, !k.dyn);
        if (k.dyn) {
            launch_abs_quantile(k.x0hat, B, k.dyn_n, k.dyn_plan, k.dyn_max, k.dyn_bins, nullptr, nullptr, k.dyn_s, c->stream);
            launch_threshold_apply(k.x0hat, B, k.dyn_n, k.dyn_s, c->stream);
        }
        if (k.lr) launch_lr_project(k.x0hat, B * u.C, u.C, k.lr_ops, c->lr, c->d_lr, k.lr_lds, k.lr_scratch, c->stream);
        launch_update_from_x0(u, k.x0hat, B, c->stream);
    }
    c->pend();
}

// the launches of one p_sample step (embedding, UNet body, DDPM update); every per-step value is
// read from c->d_step, so the sequence is identical for every t
// k.depth > 0: the shallow step of the feature cache (run_unet_body); the update half is the same
void enqueue_step(sr3_ctx *c, const StepKey &k) {
    if (k.rows) {
        // every row's own level: the embedding over B rows, each conv reading its row of the FeatureWiseAffine biases
        const int B = k.batch ? k.batch : c->wB;
        run_embed(c, &k.rows->nl, (int)(sizeof(RowArgs) / sizeof(float)), B);
        run_unet_body(c, B, c->wH, c->wW, 0);
        enqueue_update(c, k);
        return;
    }
    // noise_level = float32(sqrt_alphas_cumprod_prev[t+1]) repeated over the batch (diffusion.py:166-167)
    run_embed(c, &c->d_step->nl, 0, c->wB);
    run_unet_body(c, c->wB, c->wH, c->wW, k.depth);
    enqueue_update(c, k);
}

int launch_step(sr3_ctx *c, const StepKey &key);

int step_impl(sr3_ctx *c, int t, const float *noise_slab, float *frame) {
    if (c->rows_on) return fail("sr3_sample_step inside a row session (sr3_rows_begin): its rows move with sr3_rows_step");
    if (!c->sampling) return fail("sr3_sample_step before sr3_sample_begin");
    if (t < 0 || t >= c->T) return fail("step t=%d outside schedule of %d steps", t, c->T);
    // (the arithmetic mode may have been switched between steps: the F8C weight copies are made on demand)
    if (prepare_f8(c)) return -1;
    if (c->lr_on() && (c->lr_cur.lh != c->lr_lh || c->lr_cur.lw != c->lr_lw || c->lr_cur.H != c->wH || c->lr_cur.W != c->wW ||
                       c->x0hat_floats < (size_t)c->wB * c->cfg.out_channel * c->wH * c->wW))
        return fail("p_sample step: low-resolution consistency was turned on or resized after sr3_sample_begin; set it before");
    if (c->dyn_on()) {
        const int64_t n = (int64_t)c->cfg.out_channel * c->wH * c->wW;
        if (c->dyn_n != n || c->dyn_rows < c->wB || c->x0hat_floats < (size_t)c->wB * n || c->dyn_plan.k != threshold_plan(c->dyn_ratio, n).k)
            return fail("p_sample step: the dynamic threshold was turned on or changed after sr3_sample_begin; set it before");
        ++c->dyn_steps;
    }
    StepArgs *slot = next_step_slot(c);
    if (!slot) return -1;
    StepArgs &sa = *slot;
    sa.nl = c->s_nl[t + 1];
    sa.a = c->s_a[t]; sa.b = c->s_b[t]; sa.c1 = c->s_c1[t]; sa.c2 = c->s_c2[t]; sa.c3 = c->s_c3[t];
    sa.sigma = c->s_sig[t];
    // a call begun below the top of the schedule (sr3_sample_begin_from): its first step has no previous x0, and c1[t]
    // alone is the second-order weight; with c3[t] folded in, the step is the first-order one exactly
    if (c->fold_first && c->uses_hist && !c->hist_valid) sa.c1 = c->s_c1[t] + c->s_c3[t];
    sa.draw = (uint32_t)(c->T - t); sa.pad_ = 0;
    // the first step after sr3_sample_begin has no previous x0: it only stores its own
    sa.hist = c->uses_hist ? (c->hist_valid ? 2u : 1u) : 0u;
    if (c->uses_hist) c->hist_valid = true;
    sa.noise = noise_slab; sa.frame = frame;
    sa.seed = c->seed; sa.image_offset = c->image_offset;
    // (the masks of step t are a function of t: a replayed segment draws the same ones)
    if (c->drop_live() && fill_drop_args(c, "p_sample step", sa.drop, sa.draw, c->image_offset)) return -1;
    if (push_step_args(c, &sa)) return -1;

    // Feature cache: step k of the call is shallow when k is no multiple of the interval and the workspace holds the
    // whole forward of an earlier step of THIS call in the arithmetic this step runs in (a step-down of the guard, a
    // forward from outside, a new workspace or new weights make the step whole, whatever k is).
    const bool shallow = c->fc_on() && (c->fc_k % c->fc_interval) != 0 && c->fc_call && c->fc_mode == (int)c->mode;
    const int depth = shallow ? c->fc_depth : 0;
    ++c->fc_k;
    ++(shallow ? c->fc_shallow : c->fc_whole);
    if (!shallow) { c->fc_mode = (int)c->mode; c->fc_call = true; }
    return launch_step(c, step_key(c, depth));
}

// one step of `key`: replayed from its graph, or run eagerly (profiling, SR3_NO_GRAPH=1, the first step of a key) and
// then captured
int launch_step(sr3_ctx *c, const StepKey &key) {
    if (c->prof || c->no_graph) {
        enqueue_step(c, key);
        return 0;
    }
    StepGraph *g = nullptr;
    for (StepGraph &e : c->step_graphs)
        if (e.key.same_slot(key)) { g = &e; break; }
    if (!g) {
        if (key.batch) {
            // an elastic rows step at a batch value without a graph: its form keeps kRowsBatchGraphs of them, the least
            // recently used one goes
            int n = 0;
            size_t lru = 0;
            for (size_t i = 0; i < c->step_graphs.size(); ++i) {
                const StepGraph &e = c->step_graphs[i];
                if (!e.key.batch || !e.key.same_form(key)) continue;
                if (!n++ || e.used < c->step_graphs[lru].used) lru = i;
            }
            if (n >= sr3_ctx::kRowsBatchGraphs) {
                if (c->step_graphs[lru].exec) (void)hipGraphExecDestroy(c->step_graphs[lru].exec);
                c->step_graphs.erase(c->step_graphs.begin() + (long)lru);
            }
        }
        c->step_graphs.push_back(StepGraph{key});
        g = &c->step_graphs.back();
    } else if (!(g->key == key)) {      // a baked-in value changed: as for a new key, one eager step and one capture
        if (g->exec) (void)hipGraphExecDestroy(g->exec);
        *g = StepGraph{key};
    }
    g->used = ++c->graph_clock;
    if (!g->exec) {
        if (g->warm < 1) {          // first step runs eagerly (one-time function attributes)
            ++g->warm;
            enqueue_step(c, key);
            return 0;
        }
        hipGraph_t graph = nullptr;
        HIP_OK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        enqueue_step(c, key);
        HIP_OK(hipStreamEndCapture(c->stream, &graph));
        hipError_t e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) return fail("hipGraphInstantiate: %s", hipGetErrorString(e));
        ++c->step_graph_captures;
    }
    HIP_OK(hipGraphLaunch(g->exec, c->stream));
    return 0;
}

int step_checked(sr3_ctx *c, int t, const float *noise_slab, float *frame) {
    if (step_impl(c, t, noise_slab, frame)) return -1;
    if (const char *e = conv_take_error()) return fail("p_sample step t=%d: %s", t, e);
    return 0;
}

// ---- one conv on scratch buffers (sr3_op_conv2d, sr3_bench_conv) ------------------------------------------------
// device memory of one call: freed on every return
struct DevBuf {
    float *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    ~DevBuf() { (void)hipFree(p); }            // (a null pointer is a no-op)
    int alloc(size_t floats) { HIP_OK(hipMalloc(&p, floats * sizeof(float))); return 0; }
    int upload(const float *host, size_t floats) {
        if (alloc(floats)) return -1;
        HIP_OK(hipMemcpy(p, host, floats * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
};

void fill_random(sr3_ctx *c, float *q, size_t n, int seed) {
    launch_philox_normal(seed, 0, 0, (int)std::min<size_t>(n, 1u << 30), q, c->stream);
}

// The timing tail of the per-shape benchmarks: `iters` back-to-back repetitions of `first`, then of `second`, on the
// context's stream between three events (the caller warms up); the average of each phase in ms. The events are
// destroyed on every return.
template <class First, class Second>
int time_two_phases(sr3_ctx *c, int iters, First &&first, Second &&second, float *first_ms, float *second_ms) {
    struct Events {
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev); }
    } ev;
    for (hipEvent_t &e : ev.e) HIP_OK(hipEventCreate(&e));
    HIP_OK(hipEventRecord(ev.e[0], c->stream));
    for (int i = 0; i < iters; ++i) first();
    HIP_OK(hipEventRecord(ev.e[1], c->stream));
    for (int i = 0; i < iters; ++i) second();
    HIP_OK(hipEventRecord(ev.e[2], c->stream));
    HIP_OK(hipEventSynchronize(ev.e[2]));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    *first_ms = ms / iters;
    HIP_OK(hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
    *second_ms = ms / iters;
    return 0;
}

// the weights of conv2's fused 1x1 term as run_res hands them over: a res_conv (w2_host: [Cout][C2], OIHW of a 1x1
// conv), or — split-f16 arithmetics — the identity skip as extra K-steps (ident: ResBlock::ident_w)
struct FusedTerm {
    const float *w2_host = nullptr;
    int C2 = 0;
    bool ident = false;
};

// A single conv as the engine runs this shape: the plan of the shape with every buffer offered (fused statistics only
// with `stats`: the caller then passes ConvParams::stats with the plan's stats_slices)
// names the weight layouts and scratch buffers; p comes back with input, weights, partials and Winograd workspace
// filled in — output, bias, residual and FeatureWiseAffine bias are the caller's.
struct ScratchConv {
    ConvPlan plan;
    bool f8 = false;                // "f16f8" mode and the shape takes the F8C operand format
    DevBuf act, w, w2, wino_w, wino_wf, up_wino_w, wino_ws, part;
    ConvParams p;

    // weight_host: OIHW weights, nullptr: random values (timing). The activated input `act` (zero-bordered, Cin
    // channels) is allocated and left for the caller to fill.
    // fused (with weight_host): p.w2 in the layout and, in the split-f16 arithmetics, with the common weight scale
    // prepare_fused gives the pair; p.in2 / p.in2b are the caller's.
    int setup(sr3_ctx *c, int B, int Hin, int Win, int C0, int C1, int Cout, int ks, int stride, int up2, const float *weight_host,
              bool stats = false, const FusedTerm *fused = nullptr) {
        const int Cin = C0 + C1;
        f8 = c->f8() && ks == 3 && stride == 1 && !up2 && conv_f8_supported(B, Hin, Win, Cout, Cin);
        plan = conv_plan_offered(B, Hin, Win, Cin, Cout, ks, stride, up2, c->split() ? 1 : 0, f8, stats);
        const bool wino = plan.kernel == CK_WINO_ONE_PASS || plan.kernel == CK_WINO_THREE_PASS;
        const size_t n_w = (size_t)(up2 ? 16 : ks * ks) * Cout * Cin;     // up2: 4 phases x 2x2 taps
        const size_t n_wino = (size_t)16 * Cout * Cin;
        if (weight_host) {
            std::vector<float> packed((size_t)ks * ks * Cout * Cin), tmp;
            pack_conv_weight(weight_host, Cout, Cin, ks, Cin, packed.data());
            if (plan.up2_wino) {
                tmp.resize(up2_wino_floats(Cout, Cin));
                make_up2_wino_weights(packed.data(), Cout, Cin, tmp.data());
                if (up_wino_w.upload(tmp.data(), tmp.size())) return -1;
            }
            if (up2) {
                tmp.resize(n_w);
                make_up2_phase_weights(packed.data(), Cout, Cin, tmp.data());
                packed.swap(tmp);
            }
            if (wino) {
                std::vector<float> wv(n_wino);
                make_wino_weights(packed.data(), Cout, Cin, wv.data());
                if (plan.wino_fused_rows) {     // both layouts: the three-pass plan asks for w_wino, this form reads w_wino_f
                    tmp.resize(n_wino);
                    make_wino_weights_frag(wv.data(), Cout, Cin, tmp.data());
                    if (wino_wf.upload(tmp.data(), n_wino)) return -1;
                }
                if (plan.needs_wino_frag) {
                    tmp.resize(n_wino);
                    make_wino_weights_frag(wv.data(), Cout, Cin, tmp.data());
                    wv.swap(tmp);
                }
                if (wino_w.upload(wv.data(), n_wino)) return -1;
            }
            std::vector<float> w2v;
            if (fused && fused->w2_host) {
                w2v.resize((size_t)Cout * fused->C2);
                pack_conv_weight(fused->w2_host, Cout, fused->C2, 1, fused->C2, w2v.data());
            }
            if (c->split()) {
                tmp.resize(n_w);
                if (!w2v.empty()) {         // prepare_fused: conv2 and the res_conv share one 2^k
                    const int k = std::min(split_scale_exponent(packed.data(), n_w), split_scale_exponent(w2v.data(), w2v.size()));
                    p.w_unscale = split_conv_weight_k(packed.data(), n_w / Cin, Cin, k, tmp.data());
                    std::vector<float> sp(w2v.size());
                    split_conv_weight_k(w2v.data(), (size_t)Cout, fused->C2, k, sp.data());
                    w2v.swap(sp);
                } else {
                    p.w_unscale = split_conv_weight(packed.data(), n_w / Cin, Cin, tmp.data());
                    if (fused && fused->ident) {
                        std::vector<float> sp;
                        p.w_unscale = ident_skip_weights(packed.data(), n_w, Cout, Cin, p.w_unscale, sp, w2v);
                        if (!sp.empty()) tmp.swap(sp);
                    }
                }
                packed.swap(tmp);
            }
            if (w.upload(packed.data(), n_w)) return -1;
            if (!w2v.empty() && w2.upload(w2v.data(), w2v.size())) return -1;
            p.w2 = w2.p;
            if (f8) {
                DevBuf w8;
                if (w8.alloc(n_w)) return -1;
                launch_make_f8_weights(w.p, w8.p, n_w / 32, c->stream);
                HIP_OK(hipStreamSynchronize(c->stream));
                std::swap(w.p, w8.p);
            }
        } else {
            if (w.alloc(n_w)) return -1;
            fill_random(c, w.p, n_w, 3);
            if (wino) {
                if (wino_w.alloc(n_wino)) return -1;
                fill_random(c, wino_w.p, n_wino, 10);       // (either layout: random values)
                if (plan.wino_fused_rows) {
                    if (wino_wf.alloc(n_wino)) return -1;
                    fill_random(c, wino_wf.p, n_wino, 12);
                }
            }
            if (plan.up2_wino) {
                if (up_wino_w.alloc(up2_wino_floats(Cout, Cin))) return -1;
                fill_random(c, up_wino_w.p, up2_wino_floats(Cout, Cin), 11);
            }
        }
        if (plan.wino_ws_floats && wino_ws.alloc(plan.wino_ws_floats)) return -1;
        if (plan.part_floats && part.alloc(plan.part_floats)) return -1;
        TDesc a; a.C = Cin; a.H = Hin; a.W = Win; a.pad = 1;
        if (act.alloc(a.floats(B))) return -1;
        a.p = act.p;
        const int pad = ks / 2, Hv = Hin << up2, Wv = Win << up2;
        p.in0 = a; p.B = B;
        p.Hout = (Hv + 2 * pad - ks) / stride + 1; p.Wout = (Wv + 2 * pad - ks) / stride + 1;
        p.ks = ks; p.stride = stride; p.up2 = up2;
        p.prec = c->split() ? 1 : 0; p.f8 = f8 ? 1 : 0;
        p.w = w.p;
        (plan.needs_wino_frag ? p.w_wino_f : p.w_wino) = wino_w.p;
        if (plan.wino_fused_rows) p.w_wino_f = wino_wf.p;
        p.w_up_wino = up_wino_w.p;
        p.wino_ws = wino_ws.p;
        p.part = part.p;
        if (part.p) p.tile_cnt = c->tile_cnt;
        p.ovf = c->d_ovf;            // (range bits of twin stores and the 'wait gave up' bit of the in-place split-K)
        return 0;
    }
    // the engine's rule (gn_pass_writes_u): the apply pass in front of this conv writes U into wino_ws
    bool gn_writes_u(const sr3_ctx *c) const { return gn_pass_writes_u(c->split(), plan, false, 0); }
};

} // namespace

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

const char *sr3_last_error(void) { return g_err.c_str(); }

int sr3_create(const sr3_unet_cfg *cfg, int device, sr3_ctx **out) {
    if (!cfg || !out) return fail("sr3_create: null argument");
    if (cfg->inner_channel <= 0 || cfg->inner_channel % 32)
        return fail("inner_channel=%d: must be a positive multiple of 32", cfg->inner_channel);
    if (cfg->norm_groups <= 0 || cfg->inner_channel % cfg->norm_groups)
        return fail("norm_groups=%d does not divide inner_channel=%d", cfg->norm_groups, cfg->inner_channel);
    if (cfg->n_mults < 1 || cfg->n_mults > SR3_MAX_MULTS) return fail("n_mults=%d out of range", cfg->n_mults);
    if (cfg->n_attn_res < 0 || cfg->n_attn_res > SR3_MAX_ATTN_RES) return fail("n_attn_res out of range");
    if (cfg->in_channel < cfg->out_channel || cfg->out_channel < 1) return fail("in_channel/out_channel invalid");
    if (cfg->res_blocks < 1) return fail("res_blocks must be >= 1");
    if (!(cfg->dropout >= 0.f) || cfg->dropout >= 1.f) return fail("dropout=%g: must be in [0, 1)", (double)cfg->dropout);
    for (int i = 0; i < cfg->n_mults; ++i)
        if (cfg->channel_mults[i] < 1) return fail("channel_mults[%d] invalid", i);
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("device %d not present (%d HIP devices)", device, ndev);
    HIP_OK(hipSetDevice(device));
    sr3_ctx *c = new sr3_ctx();
    c->cfg = *cfg;
    c->device = device;
    c->no_graph = env_switch_now(SW_NO_GRAPH) != 0;                 // product switch, read per context
    if (build_graph(c)) { delete c; return -1; }
    if (alloc_weights(c)) { sr3_destroy(c); return -1; }
    if (hipStreamCreate(&c->own_stream) != hipSuccess) { sr3_destroy(c); return fail("hipStreamCreate failed"); }
    c->stream = c->own_stream;
    if (hipMalloc(&c->d_ovf, sizeof(int)) != hipSuccess || hipMemset(c->d_ovf, 0, sizeof(int)) != hipSuccess ||
        hipMalloc(&c->tile_cnt, CONV_TILE_COUNTERS * sizeof(unsigned)) != hipSuccess ||
        hipMemset(c->tile_cnt, 0, CONV_TILE_COUNTERS * sizeof(unsigned)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&c->h_ovf), sizeof(int), hipHostMallocDefault) != hipSuccess) {
        sr3_destroy(c);
        return fail("allocating the range-check flag failed");
    }
    *c->h_ovf = 0;
    *out = c;
    return 0;
}

void sr3_destroy(sr3_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto &m : c->mods) {
        if (m.rb.fused_bias) (void)hipFree(m.rb.fused_bias);
        if (m.rb.ident_w) (void)hipFree(m.rb.ident_w);
    }
    for (auto &p : c->params) {
        if (p.owns && p.dev) (void)hipFree(p.dev);
        if (p.dev_split) (void)hipFree(p.dev_split);
        if (p.dev_f8) (void)hipFree(p.dev_f8);
        if (p.dev_wino) (void)hipFree(p.dev_wino);
        if (p.dev_wino_f) (void)hipFree(p.dev_wino_f);
        if (p.dev_up_wino) (void)hipFree(p.dev_up_wino);
    }
    if (c->final_wq) (void)hipFree(c->final_wq);
    if (c->ci_w) (void)hipFree(c->ci_w);
    if (c->final_wm) (void)hipFree(c->final_wm);
    if (c->nfw) (void)hipFree(c->nfw);
    if (c->nfb) (void)hipFree(c->nfb);
    if (c->arena) (void)hipFree(c->arena);
    if (c->d_nl) (void)hipFree(c->d_nl);
    if (c->d_start) (void)hipFree(c->d_start);
    drop_graphs(c);
    if (c->d_ovf) (void)hipFree(c->d_ovf);
    if (c->ckpt) (void)hipFree(c->ckpt);
    if (c->metrics_ws) (void)hipFree(c->metrics_ws);
    if (c->tile_cnt) (void)hipFree(c->tile_cnt);
    if (c->d_wmax) (void)hipFree(c->d_wmax);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_ovf) (void)hipHostFree(c->h_ovf);
    if (c->h_ring) (void)hipHostFree(c->h_ring);
    if (c->d_step) (void)hipFree(c->d_step);
    if (c->h_rows) (void)hipHostFree(c->h_rows);
    if (c->d_rows) (void)hipFree(c->d_rows);
    if (c->d_row_start) (void)hipFree(c->d_row_start);
    if (c->rows_lr_buf) (void)hipFree(c->rows_lr_buf);
    for (auto &kv : c->lr_ops) { (void)hipFree(kv.second.buf); (void)hipFree(kv.second.bounds); }
    if (c->d_lr) (void)hipFree(c->d_lr);
    if (c->h_lr) (void)hipHostFree(c->h_lr);
    if (c->x0hat) (void)hipFree(c->x0hat);
    if (c->lr_scratch) (void)hipFree(c->lr_scratch);
    if (c->dyn_s) (void)hipFree(c->dyn_s);
    if (c->dyn_bins) (void)hipFree(c->dyn_bins);
    if (c->thr_op_bins) (void)hipFree(c->thr_op_bins);
    for (auto &r : c->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->order_ev) (void)hipEventDestroy(c->order_ev);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int sr3_set_stream(sr3_ctx *c, void *hip_stream) {
    if (!c) return fail("null context");
    c->pflush();
    c->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
    return 0;
}

// Stream ordering without host synchronisation (hosts that keep their own streams, e.g. torch): an event is
// recorded on one stream and the other stream waits for it on the device.
static int order_streams(sr3_ctx *c, hipStream_t first, hipStream_t then) {
    if (first == then) return 0;
    if (!c->order_ev) HIP_OK(hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming));
    HIP_OK(hipEventRecord(c->order_ev, first));
    HIP_OK(hipStreamWaitEvent(then, c->order_ev, 0));
    return 0;
}
int sr3_wait_for_stream(sr3_ctx *c, void *other_stream) {
    if (!c) return fail("null context");
    HIP_OK(hipSetDevice(c->device));
    return order_streams(c, reinterpret_cast<hipStream_t>(other_stream), c->stream);
}
int sr3_stream_wait_for_ctx(sr3_ctx *c, void *other_stream) {
    if (!c) return fail("null context");
    HIP_OK(hipSetDevice(c->device));
    return order_streams(c, c->stream, reinterpret_cast<hipStream_t>(other_stream));
}

int sr3_set_precision(sr3_ctx *c, int prec) {
    if (!c) return fail("null context");
    if (prec < 0 || prec > 2)
        return fail("precision %d unknown (0 = f32 exact, 1 = split-f16, 2 = split-f16 with fp8 correction products)", prec);
    c->mode = (Arith)prec;
    c->fc_invalidate();
    return 0;
}

int sr3_conv_f8_supported(int B, int H, int W, int Cout, int Cin) { return conv_f8_supported(B, H, W, Cout, Cin) ? 1 : 0; }

int sr3_conv_plan(int B, int H, int W, int Cin, int Cout, int ks, int stride, int up2, int precision, int with_stats,
                  int64_t *out12, char *kernel_name, int name_cap) {
    if (!out12) return fail("sr3_conv_plan: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin % 32) || !(ks == 1 || ks == 3) || !(stride == 1 || stride == 2) ||
        (up2 & ~1) || (up2 && (ks != 3 || stride != 1)) || precision < 0 || precision > 2)
        return fail("sr3_conv_plan: unsupported conv (Cin a multiple of 32, ks 1 | 3, stride 1 | 2, up2 with ks 3 / stride 1, precision 0..2)");
    const bool f8 = precision == 2 && ks == 3 && stride == 1 && !up2 && conv_f8_supported(B, H, W, Cout, Cin);
    const ConvPlan pl = conv_plan_offered(B, H, W, Cin, Cout, ks, stride, up2, precision ? 1 : 0, f8, with_stats != 0);
    if (pl.error) return fail("sr3_conv_plan: %s", pl.error);
    const int64_t v[12] = {pl.kernel, pl.tile_m, pl.tile_n, pl.split, pl.splits, pl.phases, (int64_t)pl.part_floats,
                           pl.needs_counters, pl.stats_slices, (int64_t)pl.wino_ws_floats, pl.needs_wino_frag, f8};
    std::copy(v, v + 12, out12);
    if (kernel_name && name_cap > 0) snprintf(kernel_name, (size_t)name_cap, "%s", conv_kernel_name(pl.kernel));
    return 0;
}

// Batch-invariant mode. Everything that bakes a plan in goes: the workspace (its statistics slices and
// buffer sizes follow the plans), the feature cache it holds and the captured steps. No weight layout depends on the mode
// (the F8C copies exist for every 3x3 conv; which of them a call reads is the plan's answer).
int sr3_set_batch_invariant(sr3_ctx *c, int plan_batch) {
    if (!c) return fail("null context");
    if (plan_batch < 0 || plan_batch > (1 << 20)) return fail("sr3_set_batch_invariant: planning batch %d outside [0, 2^20] (0 = off)", plan_batch);
    if (plan_batch == c->plan_batch) return 0;
    if (c->rows_on)
        return fail("sr3_set_batch_invariant: a row session is open (its steps were planned under the current setting; sr3_rows_end first)");
    c->sampling = false;        // (the state of a step session goes with the workspace: sr3_sample_begin again)
    HIP_OK(hipSetDevice(c->device));
    if (c->arena) {
        HIP_OK(hipStreamSynchronize(c->stream));
        HIP_OK(hipFree(c->arena));
        c->arena = nullptr;
        c->arena_bytes = 0;
        c->wB = c->wH = c->wW = 0;
    }
    drop_graphs(c);
    c->fc_invalidate();
    c->plan_batch = plan_batch;
    return 0;
}

int sr3_get_batch_invariant(sr3_ctx *c) { return c ? c->plan_batch : fail("null context"); }

int sr3_conv_plan_invariant(int plan_batch, int B, int H, int W, int Cin, int Cout, int ks, int stride, int up2, int precision,
                            int with_stats, int64_t *out12, char *kernel_name, int name_cap) {
    if (plan_batch <= 0) return fail("sr3_conv_plan_invariant: the planning batch must be positive");
    const int was = set_plan_batch(plan_batch);
    const int r = sr3_conv_plan(B, H, W, Cin, Cout, ks, stride, up2, precision, with_stats, out12, kernel_name, name_cap);
    set_plan_batch(was);
    return r;
}

int64_t sr3_conv_plan_invariant_max_batch(int plan_batch, int H, int W, int Cin, int Cout, int ks, int stride, int up2, int precision,
                                          int with_stats) {
    int64_t out12[12];
    if (plan_batch <= 0) return fail("sr3_conv_plan_invariant_max_batch: the planning batch must be positive");
    if (sr3_conv_plan_invariant(plan_batch, 1, H, W, Cin, Cout, ks, stride, up2, precision, with_stats, out12, nullptr, 0)) return -1;
    const int was = set_plan_batch(plan_batch);
    const ConvPlan pl = conv_plan_offered(1, H, W, Cin, Cout, ks, stride, up2, precision ? 1 : 0, out12[11] != 0, with_stats != 0);
    set_plan_batch(was);
    // the tensors of the conv itself stay below 4 GiB (what sr3_max_batch asks of every activation tensor of a UNet)
    const int pad = ks / 2, Ho = ((H << up2) + 2 * pad - ks) / stride + 1, Wo = ((W << up2) + 2 * pad - ks) / stride + 1;
    const uint64_t per = std::max((uint64_t)(H + 2) * (W + 2) * Cin, (uint64_t)(Ho + 2) * (Wo + 2) * Cout) * sizeof(float);
    uint64_t bound = std::min<uint64_t>(((1ull << 32) - 1) / per, 65535);
    if (pl.batch_limit > 0) bound = std::min<uint64_t>(bound, (uint64_t)pl.batch_limit);
    return (int64_t)bound;
}

int sr3_wino_weights_host(const float *packed_host, int Cout, int CinPad, int frag, float *dst_host) {
    if (!packed_host || !dst_host || Cout <= 0 || CinPad <= 0 || (CinPad % 8))
        return fail("sr3_wino_weights_host: Cout > 0 and CinPad a positive multiple of 8");
    if (frag == 2) { make_up2_wino_weights(packed_host, Cout, CinPad, dst_host); return 0; }
    if (!frag) { make_wino_weights(packed_host, Cout, CinPad, dst_host); return 0; }
    std::vector<float> wv((size_t)16 * Cout * CinPad);
    make_wino_weights(packed_host, Cout, CinPad, wv.data());
    make_wino_weights_frag(wv.data(), Cout, CinPad, dst_host);
    return 0;
}

int sr3_lr_operators_host(int l, int r, double *A, double *P) {
    if (!A || !P || l <= 0 || r <= l) return fail("sr3_lr_operators_host: needs 0 < l < r and both outputs");
    if (!lr_operators(l, r, A, P, nullptr)) return fail("sr3_lr_operators_host: the Gram matrix of %d -> %d is not positive definite", r, l);
    return 0;
}

int sr3_synchronize(sr3_ctx *c) {
    if (!c) return fail("null context");
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

int sr3_num_params(sr3_ctx *c) { return c ? (int)c->params.size() : fail("null context"); }

int sr3_param_info(sr3_ctx *c, int index, char *name, int name_cap, int64_t *shape4, int *ndim) {
    if (!c) return fail("null context");
    if (index < 0 || index >= (int)c->params.size()) return fail("param index %d out of range", index);
    const Param &p = c->params[index];
    if (name && name_cap > 0) {
        strncpy(name, p.name.c_str(), name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (ndim) *ndim = (int)p.shape.size();
    if (shape4)
        for (size_t i = 0; i < 4; ++i) shape4[i] = i < p.shape.size() ? p.shape[i] : 1;
    return 0;
}

int sr3_load_weight(sr3_ctx *c, const char *name, const float *host, const int64_t *shape, int ndim) {
    if (!c || !name || !host || !shape) return fail("sr3_load_weight: null argument");
    HIP_OK(hipSetDevice(c->device));
    for (auto &p : c->params) {
        if (p.name != name) continue;
        if ((int)p.shape.size() != ndim) return fail("%s: expected %zu dims, got %d", name, p.shape.size(), ndim);
        for (int i = 0; i < ndim; ++i)
            if (p.shape[i] != shape[i]) return fail("%s: dim %d is %lld, expected %lld", name, i, (long long)shape[i], (long long)p.shape[i]);
        // weights may change while earlier launches are still reading them
        HIP_OK(hipStreamSynchronize(c->stream));
        c->fc_invalidate();     // (the cached features are those of the old weights)
        if (p.kind == P_CONV) {
            if (c->ci_w && &p == &c->params[c->mods[0].conv.w]) {
                std::vector<float> wf(conv_in_weight_floats(p.cout));
                c->ci_unscale = pack_conv_in_weight(host, p.cout, p.cin, wf.data());
                HIP_OK(hipMemcpy(c->ci_w, wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice));
            }
            if (c->final_wm && &p == &c->params[c->final_conv.w]) {
                std::vector<float> wf(final_conv_mfma_weight_floats(p.cin));
                c->final_unscale = pack_final_conv_mfma_weight(host, p.cin, wf.data());
                HIP_OK(hipMemcpy(c->final_wm, wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice));
            }
            if (c->final_wq && &p == &c->params[c->final_conv.w]) {
                std::vector<float> wq((size_t)9 * p.cin * 4);
                pack_final_conv_weight(host, p.cout, p.cin, wq.data());
                HIP_OK(hipMemcpy(c->final_wq, wq.data(), wq.size() * sizeof(float), hipMemcpyHostToDevice));
            }
            std::vector<float> packed((size_t)p.ks * p.ks * p.cout * p.cin_pad);
            pack_conv_weight(host, p.cout, p.cin, p.ks, p.cin_pad, packed.data());
            size_t rows = (size_t)p.ks * p.ks * p.cout;
            if (p.dev_up_wino) {    // (from the nine taps, before the phase planes replace them)
                std::vector<float> uw(up2_wino_floats(p.cout, p.cin_pad));
                make_up2_wino_weights(packed.data(), p.cout, p.cin_pad, uw.data());
                HIP_OK(hipMemcpy(p.dev_up_wino, uw.data(), uw.size() * sizeof(float), hipMemcpyHostToDevice));
            }
            if (p.up_phase) {       // nearest x2 + 3x3 == four 2x2 phase convs on the low-res input
                std::vector<float> ph(p.dev_floats);
                make_up2_phase_weights(packed.data(), p.cout, p.cin_pad, ph.data());
                packed.swap(ph);
                rows = (size_t)16 * p.cout;
            }
            HIP_OK(hipMemcpy(p.dev, packed.data(), p.dev_floats * sizeof(float), hipMemcpyHostToDevice));
            if (p.dev_wino) {
                std::vector<float> wv((size_t)16 * p.cout * p.cin_pad);
                make_wino_weights(packed.data(), p.cout, p.cin_pad, wv.data());
                HIP_OK(hipMemcpy(p.dev_wino, wv.data(), wv.size() * sizeof(float), hipMemcpyHostToDevice));
                if (p.dev_wino_f) {
                    std::vector<float> wf(wv.size());
                    make_wino_weights_frag(wv.data(), p.cout, p.cin_pad, wf.data());
                    HIP_OK(hipMemcpy(p.dev_wino_f, wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice));
                }
            }
            if (p.keep_host) p.host = packed;
            std::vector<float> sp(p.dev_floats);
            p.w_unscale = split_conv_weight(packed.data(), rows, p.cin_pad, sp.data());
            HIP_OK(hipMemcpy(p.dev_split, sp.data(), p.dev_floats * sizeof(float), hipMemcpyHostToDevice));
        } else {
            HIP_OK(hipMemcpy(p.dev, host, p.dev_floats * sizeof(float), hipMemcpyHostToDevice));
            if (p.keep_host) p.host.assign(host, host + p.dev_floats);
        }
        p.loaded = true;
        c->fused_dirty = true;
        c->f8_dirty = true;
        drop_graphs(c);     // captured steps hold the old w_unscale scalars in their kernel arguments
        return 0;
    }
    return fail("unknown parameter '%s'", name);
}

namespace {

// split_scale_exponent, from the maximum the device reduced
int scale_exponent_of_max(float mx) {
    if (!(mx > 0.f)) return 0;
    int e;
    frexpf(mx, &e);
    return 11 - e;
}

int find_param(sr3_ctx *c, const char *name, const int64_t *shape, int ndim) {
    for (size_t i = 0; i < c->params.size(); ++i) {
        const Param &p = c->params[i];
        if (p.name != name) continue;
        if ((int)p.shape.size() != ndim) return fail("%s: expected %zu dims, got %d", name, p.shape.size(), ndim);
        for (int d = 0; d < ndim; ++d)
            if (p.shape[d] != shape[d])
                return fail("%s: dim %d is %lld, expected %lld", name, d, (long long)shape[d], (long long)p.shape[d]);
        return (int)i;
    }
    return fail("unknown parameter '%s'", name);
}

// layout of h_stage in floats: [maxima : nparams][conv_in OIHW][final_conv OIHW][ci_w][final_wm][final_wq]
struct StageLayout { size_t ci_src, fc_src, ci_w, final_wm, final_wq, total; };
StageLayout stage_layout(const sr3_ctx *c) {
    StageLayout L;
    const Param &ci = c->params[c->mods[0].conv.w], &fc = c->params[c->final_conv.w];
    size_t o = c->params.size();
    L.ci_src = o;   o += (size_t)ci.cout * ci.cin * 9;
    L.fc_src = o;   o += (size_t)fc.cout * fc.cin * 9;
    L.ci_w = o;     o += c->ci_w ? conv_in_weight_floats(ci.cout) : 0;
    L.final_wm = o; o += c->final_wm ? final_conv_mfma_weight_floats(fc.cin) : 0;
    L.final_wq = o; o += c->final_wq ? (size_t)9 * fc.cin * 4 : 0;
    L.total = o;
    return L;
}

} // namespace

// The device route of sr3_load_weight. Phase one (enqueued): every layout that does not depend on the split exponent is
// written straight from the caller's tensors, and max|w| of every conv tensor is reduced into d_wmax. One small copy brings
// the maxima (and the two edge convs' few thousand source floats) to the host and the stream is synchronised ONCE. The host
// derives every exponent, with prepare_fused's rules for the fused (conv2 + res_conv) pairs and the identity-skip blocks,
// and phase two enqueues the split passes and the products of prepare_fused for the blocks it touched. The host copies
// (Param::host) of the refreshed tensors are dropped; a later prepare_fused fetches them from the device again.
int sr3_load_weights_dev(sr3_ctx *c, int n, const char *const *names, const float *const *dev_ptrs, const int64_t *shapes,
                         const int *ndims) {
    if (!c || n < 0 || (n > 0 && (!names || !dev_ptrs || !shapes || !ndims))) return fail("sr3_load_weights_dev: null argument");
    if (n == 0) return 0;
    HIP_OK(hipSetDevice(c->device));
    const size_t np = c->params.size();
    std::vector<int> idx(n);
    std::vector<char> touched(np, 0);
    for (int e = 0; e < n; ++e) {
        if (!names[e] || !dev_ptrs[e]) return fail("sr3_load_weights_dev: null argument");
        if (ndims[e] < 0 || ndims[e] > 4) return fail("%s: expected at most 4 dims, got %d", names[e], ndims[e]);
        idx[e] = find_param(c, names[e], shapes + (size_t)4 * e, ndims[e]);
        if (idx[e] < 0) return -1;
        if (touched[idx[e]]) return fail("%s: listed twice in one sr3_load_weights_dev call", names[e]);
        touched[idx[e]] = 1;
    }
    c->fc_invalidate();     // (the cached features are those of the old weights)
    const StageLayout L = stage_layout(c);
    if (!c->d_wmax) {
        HIP_OK(hipMalloc(&c->d_wmax, np * sizeof(unsigned)));
        c->weight_bytes += np * sizeof(unsigned);
    }
    if (!c->h_stage) HIP_OK(hipHostMalloc(reinterpret_cast<void **>(&c->h_stage), L.total * sizeof(float), hipHostMallocDefault));
    hipStream_t s = c->stream;
    const int ci_idx = c->mods[0].conv.w, fc_idx = c->final_conv.w;

    // ---- phase one ----
    HIP_OK(hipMemsetAsync(c->d_wmax, 0, np * sizeof(unsigned), s));
    for (int e = 0; e < n; ++e) {
        Param &p = c->params[idx[e]];
        const float *src = dev_ptrs[e];
        if (p.kind != P_CONV) {
            HIP_OK(hipMemcpyAsync(p.dev, src, p.dev_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
        } else {
            const size_t src_bytes = (size_t)p.cout * p.cin * p.ks * p.ks * sizeof(float);
            if (idx[e] == ci_idx && c->ci_w) HIP_OK(hipMemcpyAsync(c->h_stage + L.ci_src, src, src_bytes, hipMemcpyDeviceToHost, s));
            if (idx[e] == fc_idx && (c->final_wm || c->final_wq))
                HIP_OK(hipMemcpyAsync(c->h_stage + L.fc_src, src, src_bytes, hipMemcpyDeviceToHost, s));
            launch_weight_pack(src, p.cout, p.cin, p.ks, p.cin_pad, p.up_phase, p.dev, p.dev_wino, c->d_wmax + idx[e], s, p.dev_up_wino);
            if (p.dev_wino && p.dev_wino_f) launch_wino_frag(p.dev_wino, p.cout, p.cin_pad, p.dev_wino_f, s);
        }
        p.host.clear();
    }
    // blocks with fused products: the partner of a refreshed tensor is split again with the common exponent, from its own
    // packed copy, and needs its maximum too
    bool every_block = true;        // this call refreshed every tensor prepare_fused reads
    for (auto &m : c->mods) {
        if (m.kind != M_RES) continue;
        ResBlock &rb = m.rb;
        if (rb.has_res) {
            every_block = every_block && touched[rb.c2.w] && touched[rb.res.w] && touched[rb.c2.b] && touched[rb.res.b];
            if (touched[rb.c2.w] != touched[rb.res.w]) {
                const int other = touched[rb.c2.w] ? rb.res.w : rb.c2.w;
                launch_weight_absmax(c->params[other].dev, c->params[other].dev_floats, c->d_wmax + other, s);
            }
            if (touched[rb.c2.b] || touched[rb.res.b]) {
                if (!rb.fused_bias) HIP_OK(hipMalloc(&rb.fused_bias, (size_t)rb.cout * sizeof(float)));
                launch_weight_bias_sum(c->params[rb.c2.b].dev, c->params[rb.res.b].dev, rb.cout, rb.fused_bias, s);
            }
        } else if (ident_eligible(rb)) {
            every_block = every_block && touched[rb.c2.w];
        }
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(c->h_stage, c->d_wmax, np * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));        // the one host synchronisation of a refresh

    // ---- the exponents ----
    std::vector<int> kexp(np, 0);
    std::vector<char> resplit(np, 0);
    for (size_t i = 0; i < np; ++i) {
        if (c->params[i].kind != P_CONV) continue;
        kexp[i] = scale_exponent_of_max(c->h_stage[i]);
        resplit[i] = touched[i];
    }
    for (auto &m : c->mods) {
        if (m.kind != M_RES) continue;
        ResBlock &rb = m.rb;
        if (rb.has_res && (touched[rb.c2.w] || touched[rb.res.w])) {
            const int k = std::min(kexp[rb.c2.w], kexp[rb.res.w]);
            kexp[rb.c2.w] = kexp[rb.res.w] = k;
            resplit[rb.c2.w] = resplit[rb.res.w] = 1;
        } else if (!rb.has_res && ident_eligible(rb) && touched[rb.c2.w]) {
            kexp[rb.c2.w] = std::min(kexp[rb.c2.w], 15);      // the identity matrix holds 2^k as a half (prepare_fused)
        }
    }

    // ---- phase two ----
    for (size_t i = 0; i < np; ++i) {
        if (!resplit[i]) continue;
        Param &p = c->params[i];
        launch_weight_split(p.dev, p.dev_floats, kexp[i], p.dev_split, s);
        p.w_unscale = ldexpf(1.0f, -kexp[i]);
    }
    for (auto &m : c->mods) {
        if (m.kind != M_RES || m.rb.has_res || !ident_eligible(m.rb) || !touched[m.rb.c2.w]) continue;
        ResBlock &rb = m.rb;
        if (!rb.ident_w) HIP_OK(hipMalloc(&rb.ident_w, (size_t)rb.cout * rb.cout * sizeof(float)));
        launch_weight_ident(rb.cout, 1.0f / c->params[rb.c2.w].w_unscale, rb.ident_w, s);
    }
    if (touched[ci_idx] && c->ci_w) {
        const Param &p = c->params[ci_idx];
        c->ci_unscale = pack_conv_in_weight(c->h_stage + L.ci_src, p.cout, p.cin, c->h_stage + L.ci_w);
        HIP_OK(hipMemcpyAsync(c->ci_w, c->h_stage + L.ci_w, conv_in_weight_floats(p.cout) * sizeof(float), hipMemcpyHostToDevice, s));
    }
    if (touched[fc_idx] && c->final_wm) {
        const Param &p = c->params[fc_idx];
        c->final_unscale = pack_final_conv_mfma_weight(c->h_stage + L.fc_src, p.cin, c->h_stage + L.final_wm);
        HIP_OK(hipMemcpyAsync(c->final_wm, c->h_stage + L.final_wm, final_conv_mfma_weight_floats(p.cin) * sizeof(float),
                              hipMemcpyHostToDevice, s));
    }
    if (touched[fc_idx] && c->final_wq) {
        const Param &p = c->params[fc_idx];
        pack_final_conv_weight(c->h_stage + L.fc_src, p.cout, p.cin, c->h_stage + L.final_wq);
        HIP_OK(hipMemcpyAsync(c->final_wq, c->h_stage + L.final_wq, (size_t)9 * p.cin * 4 * sizeof(float), hipMemcpyHostToDevice, s));
    }
    HIP_OK(hipGetLastError());

    for (int e = 0; e < n; ++e) c->params[idx[e]].loaded = true;
    // sr3_load_weight leaves the fused products to prepare_fused (fused_dirty); here the blocks this call touched are up to
    // date already, so the flag only stays set for what was pending before — and not even that when this call covered
    // every such tensor
    if (every_block) c->fused_dirty = false;
    c->f8_dirty = true;
    drop_graphs(c);         // captured steps hold the old w_unscale scalars in their kernel arguments
    return n;
}

int64_t sr3_read_weight_layout(sr3_ctx *c, const char *name, int layout, void *host, int64_t cap_bytes) {
    if (!c || !name || cap_bytes < 0 || (cap_bytes > 0 && !host)) return fail("sr3_read_weight_layout: bad argument");
    if (layout < 0 || layout >= SR3_N_WEIGHT_LAYOUTS) return fail("sr3_read_weight_layout: layout %d unknown", layout);
    HIP_OK(hipSetDevice(c->device));
    int pi = -1;
    for (size_t i = 0; i < c->params.size(); ++i)
        if (c->params[i].name == name) { pi = (int)i; break; }
    if (pi < 0) return fail("unknown parameter '%s'", name);
    const Param &p = c->params[pi];
    const float *src = nullptr;
    size_t floats = 0;
    const bool conv = p.kind == P_CONV;
    const size_t wino_floats = (size_t)16 * p.cout * p.cin_pad;
    switch (layout) {
    case SR3_WL_PLAIN: src = p.dev; floats = p.dev_floats; break;
    case SR3_WL_SPLIT: src = p.dev_split; floats = p.dev_floats; break;
    case SR3_WL_F8: src = p.dev_f8; floats = p.dev_floats; break;
    case SR3_WL_WINO: src = p.dev_wino; floats = wino_floats; break;
    case SR3_WL_WINO_FRAG: src = p.dev_wino_f; floats = wino_floats; break;
    case SR3_WL_UP_WINO_FRAG: src = p.dev_up_wino; floats = up2_wino_floats(p.cout, p.cin_pad); break;
    case SR3_WL_CONV_IN:
        if (conv && pi == c->mods[0].conv.w) { src = c->ci_w; floats = conv_in_weight_floats(p.cout); }
        break;
    case SR3_WL_FINAL_MFMA:
        if (conv && pi == c->final_conv.w) { src = c->final_wm; floats = final_conv_mfma_weight_floats(p.cin); }
        break;
    case SR3_WL_FINAL_VALU:
        if (conv && pi == c->final_conv.w) { src = c->final_wq; floats = (size_t)9 * p.cin * 4; }
        break;
    case SR3_WL_FUSED_BIAS:
        for (auto &m : c->mods)
            if (m.kind == M_RES && m.rb.has_res && m.rb.c2.b == pi) { src = m.rb.fused_bias; floats = (size_t)m.rb.cout; }
        break;
    case SR3_WL_IDENT:
        for (auto &m : c->mods)
            if (m.kind == M_RES && !m.rb.has_res && m.rb.c2.w == pi) { src = m.rb.ident_w; floats = (size_t)m.rb.cout * m.rb.cout; }
        break;
    }
    if (!src) return 0;
    const int64_t bytes = (int64_t)(floats * sizeof(float));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (cap_bytes > 0) HIP_OK(hipMemcpy(host, src, (size_t)std::min(bytes, cap_bytes), hipMemcpyDeviceToHost));
    return bytes;
}

float sr3_weight_unscale(sr3_ctx *c, const char *name) {
    if (!c || !name) { fail("sr3_weight_unscale: null argument"); return 0.f; }
    for (auto &p : c->params)
        if (p.name == name) {
            return p.w_unscale;
        }
    fail("unknown parameter '%s'", name);
    return 0.f;
}

int sr3_weights_missing(sr3_ctx *c) {
    if (!c) return fail("null context");
    int n = 0;
    for (auto &p : c->params) n += p.loaded ? 0 : 1;
    return n;
}

int sr3_chan_bias_total(sr3_ctx *c) { return c ? c->nf_total : fail("null context"); }

// one evaluation in the context's current arithmetic (the callable of guarded_eval)
// depth > 0: the shallow forward; a whole one leaves the workspace as the cache of this arithmetic
static int unet_forward_once(sr3_ctx *c, const float *x_dev, const float *noise_level_dev, int B, int H, int W, int depth,
                             float *out_dev) {
    c->pbegin(F_MISC);
    launch_nchw_to_nhwc(x_dev, B, c->cfg.in_channel, c->x0, 0, c->stream);
    if (c->x0p) launch_pack_state(c->x0, B, c->x0p, c->stream, c->d_ovf);
    c->pend();
    run_embed(c, noise_level_dev, 1, B);
    run_unet_body(c, B, H, W, depth);
    if (!depth) c->fc_mode = (int)c->mode;
    c->pbegin(F_MISC);
    launch_nhwc_to_nchw(c->eps, 0, B, c->cfg.out_channel, out_dev, c->stream);
    c->pend();
    HIP_OK(hipGetLastError());
    if (const char *e = conv_take_error()) return fail("sr3_unet_forward: %s", e);
    return 0;
}

int sr3_unet_forward(sr3_ctx *c, const float *x_dev, const float *noise_level_dev, int B, int H, int W,
                     float *out_dev) {
    PlanScope plan_scope(c);
    if (check_ready(c)) return -1;
    if (!x_dev || !noise_level_dev || !out_dev) return fail("sr3_unet_forward: null pointer");
    if (ensure_workspace(c, B, H, W)) return -1;
    c->sampling = false; c->rows_on = false;
    if (push_drop_args(c, "sr3_unet_forward", c->drop_offset)) return -1;
    c->fc_invalidate();
    // (each evaluation records its arithmetic: after a step down the workspace holds the features of the rung landed on)
    const int r = guarded_eval(c, "sr3_unet_forward", "the forward pass", true,
                               [&] { return unet_forward_once(c, x_dev, noise_level_dev, B, H, W, 0, out_dev); });
    if (r < 0) c->fc_invalidate();
    return r;
}

// the modules of a shallow forward of `depth`, checked against the graph this context built
static int check_cache_depth(sr3_ctx *c, const char *what, int depth) {
    if (depth < 1 || depth > c->fc_max_depth())
        return fail("%s: depth %d outside [1, %d] (the resolution levels kept fresh; n_mults - 1 at the most)", what, depth,
                    c->fc_max_depth());
    const ShallowSplit sh = shallow_split(c, depth);
    if (sh.down_end > c->n_downs || sh.up_begin <= c->n_downs + c->n_mid || c->mods[sh.up_begin - 1].kind != M_UP)
        return fail("internal: the shallow forward of depth %d does not resume behind an Upsample", depth);
    return 0;
}

int sr3_unet_forward_cached(sr3_ctx *c, const float *x_dev, const float *noise_level_dev, int B, int H, int W, int depth,
                            float *out_dev) {
    PlanScope plan_scope(c);
    if (check_ready(c)) return -1;
    if (!x_dev || !noise_level_dev || !out_dev) return fail("sr3_unet_forward_cached: null pointer");
    if (check_cache_depth(c, "sr3_unet_forward_cached", depth)) return -1;
    if (!c->arena || c->wB != B || c->wH != H || c->wW != W || c->fc_mode != (int)c->mode)
        return fail("sr3_unet_forward_cached: the workspace holds no whole forward of B=%d H=%d W=%d in the current arithmetic "
                    "(run sr3_unet_forward at that shape first; a new shape, sr3_set_precision, a weight load and a forward "
                    "that the range policy finished in another arithmetic all discard it)", B, H, W);
    c->sampling = false; c->rows_on = false;
    c->fc_call = false;
    if (push_drop_args(c, "sr3_unet_forward_cached", c->drop_offset)) return -1;
    // (no step down: the deep features are those of this arithmetic; out of range is an error that names it)
    return guarded_eval(c, "sr3_unet_forward_cached", "the shallow forward pass", false,
                        [&] { return unet_forward_once(c, x_dev, noise_level_dev, B, H, W, depth, out_dev); });
}

int sr3_set_feature_cache(sr3_ctx *c, int interval, int depth) {
    if (!c) return fail("null context");
    if (interval <= 1) { c->fc_interval = 0; return 0; }
    if (check_cache_depth(c, "sr3_set_feature_cache", depth)) return -1;
    c->fc_interval = interval; c->fc_depth = depth;
    return 0;
}

int sr3_feature_cache_steps(sr3_ctx *c, int *whole, int *shallow) {
    if (!c || !whole || !shallow) return fail("sr3_feature_cache_steps: null argument");
    *whole = c->fc_whole; *shallow = c->fc_shallow;
    return 0;
}

// ---- the denoising loss (diffusion.py:284-313, evaluation only) ---------------------------------
namespace {
struct LossCall {
    const float *hr, *cond, *level, *s;
    NoiseRef nz;
    int N, row_offset, B, H, W, loss_type;
    double *per_image;
    float *x_noisy_out, *eps_out;
};
}

// fp64 partial sums of the reductions (metrics, loss): one buffer, grown on demand
static int ensure_partials(sr3_ctx *c, size_t need) {
    if (c->metrics_ws_n >= need) return 0;
    if (c->metrics_ws) HIP_OK(hipFree(c->metrics_ws));   // (hipFree waits for the kernels still reading it)
    c->metrics_ws = nullptr; c->metrics_ws_n = 0;
    HIP_OK(hipMalloc(&c->metrics_ws, need * sizeof(double)));
    c->metrics_ws_n = need;
    return 0;
}

// one evaluation in the context's current arithmetic: state kernel, embedding, UNet body, loss kernels
static int denoise_loss_once(sr3_ctx *c, const LossCall &k) {
    const int C = c->cfg.out_channel, nc = c->cfg.in_channel - C;
    c->pbegin(F_MISC);
    launch_q_sample_state(k.hr, k.cond, k.N, k.row_offset, k.level, k.s, k.nz, k.B, C, nc, c->x0, c->x0p, c->d_ovf,
                          k.x_noisy_out, c->stream);
    c->pend();
    run_embed(c, k.level, 1, k.B);
    run_unet_body(c, k.B, k.H, k.W);
    c->pbegin(F_MISC);
    launch_denoise_loss(c->eps, k.nz, k.N, k.row_offset, k.B, C, k.loss_type, c->metrics_ws, k.per_image, k.eps_out, c->stream);
    c->pend();
    HIP_OK(hipGetLastError());
    if (const char *e = conv_take_error()) return fail("sr3_denoise_loss: %s", e);
    return 0;
}

int sr3_denoise_loss(sr3_ctx *c, const float *hr_dev, const float *cond_dev, int N, int row_offset, const float *level_dev,
                     const float *s_dev, const float *noise_dev, int noise_per_source, uint64_t seed, uint64_t image_offset,
                     int B, int H, int W, int loss_type, double *per_image_dev, float *x_noisy_out, float *eps_out) {
    PlanScope plan_scope(c);
    if (check_ready(c)) return -1;
    if (!hr_dev || !level_dev || !s_dev || !per_image_dev) return fail("sr3_denoise_loss: null pointer");
    if (loss_type != 0 && loss_type != 1) return fail("sr3_denoise_loss: loss_type %d is neither 0 (l1) nor 1 (l2)", loss_type);
    if (N < 1 || row_offset < 0) return fail("sr3_denoise_loss: bad rows (N=%d row_offset=%d)", N, row_offset);
    const int C = c->cfg.out_channel, nc = c->cfg.in_channel - C;
    if (cond_dev && nc <= 0) return fail("sr3_denoise_loss: conditioning given but in_channel == out_channel");
    if (!cond_dev && nc != 0) return fail("sr3_denoise_loss: the unconditional loss needs in_channel == out_channel");
    if (c->cfg.in_channel > 8)
        return fail("sr3_denoise_loss: in_channel = %d, the state kernel builds at most 8 input channels", c->cfg.in_channel);
    if (ensure_workspace(c, B, H, W)) return -1;
    if (ensure_partials(c, (size_t)B * loss_blocks(H, W))) return -1;
    c->sampling = false; c->rows_on = false;
    c->fc_invalidate();
    LossCall k;
    k.hr = hr_dev; k.cond = cond_dev; k.level = level_dev; k.s = s_dev;
    k.nz.noise = noise_dev; k.nz.seed = seed; k.nz.image_offset = image_offset; k.nz.per_source = noise_per_source != 0;
    k.N = N; k.row_offset = row_offset; k.B = B; k.H = H; k.W = W; k.loss_type = loss_type;
    k.per_image = per_image_dev; k.x_noisy_out = x_noisy_out; k.eps_out = eps_out;
    // (dropout masks follow the batch ROW: with one noise image per source, image_offset does not advance with the rows
    // of a chunked call, row_offset does)
    if (push_drop_args(c, "sr3_denoise_loss", image_offset + (noise_per_source ? (uint64_t)row_offset : 0))) return -1;
    return guarded_eval(c, "sr3_denoise_loss", "the loss evaluation", true, [&] { return denoise_loss_once(c, k); });
}

int sr3_op_q_sample(sr3_ctx *c, const float *hr_dev, int N, int row_offset, const float *level_dev, const float *s_dev,
                    const float *noise_dev, int noise_per_source, uint64_t seed, uint64_t image_offset, int B, int C, int H,
                    int W, float *x_noisy_out) {
    if (!c || !hr_dev || !level_dev || !s_dev || !x_noisy_out) return fail("sr3_op_q_sample: null argument");
    if (N < 1 || row_offset < 0 || B < 1 || C < 1 || C > 4 || H < 1 || W < 1)
        return fail("sr3_op_q_sample: bad size (N=%d row_offset=%d B=%d C=%d H=%d W=%d)", N, row_offset, B, C, H, W);
    HIP_OK(hipSetDevice(c->device));
    NoiseRef nz;
    nz.noise = noise_dev; nz.seed = seed; nz.image_offset = image_offset; nz.per_source = noise_per_source != 0;
    TDesc geom;                 // geometry only (p == nullptr): no state is written
    geom.C = C; geom.H = H; geom.W = W;
    launch_q_sample_state(hr_dev, nullptr, N, row_offset, level_dev, s_dev, nz, B, C, 0, geom, nullptr, nullptr, x_noisy_out,
                          c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

static int set_step_tables(sr3_ctx *c, int T, const float *noise_level, const float *a, const float *b,
                           const float *c1, const float *c2, const float *c3, const std::vector<float> &sigma,
                           bool uses_hist) {
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->stream));
    c->T = T;
    c->s_nl.assign(noise_level, noise_level + T + 1);
    c->s_a.assign(a, a + T);
    c->s_b.assign(b, b + T);
    c->s_c1.assign(c1, c1 + T);
    c->s_c2.assign(c2, c2 + T);
    if (c3) c->s_c3.assign(c3, c3 + T);
    else c->s_c3.assign((size_t)T, 0.f);
    c->s_sig = sigma;
    c->uses_hist = uses_hist;
    if (c->d_nl) HIP_OK(hipFree(c->d_nl));
    HIP_OK(hipMalloc(&c->d_nl, (size_t)(T + 1) * sizeof(float)));
    HIP_OK(hipMemcpy(c->d_nl, noise_level, (size_t)(T + 1) * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int sr3_set_schedule(sr3_ctx *c, int T, const float *noise_level, const float *recip, const float *recipm1,
                     const float *logvar, const float *coef1, const float *coef2) {
    if (!c) return fail("null context");
    if (T < 1 || !noise_level || !recip || !recipm1 || !logvar || !coef1 || !coef2)
        return fail("sr3_set_schedule: invalid argument");
    std::vector<float> sigma((size_t)T);
    for (int t = 0; t < T; ++t) sigma[t] = t > 0 ? expf(0.5f * logvar[t]) : 0.f;
    return set_step_tables(c, T, noise_level, recip, recipm1, coef1, coef2, nullptr, sigma, false);
}

int sr3_set_sampler_schedule(sr3_ctx *c, int S, const float *noise_level, const float *a, const float *b,
                             const float *c1, const float *c2, const float *c3, const float *sigma, int uses_history) {
    if (!c) return fail("null context");
    if (S < 1 || !noise_level || !a || !b || !c1 || !c2 || !c3 || !sigma)
        return fail("sr3_set_sampler_schedule: invalid argument");
    for (int i = 0; i < S; ++i)
        if (!std::isfinite(c1[i]) || !std::isfinite(c2[i]) || !std::isfinite(c3[i]) || !std::isfinite(sigma[i]) || sigma[i] < 0.f)
            return fail("sr3_set_sampler_schedule: coefficients of step %d are not finite (or sigma < 0)", i);
    return set_step_tables(c, S, noise_level, a, b, c1, c2, c3, std::vector<float>(sigma, sigma + S), uses_history != 0);
}

int sr3_max_batch(sr3_ctx *c, int H, int W) {
    PlanScope plan_scope(c);
    if (!c) return fail("null context");
    const int b = max_batch(c, H, W);
    if (b < 0) return fail("unsupported shape H=%d W=%d: attention over more than 1024 tokens at more than 512 channels", H, W);
    if (b == 0) return fail("unsupported shape H=%d W=%d: H and W must be multiples of %d", H, W, 1 << (c->cfg.n_mults - 1));
    return b;
}

int sr3_num_frames_from(sr3_ctx *c, int start_step) {
    if (!c) return fail("null context");
    if (c->T < 1) return fail("no schedule set");
    if (start_step < 1 || start_step > c->T)
        return fail("sr3_num_frames_from: start_step %d outside [1, %d]", start_step, c->T);
    const int si = 1 | (c->T / 10);
    int n = 0;
    for (int i = 0; i < start_step; ++i) n += (i % si == 0) ? 1 : 0;
    return n;
}

int sr3_num_frames(sr3_ctx *c) {
    if (!c) return fail("null context");
    if (c->T < 1) return fail("no schedule set");
    return sr3_num_frames_from(c, c->T);
}

namespace {
// float32 sqrt(1 - a^2) of q_sample (diffusion.py:281), every operation rounded by itself as noise_coefficient
// (diffusion.py of this package) forms it: the product must not meet the difference in one fused multiply-add
float q_sample_noise_coefficient(float a) {
#pragma clang fp contract(off)
    const float aa = a * a;
    const float d = 1.0f - aa;
    return sqrtf(d);
}

// What sr3_sample_begin (init_dev null) and sr3_sample_begin_from share behind their own argument checks: the workspace,
// the per-call resets, the features' buffers and the first state. That state: q_sample(init) at the level of the state
// before step start_step - 1 (noised) | init itself | without an init, the noise (noise0_dev, or null: Philox draw 0).
int begin_impl(sr3_ctx *c, const char *what, const float *cond_dev, int B, int H, int W, const float *init_dev, int start_step,
               bool noised, const float *noise0_dev, uint64_t seed, uint64_t image_offset) {
    const int C = c->cfg.out_channel, nc = c->cfg.in_channel - C;
    if (cond_dev && nc <= 0) return fail("conditioning given but in_channel == out_channel");
    if (!cond_dev && nc != 0) return fail("unconditional sampling needs in_channel == out_channel");
    if (init_dev && init_dev == cond_dev && nc != C)
        return fail("%s: the conditioning image has %d channels and cannot start a state of %d", what, nc, C);
    if (noised && c->cfg.in_channel > 8)
        return fail("%s: in_channel = %d, the state kernel builds at most 8 input channels", what, c->cfg.in_channel);
    if (ensure_workspace(c, B, H, W)) return -1;
    c->rows_on = false;         // (a sampling call during a row session takes the workspace over, as it does during a step session)
    if (noised && c->start_rows < B) {
        if (c->d_start) HIP_OK(hipFree(c->d_start));   // (hipFree waits for the kernels still reading it)
        c->d_start = nullptr; c->start_rows = 0;
        HIP_OK(hipMalloc(&c->d_start, (size_t)2 * B * sizeof(float)));
        c->start_rows = B;
    }
    c->seed = seed;
    c->image_offset = image_offset;
    c->hist_valid = false;
    c->fc_k = 0; c->fc_call = false; c->fc_whole = c->fc_shallow = 0;
    if (c->lr_on() && prepare_lr_step(c, B, H, W)) return -1;
    if (c->dyn_on() && prepare_dyn_step(c, B, H, W)) return -1;
    if (range_reset(c)) return -1;
    c->pbegin(F_MISC);
    if (noised) {
        // the reference's q_sample (diffusion.py:275-282) at the level of the state before step start_step - 1
        const float level = c->s_nl[start_step];
        float *a = c->d_start, *s = c->d_start + c->start_rows;
        launch_fill_pair(a, s, level, q_sample_noise_coefficient(level), B, c->stream);
        NoiseRef nz;
        nz.noise = noise0_dev; nz.seed = seed; nz.image_offset = image_offset; nz.per_source = 0;
        launch_q_sample_state(init_dev, cond_dev, B, 0, a, s, nz, B, C, nc, c->x0, c->x0p, c->d_ovf, nullptr, c->stream);
    } else {
        // the image itself, bit for bit (as Checkpoint::restore reloads a state), or the start noise
        if (cond_dev) launch_nchw_to_nhwc(cond_dev, B, nc, c->x0, 0, c->stream);
        launch_init_state(c->x0, nc, C, init_dev ? init_dev : noise0_dev, seed, image_offset, B, c->stream);
        if (c->x0p) launch_pack_state(c->x0, B, c->x0p, c->stream, c->d_ovf);
    }
    c->pend();
    c->sampling = true; c->rows_on = false;
    HIP_OK(hipGetLastError());
    return 0;
}
}

int sr3_sample_begin(sr3_ctx *c, const float *cond_dev, int B, int H, int W, const float *init_noise_dev,
                     uint64_t seed, uint64_t image_offset) {
    PlanScope plan_scope(c);
    if (check_ready(c)) return -1;
    if (c->T < 1) return fail("sr3_sample_begin: no schedule set (sr3_set_schedule)");
    if (begin_impl(c, "sr3_sample_begin", cond_dev, B, H, W, nullptr, c->T, false, init_noise_dev, seed, image_offset)) return -1;
    c->fold_first = false;
    return 0;
}

int sr3_sample_begin_from(sr3_ctx *c, const float *cond_dev, int B, int H, int W, const float *init_dev, int start_step,
                          int noised, const float *noise0_dev, uint64_t seed, uint64_t image_offset) {
    PlanScope plan_scope(c);
    if (check_ready(c)) return -1;
    if (c->T < 1) return fail("sr3_sample_begin_from: no schedule set (sr3_set_schedule)");
    if (!init_dev) return fail("sr3_sample_begin_from: init_dev is null");
    if (start_step < 1 || start_step > c->T)
        return fail("sr3_sample_begin_from: start_step %d outside [1, %d]", start_step, c->T);
    if (B < 1) return fail("sr3_sample_begin_from: bad batch B=%d", B);
    if (begin_impl(c, "sr3_sample_begin_from", cond_dev, B, H, W, init_dev, start_step, noised != 0, noise0_dev, seed, image_offset))
        return -1;
    c->fold_first = true;
    return 0;
}

int sr3_sample_step(sr3_ctx *c, int t, const float *noise_slab_dev) {
    PlanScope plan_scope(c);
    if (!c) return fail("null context");
    HIP_OK(hipSetDevice(c->device));
    if (step_checked(c, t, noise_slab_dev, nullptr)) return -1;
    HIP_OK(hipGetLastError());
    return 0;
}

// the sampler state (channels after the conditioning) as NCHW
static int sample_copy_out(sr3_ctx *c, float *out_dev) {
    const int C = c->cfg.out_channel;
    c->pbegin(F_MISC);
    launch_nhwc_to_nchw(c->x0, c->cfg.in_channel - C, c->wB, C, out_dev, c->stream);
    c->pend();
    HIP_OK(hipGetLastError());
    return 0;
}

int sr3_sample_end(sr3_ctx *c, float *out_dev) {
    PlanScope plan_scope(c);
    if (!c || !out_dev) return fail("sr3_sample_end: null argument");
    if (!c->sampling) return fail("sr3_sample_end before sr3_sample_begin");
    if (sample_copy_out(c, out_dev)) return -1;
    // split-f16 mode: synchronises and fails if an activation left the fp16 range during the steps
    return c->split() ? range_check(c, "sr3_sample_end") : 0;
}

int sr3_range_check(sr3_ctx *c) {
    if (!c) return fail("null context");
    HIP_OK(hipSetDevice(c->device));
    return range_check(c, "sr3_range_check");
}


// ---- rolling batch: every row at its own position -------------------------------------------------
namespace {
// one row of the workspace as a batch of its own: the existing one-batch kernels then admit and retire single rows
TDesc row_desc(const TDesc &d, int row) {
    TDesc r = d;
    r.p = d.p + (size_t)row * d.Hp() * d.Wp() * d.C;
    return r;
}
float *row_packed(sr3_ctx *c, int row) {
    return c->x0p ? c->x0p + (size_t)row * (c->wH + 2) * (c->wW + 2) * 8 : nullptr;
}

int rows_check(sr3_ctx *c, const char *what, int row) {
    if (!c) return fail("null context");
    if (!c->rows_on || (int)c->rows.size() != c->wB) return fail("%s outside a row session (sr3_rows_begin)", what);
    if (row < 0 || row >= c->wB) return fail("%s: row %d outside the session's %d slots", what, row, c->wB);
    return 0;
}

// table, pinned ring and q_sample coefficients for B slots (their addresses change only when B outgrows them)
int rows_reserve(sr3_ctx *c, int B) {
    if (c->rows_cap >= B) return 0;
    HIP_OK(hipStreamSynchronize(c->stream));
    if (c->h_rows) HIP_OK(hipHostFree(c->h_rows));
    if (c->d_rows) HIP_OK(hipFree(c->d_rows));
    if (c->d_row_start) HIP_OK(hipFree(c->d_row_start));
    c->h_rows = nullptr; c->d_rows = nullptr; c->d_row_start = nullptr; c->rows_cap = 0;
    HIP_OK(hipHostMalloc(reinterpret_cast<void **>(&c->h_rows), sizeof(RowArgs) * sr3_ctx::kRowRing * B, hipHostMallocDefault));
    HIP_OK(hipMalloc(&c->d_rows, sizeof(RowArgs) * B));
    HIP_OK(hipMalloc(&c->d_row_start, sizeof(float) * 2 * B));
    c->rows_cap = B;
    return 0;
}
}

int sr3_rows_begin(sr3_ctx *c, int B, int H, int W, uint64_t seed) {
    PlanScope plan_scope(c);
    if (check_ready(c)) return -1;
    if (c->T < 1) return fail("sr3_rows_begin: no schedule set (sr3_set_schedule)");
    if (B < 1) return fail("sr3_rows_begin: bad slot count B=%d", B);
    if (c->cfg.in_channel - c->cfg.out_channel <= 0)
        return fail("sr3_rows_begin: the unconditional model (in_channel == out_channel) has no per-request input to admit");
    if (c->lr_on())
        return fail("sr3_rows_begin: low-resolution consistency (sr3_set_lr_consistency) is on: its LR rows follow one image "
                    "offset per call, not a row session; turn it off first");
    if (c->fc_on())
        return fail("sr3_rows_begin: the feature cache (sr3_set_feature_cache) is on: its whole and shallow steps are counted "
                    "per call, not per row; turn it off first");
    if (c->drop_live())
        return fail("sr3_rows_begin: Dropout sampling (sr3_set_dropout) is on: its masks are keyed by one image offset and one "
                    "draw per step; turn it off first");
    if (ensure_workspace(c, B, H, W)) return -1;
    c->sampling = false; c->rows_on = false;
    if (rows_reserve(c, B)) return -1;
    if (c->dyn_on() && prepare_dyn_step(c, B, H, W)) return -1;
    c->seed = seed;
    c->image_offset = 0;
    c->hist_valid = false;
    c->fc_invalidate();
    c->rows.assign((size_t)B, sr3_ctx::RowState());
    c->rows_lr = false; c->rows_admitted = false;
    if (range_reset(c)) return -1;
    // every slot idle and zero: an idle row still runs through the UNet, and must never carry a NaN or Inf into it
    // (the borders and pad channels of the state are zero already and stay so)
    HIP_OK(hipMemsetAsync(c->x0.p, 0, c->x0.floats(B) * sizeof(float), c->stream));
    if (c->x0p) HIP_OK(hipMemsetAsync(c->x0p, 0, (size_t)B * (H + 2) * (W + 2) * 8 * sizeof(float), c->stream));
    HIP_OK(hipMemsetAsync(c->xhist, 0, (size_t)B * c->cfg.out_channel * H * W * sizeof(float), c->stream));
    c->rows_on = true;
    return 0;
}

int sr3_rows_lr_consistency(sr3_ctx *c, int lh, int lw) {
    PlanScope plan_scope(c);
    if (rows_check(c, "sr3_rows_lr_consistency", 0)) return -1;
    HIP_OK(hipSetDevice(c->device));
    if (c->rows_admitted)
        return fail("sr3_rows_lr_consistency: a row was admitted already; arm the session right after sr3_rows_begin");
    const int B = c->wB, C = c->cfg.out_channel, H = c->wH, W = c->wW;
    if (check_lr_shape("sr3_rows_lr_consistency", C, H, W, B, lh, lw)) return -1;
    LrOps o;
    if (get_lr_ops(c, lh, lw, H, W, &o)) return -1;
    const bool lds = lr_lds_fits(o);
    if (ensure_x0hat(c, (size_t)B * C * H * W)) return -1;
    if (!lds && ensure_lr_scratch(c, lr_scratch_floats(B * C, o))) return -1;
    const size_t need = (size_t)B * C * lh * lw;
    if (c->rows_lr_floats < need) {
        HIP_OK(hipStreamSynchronize(c->stream));
        if (c->rows_lr_buf) HIP_OK(hipFree(c->rows_lr_buf));
        c->rows_lr_buf = nullptr; c->rows_lr_floats = 0;
        HIP_OK(hipMalloc(&c->rows_lr_buf, need * sizeof(float)));
        c->rows_lr_floats = need;
    }
    c->rows_lr_ops = o; c->rows_lr_lds = lds;
    c->rows_lr = true;
    return 0;
}

namespace {
int rows_admit_impl(sr3_ctx *c, const char *what, int row, const float *cond_dev, const float *init_dev, int start_step, int noised,
                    const float *noise0_dev, uint64_t image_id, const float *lr_dev, float strength) {
    if (rows_check(c, what, row)) return -1;
    HIP_OK(hipSetDevice(c->device));
    if (!cond_dev) return fail("%s: cond_dev is null", what);
    sr3_ctx::RowState &r = c->rows[row];
    if (r.live) return fail("%s: slot %d is live (%d steps left); retire or drop it first", what, row, r.pos);
    const int C = c->cfg.out_channel, nc = c->cfg.in_channel - C;
    if (init_dev ? (start_step < 1 || start_step > c->T) : start_step != c->T)
        return fail("%s: start_step %d outside [1, %d] (%d without init_dev)", what, start_step, c->T, c->T);
    if (init_dev && init_dev == cond_dev && nc != C)
        return fail("%s: the conditioning image has %d channels and cannot start a state of %d", what, nc, C);
    const bool q = init_dev && noised;
    if (q && c->cfg.in_channel > 8)
        return fail("%s: in_channel = %d, the state kernel builds at most 8 input channels", what, c->cfg.in_channel);
    if (!(strength >= 0.f) || strength > 1.f) return fail("%s: strength must lie in [0, 1], got %g", what, (double)strength);
    const bool held = lr_dev != nullptr && strength != 0.f;
    if (held && !c->rows_lr)
        return fail("%s: an LR image for a session that is not armed; call sr3_rows_lr_consistency after sr3_rows_begin", what);
    const TDesc x0r = row_desc(c->x0, row);
    float *xpr = row_packed(c, row);
    c->pbegin(F_MISC);
    if (q) {
        // sr3_sample_begin_from's kernel on this row alone: the same expression, the same stores
        const float level = c->s_nl[start_step];
        float *a = c->d_row_start + row, *s = c->d_row_start + c->rows_cap + row;
        launch_fill_pair(a, s, level, q_sample_noise_coefficient(level), 1, c->stream);
        NoiseRef nz;
        nz.noise = noise0_dev; nz.seed = c->seed; nz.image_offset = image_id; nz.per_source = 0;
        launch_q_sample_state(init_dev, cond_dev, 1, 0, a, s, nz, 1, C, nc, x0r, xpr, c->d_ovf, nullptr, c->stream);
    } else {
        launch_nchw_to_nhwc(cond_dev, 1, nc, x0r, 0, c->stream);
        launch_init_state(x0r, nc, C, init_dev ? init_dev : noise0_dev, c->seed, image_id, 1, c->stream);
        if (xpr) launch_pack_state(x0r, 1, xpr, c->stream, c->d_ovf);
    }
    c->pend();
    HIP_OK(hipGetLastError());
    // the slot's own copy of the LR image, behind the steps enqueued so far (they read the previous occupant's, if any)
    if (held) {
        const size_t n = (size_t)C * c->rows_lr_ops.lh * c->rows_lr_ops.lw;
        HIP_OK(hipMemcpyAsync(c->rows_lr_buf + (size_t)row * n, lr_dev, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    r = sr3_ctx::RowState();            // (not held, no frames: nothing of the previous occupant is left)
    r.live = true; r.pos = r.start = start_step; r.image = image_id;
    r.fold = init_dev != nullptr;       // (as sr3_sample_begin_from: the first step of a multistep sampler is first order)
    r.lr_strength = held ? strength : 0.f;
    c->rows_admitted = true;
    return 0;
}
}

int sr3_rows_admit(sr3_ctx *c, int row, const float *cond_dev, const float *init_dev, int start_step, int noised,
                   const float *noise0_dev, uint64_t image_id) {
    PlanScope plan_scope(c);
    return rows_admit_impl(c, "sr3_rows_admit", row, cond_dev, init_dev, start_step, noised, noise0_dev, image_id, nullptr, 0.f);
}

int sr3_rows_admit_lr(sr3_ctx *c, int row, const float *cond_dev, const float *init_dev, int start_step, int noised,
                      const float *noise0_dev, uint64_t image_id, const float *lr_dev, float strength) {
    PlanScope plan_scope(c);
    return rows_admit_impl(c, "sr3_rows_admit_lr", row, cond_dev, init_dev, start_step, noised, noise0_dev, image_id, lr_dev,
                           strength);
}

int sr3_rows_frames(sr3_ctx *c, int row, float *frames_dev, int capacity) {
    if (rows_check(c, "sr3_rows_frames", row)) return -1;
    if (!frames_dev) return fail("sr3_rows_frames: frames_dev is null");
    sr3_ctx::RowState &r = c->rows[row];
    if (!r.live || r.pos != r.start)
        return fail("sr3_rows_frames: slot %d is %s; call it after sr3_rows_admit and before the row's first step", row,
                    r.live ? "past its first step" : "idle");
    const int n = sr3_num_frames_from(c, r.start);
    if (n < 0) return -1;
    if (capacity < n) return fail("sr3_rows_frames: a row begun at step %d writes %d frames, capacity is %d", r.start, n, capacity);
    r.frames = frames_dev; r.frames_n = 0; r.frames_cap = n;
    return 0;
}

int sr3_rows_step(sr3_ctx *c, const float *const *noise_rows) {
    if (rows_check(c, "sr3_rows_step", 0)) return -1;
    return sr3_rows_step_batch(c, noise_rows, c->wB);
}

// (B below is the step's batch: every loop and every launch covers slots [0, B); with B == wB the key carries batch 0 and
// the step is the one sr3_rows_step always launched)
int sr3_rows_step_batch(sr3_ctx *c, const float *const *noise_rows, int batch) {
    PlanScope plan_scope(c);
    if (rows_check(c, "sr3_rows_step", 0)) return -1;
    HIP_OK(hipSetDevice(c->device));
    if (batch < 1 || batch > c->wB) return fail("sr3_rows_step_batch: batch %d outside [1, %d], the session's slots", batch, c->wB);
    if (batch < c->wB && c->plan_batch <= 0)
        return fail("sr3_rows_step_batch: batch %d below the session's %d slots needs the batch-invariant mode (sr3_set_batch_invariant "
                    "before sr3_rows_begin): the workspace was sized by plans that follow the batch, and a smaller batch may "
                    "ask more of it", batch, c->wB);
    const int B = batch;
    int live = 0;
    for (int n = 0; n < c->wB; ++n) {
        const auto &r = c->rows[n];
        // (positions index the step tables: a schedule set after a row was admitted may be shorter)
        if (r.live && r.pos > c->T) return fail("sr3_rows_step: a row has %d steps left and the schedule %d: the schedule was changed after sr3_rows_admit", r.pos, c->T);
        if (r.live && r.pos > 0 && n >= B)
            return fail("sr3_rows_step_batch: slot %d is live with %d steps left and lies outside batch %d (sr3_rows_move it below the batch, or step a larger one)", n, r.pos, B);
        live += (r.live && r.pos > 0) ? 1 : 0;
    }
    if (!live) return 0;
    if (B < c->wB && std::find(c->rows_batch_ok.begin(), c->rows_batch_ok.end(), B) == c->rows_batch_ok.end()) {
        if (rows_batch_fits(c, B)) return -1;
        c->rows_batch_ok.push_back(B);
    }
    if (prepare_f8(c)) return -1;
    if (c->lr_on() || c->fc_on() || c->drop_live())
        return fail("sr3_rows_step: low-resolution consistency, the feature cache or Dropout sampling was turned on after sr3_rows_begin");
    if (c->dyn_on()) {
        const int64_t n = (int64_t)c->cfg.out_channel * c->wH * c->wW;
        if (c->dyn_n != n || c->dyn_rows < B || c->x0hat_floats < (size_t)B * n || c->dyn_plan.k != threshold_plan(c->dyn_ratio, n).k)
            return fail("sr3_rows_step: the dynamic threshold was turned on or changed after sr3_rows_begin; set it before");
    }
    if (c->rows_lr && (c->x0hat_floats < (size_t)B * c->cfg.out_channel * c->wH * c->wW ||
                       (!c->rows_lr_lds && c->lr_scratch_n < lr_scratch_floats(B * c->cfg.out_channel, c->rows_lr_ops))))
        return fail("sr3_rows_step: the buffers of the armed session are gone; arm it again after sr3_rows_begin");
    const int frame_every = 1 | (c->T / 10);        // (sr3_sample's rule: a frame after every step t with t % (1 | T/10) == 0)
    // the host may run ahead of the GPU: never reuse a ring slot that may still be pending
    if (c->rows_count && (c->rows_count % (sr3_ctx::kRowRing / 2)) == 0) HIP_OK(hipStreamSynchronize(c->stream));
    RowArgs *slot = c->h_rows + (size_t)(c->rows_count % sr3_ctx::kRowRing) * c->rows_cap;
    ++c->rows_count;
    // the positions as they stand after this step: committed only once the step is enqueued, so that a failed call
    // leaves the host where the device is
    std::vector<sr3_ctx::RowState> next = c->rows;
    for (int n = 0; n < B; ++n) {
        sr3_ctx::RowState &r = next[n];
        RowArgs ra = RowArgs();
        ra.nl = c->s_nl[0];             // an idle row runs through the UNet at the level of a finished image
        if (r.live && r.pos > 0) {
            const int t = r.pos - 1;
            ra.live = 1;
            ra.nl = c->s_nl[t + 1];
            ra.a = c->s_a[t]; ra.b = c->s_b[t]; ra.c1 = c->s_c1[t]; ra.c2 = c->s_c2[t]; ra.c3 = c->s_c3[t];
            ra.sigma = c->s_sig[t];
            if (r.fold && c->uses_hist && !r.hist_valid) ra.c1 = c->s_c1[t] + c->s_c3[t];
            ra.draw = (uint32_t)(c->T - t);
            ra.hist = c->uses_hist ? (r.hist_valid ? 2u : 1u) : 0u;
            if (c->uses_hist) r.hist_valid = true;
            ra.image = r.image; ra.seed = c->seed;
            ra.noise = (noise_rows && t > 0) ? noise_rows[n] : nullptr;
            ra.lr_strength = c->rows_lr ? r.lr_strength : 0.f;
            if (r.frames && t % frame_every == 0 && r.frames_n < r.frames_cap)
                ra.frame = r.frames + (size_t)(r.frames_n++) * c->cfg.out_channel * c->wH * c->wW;
            --r.pos;
        }
        slot[n] = ra;
    }
    HIP_OK(hipMemcpyAsync(c->d_rows, slot, sizeof(RowArgs) * B, hipMemcpyHostToDevice, c->stream));
    c->fc_invalidate();
    StepKey key = step_key(c, 0);
    key.rows = c->d_rows;
    key.batch = B < c->wB ? B : 0;
    if (c->rows_lr) {       // (the members step_key fills for the per-call projection, from the session's own)
        key.lr = true; key.x0hat = c->x0hat;
        key.lr_ops = c->rows_lr_ops; key.lr_lds = c->rows_lr_lds;
        if (!key.lr_lds) key.lr_scratch = c->lr_scratch;
        key.rows_lr = c->rows_lr_buf;
    }
    if (launch_step(c, key)) return -1;
    if (const char *e = conv_take_error()) return fail("sr3_rows_step: %s", e);
    if (c->prof) c->pflush();           // bound the number of live events
    HIP_OK(hipGetLastError());
    c->rows.swap(next);
    c->rows_run += (uint64_t)B;
    if (c->dyn_on()) ++c->dyn_steps;
    return live;
}

uint64_t sr3_rows_rows_run(sr3_ctx *c) { return c ? c->rows_run : 0; }

int sr3_rows_move(sr3_ctx *c, int src, int dst) {
    if (rows_check(c, "sr3_rows_move", src) || rows_check(c, "sr3_rows_move", dst)) return -1;
    HIP_OK(hipSetDevice(c->device));
    if (!c->rows[src].live) return fail("sr3_rows_move: source slot %d is idle", src);
    if (c->rows[dst].live) return fail("sr3_rows_move: destination slot %d is live (%d steps left); retire or drop it first", dst, c->rows[dst].pos);
    // (src != dst follows: one slot cannot be both)
    const int C = c->cfg.out_channel;
    const TDesc xs = row_desc(c->x0, src), xd = row_desc(c->x0, dst);
    RowsMoveParams mv;
    auto seg = [&](float *from, float *to, size_t n, int zero) {
        RowsMoveSeg &g = mv.seg[mv.nseg++];
        g.src = from; g.dst = to; g.n = n; g.zero = zero;
    };
    seg(xs.p, xd.p, xs.floats(1), 1);
    if (c->x0p) seg(row_packed(c, src), row_packed(c, dst), (size_t)(c->wH + 2) * (c->wW + 2) * 8, 1);
    const size_t nh = (size_t)C * c->wH * c->wW;
    seg(c->xhist + (size_t)src * nh, c->xhist + (size_t)dst * nh, nh, 0);
    if (c->rows_lr) {       // (every slot of an armed session has its slab, held or not)
        const size_t nl = (size_t)C * c->rows_lr_ops.lh * c->rows_lr_ops.lw;
        seg(c->rows_lr_buf + (size_t)src * nl, c->rows_lr_buf + (size_t)dst * nl, nl, 0);
    }
    c->pbegin(F_MISC);
    launch_rows_move(mv, c->stream);
    c->pend();
    HIP_OK(hipGetLastError());
    c->rows[dst] = c->rows[src];
    c->rows[src] = sr3_ctx::RowState();
    return 0;
}

int64_t sr3_read_history(sr3_ctx *c, float *hist_host) {
    if (!c) return fail("null context");
    if (!c->arena || c->wB <= 0) return fail("sr3_read_history: no call has set up a workspace yet");
    if (!hist_host) return fail("sr3_read_history: hist_host is null");
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)c->wB * c->cfg.out_channel * c->wH * c->wW;
    HIP_OK(hipMemcpy(hist_host, c->xhist, n * sizeof(float), hipMemcpyDeviceToHost));
    return (int64_t)n;
}

int sr3_rows_position(sr3_ctx *c, int row) {
    if (rows_check(c, "sr3_rows_position", row)) return -2;
    return c->rows[row].live ? c->rows[row].pos : -1;
}

int sr3_rows_retire(sr3_ctx *c, int row, float *out_dev) {
    PlanScope plan_scope(c);
    if (rows_check(c, "sr3_rows_retire", row)) return -1;
    HIP_OK(hipSetDevice(c->device));
    if (!out_dev) return fail("sr3_rows_retire: out_dev is null");
    sr3_ctx::RowState &r = c->rows[row];
    if (!r.live) return fail("sr3_rows_retire: slot %d is idle", row);
    if (r.pos != 0) return fail("sr3_rows_retire: slot %d has %d steps left (sr3_rows_drop abandons a row)", row, r.pos);
    const int C = c->cfg.out_channel;
    c->pbegin(F_MISC);
    launch_nhwc_to_nchw(row_desc(c->x0, row), c->cfg.in_channel - C, 1, C, out_dev, c->stream);
    c->pend();
    HIP_OK(hipGetLastError());
    r = sr3_ctx::RowState();
    return 0;
}

int sr3_rows_drop(sr3_ctx *c, int row) {
    if (rows_check(c, "sr3_rows_drop", row)) return -1;
    HIP_OK(hipSetDevice(c->device));
    if (c->rows[row].live) {
        // a row abandoned mid-trajectory may hold anything (an unclamped prediction, an injected slab): as an idle row it
        // would go on running through the UNet and could keep raising the range flag. Back to the zeros of sr3_rows_begin
        // (one row of the state is contiguous, borders and pad channels included: they are zero already).
        const TDesc x0r = row_desc(c->x0, row);
        HIP_OK(hipMemsetAsync(x0r.p, 0, x0r.floats(1) * sizeof(float), c->stream));
        if (float *xpr = row_packed(c, row))
            HIP_OK(hipMemsetAsync(xpr, 0, (size_t)(c->wH + 2) * (c->wW + 2) * 8 * sizeof(float), c->stream));
    }
    c->rows[row] = sr3_ctx::RowState();
    return 0;
}

int sr3_rows_end(sr3_ctx *c) {
    if (!c) return fail("null context");
    if (!c->rows_on) return fail("sr3_rows_end outside a row session (sr3_rows_begin)");
    c->rows_on = false;
    c->rows_lr = false;     // (the LR buffer stays for the next session, as the table and the ring do)
    c->rows.clear();
    return 0;
}

namespace {
// sr3_sample's checkpoint (c->ckpt): the sampler state as NCHW, the x0 history of a multistep sampler (its update also
// reads the previous step's x0) and hist_valid, as they were BEFORE step t, when `frames` frames had been written.
// save / restore: 0, or -1 with the error set
struct Checkpoint {
    sr3_ctx *c;
    size_t slab;            // floats of the state (and of the history)
    int t = 0, frames = 0, k = 0;   // k: the feature cache's step counter (a multiple of its interval: the next step is whole)
    bool hist_valid = false;

    Checkpoint(sr3_ctx *ctx, size_t slab_floats) : c(ctx), slab(slab_floats) {}
    int reserve() {
        const size_t need = c->uses_hist ? 2 * slab : slab;
        if (c->ckpt_floats >= need) return 0;
        if (c->ckpt) HIP_OK(hipFree(c->ckpt));
        c->ckpt = nullptr; c->ckpt_floats = 0;
        HIP_OK(hipMalloc(&c->ckpt, need * sizeof(float)));
        c->ckpt_floats = need;
        return 0;
    }
    int save(int before_step, int frames_written) {
        const int C = c->cfg.out_channel;
        launch_nhwc_to_nchw(c->x0, c->cfg.in_channel - C, c->wB, C, c->ckpt, c->stream);
        if (c->uses_hist) {
            const hipError_t e = hipMemcpyAsync(c->ckpt + slab, c->xhist, slab * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
            if (e != hipSuccess) return fail("sr3_sample: checkpoint of the x0 history: %s", hipGetErrorString(e));
        }
        t = before_step; frames = frames_written; hist_valid = c->hist_valid; k = c->fc_k;
        return 0;
    }
    int restore() {
        const int C = c->cfg.out_channel;
        launch_init_state(c->x0, c->cfg.in_channel - C, C, c->ckpt, c->seed, c->image_offset, c->wB, c->stream);
        if (c->x0p) launch_pack_state(c->x0, c->wB, c->x0p, c->stream, c->d_ovf);
        if (c->uses_hist) {
            const hipError_t e = hipMemcpyAsync(c->xhist, c->ckpt + slab, slab * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
            if (e != hipSuccess) return fail("sr3_sample: restore of the x0 history: %s", hipGetErrorString(e));
        }
        c->hist_valid = hist_valid;
        c->fc_k = k;
        return 0;
    }
};
}

namespace {
// sr3_sample (init_dev == nullptr: from pure noise, start_step = T) and sr3_sample_from: steps t = start_step-1 .. 0
int sample_impl(sr3_ctx *c, const char *what, const float *cond_dev, int B, int H, int W, const float *init_dev,
                int start_step, int noised, const float *noise_dev, uint64_t seed, uint64_t image_offset, float *out_dev,
                float *frames_dev) {
    if (!out_dev) return fail("%s: out_dev is null", what);
    if (c && c->drop_live() && c->drop_masks)
        return fail("%s: injected dropout masks are set, and one buffer cannot hold the masks of every step — drive the "
                    "loop with sr3_sample_step (each step consumes the buffer set at that moment) or return to the Philox "
                    "masks with sr3_set_dropout_masks(ctx, NULL, 0)", what);
    if (init_dev ? sr3_sample_begin_from(c, cond_dev, B, H, W, init_dev, start_step, noised, noise_dev, seed, image_offset)
                 : sr3_sample_begin(c, cond_dev, B, H, W, noise_dev, seed, image_offset))
        return -1;
    const int T = c->T, si = 1 | (T / 10);
    const int s0 = init_dev ? start_step : T;      // steps of this call; the injected noise is [s0, B, C, H, W]
    const size_t slab = (size_t)B * c->cfg.out_channel * H * W;
    // Guard of the split-f16 modes (the policy of guarded_eval, with a segment of `seg` steps as the unit of replay): at
    // the end of every segment the device flag is read (one stream synchronisation: ~10 per call); while it is clean the
    // sampler state is saved (NCHW copy, 12 B per pixel). A WAIT that gave up replays the segment from that checkpoint in
    // the same arithmetic, whatever the policy. Out of RANGE fails the call under the strict policy; else the checkpoint
    // is restored and the REST of the loop runs one arithmetic down (step_down) — every draw of the noise (injected slab
    // or Philox draw index) and every frame slot is a function of t, so the replay is exact.
    // With the feature cache on, a segment is a whole number of its intervals: every checkpoint then stands in front of a
    // whole step, so a restore needs no copy of the cache (the replayed segment rebuilds it first, in the arithmetic it now
    // runs in), and which steps are whole stays a function of the step index alone.
    int seg = std::max(1, T / 10);
    if (c->fc_on()) seg = (seg + c->fc_interval - 1) / c->fc_interval * c->fc_interval;
    ModeScope scope(c);                  // (the mode is restored on every return)
    Checkpoint ck(c, slab);
    bool guard = c->split();             // false in exact f32, from the start or after stepping down: no more checks
    bool stepped_down = false, replayed = false;
    if (guard) {
        if (ck.reserve()) return -1;
        const int r = range_read(c);     // (the initial state / its packed copy)
        if (r < 0) return -1;
        if (r == 1 && c->strict_range) return range_fail(c, what);
        if (r == 1) { step_down(c, true); guard = false; stepped_down = true; }
        else if (ck.save(s0 - 1, 0)) return -1;
    }
    for (int t = s0 - 1, f = 0; t >= 0; --t) {
        const float *nz = (noise_dev && t > 0) ? noise_dev + (size_t)(s0 - t) * slab : nullptr;
        float *fr = (frames_dev && (t % si == 0)) ? frames_dev + (size_t)(f++) * slab : nullptr;
        if (step_checked(c, t, nz, fr)) return -1;
        if (c->prof && (t % 8) == 0) c->pflush();  // bound the number of live events
        if (!guard || (t != 0 && ((s0 - t) % seg) != 0)) continue;
        // a segment ends here: the state is the one before step t - 1 (after the last step: the result)
        const int r = range_read(c);
        if (r < 0) return -1;
        if (r == 0) {
            if (t > 0 && ck.save(t - 1, f)) return -1;
            continue;
        }
        if (r == 1 && c->strict_range) return range_fail(c, what);
        if (ck.restore()) return -1;
        if (r == 2) replayed = true;
        else { guard = step_down(c) != A_F32; stepped_down = true; }
        t = ck.t + 1; f = ck.frames;     // (the loop's --t resumes at the checkpoint; the frame index rewinds with t)
    }
    if (sample_copy_out(c, out_dev)) return -1;
    // (nothing reads the flag once the loop runs in f32, and the packed-state stores still raise it: leave it clean)
    if (stepped_down && range_reset(c)) return -1;
    if (stepped_down) return warn_fallback(c, what, "the rest of the loop from the last in-range checkpoint", c->split());
    return replayed ? warn_replay(c, what, "the segment of T/10 steps it happened in") : 0;
}
}

int sr3_sample(sr3_ctx *c, const float *cond_dev, int B, int H, int W, const float *noise_dev, uint64_t seed,
               uint64_t image_offset, float *out_dev, float *frames_dev) {
    PlanScope plan_scope(c);
    return sample_impl(c, "sr3_sample", cond_dev, B, H, W, nullptr, 0, 0, noise_dev, seed, image_offset, out_dev, frames_dev);
}

int sr3_sample_from(sr3_ctx *c, const float *cond_dev, int B, int H, int W, const float *init_dev, int start_step, int noised,
                    const float *noise_dev, uint64_t seed, uint64_t image_offset, float *out_dev, float *frames_dev) {
    PlanScope plan_scope(c);
    if (!init_dev) return fail("sr3_sample_from: init_dev is null");
    return sample_impl(c, "sr3_sample_from", cond_dev, B, H, W, init_dev, start_step, noised, noise_dev, seed, image_offset,
                       out_dev, frames_dev);
}

int sr3_set_range_policy(sr3_ctx *c, int strict) {
    if (!c) return fail("null context");
    c->strict_range = strict != 0;
    return 0;
}
int sr3_fallback_calls(sr3_ctx *c) { return c ? c->fallback_calls : fail("null context"); }
int sr3_gn_wino_passes(sr3_ctx *c) { return c ? c->gn_wino_passes : fail("null context"); }
int sr3_wino_gemm_out_launches(sr3_ctx *c) { return c ? c->wino_gemm_out_launches : fail("null context"); }
int sr3_conv_in_f32_launches(sr3_ctx *c) { return c ? c->conv_in_f32_launches : fail("null context"); }
int sr3_conv_in_f32_gate(int Cin, int Cout, int H, int W, int precision) {
    return conv_in_f32_gate(precision != 0, Cin, Cout, H, W) ? 1 : 0;
}
int sr3_step_graph_captures(sr3_ctx *c) { return c ? c->step_graph_captures : fail("null context"); }
int sr3_up2_wino_launches(sr3_ctx *c) { return c ? c->up2_wino_launches : fail("null context"); }
int sr3_dynamic_threshold_launches(sr3_ctx *c) { return c ? c->dyn_steps : fail("null context"); }
int sr3_wino_fused_rows_launches(sr3_ctx *c) { return c ? c->wino_fused_rows_launches : fail("null context"); }
int sr3_gn_res1x1_launches(sr3_ctx *c) { return c ? c->gn_res1x1_launches : fail("null context"); }
int sr3_replay_calls(sr3_ctx *c) { return c ? c->replay_calls : fail("null context"); }
void *sr3_test_flag_address(sr3_ctx *c) { return c ? c->d_ovf : nullptr; }
const char *sr3_last_warning(void) { return g_warn.c_str(); }

int sr3_philox_normal(sr3_ctx *c, uint64_t seed, uint64_t image, uint32_t draw, int n, float *out_dev) {
    if (!c || !out_dev) return fail("sr3_philox_normal: null argument");
    HIP_OK(hipSetDevice(c->device));
    launch_philox_normal(seed, image, draw, n, out_dev, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- train-mode Dropout (unet.py:81-91) ---------------------------------------------------------
int sr3_set_dropout(sr3_ctx *c, int enable, uint64_t seed, uint64_t image_offset) {
    if (!c) return fail("null context");
    const bool was_live = c->drop_live();
    if (!enable) {
        c->drop_on = false;
    } else {
        const double p = (double)c->cfg.dropout;
        if (!(p >= 0.0) || p >= 1.0) return fail("sr3_set_dropout: dropout p = %g outside [0, 1)", p);
        if (c->n_res > DROP_MAX_LAYERS)
            return fail("sr3_set_dropout: %d ResnetBlocks, the mask stream numbers at most %d layers", c->n_res, DROP_MAX_LAYERS);
        c->drop_on = true;
        c->drop_seed = seed; c->drop_offset = image_offset;
        c->drop_thr = (uint32_t)nearbyint(p * 65536.0);     // round half to even (the default rounding mode)
        c->drop_s = (float)(1.0 / (1.0 - p));
    }
    if (was_live != c->drop_live()) drop_graphs(c);         // the block2 apply passes launch other kernels
    return 0;
}

int sr3_set_dropout_masks(sr3_ctx *c, const uint8_t *dev, uint64_t bytes) {
    if (!c) return fail("null context");
    if (dev && !bytes) return fail("sr3_set_dropout_masks: empty buffer");
    c->drop_masks = dev;                    // (read from device memory by the kernels: captured steps stay valid)
    c->drop_mask_bytes = dev ? bytes : 0;
    return 0;
}

int sr3_dropout_layers(sr3_ctx *c, int H, int W, int *n, int *chw) {
    PlanScope plan_scope(c);
    if (!c || !n) return fail("sr3_dropout_layers: null argument");
    const int b = max_batch(c, H, W);
    if (b <= 0) return fail("sr3_dropout_layers: unsupported shape H=%d W=%d", H, W);
    *n = c->n_res;
    (void)dropout_layers(c, H, W, chw);
    return 0;
}

int64_t sr3_dropout_mask_bytes(sr3_ctx *c, int B, int H, int W) {
    PlanScope plan_scope(c);
    if (!c) return fail("null context");
    if (B < 1 || max_batch(c, H, W) <= 0) return fail("sr3_dropout_mask_bytes: unsupported shape B=%d H=%d W=%d", B, H, W);
    return (int64_t)((uint64_t)B * dropout_layers(c, H, W, nullptr));
}

int sr3_op_dropout_mask(sr3_ctx *c, uint64_t seed, uint64_t image, uint32_t draw, int layer, int C, int H, int W,
                        uint8_t *out_dev) {
    if (!c || !out_dev) return fail("sr3_op_dropout_mask: null argument");
    if (layer < 0 || layer >= DROP_MAX_LAYERS) return fail("sr3_op_dropout_mask: layer %d outside [0, %d)", layer, DROP_MAX_LAYERS);
    if (draw >= DROP_MAX_DRAW) return fail("sr3_op_dropout_mask: draw %u does not fit 24 bits", draw);
    if (C < 8 || (C % 8) || H < 1 || W < 1 || (uint64_t)C / 8 * H * W > 0xffffffffull)
        return fail("sr3_op_dropout_mask: bad size C=%d H=%d W=%d (C a multiple of 8)", C, H, W);
    const double p = (double)c->cfg.dropout;
    if (!(p >= 0.0) || p >= 1.0) return fail("sr3_op_dropout_mask: dropout p = %g outside [0, 1)", p);
    HIP_OK(hipSetDevice(c->device));
    launch_dropout_mask(seed, image, draw, layer, (uint32_t)nearbyint(p * 65536.0), C, H, W, out_dev, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- measurement ------------------------------------------------------------------------------
int sr3_profile_enable(sr3_ctx *c, int on) {
    if (!c) return fail("null context");
    c->pflush();
    c->prof = on != 0;
    return 0;
}
int sr3_profile_reset(sr3_ctx *c) {
    if (!c) return fail("null context");
    c->pflush();
    for (int i = 0; i < SR3_N_FAMILIES; ++i) { c->acc_ms[i] = 0; c->acc_flops[i] = 0; c->acc_n[i] = 0; }
    c->by_tag.clear();
    return 0;
}
int sr3_profile_dump_csv(sr3_ctx *c, const char *path) {
    if (!c || !path) return fail("null argument");
    c->pflush();
    FILE *f = fopen(path, "w");
    if (!f) return fail("cannot open %s", path);
    fprintf(f, "shape,launches,total_ms,avg_ms,gflop_per_launch,tflops\n");
    for (auto &kv : c->by_tag) {
        const ProfAgg &g = kv.second;
        fprintf(f, "%s,%lld,%.4f,%.4f,%.3f,%.2f\n", kv.first.c_str(), (long long)g.n, g.ms, g.ms / g.n,
                g.flops / g.n / 1e9, g.ms > 0 ? g.flops / (g.ms * 1e-3) / 1e12 : 0.0);
    }
    fclose(f);
    return 0;
}
int sr3_profile_get(sr3_ctx *c, int family, double *total_ms, int64_t *launches, double *flops) {
    if (!c) return fail("null context");
    if (family < 0 || family >= SR3_N_FAMILIES) return fail("family %d out of range", family);
    c->pflush();
    if (total_ms) *total_ms = c->acc_ms[family];
    if (launches) *launches = c->acc_n[family];
    if (flops) *flops = c->acc_flops[family];
    return 0;
}

// ---- single ops --------------------------------------------------------------------------------
// what sr3_op_conv2d_fused adds to sr3_op_conv2d_stats: the rest of the launch run_res builds for conv2
struct FusedArgs {
    const float *in2_dev = nullptr, *in2b_dev = nullptr;    // fp32 NHWC at the output pixels
    int C2a = 0, C2b = 0;
    const float *w2_host = nullptr, *b2_host = nullptr;     // [Cout][C2a + C2b], [Cout]
    int flags = 0;                                          // SR3_FUSED_*
    float *out_split_dev = nullptr;
    bool any() const { return in2_dev || flags || out_split_dev; }
};

// sr3_op_conv2d (stats_dev == null), sr3_op_conv2d_stats and sr3_op_conv2d_fused (fa): one body. With statistics the plan
// is the one the engine's convs get (fused statistics offered); a shape whose plan has none runs without them and reports
// 0 slices.
static int op_conv2d_impl(const char *what, sr3_ctx *c, const float *in0_dev, int C0, const float *in1_dev, int C1, int B, int Hin,
                          int Win, const float *weight_host, const float *bias_host, int Cout, int ks, int stride,
                          int up2, const float *gn_scale_dev, const float *gn_shift_dev, int swish,
                          const float *chan_bias_dev, const float *resid_dev, float *out_dev, double *stats_dev,
                          uint64_t stats_capacity_doubles, int *slices_out, const FusedArgs &fa = FusedArgs()) {
    if (!c || !in0_dev || !weight_host || !out_dev) return fail("%s: null argument", what);
    if ((C0 % 32) || (C1 % 32) || C0 <= 0 || C1 < 0) return fail("%s: C0=%d C1=%d must be multiples of 32", what, C0, C1);
    if (!(ks == 1 || ks == 3) || !(stride == 1 || stride == 2) || (up2 & ~1)) return fail("%s: bad ks/stride/up2", what);
    if ((gn_scale_dev == nullptr) != (gn_shift_dev == nullptr)) return fail("%s: scale and shift go together", what);
    if (up2 && (ks != 3 || stride != 1)) return fail("%s: up2 needs ks 3, stride 1", what);
    HIP_OK(hipSetDevice(c->device));
    if (!in1_dev) C1 = 0;
    const bool ident = (fa.flags & SR3_FUSED_IDENT) != 0;
    const int C2a = fa.in2_dev ? fa.C2a : 0, C2b = fa.in2b_dev ? fa.C2b : 0;
    if (fa.any()) {
        if (fa.flags & ~(SR3_FUSED_IDENT | SR3_FUSED_NO_F32 | SR3_FUSED_RESID_SPLIT)) return fail("%s: unknown flag in %d", what, fa.flags);
        if ((fa.flags || fa.out_split_dev) && !c->split())
            return fail("%s: the identity K-steps, the split twin, the twin-only output and a split residual exist in the "
                        "split-f16 arithmetics only (sr3_set_precision 1 | 2)", what);
        if ((fa.out_split_dev || (fa.flags & SR3_FUSED_RESID_SPLIT)) && (Cout % 32)) return fail("%s: the split format needs Cout %% 32 == 0 (Cout=%d)", what, Cout);
        if ((fa.flags & SR3_FUSED_NO_F32) && !fa.out_split_dev) return fail("%s: no fp32 output and no twin: nothing to write", what);
        if ((fa.flags & SR3_FUSED_RESID_SPLIT) && !resid_dev) return fail("%s: a split residual was announced, there is none", what);
        if (fa.in2b_dev && !fa.in2_dev) return fail("%s: in2b without in2", what);
        // the engine's fused_ok (run_res): the 1x1 K-steps read their operands in 32-channel chunks
        if (fa.in2_dev && ((C2a % 32) || (C2b % 32) || C2a <= 0 || C2b < 0))
            return fail("%s: C2a=%d C2b=%d must be multiples of 32", what, C2a, C2b);
        if (ident) {
            // ident_eligible + run_res: a narrow block that keeps its width, its input as the split operand
            if (fa.w2_host || fa.in2b_dev || !fa.in2_dev) return fail("%s: the identity K-steps take in2 alone, and no 1x1 weights", what);
            if (Cout > 128 || (Cout % 32) || C2a != Cout) return fail("%s: the identity K-steps need Cout <= 128, Cout %% 32 == 0 and C2a == Cout (Cout=%d C2a=%d)", what, Cout, C2a);
        } else if ((fa.in2_dev != nullptr) != (fa.w2_host != nullptr)) {
            return fail("%s: in2 and w2 go together", what);
        }
    }
    FusedTerm ft;
    ft.w2_host = fa.w2_host; ft.C2 = C2a + C2b; ft.ident = ident;
    ScratchConv sc;
    if (sc.setup(c, B, Hin, Win, C0, C1, Cout, ks, stride, up2, weight_host, stats_dev != nullptr, fa.in2_dev ? &ft : nullptr)) return -1;
    DevBuf bias, in2s, in2bs;
    std::vector<float> bsum;
    if (fa.b2_host && fa.in2_dev && !ident) {       // prepare_fused: the two biases are pre-added
        bsum.assign(fa.b2_host, fa.b2_host + Cout);
        if (bias_host) for (int i = 0; i < Cout; ++i) bsum[i] = bias_host[i] + fa.b2_host[i];
        bias_host = bsum.data();
    }
    if (bias_host && bias.upload(bias_host, (size_t)Cout)) return -1;
    ConvParams &p = sc.p;
    p.bias = bias.p; p.chan_bias = chan_bias_dev; p.chan_bias_stride = Cout;
    p.out = unpadded(out_dev, Cout, p.Hout, p.Wout);
    if (resid_dev) p.resid = unpadded(const_cast<float *>(resid_dev), Cout, p.Hout, p.Wout);
    p.resid_split = (fa.flags & SR3_FUSED_RESID_SPLIT) ? 1 : 0;
    if (fa.out_split_dev) p.out_split = unpadded(fa.out_split_dev, Cout, p.Hout, p.Wout);
    p.out_f32 = (fa.flags & SR3_FUSED_NO_F32) ? 0 : 1;
    // the 1x1 operands at the output pixels: the fp32 tensors themselves in f32, copies in the plain split format (what a
    // twin or run_res's raw1 holds, also under F8C) in the split-f16 arithmetics
    const TDesc i2 = fa.in2_dev ? unpadded(const_cast<float *>(fa.in2_dev), C2a, p.Hout, p.Wout) : TDesc();
    const TDesc i2b = C2b ? unpadded(const_cast<float *>(fa.in2b_dev), C2b, p.Hout, p.Wout) : TDesc();
    p.in2 = i2; p.in2b = i2b;
    if (c->split()) {
        if (i2.p && in2s.alloc(i2.floats(B))) return -1;
        if (i2b.p && in2bs.alloc(i2b.floats(B))) return -1;
        p.in2.p = in2s.p; p.in2b.p = in2bs.p;
    }
    if (stats_dev && sc.plan.stats_slices > 0) {
        const uint64_t need = (uint64_t)B * sc.plan.stats_slices * Cout * 2;
        if (stats_capacity_doubles < need)
            return fail("%s: the statistics take %llu doubles ([B][%d slices][Cout][2]), the buffer holds %llu", what,
                        (unsigned long long)need, sc.plan.stats_slices, (unsigned long long)stats_capacity_doubles);
        p.stats = stats_dev; p.stats_slices = sc.plan.stats_slices;
    }
    if (slices_out) *slices_out = p.stats_slices;
    // the engine's own sequence: (GroupNorm apply | copy) + concat into a zero-bordered tensor, then conv; in front of a
    // three-pass Winograd conv the pass writes the transformed input instead (nothing reads p.in0 then)
    const bool to_u = sc.gn_writes_u(c);
    if (!to_u) HIP_OK(hipMemsetAsync(p.in0.p, 0, p.in0.floats(B) * sizeof(float), c->stream));
    const TDesc i0 = unpadded(const_cast<float *>(in0_dev), C0, Hin, Win);
    const TDesc i1 = in1_dev ? unpadded(const_cast<float *>(in1_dev), C1, Hin, Win) : kNone;
    // (this entry point owns its inputs: an in-place split-K wait that gave up is answered by running the pass and the
    // conv again on the non-waiting path, as sr3_unet_forward / sr3_sample do; it never leaves the arithmetic it was asked for)
    return guarded_eval(c, what, "the conv", false, [&]() -> int {
        const int mode = gn_scale_dev ? (swish ? 2 : 1) : 0;
        // (0xFF bytes read back as NaN: a slice no kernel wrote stays visible)
        if (stats_dev) HIP_OK(hipMemsetAsync(stats_dev, 0xFF, stats_capacity_doubles * sizeof(double), c->stream));
        if (to_u) {
            launch_gn_wino_input(i0, i1, B, gn_scale_dev, gn_shift_dev, mode, p.wino_ws, c->stream);
            ++c->gn_wino_passes;
        } else {
            launch_gn_apply(i0, i1, B, gn_scale_dev, gn_shift_dev, mode, c->act_format(sc.f8), p.in0, c->stream, TDesc(), 0, c->d_ovf);
        }
        if (c->split() && i2.p) launch_gn_apply(i2, kNone, B, nullptr, nullptr, 0, 1, p.in2, c->stream, TDesc(), 0, c->d_ovf);
        if (c->split() && i2b.p) launch_gn_apply(i2b, kNone, B, nullptr, nullptr, 0, 1, p.in2b, c->stream, TDesc(), 0, c->d_ovf);
        p.u_ready = to_u ? 1 : 0;
        p.no_halo_split = c->halo_split_off ? 1 : 0;
        if (fa.any() && !p.no_halo_split) {
            // the fused term, the twin and the residual's format change no plan: the launch is the 3x3 shape's
            const ConvPlan run = conv_plan(p);
            if (run.kernel != sc.plan.kernel || run.split != sc.plan.split || run.splits != sc.plan.splits ||
                run.wino_gemm_out != sc.plan.wino_gemm_out || run.wino_fused_rows != sc.plan.wino_fused_rows)
                return fail("%s: internal: the fused launch takes %s, the plan of the 3x3 shape names %s", what,
                            conv_kernel_name(run.kernel), conv_kernel_name(sc.plan.kernel));
        }
        ctx_launch_conv(c, p);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) return fail("%s: launch failed", what);
        if (const char *e = conv_take_error()) return fail("%s: %s", what, e);
        return 0;
    });
}

int sr3_op_conv2d(sr3_ctx *c, const float *in0_dev, int C0, const float *in1_dev, int C1, int B, int Hin,
                  int Win, const float *weight_host, const float *bias_host, int Cout, int ks, int stride,
                  int up2, const float *gn_scale_dev, const float *gn_shift_dev, int swish,
                  const float *chan_bias_dev, const float *resid_dev, float *out_dev) {
    PlanScope plan_scope(c);
    return op_conv2d_impl("sr3_op_conv2d", c, in0_dev, C0, in1_dev, C1, B, Hin, Win, weight_host, bias_host, Cout, ks, stride, up2,
                          gn_scale_dev, gn_shift_dev, swish, chan_bias_dev, resid_dev, out_dev, nullptr, 0, nullptr);
}

int sr3_op_conv2d_stats(sr3_ctx *c, const float *in0_dev, int C0, const float *in1_dev, int C1, int B, int Hin,
                        int Win, const float *weight_host, const float *bias_host, int Cout, int ks, int stride,
                        int up2, const float *gn_scale_dev, const float *gn_shift_dev, int swish,
                        const float *chan_bias_dev, const float *resid_dev, float *out_dev, double *stats_dev,
                        uint64_t stats_capacity_doubles, int *slices_out) {
    PlanScope plan_scope(c);
    if (!stats_dev || !slices_out) return fail("sr3_op_conv2d_stats: null argument");
    return op_conv2d_impl("sr3_op_conv2d_stats", c, in0_dev, C0, in1_dev, C1, B, Hin, Win, weight_host, bias_host, Cout, ks, stride,
                          up2, gn_scale_dev, gn_shift_dev, swish, chan_bias_dev, resid_dev, out_dev, stats_dev,
                          stats_capacity_doubles, slices_out);
}

int sr3_op_conv2d_fused(sr3_ctx *c, const float *in0_dev, int C0, const float *in1_dev, int C1, int B, int Hin, int Win,
                        const float *weight_host, const float *bias_host, int Cout, const float *gn_scale_dev,
                        const float *gn_shift_dev, int swish, const float *chan_bias_dev, const float *resid_dev,
                        const float *in2_dev, int C2a, const float *in2b_dev, int C2b, const float *w2_host,
                        const float *b2_host, int flags, float *out_dev, float *out_split_dev, double *stats_dev,
                        uint64_t stats_capacity_doubles, int *slices_out) {
    PlanScope plan_scope(c);
    if (!stats_dev || !slices_out) return fail("sr3_op_conv2d_fused: null argument");
    FusedArgs fa;
    fa.in2_dev = in2_dev; fa.C2a = C2a; fa.in2b_dev = in2b_dev; fa.C2b = C2b;
    fa.w2_host = w2_host; fa.b2_host = b2_host; fa.flags = flags; fa.out_split_dev = out_split_dev;
    return op_conv2d_impl("sr3_op_conv2d_fused", c, in0_dev, C0, in1_dev, C1, B, Hin, Win, weight_host, bias_host, Cout, 3, 1, 0,
                          gn_scale_dev, gn_shift_dev, swish, chan_bias_dev, resid_dev, out_dev, stats_dev, stats_capacity_doubles,
                          slices_out, fa);
}

// ---- the edge convs (kernels_edge.hip) on scratch buffers: the forward's launchers, weight packers and gates ----
int sr3_op_conv_in(sr3_ctx *c, const float *state_nchw_dev, int B, int H, int W, int Cin, const float *weight_host,
                   const float *bias_host, int Cout, float *out_dev, float *twin_dev, double *stats_dev,
                   uint64_t stats_capacity_doubles, int *slices_out, void *packed_host) {
    PlanScope plan_scope(c);
    const char *what = "sr3_op_conv_in";
    if (!c || !state_nchw_dev || !weight_host) return fail("%s: null argument", what);
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return fail("%s: bad shape", what);
    // run_unet_body's gate (M_CONV_IN): c->split() && c->x0p, the latter decided by conv_in_supported
    if (!c->split())
        return fail("%s: the packed-state conv runs in the split-f16 arithmetics only (sr3_set_precision 1 | 2)", what);
    if (!conv_in_supported(Cin, Cout, H, W))
        return fail("%s: Cin=%d Cout=%d H=%d W=%d is no shape of the packed-state conv (Cin <= 8, Cout 32 | 64, W %% 16 == 0, "
                    "H*W %% 256 == 0)", what, Cin, Cout, H, W);
    const int slices = H * W / 256;
    if (stats_dev) {
        const uint64_t need = (uint64_t)B * slices * Cout * 2;
        if (stats_capacity_doubles < need)
            return fail("%s: the statistics take %llu doubles ([B][%d slices][Cout][2]), the buffer holds %llu", what,
                        (unsigned long long)need, slices, (unsigned long long)stats_capacity_doubles);
    }
    if (slices_out) *slices_out = slices;
    HIP_OK(hipSetDevice(c->device));
    // the workspace's x0 / x0p (ensure_workspace): zero-bordered fp32 state of in_pad channels, packed twin + 16 floats of slack
    TDesc x0; x0.C = round_up(Cin, 32); x0.H = H; x0.W = W; x0.pad = 1;
    const size_t npix = (size_t)B * (H + 2) * (W + 2), xp_floats = npix * 8 + 16;
    DevBuf state, xp, wci, bias;
    if (state.alloc(x0.floats(B)) || xp.alloc(xp_floats)) return -1;
    x0.p = state.p;
    std::vector<float> wf(conv_in_weight_floats(Cout));
    const float unscale = pack_conv_in_weight(weight_host, Cout, Cin, wf.data());
    if (wci.upload(wf.data(), wf.size())) return -1;
    if (bias_host && bias.upload(bias_host, (size_t)Cout)) return -1;
    const TDesc out = unpadded(out_dev, Cout, H, W);
    const TDesc twin = twin_dev ? unpadded(twin_dev, Cout, H, W) : TDesc();
    const int rc = guarded_eval(c, what, "the conv", false, [&]() -> int {
        HIP_OK(hipMemsetAsync(state.p, 0, x0.floats(B) * sizeof(float), c->stream));
        HIP_OK(hipMemsetAsync(xp.p, 0, xp_floats * sizeof(float), c->stream));
        if (stats_dev) HIP_OK(hipMemsetAsync(stats_dev, 0xFF, stats_capacity_doubles * sizeof(double), c->stream));
        launch_nchw_to_nhwc(state_nchw_dev, B, Cin, x0, 0, c->stream);
        launch_pack_state(x0, B, xp.p, c->stream, c->d_ovf);
        launch_conv_in(xp.p, wci.p, bias.p, unscale, B, out, twin, out_dev ? 1 : 0, stats_dev, slices, c->d_ovf, c->stream);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) return fail("%s: launch failed", what);
        return 0;
    });
    if (rc < 0) return rc;
    if (packed_host) HIP_OK(hipMemcpy(packed_host, xp.p, npix * 16 * sizeof(_Float16), hipMemcpyDeviceToHost));
    return rc;
}

int sr3_op_conv_in_f32(sr3_ctx *c, const float *state_nchw_dev, int B, int H, int W, int Cin, const float *weight_host,
                       const float *bias_host, int Cout, float *out_dev, double *stats_dev, uint64_t stats_capacity_doubles,
                       int *slices_out) {
    PlanScope plan_scope(c);
    const char *what = "sr3_op_conv_in_f32";
    if (!c || !state_nchw_dev || !weight_host || !out_dev) return fail("%s: null argument", what);
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return fail("%s: bad shape", what);
    // run_unet_body's gate (M_CONV_IN): conv_in_f32_gate, its three terms named one by one
    if (c->split())
        return fail("%s: the f32 first-conv kernel runs in the exact-f32 arithmetic only (sr3_set_precision 0)", what);
    if (!conv_in_supported(Cin, Cout, H, W))
        return fail("%s: Cin=%d Cout=%d H=%d W=%d is no shape of the f32 first-conv kernel (Cin <= 8, Cout 32 | 64, W %% 16 == 0, "
                    "H*W %% 256 == 0)", what, Cin, Cout, H, W);
    if (!conv_in_f32_gate(false, Cin, Cout, H, W)) return fail("%s: switched off (SR3_NO_CONV_IN_F32=1)", what);
    if ((uint64_t)B * H * W >= (1ull << 31)) return fail("%s: B*H*W must stay under 2^31 pixels", what);
    const int slices = H * W / 256;
    if (stats_dev) {
        const uint64_t need = (uint64_t)B * slices * Cout * 2;
        if (stats_capacity_doubles < need)
            return fail("%s: the statistics take %llu doubles ([B][%d slices][Cout][2]), the buffer holds %llu", what,
                        (unsigned long long)need, slices, (unsigned long long)stats_capacity_doubles);
    }
    if (slices_out) *slices_out = slices;
    HIP_OK(hipSetDevice(c->device));
    // the workspace's x0 (ensure_workspace): zero-bordered fp32 state of in_pad channels; the weights as alloc_weights
    // keeps them ([tap][Cout][cin_pad], pack_conv_weight)
    const int cin_pad = round_up(Cin, 32);
    TDesc x0; x0.C = cin_pad; x0.H = H; x0.W = W; x0.pad = 1;
    DevBuf state, wdev, bias;
    if (state.alloc(x0.floats(B))) return -1;
    x0.p = state.p;
    std::vector<float> wf((size_t)9 * Cout * cin_pad);
    pack_conv_weight(weight_host, Cout, Cin, 3, cin_pad, wf.data());
    if (wdev.upload(wf.data(), wf.size())) return -1;
    if (bias_host && bias.upload(bias_host, (size_t)Cout)) return -1;
    const TDesc out = unpadded(out_dev, Cout, H, W);
    return guarded_eval(c, what, "the conv", false, [&]() -> int {
        HIP_OK(hipMemsetAsync(state.p, 0, x0.floats(B) * sizeof(float), c->stream));
        if (stats_dev) HIP_OK(hipMemsetAsync(stats_dev, 0xFF, stats_capacity_doubles * sizeof(double), c->stream));
        launch_nchw_to_nhwc(state_nchw_dev, B, Cin, x0, 0, c->stream);
        launch_conv_in_f32(x0, wdev.p, cin_pad, bias.p, B, out, stats_dev, slices, c->stream);
        ++c->conv_in_f32_launches;
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) return fail("%s: launch failed", what);
        return 0;
    });
}

int sr3_op_final_conv(sr3_ctx *c, const float *in_dev, int B, int H, int W, int C, const float *gn_scale_dev,
                      const float *gn_shift_dev, const float *weight_host, const float *bias_host, int Cout,
                      float *out_dev, int *form_out) {
    PlanScope plan_scope(c);
    const char *what = "sr3_op_final_conv";
    if (!c || !in_dev || !gn_scale_dev || !gn_shift_dev || !weight_host || !bias_host || !out_dev) return fail("%s: null argument", what);
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Cout <= 0) return fail("%s: bad shape", what);
    // run_unet_body's gates: the fused final conv is entered where the VALU weights exist (alloc_weights:
    // final_conv_supported); in the split-f16 arithmetics it takes the MFMA form where those weights exist too
    if (!final_conv_supported(C, Cout))
        return fail("%s: C=%d Cout=%d is no shape of the fused final conv (C %% 64 == 0, Cout 1..4)", what, C, Cout);
    const bool mfma = c->split() && final_conv_mfma_supported(C, Cout);
    if (form_out) *form_out = mfma ? 2 : 1;
    HIP_OK(hipSetDevice(c->device));
    TDesc cur; cur.C = C; cur.H = H; cur.W = W; cur.pad = 1;      // a module output: zero-bordered (the kernels read the border, masked)
    DevBuf act, w, bias;
    if (act.alloc(cur.floats(B)) || bias.upload(bias_host, (size_t)Cout)) return -1;
    cur.p = act.p;
    float unscale = 1.f;
    if (mfma) {
        std::vector<float> wf(final_conv_mfma_weight_floats(C));
        unscale = pack_final_conv_mfma_weight(weight_host, C, wf.data());
        if (w.upload(wf.data(), wf.size())) return -1;
    } else {
        std::vector<float> wq((size_t)9 * C * 4);
        pack_final_conv_weight(weight_host, Cout, C, wq.data());
        if (w.upload(wq.data(), wq.size())) return -1;
    }
    const TDesc out = unpadded(out_dev, Cout, H, W);
    return guarded_eval(c, what, "the conv", false, [&]() -> int {
        HIP_OK(hipMemsetAsync(act.p, 0, cur.floats(B) * sizeof(float), c->stream));
        launch_gn_apply(unpadded(const_cast<float *>(in_dev), C, H, W), kNone, B, nullptr, nullptr, 0, 0, cur, c->stream);
        if (mfma) launch_final_conv_mfma(cur, B, gn_scale_dev, gn_shift_dev, w.p, unscale, bias.p, out, c->stream, c->d_ovf);
        else launch_final_conv(cur, B, gn_scale_dev, gn_shift_dev, w.p, bias.p, out, c->stream);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) return fail("%s: launch failed", what);
        return 0;
    });
}

int64_t sr3_read_packed_state(sr3_ctx *c, float *state_host, void *packed_host, int *dims3) {
    if (!c) return fail("null context");
    if (!c->arena || c->wB <= 0) return fail("sr3_read_packed_state: no call has set up a workspace yet");
    if (dims3) { dims3[0] = c->wB; dims3[1] = c->wH; dims3[2] = c->wW; }
    if (!c->x0p) return 0;
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->stream));
    const size_t npix = (size_t)c->wB * (c->wH + 2) * (c->wW + 2);
    if (state_host)
        HIP_OK(hipMemcpy2D(state_host, 8 * sizeof(float), c->x0.p, (size_t)c->x0.C * sizeof(float), 8 * sizeof(float), npix,
                           hipMemcpyDeviceToHost));
    if (packed_host) HIP_OK(hipMemcpy(packed_host, c->x0p, npix * 16 * sizeof(_Float16), hipMemcpyDeviceToHost));
    return (int64_t)npix;
}

// Times `iters` launches of one conv shape on scratch buffers (random contents; f32 MFMA time does
// not depend on the data). `mode` > 0 additionally times the GroupNorm apply pass that precedes the
// conv in the engine (1 affine, 2 affine + Swish) and reports it in *apply_ms.
int sr3_bench_conv(sr3_ctx *c, int B, int Hin, int Win, int C0, int C1, int Cout, int ks, int stride, int up2,
                   int mode, int with_resid, int with_chan_bias, int iters, float *avg_ms, float *apply_ms) {
    PlanScope plan_scope(c);
    if (!c || !avg_ms) return fail("null argument");
    if ((C0 % 32) || (C1 % 32) || C0 <= 0) return fail("sr3_bench_conv: channels must be multiples of 32");
    HIP_OK(hipSetDevice(c->device));
    ScratchConv sc;
    if (sc.setup(c, B, Hin, Win, C0, C1, Cout, ks, stride, up2, nullptr)) return -1;
    ConvParams &p = sc.p;
    const int Cin = C0 + C1;
    TDesc i0, i1, out, res;
    i0.C = C0; i1.C = C1; out.C = res.C = Cout;
    i0.H = i1.H = Hin; i0.W = i1.W = Win; out.H = res.H = p.Hout; out.W = res.W = p.Wout;
    i0.pad = i1.pad = out.pad = res.pad = 1;
    DevBuf d_i0, d_i1, d_out, d_res, bias, scale, shift, cb;
    if (d_i0.alloc(i0.floats(B)) || (C1 && d_i1.alloc(i1.floats(B))) || d_out.alloc(out.floats(B)) || d_res.alloc(res.floats(B)) ||
        bias.alloc((size_t)Cout) || scale.alloc((size_t)B * Cin) || shift.alloc((size_t)B * Cin) || cb.alloc((size_t)B * Cout))
        return -1;
    i0.p = d_i0.p; i1.p = d_i1.p; out.p = d_out.p; res.p = d_res.p;
    fill_random(c, i0.p, i0.floats(B), 1);
    if (C1) fill_random(c, i1.p, i1.floats(B), 2);
    fill_random(c, p.in0.p, p.in0.floats(B), 9); fill_random(c, bias.p, Cout, 4); fill_random(c, res.p, res.floats(B), 5);
    fill_random(c, scale.p, (size_t)B * Cin, 6); fill_random(c, shift.p, (size_t)B * Cin, 7); fill_random(c, cb.p, (size_t)B * Cout, 8);
    p.bias = bias.p;
    p.chan_bias = with_chan_bias ? cb.p : nullptr; p.chan_bias_stride = Cout;
    if (with_resid) p.resid = res;
    p.out = out;
    // as the engine runs the shape: behind the fused pass the conv starts from U (random contents like every input here)
    const bool to_u = sc.gn_writes_u(c);
    if (to_u) { fill_random(c, p.wino_ws, (size_t)16 * B * (Hin / 2) * (Win / 2) * Cin, 11); p.u_ready = 1; }
    auto conv = [&] { ctx_launch_conv(c, p); };              // (the counters tell a tool which form it timed)
    auto apply = [&] {
        if (to_u) launch_gn_wino_input(i0, C1 ? i1 : kNone, B, scale.p, shift.p, mode, p.wino_ws, c->stream);
        else launch_gn_apply(i0, C1 ? i1 : kNone, B, scale.p, shift.p, mode, c->act_format(sc.f8), p.in0, c->stream);
    };
    float ms_apply = 0.f;
    for (int i = 0; i < 2; ++i) conv();
    if (time_two_phases(c, iters, conv, apply, avg_ms, &ms_apply)) return -1;
    if (apply_ms) *apply_ms = ms_apply;
    HIP_OK(hipGetLastError());
    return 0;
}

// Per-shape timing of block1's pass + the res_conv (tools/conv_bench.py --set gnres): pair_ms = what the engine launches
// without gn_res1x1_kernel — the apply pass on the route gn_route names (with its finalize launch where that route has
// one) and the 1x1 side launch of conv2's Winograd plan; one_ms = finalize launch + gn_res1x1_kernel. Random inputs, the
// statistics as two conv epilogues would have left them (x and skip separately), `iters` back-to-back repetitions each.
int sr3_bench_gn_res1x1(sr3_ctx *c, int B, int H, int W, int C0, int C1, int Cout, int groups, int iters, float *pair_ms, float *one_ms,
                        int *route_out) {
    PlanScope plan_scope(c);
    const char *what = "sr3_bench_gn_res1x1";
    if (!c || !pair_ms || !one_ms || iters < 1) return fail("%s: bad argument", what);
    const int C = C0 + C1;
    if (B < 1 || groups <= 0 || C % groups || !gn_res1x1_gate_op(c->split() ? 1 : 0, B, H, W, C0, C1, Cout).valid)
        return fail("%s: shape refused by the gate", what);
    HIP_OK(hipSetDevice(c->device));
    TDesc x, sk, act, out;
    x.C = C0; sk.C = C1; act.C = C; out.C = Cout;
    for (TDesc *d : {&x, &sk, &act, &out}) { d->H = H; d->W = W; d->pad = 1; }
    DevBuf bx, bsk, bact, bout, dg, db, scale, shift, p0, p1, w2;
    if (bx.alloc(x.floats(B)) || (C1 && bsk.alloc(sk.floats(B))) || bact.alloc(act.floats(B)) || bout.alloc(out.floats(B)) ||
        dg.alloc((size_t)C) || db.alloc((size_t)C) || scale.alloc((size_t)B * C) || shift.alloc((size_t)B * C) ||
        p0.alloc(gn_workspace_floats(B, C)) || p1.alloc(gn_workspace_floats(B, C)) || w2.alloc((size_t)Cout * C))
        return -1;
    x.p = bx.p; sk.p = bsk.p; act.p = bact.p; out.p = bout.p;
    HIP_OK(hipMemsetAsync(act.p, 0, act.floats(B) * sizeof(float), c->stream));
    HIP_OK(hipMemsetAsync(out.p, 0, out.floats(B) * sizeof(float), c->stream));
    fill_random(c, x.p, x.floats(B), 21);
    if (C1) fill_random(c, sk.p, sk.floats(B), 22);
    fill_random(c, dg.p, (size_t)C, 23); fill_random(c, db.p, (size_t)C, 24); fill_random(c, w2.p, (size_t)Cout * C, 25);
    const TDesc b = C1 ? sk : kNone;
    const StatsRef sa = launch_groupnorm_partials(x, kNone, B, p0.p, c->stream);
    const StatsRef sb = C1 ? launch_groupnorm_partials(sk, kNone, B, p1.p, c->stream) : StatsRef();
    const GnRoute route = gn_route(x, b, B, sa, sb);
    if (route_out) *route_out = (int)route;
    GnScratch ws;
    ws.scale = scale.p; ws.shift = shift.p;
    GnRes1x1 res;
    res.w2 = w2.p; res.out = out;
    ConvParams r;                       // the side launch, as launch_conv_wino builds it
    r.in0 = x; r.in1 = b;
    r.B = B; r.Hout = H; r.Wout = W;
    r.ks = 1; r.prec = 0;
    r.w = w2.p;
    r.out = out;
    auto pair = [&] {
        launch_gn_act(route, x, b, B, groups, dg.p, db.p, 2, 0, act, sa, sb, ws, TDesc(), 0, nullptr, nullptr, DropLayer(), c->stream);
        launch_conv(r, c->stream);
    };
    auto one = [&] {
        launch_gn_act(route, x, b, B, groups, dg.p, db.p, 2, 0, act, sa, sb, ws, TDesc(), 0, nullptr, nullptr, DropLayer(), c->stream, &res);
    };
    for (int i = 0; i < 2; ++i) { pair(); one(); }
    if (time_two_phases(c, iters, pair, one, pair_ms, one_ms)) return -1;
    if (const char *e = conv_take_error()) return fail("%s: %s", what, e);
    HIP_OK(hipGetLastError());
    return 0;
}

int sr3_op_groupnorm_affine(sr3_ctx *c, const float *in0_dev, int C0, const float *in1_dev, int C1, int B,
                            int H, int W, int groups, const float *gamma_host, const float *beta_host,
                            float *scale_dev, float *shift_dev) {
    PlanScope plan_scope(c);
    if (!c || !in0_dev || !gamma_host || !beta_host || !scale_dev || !shift_dev) return fail("sr3_op_groupnorm_affine: null argument");
    if (!in1_dev) C1 = 0;
    const int C = C0 + C1;
    if (groups <= 0 || C % groups) return fail("groups=%d does not divide C=%d", groups, C);
    HIP_OK(hipSetDevice(c->device));
    DevBuf dg, db, part;
    if (dg.upload(gamma_host, (size_t)C) || db.upload(beta_host, (size_t)C) || part.alloc(gn_workspace_floats(B, C))) return -1;
    launch_groupnorm_affine(unpadded(const_cast<float *>(in0_dev), C0, H, W),
                            in1_dev ? unpadded(const_cast<float *>(in1_dev), C1, H, W) : kNone, B, groups, dg.p, db.p,
                            1e-5f, part.p, scale_dev, shift_dev, c->stream);
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipGetLastError());
    return 0;
}

int sr3_op_groupnorm_apply(sr3_ctx *c, const float *in0_dev, int C0, const float *in1_dev, int C1, int B, int H, int W,
                           int groups, const float *gamma_host, const float *beta_host, const double *stats0_dev, int slices0,
                           const double *stats1_dev, int slices1, int mode, int format, int in_split, int route,
                           float *out_dev, float *raw_out_dev, int *route_out, int *range_out) {
    PlanScope plan_scope(c);
    if (!c || !in0_dev || !gamma_host || !beta_host || !out_dev) return fail("sr3_op_groupnorm_apply: null argument");
    if (!in1_dev) C1 = 0;
    const int C = C0 + C1;
    if (B < 1 || H < 1 || W < 1 || C0 <= 0 || (C0 % 8) || (C1 % 8) || C > 2048)
        return fail("sr3_op_groupnorm_apply: bad size B=%d H=%d W=%d C0=%d C1=%d (channels in multiples of 8, at most 2048)", B, H, W, C0, C1);
    if (groups <= 0 || C % groups) return fail("sr3_op_groupnorm_apply: groups=%d does not divide C=%d", groups, C);
    if (mode < 0 || mode > 2 || format < 0 || format > 2 || (in_split & ~3) || route < 0 || route > 2)
        return fail("sr3_op_groupnorm_apply: mode %d / format %d / in_split %d / route %d out of range", mode, format, in_split, route);
    if ((in_split & 2) && !in1_dev) return fail("sr3_op_groupnorm_apply: in_split names a second input, there is none");
    // the split formats are laid out in 32-channel chunks: of the output, and of each input stored that way
    if ((format && ((C0 % 32) || (C1 % 32))) || ((in_split & 1) && (C0 % 32)) || ((in_split & 2) && (C1 % 32)))
        return fail("sr3_op_groupnorm_apply: the split formats need channels in multiples of 32 (C0=%d C1=%d)", C0, C1);
    if (stats0_dev ? (slices0 < 1 || (in1_dev && (!stats1_dev || slices1 < 1))) : stats1_dev != nullptr)
        return fail("sr3_op_groupnorm_apply: partials of both inputs (at least one slice each) or of neither");
    // (without partials the statistics kernel reads the inputs as fp32)
    if (!stats0_dev && in_split) return fail("sr3_op_groupnorm_apply: split-f16 inputs need their partials");
    HIP_OK(hipSetDevice(c->device));
    DevBuf dg, db, scale, shift, part;
    if (dg.upload(gamma_host, (size_t)C) || db.upload(beta_host, (size_t)C) || scale.alloc((size_t)B * C) || shift.alloc((size_t)B * C) ||
        part.alloc(gn_workspace_floats(B, C)))
        return -1;
    const TDesc a = unpadded(const_cast<float *>(in0_dev), C0, H, W);
    const TDesc b = in1_dev ? unpadded(const_cast<float *>(in1_dev), C1, H, W) : kNone;
    const TDesc act = unpadded(out_dev, C, H, W);
    const TDesc raw = raw_out_dev ? unpadded(raw_out_dev, C, H, W) : TDesc();
    StatsRef sa, sb;
    sa.p = stats0_dev; sa.slices = stats0_dev ? slices0 : 0;
    if (in1_dev) { sb.p = stats1_dev; sb.slices = stats1_dev ? slices1 : 0; }
    const GnRoute r = route == 0 ? gn_route(a, b, B, sa, sb) : (GnRoute)route;
    if (r == GN_FINALIZE_ROWS && (long)B * H / ((H % 2) ? 1 : 2) > 65535)
        return fail("sr3_op_groupnorm_apply: B=%d x H=%d rows exceed the streaming form's grid", B, H);
    GnScratch ws;
    ws.scale = scale.p; ws.shift = shift.p; ws.part = part.p;
    if (range_reset(c)) return -1;
    launch_gn_act(r, a, b, B, groups, dg.p, db.p, mode, format, act, sa, sb, ws, raw, in_split, nullptr, c->d_ovf, DropLayer(), c->stream);
    const int flag = range_read(c);         // (synchronises; clears the flag)
    if (flag < 0) return -1;
    HIP_OK(hipGetLastError());
    if (route_out) *route_out = (int)r;
    if (range_out) *range_out = flag ? 1 : 0;
    return 0;
}

int sr3_gn_res1x1_gate(int B, int H, int W, int C0, int C1, int Cout, int precision, int flags, int mode) {
    if (B <= 0 || H <= 0 || W <= 0 || C0 <= 0 || C1 < 0 || Cout <= 0 || precision < 0 || precision > 2 || (flags & ~15))
        return fail("sr3_gn_res1x1_gate: bad argument");
    const bool has_res = flags & 1, direct = flags & 2, raw_wanted = flags & 4, in_split = flags & 8;
    ConvPlan pl1, pl2;
    bool reads_u = false;
    if (((C0 + C1) % 32) == 0 && (Cout % 32) == 0) {
        // the engine's convs: fused statistics offered, every buffer offered
        pl1 = conv_plan_offered(B, H, W, C0 + C1, Cout, 3, 1, 0, precision ? 1 : 0, false, true);
        pl2 = conv_plan_offered(B, H, W, Cout, Cout, 3, 1, 0, precision ? 1 : 0, false, true);
        reads_u = gn_pass_writes_u(precision != 0, pl1, raw_wanted, in_split ? 1 : 0);
    }
    const GnResGate g = gn_res1x1_gate(precision ? 1 : 0, has_res, direct, raw_wanted, in_split ? 1 : 0, mode, reads_u, pl1.wino_fused_rows,
                                       pl2, B, H, W, C0, C1, Cout);
    return (g.valid ? 1 : 0) | (g.tuned ? 2 : 0) | (g.takes() ? 4 : 0);
}

int sr3_op_gn_res1x1(sr3_ctx *c, const float *x_dev, int C0, const float *skip_dev, int C1, int B, int H, int W, int groups,
                     const float *gamma_host, const float *beta_host, const float *w2_host, int Cout, float sentinel,
                     float *act_dev, float *res_dev, float *res_pair_dev) {
    PlanScope plan_scope(c);
    const char *what = "sr3_op_gn_res1x1";
    if (!c || !x_dev || !gamma_host || !beta_host || !w2_host || !act_dev || !res_dev) return fail("%s: null argument", what);
    if (!skip_dev) C1 = 0;
    const int C = C0 + C1;
    if (B < 1 || H < 1 || W < 1 || C0 <= 0 || C1 < 0 || Cout <= 0) return fail("%s: bad size B=%d H=%d W=%d C0=%d C1=%d Cout=%d", what, B, H, W, C0, C1, Cout);
    if (groups <= 0 || C % groups) return fail("%s: groups=%d does not divide C=%d", what, groups, C);
    if (!gn_res1x1_gate_op(c->split() ? 1 : 0, B, H, W, C0, C1, Cout).valid)
        return fail("%s: refused by the gate (exact f32 only; C0=%d, C1=%d in multiples of 32, at most %d together; Cout=%d a multiple of "
                    "64; H*W=%d a multiple of 128)", what, C0, C1, GN_RES1X1_MAX_CIN, Cout, H * W);
    HIP_OK(hipSetDevice(c->device));
    DevBuf dg, db, scale, shift, part, w2;
    std::vector<float> packed((size_t)Cout * C);
    pack_conv_weight(w2_host, Cout, C, 1, C, packed.data());
    if (dg.upload(gamma_host, (size_t)C) || db.upload(beta_host, (size_t)C) || scale.alloc((size_t)B * C) || shift.alloc((size_t)B * C) ||
        part.alloc(gn_workspace_floats(B, C)) || w2.upload(packed.data(), packed.size()))
        return -1;
    const TDesc a = unpadded(const_cast<float *>(x_dev), C0, H, W);
    const TDesc b = skip_dev ? unpadded(const_cast<float *>(skip_dev), C1, H, W) : kNone;
    TDesc act = unpadded(act_dev, C, H, W);
    act.pad = 1;
    GnRes1x1 res;
    res.w2 = w2.p; res.out = unpadded(res_dev, Cout, H, W);
    const unsigned bits = __builtin_bit_cast(unsigned, sentinel);
    HIP_OK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(act_dev), (int)bits, act.floats(B), c->stream));
    HIP_OK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(res_dev), (int)bits, res.out.floats(B), c->stream));
    GnScratch ws;
    ws.scale = scale.p; ws.shift = shift.p; ws.part = part.p;
    // statistics as sr3_op_groupnorm_apply gets them without partials: the streaming statistics kernel, then finalize
    launch_gn_act(GN_FINALIZE_ROWS, a, b, B, groups, dg.p, db.p, 2, 0, act, StatsRef(), StatsRef(), ws, TDesc(), 0, nullptr, nullptr,
                  DropLayer(), c->stream, &res);
    ++c->gn_res1x1_launches;
    if (res_pair_dev) {
        // the launch the kernel replaces, as launch_conv_wino builds it: the unsplit 1x1 conv without bias
        ConvParams r;
        r.in0 = a; r.in1 = b;
        r.B = B; r.Hout = H; r.Wout = W;
        r.ks = 1; r.prec = 0;
        r.w = w2.p;
        r.out = unpadded(res_pair_dev, Cout, H, W);
        HIP_OK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(res_pair_dev), (int)bits, r.out.floats(B), c->stream));
        launch_conv(r, c->stream);
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) return fail("%s: launch failed", what);
    if (const char *e = conv_take_error()) return fail("%s: %s", what, e);
    return 0;
}

// sr3_op_attention (out_split_dev == null, fp32 on) and sr3_op_attention_twin: one body
static int op_attention_impl(const char *what, sr3_ctx *c, const float *qkv_dev, int B, int N, int C, float *out_dev,
                             float *out_split_dev, bool twin_call) {
    if (C % 32 || N < 1) return fail("%s: need C %% 32 == 0 and N >= 1", what);
    const AttnCore core = attention_core(c->split(), N, C);
    if (core == ATTN_UNSUPPORTED)
        return fail("%s: over 1024 tokens the streaming core takes at most 512 channels (C = %d)", what, C);
    if (twin_call && core != ATTN_SPLIT)
        return fail("%s: the twin is written by the split-f16 core only (sr3_set_precision 1 | 2, N <= 512, C <= 512)", what);
    HIP_OK(hipSetDevice(c->device));
    if (core == ATTN_SPLIT) {
        // split-f16 mode: the engine's own sequence — q, k, v in the split operand format, fp32 result and / or its twin
        float *tmp = nullptr;
        HIP_OK(hipMalloc(&tmp, ((size_t)B * N * 3 * C + attention_vt_floats(B, N, C)) * sizeof(float)));
        if (range_reset(c)) return -1;
        const TDesc src = unpadded(const_cast<float *>(qkv_dev), 3 * C, N, 1), dst = unpadded(tmp, 3 * C, N, 1);
        launch_gn_apply_rows(src, kNone, B, nullptr, nullptr, 0, 1, dst, c->stream, TDesc(), 0, c->d_ovf);
        launch_attention_split(tmp, tmp + (size_t)B * N * 3 * C, B, N, C, out_dev, out_split_dev, c->d_ovf, c->stream);
        HIP_OK(hipStreamSynchronize(c->stream));
        HIP_OK(hipFree(tmp));
        HIP_OK(hipGetLastError());
        return range_check(c, what);
    }
    if (core == ATTN_STREAM) launch_attention_stream(qkv_dev, B, N, C, out_dev, c->stream);
    else launch_attention(qkv_dev, B, N, C, out_dev, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

int sr3_op_attention(sr3_ctx *c, const float *qkv_dev, int B, int N, int C, float *out_dev) {
    PlanScope plan_scope(c);
    if (!c || !qkv_dev || !out_dev) return fail("sr3_op_attention: null argument");
    return op_attention_impl("sr3_op_attention", c, qkv_dev, B, N, C, out_dev, nullptr, false);
}

int sr3_op_attention_twin(sr3_ctx *c, const float *qkv_dev, int B, int N, int C, float *out_dev, float *out_split_dev,
                          int fp32_off) {
    PlanScope plan_scope(c);
    if (!c || !qkv_dev || !out_split_dev || (!out_dev && !fp32_off)) return fail("sr3_op_attention_twin: null argument");
    return op_attention_impl("sr3_op_attention_twin", c, qkv_dev, B, N, C, fp32_off ? nullptr : out_dev, out_split_dev, true);
}

int sr3_op_attention_stream(sr3_ctx *c, const float *qkv_dev, int B, int N, int C, float *out_dev) {
    if (!c || !qkv_dev || !out_dev) return fail("sr3_op_attention_stream: null argument");
    if (B < 1 || B > 65535 || N < 1 || !attention_stream_supported(C))
        return fail("sr3_op_attention_stream: need 1 <= B <= 65535, N >= 1 and C a multiple of 32 in [32, 512] (B=%d N=%d C=%d)",
                    B, N, C);
    HIP_OK(hipSetDevice(c->device));
    launch_attention_stream(qkv_dev, B, N, C, out_dev, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

int sr3_op_noise_embed(sr3_ctx *c, const float *noise_level_dev, int B, float *temb_dev, float *chan_bias_dev) {
    if (check_ready(c)) return -1;
    if (!noise_level_dev || !chan_bias_dev) return fail("sr3_op_noise_embed: null argument");
    launch_noise_embed(embed_params(c, noise_level_dev, 1, temb_dev, chan_bias_dev), B, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

int sr3_op_nchw_to_nhwc(sr3_ctx *c, const float *in_dev, int B, int C, int H, int W, float *out_dev) {
    if (!c || !in_dev || !out_dev) return fail("null argument");
    HIP_OK(hipSetDevice(c->device));
    launch_nchw_to_nhwc(in_dev, B, C, unpadded(out_dev, C, H, W), 0, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}
int sr3_op_nhwc_to_nchw(sr3_ctx *c, const float *in_dev, int B, int C, int H, int W, float *out_dev) {
    if (!c || !in_dev || !out_dev) return fail("null argument");
    HIP_OK(hipSetDevice(c->device));
    launch_nhwc_to_nchw(unpadded(const_cast<float *>(in_dev), C, H, W), 0, B, C, out_dev, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- pre-processing ----------------------------------------------------------------------------
int sr3_preprocess_bicubic(sr3_ctx *c, const uint8_t *in_hwc_dev, int B, int Hin, int Win, int Hout, int Wout,
                           float *out_nchw_dev, uint8_t *out_u8_hwc_dev) {
    if (!c || !in_hwc_dev || !out_nchw_dev) return fail("sr3_preprocess_bicubic: null argument");
    if (B <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return fail("sr3_preprocess_bicubic: bad size");
    HIP_OK(hipSetDevice(c->device));
    std::vector<int> bh, kh, bv, kv;
    int ksh = 0, ksv = 0;
    if (Wout != Win) ksh = bicubic_coeffs(Win, Wout, bh, kh);
    if (Hout != Hin) ksv = bicubic_coeffs(Hin, Hout, bv, kv);
    const size_t nt = (bh.size() + kh.size() + bv.size() + kv.size()) * sizeof(int);
    const size_t ntmp = ksh ? (size_t)B * Hin * Wout * 3 : 0;
    char *buf = nullptr;
    HIP_OK(hipMalloc(&buf, nt + ntmp + 16));
    int *d_bh = reinterpret_cast<int *>(buf), *d_kh = d_bh + bh.size(), *d_bv = d_kh + kh.size(), *d_kv = d_bv + bv.size();
    uint8_t *tmp = reinterpret_cast<uint8_t *>(d_kv + kv.size());
    if (ksh) {
        HIP_OK(hipMemcpyAsync(d_bh, bh.data(), bh.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_kh, kh.data(), kh.size() * 4, hipMemcpyHostToDevice, c->stream));
        launch_resample_h(in_hwc_dev, B, Hin, Win, Wout, d_bh, d_kh, ksh, tmp, c->stream);
    }
    if (ksv) {
        HIP_OK(hipMemcpyAsync(d_bv, bv.data(), bv.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_kv, kv.data(), kv.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    launch_resample_v(ksh ? tmp : in_hwc_dev, B, Hin, Hout, Wout, ksv ? d_bv : nullptr, d_kv, ksv, out_nchw_dev,
                      out_u8_hwc_dev, c->stream);
    HIP_OK(hipStreamSynchronize(c->stream));   // the coefficient vectors and buf go out of scope
    HIP_OK(hipFree(buf));
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- post-processing ---------------------------------------------------------------------------
int sr3_postprocess_u8(sr3_ctx *c, const float *sr, int B, int H, int W, int up, int blob, uint8_t *img_u8,
                       uint8_t *up_u8, float *images, float *arcface) {
    if (!c || !sr) return fail("sr3_postprocess_u8: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || up < 0 || blob < 0) return fail("sr3_postprocess_u8: bad size");
    if (!up && (up_u8 || images)) return fail("sr3_postprocess_u8: up_u8 / images need up > 0");
    if (arcface && blob <= 0) return fail("sr3_postprocess_u8: arcface needs blob > 0");
    if (!up && H != W) return fail("sr3_postprocess_u8: up == 0 needs square images");
    HIP_OK(hipSetDevice(c->device));
    const int S = up ? up : H;                    // side of the image the blob is made from
    const bool want_up = up && (up_u8 || images || arcface);
    // blobFromImages resizes with INTER_LINEAR unless the size already matches; an exact factor
    // of 2 takes cv2's area shortcut
    const int f = !arcface ? 0 : (S == blob ? 1 : (S == 2 * blob ? 2 : 0));
    const bool blob_resize = arcface && f == 0;
    std::vector<int> tab, o, ab;
    size_t tab_up = 0, tab_blob = 0;
    auto add_tab = [&](int in_h, int in_w, int out_h, int out_w) {
        const size_t at = tab.size();
        cv_linear_coeffs(in_w, out_w, true, o, ab);
        tab.insert(tab.end(), o.begin(), o.end());
        tab.insert(tab.end(), ab.begin(), ab.end());
        cv_linear_coeffs(in_h, out_h, false, o, ab);
        tab.insert(tab.end(), o.begin(), o.end());
        tab.insert(tab.end(), ab.begin(), ab.end());
        return at;
    };
    if (want_up) tab_up = add_tab(H, W, up, up);
    if (blob_resize) tab_blob = add_tab(S, S, blob, blob);
    const size_t n_img = (size_t)B * H * W * 3, n_up = want_up ? (size_t)B * up * up * 3 : 0;
    const size_t n_bl = blob_resize ? (size_t)B * blob * blob * 3 : 0;
    char *buf = nullptr;
    HIP_OK(hipMalloc(&buf, tab.size() * 4 + n_img + n_up + n_bl + 64));
    int *d_tab = reinterpret_cast<int *>(buf);
    uint8_t *t_img = reinterpret_cast<uint8_t *>(d_tab + tab.size());
    uint8_t *t_up = t_img + n_img, *t_bl = t_up + n_up;
    if (!tab.empty()) HIP_OK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    uint8_t *img = img_u8 ? img_u8 : t_img;
    launch_tensor2img(sr, B, H, W, img, c->stream);
    const uint8_t *src = img;
    if (want_up) {
        uint8_t *u = up_u8 ? up_u8 : t_up;
        launch_resize_linear_u8(img, B, H, W, up, up, d_tab + tab_up, u, images, c->stream);
        src = u;
    }
    if (arcface) {
        const float mean = 127.5f, scale = (float)(1.0 / 127.5);
        if (blob_resize) {
            launch_resize_linear_u8(src, B, S, S, blob, blob, d_tab + tab_blob, t_bl, nullptr, c->stream);
            launch_blob(t_bl, B, blob, blob, 1, mean, scale, arcface, c->stream);
        } else {
            launch_blob(src, B, blob, blob, f, mean, scale, arcface, c->stream);
        }
    }
    HIP_OK(hipStreamSynchronize(c->stream));   // temporaries and host tables go out of scope
    HIP_OK(hipFree(buf));
    HIP_OK(hipGetLastError());
    return 0;
}

int sr3_postprocess_tensor_blob(sr3_ctx *c, const float *sr, int B, int H, int W, int blob, float *arcface) {
    if (!c || !sr || !arcface) return fail("sr3_postprocess_tensor_blob: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || blob <= 0) return fail("sr3_postprocess_tensor_blob: bad size");
    HIP_OK(hipSetDevice(c->device));
    launch_tensor_blob(sr, B, H, W, blob, blob, arcface, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- validation metrics ------------------------------------------------------------------------
int sr3_metrics_psnr_ssim(sr3_ctx *c, const float *sr, const float *hr, int B, int N, int row_offset, int H, int W,
                          const double *gauss11, int64_t *ssd, double *ssim) {
    if (!c || !sr || !hr || !gauss11 || !ssd || !ssim) return fail("sr3_metrics_psnr_ssim: null argument");
    if (B <= 0 || N <= 0 || row_offset < 0 || H <= 0 || W <= 0)
        return fail("sr3_metrics_psnr_ssim: bad size (B=%d N=%d row_offset=%d H=%d W=%d)", B, N, row_offset, H, W);
    if (H < 11 || W < 11)
        return fail("sr3_metrics_psnr_ssim: %dx%d images are smaller than the 11x11 window of the SSIM (core/metrics.py:88-93)", H, W);
    const long long blocks = metrics_blocks(B, H, W);
    if (blocks > 0x7fffffffll) return fail("sr3_metrics_psnr_ssim: B=%d at %dx%d needs %lld blocks, more than one launch takes", B, H, W, blocks);
    HIP_OK(hipSetDevice(c->device));
    if (ensure_partials(c, (size_t)blocks)) return -1;         // one fp64 partial per block
    HIP_OK(hipMemsetAsync(ssd, 0, (size_t)B * sizeof(int64_t), c->stream));   // the blocks ADD their shares
    launch_metrics(sr, hr, B, N, row_offset, H, W, gauss11, c->metrics_ws, ssd, ssim, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- low-resolution consistency --------------------------------------------------
int sr3_set_lr_consistency(sr3_ctx *c, const float *lr_dev, int N, int lh, int lw, uint64_t row_offset, float strength) {
    if (!c) return fail("null context");
    if (!lr_dev || strength == 0.f) {       // off: the steps launch what they always did
        c->lr = LrArgs();
        return 0;
    }
    if (!(strength > 0.f) || strength > 1.f) return fail("sr3_set_lr_consistency: strength must lie in [0, 1], got %g", (double)strength);
    if (N <= 0 || lh <= 0 || lw <= 0) return fail("sr3_set_lr_consistency: needs N, lh, lw > 0 (got %d, %d, %d)", N, lh, lw);
    HIP_OK(hipSetDevice(c->device));
    if (!c->d_lr) HIP_OK(hipMalloc(&c->d_lr, sizeof(LrArgs)));
    if (!c->h_lr) HIP_OK(hipHostMalloc(reinterpret_cast<void **>(&c->h_lr), sizeof(LrArgs) * sr3_ctx::kLrRing, hipHostMallocDefault));
    // (never reuse a ring slot whose copy may still be pending)
    if (c->lr_count && (c->lr_count % (sr3_ctx::kLrRing / 2)) == 0) HIP_OK(hipStreamSynchronize(c->stream));
    LrArgs &a = c->h_lr[c->lr_count++ % sr3_ctx::kLrRing];
    a = LrArgs();
    a.lr = lr_dev; a.row_offset = row_offset; a.N = N; a.strength = strength;
    // the copy runs on the stream behind the steps enqueued so far, which still read the old values
    HIP_OK(hipMemcpyAsync(c->d_lr, &a, sizeof(LrArgs), hipMemcpyHostToDevice, c->stream));
    c->lr = a; c->lr_lh = lh; c->lr_lw = lw;
    return 0;
}

int sr3_op_lr_project(sr3_ctx *c, float *x_dev, int B, int C, int H, int W, const float *lr_dev, int N, int lh, int lw,
                      uint64_t row_offset, float strength, int form) {
    if (!c || !x_dev || !lr_dev) return fail("sr3_op_lr_project: null argument");
    if (B <= 0 || form < 0 || form > 2) return fail("sr3_op_lr_project: needs B > 0 and form 0 (auto) | 1 (LDS) | 2 (scratch)");
    if (check_lr_shape("sr3_op_lr_project", C, H, W, N, lh, lw)) return -1;
    HIP_OK(hipSetDevice(c->device));
    LrOps o;
    if (get_lr_ops(c, lh, lw, H, W, &o)) return -1;
    if (form == 1 && !lr_lds_fits(o))
        return fail("sr3_op_lr_project: the LDS form needs %zu bytes per plane, above its %zu", lr_lds_bytes(o), LR_LDS_MAX_BYTES);
    const bool lds = form == 1 || (form == 0 && lr_lds_fits(o));
    if (!lds && ensure_lr_scratch(c, lr_scratch_floats(B * C, o))) return -1;
    LrArgs a;
    a.lr = lr_dev; a.row_offset = row_offset; a.N = N; a.strength = strength;
    c->pbegin(F_MISC);
    launch_lr_project(x_dev, B * C, C, o, a, nullptr, lds, c->lr_scratch, c->stream);
    c->pend();
    HIP_OK(hipGetLastError());
    return 0;
}

int sr3_op_lr_project_rows(sr3_ctx *c, float *x_dev, int B, int C, int H, int W, const float *lr_rows_dev, int lh, int lw,
                           const float *strength_host, const int *live_host, int form) {
    if (!c || !x_dev || !lr_rows_dev || !strength_host || !live_host) return fail("sr3_op_lr_project_rows: null argument");
    if (B <= 0 || form < 0 || form > 2) return fail("sr3_op_lr_project_rows: needs B > 0 and form 0 (auto) | 1 (LDS) | 2 (scratch)");
    if (check_lr_shape("sr3_op_lr_project_rows", C, H, W, B, lh, lw)) return -1;
    for (int b = 0; b < B; ++b)
        if (!(strength_host[b] >= 0.f) || strength_host[b] > 1.f)
            return fail("sr3_op_lr_project_rows: strength must lie in [0, 1], got %g for row %d", (double)strength_host[b], b);
    HIP_OK(hipSetDevice(c->device));
    LrOps o;
    if (get_lr_ops(c, lh, lw, H, W, &o)) return -1;
    if (form == 1 && !lr_lds_fits(o))
        return fail("sr3_op_lr_project_rows: the LDS form needs %zu bytes per plane, above its %zu", lr_lds_bytes(o), LR_LDS_MAX_BYTES);
    const bool lds = form == 1 || (form == 0 && lr_lds_fits(o));
    if (!lds && ensure_lr_scratch(c, lr_scratch_floats(B * C, o))) return -1;
    // a table of its own, as the session's steps read theirs (only live and lr_strength matter to the projection)
    std::vector<RowArgs> tab((size_t)B, RowArgs());
    for (int b = 0; b < B; ++b) { tab[b].live = live_host[b] ? 1u : 0u; tab[b].lr_strength = strength_host[b]; }
    RowArgs *d_tab = nullptr;
    HIP_OK(hipMalloc(&d_tab, sizeof(RowArgs) * B));
    hipError_t e = hipMemcpy(d_tab, tab.data(), sizeof(RowArgs) * B, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        c->pbegin(F_MISC);
        launch_lr_project_rows(x_dev, B, C, o, lr_rows_dev, d_tab, lds, c->lr_scratch, c->stream);
        c->pend();
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    (void)hipFree(d_tab);
    if (e != hipSuccess) return fail("sr3_op_lr_project_rows: %s", hipGetErrorString(e));
    return 0;
}

int sr3_lr_residual(sr3_ctx *c, const float *img_dev, int B, int C, int H, int W, const float *lr_dev, int N, int lh, int lw,
                    uint64_t row_offset, double *sumsq_dev, float *maxabs_dev) {
    if (!c || !img_dev || !lr_dev || !sumsq_dev || !maxabs_dev) return fail("sr3_lr_residual: null argument");
    if (B <= 0) return fail("sr3_lr_residual: needs B > 0");
    if (check_lr_shape("sr3_lr_residual", C, H, W, N, lh, lw)) return -1;
    if ((size_t)C * lh * lw > (size_t)INT_MAX) return fail("sr3_lr_residual: the LR image is too large");
    HIP_OK(hipSetDevice(c->device));
    LrOps o;
    if (get_lr_ops(c, lh, lw, H, W, &o)) return -1;
    if (ensure_lr_scratch(c, lr_scratch_floats(B * C, o))) return -1;
    LrArgs a;
    a.lr = lr_dev; a.row_offset = row_offset; a.N = N; a.strength = 0.f;
    c->pbegin(F_MISC);
    launch_lr_residual(img_dev, B, C, o, a, c->lr_scratch, sumsq_dev, maxabs_dev, c->stream);
    c->pend();
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- dynamic thresholding -----------------------------------------------------------------------------
namespace {
int check_threshold_args(const char *what, float ratio, float max_value) {
    if (!(ratio <= 1.0f)) return fail("%s: ratio must lie in (0, 1] (or <= 0 for off), got %g", what, (double)ratio);
    if (!(max_value >= 1.0f)) return fail("%s: max_value must be >= 1 (+inf: no bound), got %g", what, (double)max_value);
    return 0;
}

// scratch of the two ops, apart from the sampler's (no captured step holds it): the select's counts, then B floats of s
int ensure_thr_op_scratch(sr3_ctx *c, int B) {
    if (c->thr_op_rows >= B) return 0;
    HIP_OK(hipStreamSynchronize(c->stream));
    if (c->thr_op_bins) HIP_OK(hipFree(c->thr_op_bins));
    c->thr_op_bins = nullptr; c->thr_op_rows = 0;
    HIP_OK(hipMalloc(&c->thr_op_bins, threshold_bins_bytes(B) + (size_t)B * sizeof(float)));
    c->thr_op_rows = B;
    return 0;
}

int check_threshold_op(sr3_ctx *c, const char *what, const void *x, int B, int64_t n, float ratio, float max_value) {
    if (!c || !x) return fail("%s: null argument", what);
    if (B <= 0 || B > 65535 || n <= 0 || n > (int64_t)INT_MAX) return fail("%s: needs 0 < B <= 65535 and 0 < n < 2^31 (got %d, %lld)", what, B, (long long)n);
    if (!(ratio > 0.0f)) return fail("%s: ratio must lie in (0, 1], got %g", what, (double)ratio);
    return check_threshold_args(what, ratio, max_value);
}
}

int sr3_set_dynamic_threshold(sr3_ctx *c, float ratio, float max_value) {
    if (!c) return fail("null context");
    if (!(ratio > 0.0f) && ratio == ratio) {        // off: the steps launch what they always did
        c->dyn_ratio = 0.f;
        return 0;
    }
    if (check_threshold_args("sr3_set_dynamic_threshold", ratio, max_value)) return -1;
    c->dyn_ratio = ratio; c->dyn_max = max_value;
    return 0;
}

int sr3_op_abs_quantile(sr3_ctx *c, const float *x_dev, int B, int64_t n, float ratio, float max_value, float *lo_dev, float *hi_dev,
                        float *s_dev) {
    if (check_threshold_op(c, "sr3_op_abs_quantile", x_dev, B, n, ratio, max_value)) return -1;
    HIP_OK(hipSetDevice(c->device));
    if (ensure_thr_op_scratch(c, B)) return -1;
    c->pbegin(F_MISC);
    launch_abs_quantile(x_dev, B, n, threshold_plan(ratio, n), max_value, c->thr_op_bins, lo_dev, hi_dev, s_dev, c->stream);
    c->pend();
    HIP_OK(hipGetLastError());
    return 0;
}

int sr3_op_dynamic_threshold(sr3_ctx *c, float *x0_dev, int B, int64_t n, float ratio, float max_value, float *s_dev) {
    if (check_threshold_op(c, "sr3_op_dynamic_threshold", x0_dev, B, n, ratio, max_value)) return -1;
    HIP_OK(hipSetDevice(c->device));
    if (ensure_thr_op_scratch(c, B)) return -1;
    float *s = s_dev ? s_dev : reinterpret_cast<float *>(c->thr_op_bins + (size_t)c->thr_op_rows * THR_BINS_PER_IMAGE);
    c->pbegin(F_MISC);
    launch_abs_quantile(x0_dev, B, n, threshold_plan(ratio, n), max_value, c->thr_op_bins, nullptr, nullptr, s, c->stream);
    launch_threshold_apply(x0_dev, B, n, s, c->stream);
    c->pend();
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- device memory helpers ---------------------------------------------------------------------
int sr3_dev_malloc(sr3_ctx *c, uint64_t bytes, void **out_dev) {
    if (!c || !out_dev) return fail("null argument");
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipMalloc(out_dev, bytes ? bytes : 4));
    return 0;
}
int sr3_dev_free(sr3_ctx *c, void *dev) {
    if (!c) return fail("null context");
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipFree(dev));
    return 0;
}
int sr3_memcpy_h2d(sr3_ctx *c, void *dst_dev, const void *src_host, uint64_t bytes) {
    if (!c) return fail("null context");
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
    return 0;
}
int sr3_memcpy_d2h(sr3_ctx *c, void *dst_host, const void *src_dev, uint64_t bytes) {
    if (!c) return fail("null context");
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
    return 0;
}
uint64_t sr3_device_bytes(sr3_ctx *c) { return c ? c->weight_bytes + c->arena_bytes : 0; }

} // extern "C"
