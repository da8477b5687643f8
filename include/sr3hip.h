/*
 * sr3hip.h — C-ABI of libsr3hip.so: the MI355X (gfx950) SR3 iterative-refinement sampler.
 *
 * This is the drop-in boundary for ONE path of zouiner/3d-super-resolution-Face-reconstruction:
 * GaussianDiffusion.p_sample_loop driving the noise-level-conditioned UNet
 * (reference: model/sr/sr3_modules/diffusion.py:189-215, model/sr/sr3_modules/unet.py:235-265).
 * The reference is pure Python/PyTorch and has no FFI of its own; the Python object protocol it
 * exposes (define_G / GaussianDiffusion / UNet) is mirrored by the ctypes host layer in
 * 3d-super-resolution-face-reconstruction_amd/, which binds exactly the entry points below.
 *
 * Conventions
 *   - plain C: opaque context, plain pointers and sizes, int return codes (0 = ok, <0 = error,
 *     message via sr3_last_error()).  No torch types.
 *   - every `*_dev` pointer is a DEVICE pointer on the context's GPU (e.g. tensor.data_ptr()).
 *   - public tensors are fp32, NCHW contiguous (the reference's layout); the library keeps NHWC
 *     internally.
 *   - one context per process/GPU, not thread-safe, all work is stream-ordered on the context's
 *     stream (sr3_set_stream); calls return without synchronising unless stated.
 */
#ifndef SR3HIP_H
#define SR3HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR3_MAX_MULTS 8
#define SR3_MAX_ATTN_RES 8
#define SR3_NAME_MAX 192

typedef struct sr3_ctx sr3_ctx;

/* Mirrors the keyword arguments of UNet.__init__ (reference model/sr/sr3_modules/unet.py:161-174)
 * as filled by define_G (reference model/sr/networks.py:83-101). */
typedef struct sr3_unet_cfg {
    int32_t in_channel;      /* 6 for conditional SR3 (cond ‖ x), 3 unconditional */
    int32_t out_channel;     /* 3 */
    int32_t inner_channel;   /* 64 in every reference yml; must be a multiple of 32 here */
    int32_t norm_groups;     /* 32 */
    int32_t n_mults;
    int32_t channel_mults[SR3_MAX_MULTS];
    int32_t n_attn_res;
    int32_t attn_res[SR3_MAX_ATTN_RES];
    int32_t res_blocks;
    int32_t image_size;      /* only decides attention placement (unet.py:192-207) */
    float dropout;           /* p of the Dropout in every ResnetBlock.block2 (unet.py:81-91), in [0, 1). Identity (eval
                              * semantics) unless sr3_set_dropout enables train-mode sampling of it */
} sr3_unet_cfg;

/* ---- lifecycle -------------------------------------------------------------------------- */

/* replaces: UNet.__init__ + .cuda()  (unet.py:161-233, model/sr3d/model.py:51) */
int sr3_create(const sr3_unet_cfg *cfg, int device, sr3_ctx **out);
void sr3_destroy(sr3_ctx *ctx);
/* message of the last failing call on this thread ("" if none) */
const char *sr3_last_error(void);
/* Return codes: 0 = ok, < 0 = error (sr3_last_error), and one positive "ok, with a warning" code:
 * the call's result is complete and valid, but the split-f16 arithmetic left its range and (part of) the
 * call was recomputed in exact f32 — message via sr3_last_warning(). See sr3_set_range_policy. */
#define SR3_OK_F32_FALLBACK 1
/* ... and a second one: the result is complete and valid, but part of the call was REPLAYED in the same arithmetic on
 * another kernel path. Cause: the in-place split-K convs (deep-K convs over few tiles — the 8x8 level at B = 64) let the
 * blocks of one output tile wait for each other; that needs a free CU slot for each of them, which an otherwise idle GPU
 * always has. If another kernel (another stream or process: e.g. the ArcFace encoder that follows the SR stage,
 * model/sr3d/model.py:372-393) holds those slots, the bounded wait (5 ms) gives up, the work is replayed on the path
 * without inter-block waits and the context stays on that path. Never a hang, never a failed call.
 * sr3_replay_calls counts them; SR3_HALO_SPLITS=0 in the environment selects the non-waiting path from the start. */
#define SR3_OK_REPLAYED 2
const char *sr3_last_warning(void);
/* work is enqueued on `hip_stream` (a hipStream_t; NULL = the context's own stream) */
int sr3_set_stream(sr3_ctx *ctx, void *hip_stream);
int sr3_synchronize(sr3_ctx *ctx);
/* Device-side ordering against another stream of the host (no host synchronisation): the context's stream
 * waits for everything enqueued so far on `other_stream` / `other_stream` waits for everything enqueued so far
 * on the context's stream. (A host that keeps its tensors on its own stream — torch's default stream cannot
 * be captured into a hipGraph, so the library then runs on its own stream — calls the first before handing
 * inputs over and the second before reading results.) */
int sr3_wait_for_stream(sr3_ctx *ctx, void *other_stream);
int sr3_stream_wait_for_ctx(sr3_ctx *ctx, void *other_stream);
/* Arithmetic of the convolutions: 0 = exact f32 on v_mfma_f32_32x32x2_f32 (default; bit-faithful
 * fp32 products), 1 = split-f16 ("f16x3"): operands stored as hi + lo halfs, three
 * v_mfma_f32_32x32x16_f16 per product with fp32 accumulation — fp32-equivalent accuracy (error of
 * the same size as fp32 accumulation itself) at ~5x the matrix rate.
 * 2 = "f16f8": mode 1 with the two CORRECTION products (x_lo*w_hi + x_hi*w_lo) of the MFMA-bound 3x3 convs (32x32- and
 * 16x16-pixel levels at full batch) on the fp8 matrix path: operands additionally stored as OCP e4m3 with power-of-two
 * scales, one v_mfma_scale_f32_32x32x64_f8f6f4 instead of four f16 MFMAs per 32x32 tile and K-step. Correction terms
 * carry 2^-11 of the product, so 3 mantissa bits there cost ~2^-16 relative: 5e-5..7e-5 from the reference over whole
 * sampler runs (bar 1e-3) instead of 4e-6 if EVERY conv took that path (CPU emulation); measured with the eligible
 * layers: 1e-5. Activations beyond 448 (e4m3) in those layers raise the range flag, as 65504 does in mode 1; the default
 * policy then repeats the work in mode 1 first, in f32 if that overflows too. No reference counterpart (unet.py
 * computes in fp32). */
int sr3_set_precision(sr3_ctx *ctx, int prec);
/* 1 when mode 2 runs a 3x3 / stride-1 conv of this shape with fp8 correction products, else 0 (tests, tools). The DEFAULT
 * plan's answer: for a context in the batch-invariant mode read field 11 of sr3_conv_plan_invariant. */
int sr3_conv_f8_supported(int B, int H, int W, int Cout, int Cin);
/* The dispatch plan of one conv shape (H x W input pixels, Cin a multiple of 32) as the engine runs it in `precision`
 * (sr3_set_precision values), with every scratch buffer offered; with_stats: the conv also produces the fused GroupNorm
 * statistics of its output (the UNet's convs do, sr3_op_conv2d does not). Host only: no GPU call. out12 =
 * {kernel id, tile rows, tile columns, split kind (0 none | 1 conv + reduce kernel | 2 in place on the 64x64 tile |
 * 3 in place on the x-halo tile), K-splits, phases (4: upsample conv), floats of split-K partials, 1 if tile counters are
 * used, statistics slices per image (0: none for this shape), floats of Winograd workspace, 1 if the fragment-major
 * Winograd weights are read, 1 if the conv takes the F8C operand format}; kernel_name (optional): the kernel's name,
 * "wino_one_pass" | "wino_three_pass" | "halo_f8c" | "halo_128x128_seg32" | "halo_128x128_seg8" | "halo_128x64" |
 * "generic_128x32" | "generic_128x64" | "generic_64x64" | "generic_128x128". (tests, tools) */
int sr3_conv_plan(int B, int H, int W, int Cin, int Cout, int ks, int stride, int up2, int precision, int with_stats,
                  int64_t *out12, char *kernel_name, int name_cap);

/* ---- batch-invariant mode ------------------------------------------------
 * By default the library picks every launch's form (conv tile, split-K, Winograd form, fp8 layer set, statistics slices,
 * attention block) from the work of the call at hand, so the bytes of one image depend on the batch it ran in. With a
 * planning batch P > 0 every such decision counts P images instead of the call's B and every shape rule is asked of one
 * image: the bytes sr3_unet_forward(_cached), sr3_sample(_from), sr3_sample_begin/step/end, sr3_rows_* and
 * sr3_denoise_loss write for an image then depend on that image's own inputs (conditioning row, state or injected
 * noise, noise level, image id, seed), the weights, the precision, the sampler options and P — not on B, the row, the
 * other rows, the chunking or which batch sizes ran before. Two values of P may give different bytes. Exception: the
 * range policy acts on whole calls, so a call that steps an arithmetic down (SR3_OK_F32_FALLBACK) changes every row.
 * Limits on the real batch (arrival counters of the in-place split-K, 32-bit offsets) become the mode's maximum batch:
 * sr3_max_batch reports it and a larger call fails; the arithmetic never changes at the upper end.
 * plan_batch 0 = off (the default: every launch is today's). Changing the value frees the workspace and drops the
 * captured steps (the state sr3_sample_begin loaded goes with them); refused while a row session (sr3_rows_begin) is
 * open. No reference counterpart. */
int sr3_set_batch_invariant(sr3_ctx *ctx, int plan_batch);
int sr3_get_batch_invariant(sr3_ctx *ctx);
/* sr3_conv_plan as a context in the mode plans the conv at batch B (host only, no GPU call). Every field but the two
 * buffer sizes (which scale with B) is the same for every B up to sr3_conv_plan_invariant_max_batch: the largest batch
 * this conv's plan and tensors hold for under plan_batch (at most 65535); past it sr3_conv_plan_invariant fails. */
int sr3_conv_plan_invariant(int plan_batch, int B, int H, int W, int Cin, int Cout, int ks, int stride, int up2, int precision,
                            int with_stats, int64_t *out12, char *kernel_name, int name_cap);
int64_t sr3_conv_plan_invariant_max_batch(int plan_batch, int H, int W, int Cin, int Cout, int ks, int stride, int up2,
                                          int precision, int with_stats);

/* ---- weights: reference state_dict names and layouts ------------------------------------- */

/* replaces: nn.Module.state_dict() key enumeration for `denoise_fn.*`
 * (names are relative to the UNet, e.g. "downs.1.res_block.block1.block.3.weight"). */
int sr3_num_params(sr3_ctx *ctx);
int sr3_param_info(sr3_ctx *ctx, int index, char *name, int name_cap, int64_t *shape4, int *ndim);
/* replaces: load_state_dict for one tensor (lib/trainer_temp.py:175-179). `host` is fp32 in the
 * reference layout (Conv2d OIHW, Linear [out,in], vectors [C]); repacked to kernel layout inside. */
int sr3_load_weight(sr3_ctx *ctx, const char *name, const float *host, const int64_t *shape,
                    int ndim);
/* number of parameters that have never been loaded (0 = ready) */
int sr3_weights_missing(sr3_ctx *ctx);

/* The same for n tensors that are in DEVICE memory already (live torch parameters after an optimiser step): fp32,
 * contiguous, reference layout, on the context's device. names[i], dev_ptrs[i], shapes[4 * i .. 4 * i + ndims[i] - 1].
 * Every kernel layout is built on the device, enqueued on the context's stream, with ONE host synchronisation per call
 * (the per-tensor maxima that decide the split-f16 scales have to reach the host); the tensors must stay unchanged until
 * the call returns. Same checks and errors as the host route, and the layouts are the same bytes. The fused
 * (conv2 + res_conv) products of the blocks it touches are rebuilt by the call itself. Returns n, or < 0. */
int sr3_load_weights_dev(sr3_ctx *ctx, int n, const char *const *names, const float *const *dev_ptrs,
                         const int64_t *shapes, const int *ndims);

/* Read-only introspection (tests, tools): the kernel layouts the context keeps of one parameter. */
enum {
    SR3_WL_PLAIN = 0,      /* the fp32 copy: conv weights packed [tap][Cout][CinPad] (Upsample convs: 16 phase planes) */
    SR3_WL_SPLIT = 1,      /* split-f16 hi | lo per 32-channel chunk */
    SR3_WL_F8 = 2,         /* F8C copy of the split weights (made on demand in the f16f8 arithmetic) */
    SR3_WL_WINO = 3,       /* G g G^T [16][Cout][CinPad] */
    SR3_WL_WINO_FRAG = 4,  /* the same in the one-pass kernel's fragment order (made on demand) */
    SR3_WL_CONV_IN = 5,    /* first conv: MFMA fragments */
    SR3_WL_FINAL_MFMA = 6, /* final conv: MFMA fragments */
    SR3_WL_FINAL_VALU = 7, /* final conv: [9][C][4] */
    SR3_WL_FUSED_BIAS = 8, /* asked of a block's conv2 bias: conv2 bias + res_conv bias */
    SR3_WL_IDENT = 9,      /* asked of a block's conv2 weight: the identity-skip matrix */
    SR3_WL_UP_WINO_FRAG = 10, /* Upsample convs: sub-pixel Winograd F(2x2, 2x2) weights [4 phases][9][CinPad/8][Cout][8] */
    SR3_N_WEIGHT_LAYOUTS = 11
};
/* Copies at most cap_bytes of the layout to `host` and returns the layout's size in bytes; 0: the parameter has no such
 * layout (now); < 0: error. Synchronises the context's stream. */
int64_t sr3_read_weight_layout(sr3_ctx *ctx, const char *name, int layout, void *host, int64_t cap_bytes);
/* 2^-k of a conv parameter's split-f16 copy (1 for the others; 0 and an error message: unknown name) */
float sr3_weight_unscale(sr3_ctx *ctx, const char *name);

/* ---- the denoiser: UNet.forward(x, noise_level)  (unet.py:235-265) ------------------------ */

/* x_dev: [B, in_channel, H, W] NCHW; noise_level_dev: [B]; out_dev: [B, out_channel, H, W]. */
int sr3_unet_forward(sr3_ctx *ctx, const float *x_dev, const float *noise_level_dev, int B, int H,
                     int W, float *out_dev);

/* ---- the sampler: GaussianDiffusion.{set_new_noise_schedule,p_sample_loop} ---------------- */

/* replaces: the fp32 buffers registered by set_new_noise_schedule (diffusion.py:93-142). The host
 * computes them in float64 exactly as the reference does and passes the fp32 casts:
 *   noise_level[T+1]  = float32(sqrt_alphas_cumprod_prev)      (diffusion.py:108-109,166-167)
 *   recip[T]          = sqrt_recip_alphas_cumprod               (:125-126)
 *   recipm1[T]        = sqrt_recipm1_alphas_cumprod             (:127-128)
 *   logvar[T]         = posterior_log_variance_clipped          (:137-138)
 *   coef1[T], coef2[T]= posterior_mean_coef1/2                  (:139-142) */
int sr3_set_schedule(sr3_ctx *ctx, int T, const float *noise_level, const float *recip,
                     const float *recipm1, const float *logvar, const float *coef1,
                     const float *coef2);

/* A few-step sampler over the same noise schedule (DDIM, DPM-Solver++(2M)), replacing the one
 * sr3_set_schedule set. S steps; step i (S-1 down to 0, like the reference's t) runs the UNet at noise_level[i+1] and
 * updates x0 = clamp(a[i] x - b[i] eps, -1, 1), x' = c1[i] x0 + c2[i] x + c3[i] x0_prev + sigma[i] z, where x0_prev is
 * the clamped x0 of the previous step (used only with uses_history != 0; the first step after sr3_sample_begin, whatever
 * its t, stores its x0 without reading one. The library keeps it next to the sampler state and in the checkpoints of
 * sr3_sample). sigma is the standard deviation
 * itself (not a log-variance). Afterwards S is the step count of sr3_sample, sr3_sample_step (t in [0, S)),
 * sr3_num_frames and of the injected noise ([S, B, C, H, W]). sr3_set_schedule returns to the reference's DDPM loop
 * (c3 = 0, no history). */
int sr3_set_sampler_schedule(sr3_ctx *ctx, int S, const float *noise_level, const float *a, const float *b,
                             const float *c1, const float *c2, const float *c3, const float *sigma,
                             int uses_history);

/* replaces: p_sample_loop (diffusion.py:189-215) for a whole batch.
 *   cond_dev   [B,3,H,W] conditioning image (x_in) or NULL for the unconditional branch (:193-201)
 *   noise_dev  NULL -> device Philox4x32-10 + Box-Muller keyed by (seed, image index+image_offset,
 *              draw, element); else [(T), B, C, H, W]: slab 0 is the initial image (torch.randn,
 *              :205), slab k (1..T-1) is the randn_like of loop iteration k-1 (t = T-k, :186)
 *   out_dev    [B,C,H,W] final images (every image, not only ret_img[-1])
 *   frames_dev NULL or [n_frames,B,C,H,W]: the image after every step i with i % sample_inter == 0
 *              (:192,209-211), sample_inter = 1 | (T/10); n_frames = sr3_num_frames(ctx)
 * Stream-ordered. In f32 mode it returns after enqueueing; in split-f16 mode it synchronises every
 * T/10 steps and at the end to read the range-check flag (see sr3_range_check below). */
int sr3_sample(sr3_ctx *ctx, const float *cond_dev, int B, int H, int W, const float *noise_dev,
               uint64_t seed, uint64_t image_offset, float *out_dev, float *frames_dev);
int sr3_num_frames(sr3_ctx *ctx);
/* Largest batch ONE sr3_sample / sr3_unet_forward call takes at H x W (every activation tensor below 4 GiB: 32-bit DMA
 * offsets; ~250 images at 128x128 with the yml UNet). Larger batches — the reference's validation loop is 15 samples x N
 * images, lib/trainer_temp.py:441-446; BASELINE configs[3] is 512 images — are run as equal chunks with image_offset
 * advancing, which the Python facade does by itself (GaussianDiffusion.sample_batch). < 0: error. */
int sr3_max_batch(sr3_ctx *ctx, int H, int W);
/* One p_sample step t on the library-resident state (used by bench.py to time exact step counts):
 * sr3_sample_begin loads cond + initial noise, sr3_sample_step runs step t, sr3_sample_end copies
 * the current image out. noise_slab_dev may be NULL (Philox). */
int sr3_sample_begin(sr3_ctx *ctx, const float *cond_dev, int B, int H, int W,
                     const float *init_noise_dev, uint64_t seed, uint64_t image_offset);
int sr3_sample_step(sr3_ctx *ctx, int t, const float *noise_slab_dev);
int sr3_sample_end(sr3_ctx *ctx, float *out_dev);
/* Warm start: the loop begins at an intermediate noise level from a given image and runs only the last
 * start_step steps, t = start_step-1 .. 0 of the tables currently set (sr3_set_schedule's T or sr3_set_sampler_schedule's
 * S; start_step in [1, S]). The state before step start_step-1 is at noise_level[start_step].
 *   replaces: q_sample (model/sr/sr3_modules/diffusion.py:275-282) of init at that level, followed by the last
 *   start_step iterations of p_sample_loop (:183-215).
 *   init_dev   [B,C,H,W]; may be cond_dev itself when in_channel - out_channel == out_channel.
 *   noised != 0: state = level * init + sqrt(1 - level^2) * z, level = noise_level[start_step], product, product and
 *              sum each rounded to fp32 and the coefficient formed as float32 sqrt(1 - level*level): bit-equal to the
 *              reference's q_sample expression on the same fp32 inputs. z is Philox draw 0 of (seed, image_offset + row)
 *              or slab 0 of the injected noise. One pass writes cond, state, packed twin and range flag; needs
 *              in_channel <= 8, like sr3_denoise_loss.
 *   noised == 0: state = init, bit for bit (refining an image that already sits at that level: a frame of an earlier
 *              call, an interpolation of two noised images).
 *   noise      [start_step, B, C, H, W]: slab 0 is z (present but unread when noised == 0), slab k the draw of step
 *              t = start_step - k. Philox draws keep draw = S - t, so a tail begun from a frame of a full run repeats it.
 *   frames     after every step i < start_step with i % sample_inter == 0, sample_inter = 1 | (S/10);
 *              sr3_num_frames_from(ctx, start_step) counts them.
 * sr3_sample_from is sr3_sample's loop (the same range guard, its segments counted from the first step that runs);
 * sr3_sample_begin_from is the step API's counterpart of sr3_sample_begin. With a sampler that keeps an x0 history
 * (DPM-Solver++(2M)) the first step of a call begun through these two takes c1[t] + c3[t] (fp32 sum on the host) as its
 * c1, which makes it the first-order step exactly; a call begun with sr3_sample_begin keeps applying c1[t] alone in its
 * first step, as it always did (right only at t = S-1, where c3 is 0). */
int sr3_sample_begin_from(sr3_ctx *ctx, const float *cond_dev, int B, int H, int W, const float *init_dev,
                          int start_step, int noised, const float *noise0_dev, uint64_t seed, uint64_t image_offset);
int sr3_sample_from(sr3_ctx *ctx, const float *cond_dev, int B, int H, int W, const float *init_dev, int start_step,
                    int noised, const float *noise_dev, uint64_t seed, uint64_t image_offset, float *out_dev,
                    float *frames_dev);
int sr3_num_frames_from(sr3_ctx *ctx, int start_step);
/* Rolling batch: a session of B slots in which every batch row sits at its OWN position of the schedule,
 * so a request takes a free slot while the others are mid-trajectory and the batch stays full. No kernel mixes rows and
 * Philox is keyed by (seed, image id, draw, element): a row's result is the bytes of its row in a sr3_sample /
 * sr3_sample_from call of the SAME batch size B with the same image id and seed, whatever its slot, its neighbours and
 * the moment it was admitted. Every step runs at batch B, and which conv kernels run depends on B (the fp8 path of mode 2
 * only from 32 or 64 images on, the split-K forms): against a call at another batch size a row differs as any two batch
 * sizes do, by fp32 round-off in modes 0 / 1 and at the 1e-5 level in mode 2. The update half of
 * a step reads a per-row argument table (RowArgs, csrc/kernels_rows.hip); one captured graph serves every step of every
 * session of a size. Sampler, schedule, arithmetic and dynamic threshold are the context's; low-resolution consistency
 * and frames are per ROW (sr3_rows_lr_consistency / sr3_rows_admit_lr, sr3_rows_frames).
 *   sr3_rows_begin     opens a session of B slots at H x W, all idle, the state zeroed (an idle row still runs through the
 *                      UNet and is never written by the update). Fails, naming the setting, while low-resolution
 *                      consistency, the feature cache or Dropout sampling is on, and for the unconditional model.
 *   sr3_rows_admit     puts one request into idle slot `row`: cond_dev [in_channel - out_channel, H, W]; init_dev NULL: the
 *                      start noise at the top (start_step must be S; noise0_dev [C, H, W] or NULL: Philox draw 0 of
 *                      image_id); init_dev [C, H, W]: the warm start of sr3_sample_begin_from at start_step in [1, S] —
 *                      noised != 0: q_sample at noise_level[start_step] with z = noise0_dev or Philox draw 0, bit for bit
 *                      what sr3_sample_begin_from writes for that row; noised == 0: init itself. With a sampler that
 *                      keeps an x0 history such a row's first step takes c1 + c3 as its c1, as there, per row; a slot's
 *                      new occupant never reads the history of the previous one. Fails if the slot is live.
 *   sr3_rows_lr_consistency  arms the session for low-resolution consistency at the LR size (lh, lw): after sr3_rows_begin
 *                      and before the first admit. Builds or reuses the operators of (lh, lw) -> (H, W) and picks the
 *                      form as sr3_set_lr_consistency does; fails as it does when the size cannot constrain H x W. Every
 *                      step of an armed session runs x0 prediction | (dynamic threshold) | projection | update, the
 *                      projection on the planes of the rows admitted with an LR image only; one more captured graph.
 *   sr3_rows_admit_lr  sr3_rows_admit with the row's LR image: lr_dev [C, lh, lw] fp32 in [-1, 1], copied into the
 *                      session's own buffer (stream-ordered: the caller may free it once the call returns), and its
 *                      strength in [0, 1] (outside: an error). NULL or 0: the row is not held, as after sr3_rows_admit —
 *                      it is then the bytes of its row in the uniform call WITHOUT low-resolution consistency, a held row
 *                      those of the call with sr3_set_lr_consistency at that strength. An LR image for a session that is
 *                      not armed is an error. A slot's new occupant never reads the LR image of the previous one.
 *   sr3_rows_frames    after the admit and before the row's first step: the row writes into frames_dev, [n][C, H, W] in
 *                      order, the frames a sr3_sample / sr3_sample_from call begun at the same start_step returns for it
 *                      (n = sr3_num_frames_from(start_step); capacity < n is an error and changes nothing).
 *   sr3_rows_step      one step of every live row at its own position (t = position - 1, Philox draw S - t), then those
 *                      positions go down by one. noise_rows: NULL (Philox), or B host-side entries of device pointers,
 *                      entry r the [C, H, W] draw of row r's step (read for live rows with t > 0 only). Returns the number
 *                      of rows stepped, < 0 on error; 0 (nothing launched) when no row has a step left.
 *   sr3_rows_position  steps left for the slot, -1 for an idle one, < -1 on error.
 *   sr3_rows_retire    copies a finished row (0 steps left, else an error) to out_dev [C, H, W] and frees its slot; the
 *                      state stays where it is and is not touched again until the slot is admitted into.
 *   sr3_rows_drop      frees a slot at any point, nothing copied; the state of a live row goes back to zeros (it may hold
 *                      anything mid-trajectory, and an idle row still runs through the UNet).
 *   sr3_rows_end       closes the session.
 * Elastic steps (batch-invariant mode only, sr3_set_batch_invariant; DESIGN.md 3.5g "live rows only"): in that mode a
 * row's bytes do not depend on how many rows a launch covers, nor does what the workspace holds per image, so a step may
 * run over rows [0, batch) of the session's workspace alone and cost what `batch` images cost.
 *   sr3_rows_step_batch  sr3_rows_step over slots [0, batch): embedding, UNet and every launch of the update run for
 *                      `batch` rows; slots at or above `batch` are neither read nor written (state, packed copy, history,
 *                      their slab of the x0 prediction, LR image, frames). batch == B is sr3_rows_step itself: the same
 *                      key, graph and launches. Fails, launching nothing and leaving every position where it was, when
 *                      batch lies outside [1, B], when a live row with steps left sits at a slot >= batch (named), and
 *                      when batch < B with the batch-invariant mode off (the workspace was sized by plans that follow B: a
 *                      smaller batch may take more split-K partials than it holds; the message names
 *                      sr3_set_batch_invariant). Before the first launch at a new `batch` the host checks that what the
 *                      plans at `batch` ask of the shared buffers fits what was carved for B (an "internal:" error
 *                      otherwise; cached per value). One captured graph per (rows form, batch value), at most 16 batch
 *                      values per form (the least recently used one is evicted). noise_rows has B entries as before.
 *   sr3_rows_move      moves live slot `src` into idle slot `dst` (anything else is an error): state slab with borders and
 *                      pad channels, packed split-f16 slab, x0 history slab, in an armed session the slot's LR image, and
 *                      the host's record of the row (position, start, image id, history flags, strength, frames). `src`
 *                      is left as sr3_rows_drop leaves it (zero state, zero packed copy, idle). One kernel launch behind
 *                      the steps already enqueued, no host synchronisation. The row's Philox streams are keyed by its
 *                      image id and do not change; injected noise must follow the row (entry `dst` of noise_rows).
 *   sr3_rows_rows_run  the sum of `batch` over the row-session steps this context has launched (sr3_rows_step counts B).
 *   sr3_read_history   the x0 history of the current workspace, B * out_channel * H * W floats NCHW, to host memory;
 *                      returns that count, < 0 on error. Synchronises the context's stream. (tests)
 * Range contract: the step API's. Nothing is replayed inside the library; sr3_range_check reports an activation beyond
 * the operand range since the last check (the caller re-admits what was in flight, its requests being pure functions of
 * seed, image id and init), and sr3_set_precision is allowed between steps. sr3_sample* and sr3_unet_forward during a
 * session take the workspace over and end it, as they end a sr3_sample_begin session; sr3_sample_step fails. */
int sr3_rows_begin(sr3_ctx *ctx, int B, int H, int W, uint64_t seed);
int sr3_rows_admit(sr3_ctx *ctx, int row, const float *cond_dev, const float *init_dev, int start_step, int noised,
                   const float *noise0_dev, uint64_t image_id);
int sr3_rows_lr_consistency(sr3_ctx *ctx, int lh, int lw);
int sr3_rows_admit_lr(sr3_ctx *ctx, int row, const float *cond_dev, const float *init_dev, int start_step, int noised,
                      const float *noise0_dev, uint64_t image_id, const float *lr_dev, float strength);
int sr3_rows_frames(sr3_ctx *ctx, int row, float *frames_dev, int capacity);
int sr3_rows_step(sr3_ctx *ctx, const float *const *noise_rows);
int sr3_rows_position(sr3_ctx *ctx, int row);
int sr3_rows_retire(sr3_ctx *ctx, int row, float *out_dev);
int sr3_rows_drop(sr3_ctx *ctx, int row);
int sr3_rows_end(sr3_ctx *ctx);
int sr3_rows_step_batch(sr3_ctx *ctx, const float *const *noise_rows, int batch);
int sr3_rows_move(sr3_ctx *ctx, int src, int dst);
uint64_t sr3_rows_rows_run(sr3_ctx *ctx);
int64_t sr3_read_history(sr3_ctx *ctx, float *hist_host);
/* Range check of the split-f16 arithmetic (sr3_set_precision(ctx, 1)): the reference computes in
 * fp32 (diffusion.py:164-180, unet.py:235-265) and has no such limit, so a value that does not fit
 * the hi + lo fp16 operand format (|v| > 65504, or a NaN) must never pass silently. Every kernel that stores
 * or builds that format (conv epilogues and split-K fix-ups, GroupNorm apply, attention, the final conv's
 * on-the-fly split, state packing and the DDPM update's packed state) raises a device flag instead of clamping.
 *   sr3_unet_forward, sr3_sample — the calls that own their inputs — FINISH the call like the reference would:
 *     sr3_unet_forward evaluates the forward again in exact f32; sr3_sample reads the flag every
 *     T/10 steps (one stream synchronisation each), keeps a copy of the sampler state of the last
 *     in-range boundary and, when the flag trips, replays from that boundary to the end in exact f32
 *     (noise draws and frame slots are functions of t, so the replay is exact). Both then return
 *     SR3_OK_F32_FALLBACK (> 0) with sr3_last_warning() set; sr3_fallback_calls counts them.
 *   sr3_set_range_policy(ctx, 1) ("strict") restores the failing behaviour: those calls return < 0
 *     and the message names the f32 mode as the remedy.
 *   sr3_sample_end (step API: the caller owns the noise slabs, the library cannot replay) always
 *     fails on overflow; sr3_range_check does the same on demand between sr3_sample_step calls:
 *     0 = in range, < 0 = overflow since the last check (flag cleared). Both synchronise the stream.
 *   In mode 2 ("f16f8") the flag is also raised by an activation beyond the fp8 operand range (|v| > 448) in a conv on
 *     the fp8 correction path; the message then names mode 1 (f16x3) as the first remedy, mode 0 as the second, and the
 *     default policy of sr3_unet_forward / sr3_sample retries in exactly that order.
 *     (The ladder is written once for the owned-input calls, sr3_denoise_loss included — guarded_eval in
 *     csrc/sr3_api.hip — and once for sr3_sample's checkpointed segments.)
 *   The same flag word carries the "in-place split-K wait gave up" bit (SR3_OK_REPLAYED above): sr3_unet_forward and
 *     sr3_sample replay by themselves; sr3_sample_end / sr3_range_check fail with a message that says to repeat the call. */
int sr3_range_check(sr3_ctx *ctx);
int sr3_set_range_policy(sr3_ctx *ctx, int strict);
int sr3_fallback_calls(sr3_ctx *ctx);
int sr3_replay_calls(sr3_ctx *ctx);
/* GroupNorm apply passes launched (or captured into a graph) since sr3_create in the form that writes the Winograd input
 * transform of the three-pass conv behind them (exact f32 only; 0 under SR3_NO_GN_WINO=1): tells a test which route ran. */
int sr3_gn_wino_passes(sr3_ctx *ctx);
/* Three-pass Winograd convs this context launched (or captured into a graph) since sr3_create in the form that runs the position GEMMs
 * and the output transform in one kernel (0 under SR3_NO_WINO_GEMM_OUT=1): tells a test which form ran. */
int sr3_wino_gemm_out_launches(sr3_ctx *ctx);
/* Forwards of this context (launched or captured into a graph, sr3_op_conv_in_f32 calls included) since sr3_create whose
 * first conv ran on conv_in_f32_kernel (exact f32 only; 0 under SR3_NO_CONV_IN_F32=1): tells a test which kernel ran. */
int sr3_conv_in_f32_launches(sr3_ctx *ctx);
/* Upsample convs this context launched (or captured into a graph) since sr3_create as sub-pixel Winograd F(2x2, 2x2)
 * (wino_up2_kernel; exact f32 only; 0 under SR3_NO_UP2_WINO=1): tells a test which form ran. */
int sr3_up2_wino_launches(sr3_ctx *ctx);
/* Three-pass Winograd convs this context launched (or captured into a graph) since sr3_create on the one-pass kernel with
 * 2 | 4 tile rows per block (the 32x32 and 16x16 levels; exact f32 only; 0 under SR3_NO_WINO_FUSED_ROWS=1): tells a test
 * which form ran. */
int sr3_wino_fused_rows_launches(sr3_ctx *ctx);
/* block1 GroupNorm apply passes this context launched (or captured into a graph) since sr3_create together with the
 * block's 1x1 res_conv (gn_res1x1_kernel; exact f32 only; 0 under SR3_NO_GN_RES1X1=1), sr3_op_gn_res1x1 calls included:
 * tells a test which form ran. */
int sr3_gn_res1x1_launches(sr3_ctx *ctx);
/* The engine's decision for one ResnetBlock (host only, no context): does block1's GroupNorm + Swish pass over x (C0
 * channels) || skip (C1) also multiply the block's 1x1 res_conv into Cout channels? The two 3x3 convs' plans are those of
 * sr3_conv_plan with statistics. flags: 1 = the block has a res_conv, 2 = its operands are x / skip themselves, 4 = a raw
 * copy of the concatenation is wanted, 8 = an input is stored in the split format; mode as sr3_op_groupnorm_apply.
 * Returns bit 0 = valid, bit 1 = tuned (the level and block count are adopted), bit 2 = taken in this process (valid,
 * not SR3_NO_GN_RES1X1=1, and tuned or SR3_GN_RES1X1_FORCE=1); < 0: bad argument. Like sr3_conv_plan it describes the
 * DEFAULT plan: a context in the batch-invariant mode counts its planning batch in place of B. */
int sr3_gn_res1x1_gate(int B, int H, int W, int C0, int C1, int Cout, int precision, int flags, int mode);
/* Sampler steps this context captured into a graph since sr3_create (successful instantiations; 0 under SR3_NO_GRAPH=1
 * and while profiling): tells a test that a step was replayed from its graph, or captured anew because a value the graph
 * holds had changed. */
int sr3_step_graph_captures(sr3_ctx *ctx);
/* TEST HOOK (tests/test_gpu_round4.py): device address of the context's flag word (bit 0: range overflow, bit 1: an
 * in-place split-K wait gave up), so that a test kernel on another stream can raise a bit in the middle of a running
 * sr3_sample call and the replay logic is exercised deterministically. Not for production use. */
void *sr3_test_flag_address(sr3_ctx *ctx);

/* The documented CPU twin of the device RNG is oracle/philox.py; this dumps the device stream for
 * comparison: n floats of draw `draw` for image `image`. */
int sr3_philox_normal(sr3_ctx *ctx, uint64_t seed, uint64_t image, uint32_t draw, int n,
                      float *out_dev);

/* ---- train-mode Dropout: the UNet as the reference evaluates it under .train() ------------------ */

/* replaces: the nn.Dropout(p) between Swish and Conv3x3 of every ResnetBlock.block2 (unet.py:81-91, built with
 * p = cfg.dropout at unet.py:100-101) in train mode: the conv's input is keep ? swish(gn(h1)) * s : 0 with
 * s = float32(1.0 / (1.0 - p)) (what torch.nn.Dropout multiplies by). block1, final_conv, the attention norm and the
 * res_conv operand are never masked. Off by default (eval semantics: identity); enable = 0 restores exactly that — the
 * same kernels, the same bits. enable != 0 latches p from the config (p >= 1 fails; p = 0 has no effect) and sets the
 * key of the mask stream: keep bits are a pure function of (seed, global image index, draw, layer, channel, y, x) —
 * Philox4x32-10, one evaluation per 8 channels of a pixel, a 16-bit field per element, kept iff field >=
 * round-half-even(p * 65536): the keep probability is 1 - thr/65536 (0.80000305 for p = 0.2), p quantised to 2^-16.
 * layer = 0-based ordinal of the ResnetBlock in execution order (downs, mid, ups) = the order of the reference's
 * nn.Dropout modules in named_modules(). draw = T - t in step t of the sampler, 0 in sr3_unet_forward and
 * sr3_denoise_loss. global image index = image_offset + batch row, with the image_offset sr3_sample / sr3_sample_begin /
 * sr3_denoise_loss take (with noise_per_source, where image_offset indexes source images, the row's index is
 * image_offset + row_offset + b); sr3_unet_forward has none and uses the one given here. So a mask does not depend on the batch
 * an image sits in, on chunking, on the arithmetic mode or on the range policy's repeats (CPU twin:
 * tests/dropout_ref.py). Drops the captured step graphs when it changes what the apply passes launch. */
int sr3_set_dropout(sr3_ctx *ctx, int enable, uint64_t seed, uint64_t image_offset);
/* Injected masks instead of the Philox stream (parity with recorded masks of the reference's nn.Dropout modules,
 * unet.py:81-91): one uint8 device buffer, the layers concatenated in layer order, each [B][C][H][W] (NCHW, like the
 * reference's tensor), nonzero = keep; bytes must equal sr3_dropout_mask_bytes for the call's B, H, W or the call that
 * uses them fails. Honoured by sr3_unet_forward, sr3_denoise_loss and the step API, where each sr3_sample_step consumes
 * the buffer set at that moment (per-step masks); sr3_sample fails while masks are injected. The buffer stays the
 * caller's and must outlive the calls. NULL returns to Philox. Only read while sr3_set_dropout is enabled. */
int sr3_set_dropout_masks(sr3_ctx *ctx, const uint8_t *dev, uint64_t bytes);
/* The Dropout layers (unet.py:81-91: one per ResnetBlock) at H x W: *n = their number, chw (NULL, or 3 * n ints) =
 * {C, H, W} of each layer's masked tensor in layer order. Host only. */
int sr3_dropout_layers(sr3_ctx *ctx, int H, int W, int *n, int *chw /* 3 per layer */);
/* bytes of the injected mask buffer for a batch of B images at H x W (the sum of B*C*H*W over the layers); < 0: error */
int64_t sr3_dropout_mask_bytes(sr3_ctx *ctx, int B, int H, int W);
/* The counterpart of sr3_philox_normal for the mask stream (unet.py:81-91 has torch's generator here): one image's Philox
 * mask of one layer as uint8 [C][H][W], 1 = keep, with p from the config; C a multiple of 8, draw < 2^24, layer < 254. */
int sr3_op_dropout_mask(sr3_ctx *ctx, uint64_t seed, uint64_t image, uint32_t draw, int layer, int C, int H, int W,
                        uint8_t *out_dev);

/* ---- measurement ------------------------------------------------------------------------- */

/* When enabled every kernel launch is bracketed by HIP events on the context's stream and
 * accumulated per kernel family. */
int sr3_profile_enable(sr3_ctx *ctx, int on);
int sr3_profile_reset(sr3_ctx *ctx);
/* family: 0 conv_igemm, 1 groupnorm, 2 attention, 3 embed, 4 ddpm_update/layout.
 * Synchronises the stream. flops = algorithmic 2*MAC of the launches (0 for non-GEMM families). */
int sr3_profile_get(sr3_ctx *ctx, int family, double *total_ms, int64_t *launches, double *flops);
#define SR3_N_FAMILIES 5
/* per distinct conv launch shape: launches, total/avg ms, GFLOP per launch, TFLOP/s (CSV) */
int sr3_profile_dump_csv(sr3_ctx *ctx, const char *path);

/* Kernel micro-benchmark: average ms of `iters` launches of one conv shape on scratch buffers
 * and, in *apply_ms, of the
 * GroupNorm apply pass that precedes it (mode 0 copy, 1 affine, 2 affine + Swish), as the engine runs the shape: in front
 * of a three-pass Winograd conv the pass writes the transformed input and the conv starts from it. */
int sr3_bench_conv(sr3_ctx *ctx, int B, int Hin, int Win, int C0, int C1, int Cout, int ks, int stride,
                   int up2, int mode, int with_resid, int with_chan_bias, int iters, float *avg_ms,
                   float *apply_ms);

/* Host-side weight layouts of the exact-f32 Winograd convs (no GPU involved): packed_host is the
 * kernel layout [9][Cout][CinPad] of a 3x3 conv; dst receives 16 * Cout * CinPad floats of
 * G g G^T as [16][Cout][CinPad] (frag = 0, the three-pass path) or [16][CinPad/8][Cout][8]
 * (frag = 1, the one-pass kernel). CinPad a multiple of 8.
 * frag = 2: the Upsample conv's sub-pixel Winograd F(2x2, 2x2) weights instead, 36 * Cout * CinPad floats as
 * [py * 2 + px][3i + j][CinPad/8][Cout][8]: sums of the original taps, added in fp64 in (dy, dx) order, rounded once. */
int sr3_wino_weights_host(const float *packed_host, int Cout, int CinPad, int frag, float *dst_host);

/* ---- single ops through the same kernels (parity tests call these) ------------------------ */

/* Conv2d over NHWC device tensors. in1_dev may be NULL (C1 = 0); channel order is in0 ‖ in1
 * (torch.cat((x, skip), 1), unet.py:261). weight_host is OIHW [Cout, C0+C1, ks, ks], bias_host
 * NULL or [Cout]. up2 = nearest x2 upsample before the conv (unet.py:58-65); stride 1|2
 * (unet.py:68-74). gn_scale/gn_shift NULL or [B, C0+C1]: per (image, channel) affine applied to the
 * input before zero padding, followed by Swish if `swish`. chan_bias_dev NULL or [B, Cout]
 * (FeatureWiseAffine, unet.py:34-50); resid_dev NULL or [B,Hout,Wout,Cout]. */
int sr3_op_conv2d(sr3_ctx *ctx, const float *in0_dev, int C0, const float *in1_dev, int C1, int B,
                  int Hin, int Win, const float *weight_host, const float *bias_host, int Cout,
                  int ks, int stride, int up2, const float *gn_scale_dev,
                  const float *gn_shift_dev, int swish, const float *chan_bias_dev,
                  const float *resid_dev, float *out_dev);
/* sr3_op_conv2d as the ENGINE runs the conv: with the fused GroupNorm statistics of its output offered, so the dispatch
 * plan is the one sr3_conv_plan reports with with_stats = 1 (which may name another kernel than without). stats_dev
 * (stats_capacity_doubles doubles) is first filled with 0xFF bytes (they read back as NaN), then receives fp64 {sum, sum
 * of squares} of the stored fp32 output per (image, slice, channel) as [B][*slices_out][Cout][2]; *slices_out = the
 * plan's slices per image. A shape whose plan has no fused statistics runs without them: *slices_out = 0 and the output
 * is sr3_op_conv2d's. Fails if the buffer is too small. (tests) */
int sr3_op_conv2d_stats(sr3_ctx *ctx, const float *in0_dev, int C0, const float *in1_dev, int C1, int B,
                        int Hin, int Win, const float *weight_host, const float *bias_host, int Cout,
                        int ks, int stride, int up2, const float *gn_scale_dev,
                        const float *gn_shift_dev, int swish, const float *chan_bias_dev,
                        const float *resid_dev, float *out_dev, double *stats_dev,
                        uint64_t stats_capacity_doubles, int *slices_out);
/* The SECOND launch of a ResnetBlock as the engine builds it (run_res): sr3_op_conv2d_stats for a 3x3 / stride 1 conv,
 * plus the skip forms and output forms of that launch. The dispatch plan is the one sr3_conv_plan reports for the 3x3 shape
 * with with_stats = 1: none of the following changes it.
 *   in2_dev / in2b_dev, w2_host, b2_host   the res_conv (unet.py:102-103,110) as extra 1x1 K-steps: in2 [B,H,W,C2a] and
 *               the optional in2b [B,H,W,C2b] (x and skip of torch.cat, unet.py:261) fp32 NHWC on the device, w2_host
 *               [Cout, C2a+C2b] (OIHW of the 1x1 conv), b2_host NULL or [Cout]. The kernel gets what the engine prepares:
 *               bias + b2; in f32 w2 as packed 1x1 weights; in the split-f16 arithmetics w and w2 split with one common
 *               2^k and in2 / in2b copied into the plain split format. C2a and C2b must be multiples of 32.
 *   flags & SR3_FUSED_IDENT       (split-f16 only; Cout <= 128; no w2, no in2b) in2 [B,H,W,Cout] is the block input and
 *               the identity skip runs as extra K-steps against the engine's identity matrix (2^k on the diagonal, k the
 *               exponent of w capped at 15, w re-split where the cap bites).
 *   out_split_dev                 (split-f16 only, optional) the split-f16 twin of the output, [B,H,W,Cout] 32-bit words (per
 *               32-channel chunk 32 hi halfs | 32 lo halfs); a value beyond the fp16 range is the "range" error.
 *   flags & SR3_FUSED_NO_F32      only the twin is written; out_dev (still required) is left untouched.
 *   flags & SR3_FUSED_RESID_SPLIT resid_dev holds split-format words (a residual that exists only as its twin).
 * Any other combination is an error and launches nothing. (tests) */
#define SR3_FUSED_IDENT 1
#define SR3_FUSED_NO_F32 2
#define SR3_FUSED_RESID_SPLIT 4
int sr3_op_conv2d_fused(sr3_ctx *ctx, const float *in0_dev, int C0, const float *in1_dev, int C1, int B, int Hin,
                        int Win, const float *weight_host, const float *bias_host, int Cout,
                        const float *gn_scale_dev, const float *gn_shift_dev, int swish,
                        const float *chan_bias_dev, const float *resid_dev, const float *in2_dev, int C2a,
                        const float *in2b_dev, int C2b, const float *w2_host, const float *b2_host, int flags,
                        float *out_dev, float *out_split_dev, double *stats_dev, uint64_t stats_capacity_doubles,
                        int *slices_out);
/* The UNet's first conv as the split-f16 forward runs it (unet.py:193-194 downs.0 on cat([cond, x_t]), diffusion.py:170):
 * the zero-bordered fp32 state is built from state_nchw_dev [B, Cin, H, W] (Cin <= 8) as sr3_unet_forward builds it,
 * packed by pack_state_kernel into [B][H+2][W+2] pixels of 16 halfs (channels 0..7 hi | channels 0..7 lo) and convolved by
 * conv_in_kernel with weight_host (OIHW [Cout, Cin, 3, 3]) in the fragment layout the engine keeps (SR3_WL_CONV_IN),
 * bias_host NULL or [Cout]. Every output is optional (NULL = the kernel runs with that option off):
 *   out_dev     fp32 NHWC [B, H, W, Cout]
 *   twin_dev    the split-f16 twin as stored, [B, H, W, Cout] 32-bit words (per 32-channel chunk 32 hi halfs | 32 lo halfs)
 *   stats_dev   fp64 {sum, sum of squares} of the fp32 values per (image, 256-pixel block, channel),
 *               [B][H*W/256][Cout][2]; the whole buffer (stats_capacity_doubles) is first filled with 0xFF bytes;
 *               *slices_out = H*W/256
 *   packed_host B*(H+2)*(W+2)*16 halfs (HOST memory): the packed state the conv read, borders included
 * Fails where the forward would not take this path: an arithmetic that is not split-f16, a shape conv_in_supported
 * refuses (Cin > 8, Cout not 32 | 64, W % 16, H*W % 256); nothing is launched then. A raised range flag (a state value or,
 * with the twin, an output beyond the fp16 range, or not finite) is an error naming the range. (tests) */
int sr3_op_conv_in(sr3_ctx *ctx, const float *state_nchw_dev, int B, int H, int W, int Cin, const float *weight_host,
                   const float *bias_host, int Cout, float *out_dev, float *twin_dev, double *stats_dev,
                   uint64_t stats_capacity_doubles, int *slices_out, void *packed_host);
/* The same conv as the exact-f32 forward runs it: the zero-bordered fp32 state of 32 channels per pixel is built from
 * state_nchw_dev [B, Cin, H, W] as sr3_unet_forward builds it and convolved by conv_in_f32_kernel (fp32 operands on
 * v_mfma_f32_16x16x4_f32, 72 k-values per output) with weight_host (OIHW [Cout, Cin, 3, 3]) in the packed layout the engine
 * keeps ([tap][Cout][32]), bias_host NULL or [Cout].
 *   out_dev     fp32 NHWC [B, H, W, Cout]
 *   stats_dev   NULL, or fp64 {sum, sum of squares} of the stored values per (image, 256-pixel block, channel),
 *               [B][H*W/256][Cout][2]; the whole buffer (stats_capacity_doubles) is first filled with 0xFF bytes;
 *               *slices_out = H*W/256
 * Fails where the forward would not take this path: a split-f16 arithmetic, a shape conv_in_supported refuses (Cin > 8,
 * Cout not 32 | 64, W % 16, H*W % 256), SR3_NO_CONV_IN_F32=1; nothing is launched then. (tests) */
int sr3_op_conv_in_f32(sr3_ctx *ctx, const float *state_nchw_dev, int B, int H, int W, int Cin, const float *weight_host,
                       const float *bias_host, int Cout, float *out_dev, double *stats_dev, uint64_t stats_capacity_doubles,
                       int *slices_out);
/* Does an exact-f32 forward (precision 0; 1 | 2: never) run its first conv Cin -> Cout at H x W on conv_in_f32_kernel?
 * 1 | 0: conv_in_supported's shape rule and SR3_NO_CONV_IN_F32 (host arithmetic only; needs no context and no GPU). */
int sr3_conv_in_f32_gate(int Cin, int Cout, int H, int W, int precision);
/* The UNet's last layer as the forward runs it (unet.py:229,263 final_conv = Block: GroupNorm -> Swish -> Conv3x3) behind
 * the folded GroupNorm affine: in_dev fp32 NHWC [B, H, W, C], gn_scale_dev / gn_shift_dev [B, C]
 * (sr3_op_groupnorm_affine), weight_host OIHW [Cout, C, 3, 3], bias_host [Cout], out_dev fp32 NHWC [B, H, W, Cout];
 * zero padding applies to the activated tensor. The gates are the forward's: the fused final conv exists where
 * final_conv_supported holds (C % 64 == 0, Cout 1..4), any other shape fails and launches nothing. Exact f32:
 * final_conv_kernel (fp32 VALU), *form_out = 1. Split-f16: final_conv_mfma_kernel where final_conv_mfma_supported holds
 * as well (Cout == 3, C 64 | 128), *form_out = 2, else the VALU kernel as in the forward. In the MFMA form a raised
 * range flag (an activation beyond the fp16 range, or not finite) is an error naming the range. form_out is optional. (tests) */
int sr3_op_final_conv(sr3_ctx *ctx, const float *in_dev, int B, int H, int W, int C, const float *gn_scale_dev,
                      const float *gn_shift_dev, const float *weight_host, const float *bias_host, int Cout,
                      float *out_dev, int *form_out);
/* The sampler state of the current workspace (the last sr3_sample_begin / _step, sr3_unet_forward, sr3_denoise_loss ...
 * call): state_host receives the 8 leading channels of the zero-bordered fp32 state, B*(H+2)*(W+2)*8 floats, packed_host
 * its packed split-f16 copy, B*(H+2)*(W+2)*16 halfs (either may be NULL); dims3 (optional) = {B, H, W}. Returns the
 * number of padded pixels B*(H+2)*(W+2); 0: this shape keeps no packed state (conv_in_supported), nothing is copied;
 * < 0: error (no workspace yet). Synchronises the context's stream. (tests) */
int64_t sr3_read_packed_state(sr3_ctx *ctx, float *state_host, void *packed_host, int *dims3);
/* block1's GroupNorm + Swish pass and the block's 1x1 res_conv in one kernel (exact f32), on unpadded NHWC x (C0
 * channels) || skip (C1; skip_dev NULL: none): act_dev [B][H+2][W+2][C0+C1] receives swish(group_norm(x || skip)) at its
 * interior pixels — the bits of sr3_op_groupnorm_apply (mode 2, format 0) — and res_dev [B][H][W][Cout] receives
 * w2 . (x || skip) without bias (w2_host [Cout][C0+C1]) — the bits of the unsplit 1x1 conv. The statistics come from the
 * streaming statistics kernel and a finalize launch. Both outputs are filled with `sentinel` first, so the border of
 * act_dev still holds it afterwards. res_pair_dev (optional, [B][H][W][Cout]): additionally receives the same product from
 * the launch the kernel replaces in the engine (the 1x1 side launch of a Winograd conv2). Fails for a shape the engine's
 * gate refuses: C0, C1 multiples of 32, C0+C1 <= 1024, Cout a multiple of 64, H*W a multiple of 128; f32 mode. (tests) */
int sr3_op_gn_res1x1(sr3_ctx *ctx, const float *x_dev, int C0, const float *skip_dev, int C1, int B, int H, int W, int groups,
                     const float *gamma_host, const float *beta_host, const float *w2_host, int Cout, float sentinel,
                     float *act_dev, float *res_dev, float *res_pair_dev);
/* Per-shape timing of that kernel against the two launches it replaces, on random data with the statistics of x and skip
 * given as conv epilogues leave them: *pair_ms = the GroupNorm apply pass on the engine's route (*route_out, as
 * sr3_op_groupnorm_apply's; with its finalize launch on route 2) + the 1x1 conv; *one_ms = finalize launch + the kernel;
 * each the average of `iters` back-to-back repetitions. (tools/conv_bench.py --set gnres) */
int sr3_bench_gn_res1x1(sr3_ctx *ctx, int B, int H, int W, int C0, int C1, int Cout, int groups, int iters, float *pair_ms,
                        float *one_ms, int *route_out);
/* GroupNorm statistics folded with the affine: scale[b,c] = rstd*gamma[c],
 * shift[b,c] = beta[c] - mean*rstd*gamma[c]  (torch GroupNorm, eps 1e-5; unet.py:84,119). */
int sr3_op_groupnorm_affine(sr3_ctx *ctx, const float *in0_dev, int C0, const float *in1_dev,
                            int C1, int B, int H, int W, int groups, const float *gamma_host,
                            const float *beta_host, float *scale_dev, float *shift_dev);
/* The GroupNorm apply pass of the engine (unet.py:84-86 Block: GroupNorm -> Swish, over torch.cat((x, skip), 1)) on
 * unpadded NHWC inputs in0 ‖ in1 (in1_dev NULL: none): out = act(group_norm(in0 ‖ in1)), mode 0 copy | 1 affine |
 * 2 affine + Swish; gamma_host / beta_host [C0+C1]. Channels in multiples of 8 (32 for any split format), C0+C1 <= 2048.
 * stats0_dev / stats1_dev: fp64 partial statistics of in0 / in1 as conv epilogues leave them, [B][slices][C][2] with
 * slices0 / slices1 slices (any split of an image's pixels); both NULL: the streaming statistics kernel runs first (fp32
 * inputs only); stats1_dev NULL with in1 present is an error unless both are NULL.
 * format: 0 fp32 | 1 split-f16 (per 32-channel chunk 32 hi halfs | 32 lo halfs) | 2 the F8C variant (32 hi halfs |
 * 32 x e4m3(lo * 2^11) | 32 x e4m3(value)); out_dev [B,H,W,C0+C1] receives the 32-bit words as stored. in_split bit 0 /
 * bit 1: in0 / in1 is itself stored in format 1. raw_out_dev (optional): the un-normalised concatenation, in format 1
 * if `format` is non-zero, else fp32.
 * route: 1 = statistics finalize folded into the apply launch, 2 = finalize launch + streaming apply, 0 = what the
 * engine chooses for this pass; *route_out (optional) = the route taken (1 | 2); *range_out (optional) = 1 if a stored
 * value exceeded the range of its split format (the range flag; never in format 0), which is NOT an error here. (tests) */
int sr3_op_groupnorm_apply(sr3_ctx *ctx, const float *in0_dev, int C0, const float *in1_dev, int C1, int B, int H,
                           int W, int groups, const float *gamma_host, const float *beta_host,
                           const double *stats0_dev, int slices0, const double *stats1_dev, int slices1, int mode,
                           int format, int in_split, int route, float *out_dev, float *raw_out_dev,
                           int *route_out, int *range_out);
/* SelfAttention core (unet.py:132-139): qkv_dev [B, N, 3C] (q|k|v along the last axis) -> out
 * [B, N, C]; softmax(q.k / sqrt(C)) v, one head. Any N >= 1, C a multiple of 32: up to 1024 tokens the
 * engine's cores for the precision mode run (32 x N score tile in LDS); above, the exact-f32 streaming
 * core (online softmax, C <= 512) runs in every mode. */
int sr3_op_attention(sr3_ctx *ctx, const float *qkv_dev, int B, int N, int C, float *out_dev);
/* sr3_op_attention in the split-f16 core with the output forms the forward uses: out_split_dev [B, N, C] 32-bit words
 * receives the split-f16 twin of the result (a value beyond the fp16 range is the "range" error); fp32_off != 0: only
 * the twin is written and out_dev (may be NULL then) is left untouched. Outside the split core (another arithmetic, or a
 * shape it does not take) this is an error. (tests) */
int sr3_op_attention_twin(sr3_ctx *ctx, const float *qkv_dev, int B, int N, int C, float *out_dev, float *out_split_dev,
                          int fp32_off);
/* The streaming core alone, at any N >= 1 (C a multiple of 32 in [32, 512]), whatever the precision
 * mode: for comparing it with the tiled core on the same shape. */
int sr3_op_attention_stream(sr3_ctx *ctx, const float *qkv_dev, int B, int N, int C, float *out_dev);
/* noise_level_mlp + every FeatureWiseAffine linear (unet.py:23-31,179-184,39,49): noise_level_dev
 * [B] -> chan_bias_dev [B, total] where total = sr3_chan_bias_total(ctx) (blocks in module order). */
int sr3_op_noise_embed(sr3_ctx *ctx, const float *noise_level_dev, int B, float *temb_dev,
                       float *chan_bias_dev);
int sr3_chan_bias_total(sr3_ctx *ctx);
/* NCHW <-> NHWC copies */
int sr3_op_nchw_to_nhwc(sr3_ctx *ctx, const float *in_dev, int B, int C, int H, int W,
                        float *out_dev);
int sr3_op_nhwc_to_nchw(sr3_ctx *ctx, const float *in_dev, int B, int C, int H, int W,
                        float *out_dev);

/* ---- pre-processing in front of the sampler ------------------------------------------------- */

/* replaces: the PIL 8-bit bicubic upsample that builds the conditioning image
 * (datasets/tool/prepare_data.py:24-47: Image.resize(size, BICUBIC)) followed by ToTensor and
 * x*2-1 (datasets/util.py:76-83). in: uint8 [B,Hin,Win,3] (HWC, RGB); out: fp32 [B,3,Hout,Wout]
 * in [-1,1]; out_u8 (optional) the resized uint8 image. Bit-exact with Pillow 12.2. Synchronous. */
int sr3_preprocess_bicubic(sr3_ctx *ctx, const uint8_t *in_hwc_dev, int B, int Hin, int Win, int Hout,
                           int Wout, float *out_nchw_dev, uint8_t *out_u8_hwc_dev);

/* ---- post-processing behind the sampler ------------------------------------------------------ */

/* replaces the host chain between the sampler and the MICA / ArcFace encoder
 * (model/sr3d/model.py:372-386 and :462-471):
 *   img_u8  = Metrics.tensor2img(SR)                     core/metrics.py:16-42  [B,H,W,3] RGB
 *   up_u8   = cv2.resize(img_u8, (up, up))               model/sr3d/model.py:380 [B,up,up,3]
 *   images  = up_u8.transpose(2,0,1) / 255               model/sr3d/model.py:383-385 [B,3,up,up] fp32
 *   arcface = cv2.dnn.blobFromImages([up_u8], 1/127.5, (blob, blob), 127.5, swapRB=True)[0]
 *                                                         model/sr3d/model.py:127-131 [B,3,blob,blob]
 * sr_nchw: fp32 [B,3,H,W] in [-1,1] (the sampler's output). Every output pointer is optional
 * (null = not wanted); all are device pointers. up == 0 skips the resize (arcface is then built
 * from img_u8). cv2's 8-bit INTER_LINEAR (and its scale-2 INTER_AREA shortcut inside
 * blobFromImages) is restated from OpenCV 4.x resize.cpp — parity unpinned, cv2 is not installed.
 * Synchronous. */
int sr3_postprocess_u8(sr3_ctx *ctx, const float *sr_nchw_dev, int B, int H, int W, int up, int blob,
                       uint8_t *img_u8_dev, uint8_t *up_u8_dev, float *images_dev, float *arcface_dev);

/* replaces the tensor chain of model3 (model/sr3d/model.py:474-483):
 *   arcface = create_tensor_blob(tensor2tensor_img(SR) * 255)   model/sr3d/model.py:105-124,
 *                                                                core/metrics.py:44-50
 * i.e. clamp, [0,255] scaling, (x-127.5)/127.5, torch bilinear resize (align_corners=False) to
 * blob x blob, RGB->BGR. out: fp32 [B,3,blob,blob]. Asynchronous on the context's stream. */
int sr3_postprocess_tensor_blob(sr3_ctx *ctx, const float *sr_nchw_dev, int B, int H, int W, int blob,
                                float *arcface_dev);

/* ---- validation metrics behind the sampler -------------------------------------------------- */

/* replaces the host scoring of the validation loop (lib/trainer_temp.py:441-446 ->
 * model/sr3d/model.py:368-433), per row b of the batch against hr[(row_offset + b) % N]:
 *   a, b    = Metrics.tensor2img(SR[b]), Metrics.tensor2img(HR[..])    core/metrics.py:16-42
 *   ssd[b]  = sum((a - b)^2) over all 3*H*W uint8 pairs, exact          core/metrics.py:74-81
 *             (calculate_psnr = 20*log10(255/sqrt(ssd / (3*H*W))), inf for ssd == 0: left to the host)
 *   ssim[b] = Metrics.calculate_ssim(a, b)                               core/metrics.py:84-125
 *             (fp64; 11x11 Gaussian, sigma 1.5; 'valid' region (H-10) x (W-10); C1 = 6.5025,
 *             C2 = 58.5225; mean of the map per channel, mean of the three channels)
 * sr_nchw: fp32 [B,3,H,W], any range (the sampler's output); hr_nchw: fp32 [N,3,H,W], never
 * replicated: sample k of image i is row k*N + i of a validation batch, a shard of it starts at
 * row_offset. gauss11_host: the 11 normalised taps of cv2.getGaussianKernel(11, 1.5) in fp64 (host
 * memory; the device evaluates no exp). ssd_dev [B] int64, ssim_dev [B] fp64: device pointers.
 * H, W >= 11 (the formula has no value below the window size). Two calls on the same inputs return
 * bitwise equal results (no floating-point atomics). Asynchronous on the context's stream. */
int sr3_metrics_psnr_ssim(sr3_ctx *ctx, const float *sr_nchw_dev, const float *hr_nchw_dev, int B, int N,
                          int row_offset, int H, int W, const double *gauss11_host, int64_t *ssd_dev,
                          double *ssim_dev);

/* ---- the denoising loss: GaussianDiffusion.p_losses without a backward pass ---------------- */

/* replaces what the reference wraps around one UNet forward when it evaluates its objective
 * (model/sr/sr3_modules/diffusion.py:284-313; evaluation only: no gradient is formed), per batch row b on source
 * image n = (row_offset + b) % N:
 *   x_noisy = level[b] * HR[n] + s[b] * noise          q_sample, diffusion.py:275-282 (product, product, sum, each
 *             rounded to fp32 like torch; s[b] = float32(sqrt(1 - level[b]^2)) comes from the host, which forms it with
 *             the reference's own fp32 expression, so x_noisy is bit-equal to q_sample)
 *   eps     = denoise_fn(cat([SR[n], x_noisy], 1), level)   diffusion.py:302-306, unet.py:235-265 (cond_dev NULL:
 *             denoise_fn(x_noisy, level), the unconditional branch; needs in_channel == out_channel)
 *   per_image[b] = sum |noise - eps| (loss_type 0, L1Loss(reduction='sum')) or sum (noise - eps)^2 (1, MSELoss)
 *             diffusion.py:85-91,312 — difference and square in fp32, accumulated in fp64 in a fixed order (no
 *             floating-point atomics: two calls return bitwise equal sums). The reference's scalar is their sum.
 * hr_dev [N, out_channel, H, W], cond_dev [N, in_channel - out_channel, H, W] (never replicated: level k of image i is
 * row k*N + i of an images-x-levels batch), level_dev / s_dev [B] fp32, per_image_dev [B] fp64: device pointers.
 * noise_dev: an NCHW slab, or NULL for device Philox with the sampler's keying (seed, image_offset + j, draw 0, element
 * c*H*W + y*W + x: the stream of the sampler's initial image). noise_per_source == 0: j = b, slab [B, out_channel, H, W];
 * != 0: j = n, slab [N, out_channel, H, W] — one noise image per SOURCE image whatever the row's level. No copy of drawn
 * noise is stored: the loss pass regenerates it.
 * x_noisy_out / eps_out (optional, NCHW [B, out_channel, H, W]): the noised images and the UNet's prediction.
 * Range policy as sr3_unet_forward (the caller owns every input, so the call is simply evaluated again): SR3_OK_REPLAYED,
 * f16f8 -> f16x3 -> f32 with SR3_OK_F32_FALLBACK, an error under the strict policy. B <= sr3_max_batch. */
int sr3_denoise_loss(sr3_ctx *ctx, const float *hr_dev, const float *cond_dev, int N, int row_offset,
                     const float *level_dev, const float *s_dev, const float *noise_dev, int noise_per_source,
                     uint64_t seed, uint64_t image_offset, int B, int H, int W, int loss_type, double *per_image_dev,
                     float *x_noisy_out, float *eps_out);
/* q_sample alone (diffusion.py:275-282) into a caller buffer: x_noisy_out [B, C, H, W] from hr_dev [N, C, H, W]
 * (1 <= C <= 4), any H, W; rows, coefficients and noise as above. Needs no weights. Asynchronous. */
int sr3_op_q_sample(sr3_ctx *ctx, const float *hr_dev, int N, int row_offset, const float *level_dev,
                    const float *s_dev, const float *noise_dev, int noise_per_source, uint64_t seed,
                    uint64_t image_offset, int B, int C, int H, int W, float *x_noisy_out);

/* ---- low-resolution consistency of the sampler ---------------------------- */
/* The reference makes its LR images with Pillow's antialiased bicubic resample (datasets/tool/prepare_data.py:37-47).
 * In real arithmetic that is, per axis and for sizes r -> l (r > l, any ratio),
 *   A in R^{l x r}:  A[i][x] = w((x - (i + 0.5) r/l + 0.5) l/r) / sum over the row, for x in the clipped support
 *                    [int(c - 2r/l + 0.5), int(c + 2r/l + 0.5)) of c = (i + 0.5) r/l, w the bicubic kernel (a = -0.5)
 * (Resample.c precompute_coeffs before its fixed-point rounding); every row sums to 1. A A^T is symmetric positive
 * definite with a condition number near 2, so
 *   P = A^T (A A^T)^-1 in R^{r x l}     (Cholesky, float64),   A P = I,   P A the orthogonal projector on range(A^T).
 * Host only, no context: A receives l*r doubles (row-major [l][r]), P receives r*l ([r][l]). */
int sr3_lr_operators_host(int l, int r, double *A_host, double *P_host);
/* While set, every step of sr3_sample and of sr3_sample_begin / _step / _end projects its clamped x0 prediction onto the
 * images that downsample to the LR input, between the prediction and the posterior update:
 *   x0  = clamp(a x - b eps, -1, 1)                                        (as without the feature)
 *   x0 <- x0 + strength * P_v (Y - A_v x0 A_h^T) P_h^T                     per (image, channel) plane, fp32
 *   x'  = c1 x0 + c2 x [+ c3 x0_prev] [+ sigma z]                          (x0_prev: the PROJECTED x0 of the step before)
 * with A_v, P_v for lh -> H and A_h, P_h for lw -> W, and Y the plane of lr[(row_offset + b) % N] for batch row b (the
 * row convention of sr3_metrics_psnr_ssim: samples x images batches never replicate the LR images; a chunk or shard
 * passes its first global row). Nothing is clamped after the projection: the last step of every sampler returns
 * 1 * x0 + 0 * x, so at strength 1 the result satisfies A x = y to fp32 rounding. lr_dev: fp32 NCHW [N, out_channel,
 * lh, lw] in [-1, 1], read by every later step: it must outlive them. NULL or strength 0 turns the feature off, and a
 * step then launches exactly the kernels it always did; 0 < strength <= 1 otherwise. Set it before sr3_sample_begin.
 * The pointer, N, row_offset and strength are read from device memory, so captured step graphs survive their change;
 * a change of (lh, lw) rebuilds them. Works in all three arithmetic modes (the projection is always fp32), with the
 * range policy's replays, the x0 history and Dropout. */
int sr3_set_lr_consistency(sr3_ctx *ctx, const float *lr_dev, int N, int lh, int lw, uint64_t row_offset,
                           float strength);
/* The projection alone, in place on x_dev (fp32 NCHW [B, C, H, W]; lr_dev [N, C, lh, lw]; H > lh, W > lw):
 *   X <- X + strength * P_v (Y - A_v X A_h^T) P_h^T
 * in four stages, T = X A_h^T (banded), R = Y - A_v T (banded), U = P_v R, X += strength * U P_h^T. form 1: one block
 * per plane with T, R, U in LDS (fails if (H + lh) * lw floats exceed 64 KB); form 2: one launch per stage over global
 * scratch; form 0: form 1 where it fits, as the sampler chooses. Both forms return the same bits. Asynchronous. */
int sr3_op_lr_project(sr3_ctx *ctx, float *x_dev, int B, int C, int H, int W, const float *lr_dev, int N, int lh,
                      int lw, uint64_t row_offset, float strength, int form);
/* The rows form of the projection (the one an armed row session runs), alone: row b of x_dev is held to
 * lr_rows_dev[b] ([B, C, lh, lw]) at strength_host[b] when live_host[b] != 0 and strength_host[b] != 0 (host arrays of B
 * entries, strengths in [0, 1]); the planes of every other row are neither read nor written. form as above. A held plane
 * gets the bits sr3_op_lr_project gives it. Synchronous. */
int sr3_op_lr_project_rows(sr3_ctx *ctx, float *x_dev, int B, int C, int H, int W, const float *lr_rows_dev, int lh, int lw,
                           const float *strength_host, const int *live_host, int form);
/* The consistency score, which needs no HR image: per batch row b over its C planes,
 *   sumsq_dev[b]  = sum (A_v X A_h^T - Y)^2   (fp32 residuals, fp64 sum; mse = sumsq / (C lh lw))
 *   maxabs_dev[b] = max |A_v X A_h^T - Y|
 * with Y as above. Bitwise reproducible (no atomics). Asynchronous. */
int sr3_lr_residual(sr3_ctx *ctx, const float *img_dev, int B, int C, int H, int W, const float *lr_dev, int N,
                    int lh, int lw, uint64_t row_offset, double *sumsq_dev, float *maxabs_dev);

/* ---- dynamic thresholding of the x0 prediction ---------------------------- */
/* Replaces, while on, the static x_recon.clamp_(-1., 1.) of every sampler step (model/sr/sr3_modules/diffusion.py:175-176)
 * by the dynamic thresholding of Imagen (Saharia et al. 2022, section 2.3), which generalises it. Defined by DESIGN.md
 * 3.5e; per image b of the batch, n = out_channel * H * W, before any low-resolution projection:
 *   x0  = a x - b eps                                                   (the update's prediction, not clamped)
 *   keys: the bit patterns of |x0| as unsigned integers (a total order: -0 = +0, denormals kept, NaN above inf)
 *   pos = (double)ratio * (n - 1), k = min(floor(pos), n - 1), frac = (float)(pos - k)
 *   lo  = the k-th smallest key (0-based, ties with their multiplicity), hi = the (k+1)-th, or lo when k = n - 1
 *   s   = min(max(lo + frac * (hi - lo), 1), max_value)                 (every operation rounded by itself; NaN -> 1)
 *   x0 <- clamp(x0, -s, s) / s                                          (s = 1: the bits of the static clamp)
 * and everything downstream — the posterior mean, the x0 history of dpmpp_2m, the projection of
 * sr3_set_lr_consistency — takes that x0. The order statistics are exact (a radix select with integer counts): two
 * calls return the same bits. ratio in (0, 1] turns it on with max_value >= 1 (+inf: no upper bound); ratio <= 0
 * turns it off, and a step then launches exactly the kernels it always did. Fails for ratio > 1 or NaN, and (when on)
 * max_value < 1 or NaN. Set it before sr3_sample_begin; covers sr3_sample, sr3_sample_from and the step API in all three
 * arithmetic modes (the threshold is always fp32), with the range policy's replays. A change rebuilds the captured
 * steps that hold it. */
int sr3_set_dynamic_threshold(sr3_ctx *ctx, float ratio, float max_value);
/* The selection alone (defined by DESIGN.md 3.5e, items 2-3 above) on any fp32 x_dev [B][n], 0 < n < 2^31: lo_dev[b],
 * hi_dev[b], s_dev[b] (each may be NULL). ratio in (0, 1], max_value >= 1. Needs no weights. x_dev needs only the
 * alignment of a float. Asynchronous (stream-ordered). */
int sr3_op_abs_quantile(sr3_ctx *ctx, const float *x_dev, int B, int64_t n, float ratio, float max_value, float *lo_dev,
                        float *hi_dev, float *s_dev);
/* Selection and x0 <- clamp(x0, -s, s) / s in place on a caller buffer [B][n] (with s = 1 the reference's
 * x_recon.clamp_(-1., 1.), diffusion.py:175-176); s_dev [B] receives s when not NULL. Asynchronous. */
int sr3_op_dynamic_threshold(sr3_ctx *ctx, float *x0_dev, int B, int64_t n, float ratio, float max_value, float *s_dev);
/* Sampler steps this context issued since sr3_create in the thresholded form (x0 prediction | selection | threshold |
 * [projection] | update), one per step whether launched or replayed from a captured graph: tells a test which form ran. */
int sr3_dynamic_threshold_launches(sr3_ctx *ctx);

/* ---- feature cache: deep UNet features reused across sampler steps --------- */
/* DeepCache (Ma, Fang, Wang 2023, "DeepCache: Accelerating Diffusion Models for Free"), training-free, beside the
 * reference's UNet.forward (model/sr/sr3_modules/unet.py:235-265) and its sampling loop (diffusion.py:189-215): with
 * interval N > 1, step k of a sampling call (k counts from sr3_sample_begin / sr3_sample_begin_from) runs the whole UNet
 * when k % N == 0, and otherwise only its `depth` top resolution levels — conv_in and the down modules in front of the
 * Downsample that leaves level depth - 1, then the up modules behind the Upsample that returns to it, then final_conv —
 * on the output that Upsample had in the last whole step. The noise embedding, the noise draws, the update (every
 * sampler, x0 history, projection, dynamic threshold) and the Dropout masks of the blocks that run are those of a whole
 * step. interval <= 1 turns it off: the sampler is then bit for bit what it was. Fails for depth outside
 * [1, n_mults - 1]. A step is whole regardless of k when the workspace does not hold a whole step of this call in the
 * arithmetic the step runs in: after a new workspace, sr3_set_precision, a weight load or refresh, a step down of the
 * range policy, or any forward from outside the call. With the cache on, sr3_sample's range guard checks after whole
 * numbers of intervals, so a replayed segment starts with a whole step and repeats the same pattern. Sample quality is
 * a property of the trained weights and is not established by this library. */
int sr3_set_feature_cache(sr3_ctx *ctx, int interval, int depth);
/* whole and shallow steps of the last sampling call (since its sr3_sample_begin*), replayed ones included */
int sr3_feature_cache_steps(sr3_ctx *ctx, int *whole, int *shallow);
/* The shallow forward of `depth` alone, as sr3_unet_forward takes its arguments (Dropout setting included): the skipped
 * modules are what the most recent whole forward of the same (B, H, W) in the current arithmetic left in the workspace.
 * Fails when there is none (never run, other shape, sr3_set_precision or a weight load since, or the range policy
 * finished that forward in another arithmetic). Never steps the arithmetic down: a result out of range is an error
 * that names the mode. */
int sr3_unet_forward_cached(sr3_ctx *ctx, const float *x_dev, const float *noise_level_dev, int B, int H, int W, int depth,
                            float *out_dev);

/* ---- device memory helpers (so hosts without torch can drive the library) ---------------- */
int sr3_dev_malloc(sr3_ctx *ctx, uint64_t bytes, void **out_dev);
int sr3_dev_free(sr3_ctx *ctx, void *dev);
int sr3_memcpy_h2d(sr3_ctx *ctx, void *dst_dev, const void *src_host, uint64_t bytes);
int sr3_memcpy_d2h(sr3_ctx *ctx, void *dst_host, const void *src_dev, uint64_t bytes);
/* bytes of device memory the context currently holds (weights + workspace) */
uint64_t sr3_device_bytes(sr3_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* SR3HIP_H */
