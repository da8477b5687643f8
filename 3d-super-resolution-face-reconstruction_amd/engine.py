"""`Engine`: a thin, torch-free Python handle on one `sr3_ctx` (one per process / GPU).

Everything takes raw device addresses (ints) so it can be driven from torch tensors
(`t.data_ptr()`) or from buffers allocated through the library itself (`DeviceBuffer`).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .graph import UNetConfig


def _cfg_struct(cfg: UNetConfig) -> _lib.UnetCfg:
    s = _lib.UnetCfg()
    s.in_channel, s.out_channel = int(cfg.in_channel), int(cfg.out_channel)
    s.inner_channel, s.norm_groups = int(cfg.inner_channel), int(cfg.norm_groups)
    if len(cfg.channel_mults) > _lib.SR3_MAX_MULTS or len(cfg.attn_res) > _lib.SR3_MAX_ATTN_RES:
        raise ValueError("too many channel_mults / attn_res entries")
    s.n_mults = len(cfg.channel_mults)
    for i, m in enumerate(cfg.channel_mults):
        s.channel_mults[i] = int(m)
    s.n_attn_res = len(cfg.attn_res)
    for i, a in enumerate(cfg.attn_res):
        s.attn_res[i] = int(a)
    s.res_blocks, s.image_size = int(cfg.res_blocks), int(cfg.image_size)
    s.dropout = float(cfg.dropout)
    return s


def _host_f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


class DeviceBuffer:
    """fp32 device array owned by the library (for hosts that do not use torch)."""

    def __init__(self, eng: "Engine", n_floats: int):
        self.eng, self.n = eng, int(n_floats)
        p = C.c_void_p()
        _lib.check(eng.lib.sr3_dev_malloc(eng.ctx, self.n * 4, C.byref(p)))
        self.ptr = p.value

    def upload(self, a) -> "DeviceBuffer":
        h = _host_f32(a).ravel()
        assert h.size == self.n, (h.size, self.n)
        _lib.check(self.eng.lib.sr3_memcpy_h2d(self.eng.ctx, self.ptr, h.ctypes.data, h.nbytes))
        return self

    def download(self, shape=None) -> np.ndarray:
        h = np.empty(self.n, dtype=np.float32)
        _lib.check(self.eng.lib.sr3_memcpy_d2h(self.eng.ctx, h.ctypes.data, self.ptr, h.nbytes))
        return h.reshape(shape) if shape is not None else h

    def free(self):
        if self.ptr and self.eng.ctx:
            _lib.check(self.eng.lib.sr3_dev_free(self.eng.ctx, self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


PRECISIONS = {"f32": 0, "f16x3": 1, "f16f8": 2}
SPLIT_KINDS = ("none", "reduce", "inplace", "inplace_halo")


def conv_plan(B: int, H: int, W: int, Cin: int, Cout: int, ks: int = 3, stride: int = 1, up2: int = 0,
              precision: str = "f32", stats: bool = False, plan_batch: Optional[int] = None) -> dict:
    """The library's dispatch plan for one conv shape (H x W input pixels, Cin a multiple of 32) with every scratch buffer
    offered; stats: the conv also produces fused GroupNorm statistics (the UNet's convs do, op_conv2d does not).
    plan_batch (a positive int): the plan of an engine in the batch-invariant mode with that planning batch
    (sr3_conv_plan_invariant) — the same for every B but for the two buffer sizes. Host only: needs no GPU
    and no context."""
    v = (C.c_int64 * 12)()
    name = C.create_string_buffer(32)
    if plan_batch:
        _lib.check(_lib.load().sr3_conv_plan_invariant(int(plan_batch), B, H, W, Cin, Cout, ks, stride, up2, PRECISIONS[precision],
                                                       int(bool(stats)), v, name, len(name)))
    else:
        _lib.check(_lib.load().sr3_conv_plan(B, H, W, Cin, Cout, ks, stride, up2, PRECISIONS[precision], int(bool(stats)),
                                             v, name, len(name)))
    return {"kernel": name.value.decode(), "kernel_id": v[0], "tile": [v[1], v[2]], "split": SPLIT_KINDS[v[3]], "splits": v[4],
            "phases": v[5], "part_floats": v[6], "needs_counters": bool(v[7]), "stats_slices": v[8],
            "wino_ws_floats": v[9], "needs_wino_frag": bool(v[10]), "f8": bool(v[11])}


def conv_plan_invariant_max_batch(plan_batch: int, H: int, W: int, Cin: int, Cout: int, ks: int = 3, stride: int = 1,
                                  up2: int = 0, precision: str = "f32", stats: bool = False) -> int:
    """The largest batch the batch-invariant plan of this conv holds for under `plan_batch` (the arrival counters of an
    in-place split-K, 32-bit offsets, tensors below 4 GiB; at most 65535): Engine.max_batch is the smallest over a UNet's
    convs while the mode is on. Host only."""
    n = int(_lib.load().sr3_conv_plan_invariant_max_batch(int(plan_batch), H, W, Cin, Cout, ks, stride, up2, PRECISIONS[precision],
                                                          int(bool(stats))))
    _lib.check(min(n, 0))
    return n


def gn_res1x1_gate(B: int, H: int, W: int, C0: int, C1: int, Cout: int, precision: str = "f32", has_res: bool = True,
                   direct: bool = True, raw_wanted: bool = False, in_split: bool = False, mode: int = 2) -> dict:
    """The library's decision for one ResnetBlock at H x W pixels: does block1's GroupNorm + Swish pass over x (C0) ‖ skip
    (C1) also multiply the block's 1x1 res_conv (sr3_gn_res1x1_gate)? valid: the rules hold; tuned: the level and block
    count are adopted; takes: what this process launches (the two environment switches included). Host only: needs no GPU
    and no context — and therefore the DEFAULT plan's answer: an engine in the batch-invariant mode counts its planning
    batch in place of B."""
    flags = (1 if has_res else 0) | (2 if direct else 0) | (4 if raw_wanted else 0) | (8 if in_split else 0)
    r = int(_lib.load().sr3_gn_res1x1_gate(B, H, W, C0, C1, Cout, PRECISIONS[precision], flags, mode))
    _lib.check(min(r, 0))
    return {"valid": bool(r & 1), "tuned": bool(r & 2), "takes": bool(r & 4)}


def lr_operators(l: int, r: int) -> Tuple[np.ndarray, np.ndarray]:
    """(A [l,r], P [r,l]) in float64 for one axis of the r -> l bicubic resample: A the real weights of Pillow's
    precompute_coeffs with rows normalised, P = A^T (A A^T)^-1 (sr3_lr_operators_host). Host only: needs
    no GPU and no context."""
    A, P = np.empty((int(l), int(r)), dtype=np.float64), np.empty((int(r), int(l)), dtype=np.float64)
    _lib.check(_lib.load().sr3_lr_operators_host(int(l), int(r), A.ctypes.data, P.ctypes.data))
    return A, P


class Engine:
    def __init__(self, cfg: UNetConfig, device: int = 0):
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = int(device)
        ctx = C.c_void_p()
        _lib.check(self.lib.sr3_create(C.byref(_cfg_struct(cfg)), self.device, C.byref(ctx)))
        self.ctx = ctx
        self.T = 0

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.sr3_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- buffers -------------------------------------------------------------------------
    def buffer(self, n_floats: int) -> DeviceBuffer:
        return DeviceBuffer(self, n_floats)

    def to_device(self, a) -> DeviceBuffer:
        h = _host_f32(a)
        return DeviceBuffer(self, h.size).upload(h)

    def set_stream(self, stream_handle: Optional[int]):
        _lib.check(self.lib.sr3_set_stream(self.ctx, stream_handle or None))

    PRECISIONS = PRECISIONS

    def conv_plan(self, B: int, H: int, W: int, Cin: int, Cout: int, ks: int = 3, stride: int = 1, up2: int = 0,
                  precision: Optional[str] = None, stats: bool = False, plan_batch: Optional[int] = None) -> dict:
        """conv_plan() in this engine's precision (or the one named) and under its batch-invariant setting (or the planning
        batch named)."""
        return conv_plan(B, H, W, Cin, Cout, ks, stride, up2, precision or getattr(self, "precision", "f32"), stats,
                         self.batch_invariant() if plan_batch is None else plan_batch)

    def set_batch_invariant(self, plan_batch: int = 64):
        """Batch-invariant mode. plan_batch > 0: every dispatch decision counts `plan_batch` images in
        place of the call's batch, so the bytes of one image depend on its own inputs and on plan_batch alone — not on the
        batch size, the row, the other rows, the chunking or the rank split. 0 / False: off (the default); True: 64, the
        facade's default planning batch. Changing the
        value frees the workspace and the captured steps; refused while a row session is open. max_batch()
        reports the mode's maximum batch while it is on."""
        if isinstance(plan_batch, bool) or plan_batch is None:
            plan_batch = 64 if plan_batch else 0
        _lib.check(self.lib.sr3_set_batch_invariant(self.ctx, int(plan_batch)))

    def batch_invariant(self) -> int:
        """The planning batch of the batch-invariant mode, 0 = off."""
        n = int(self.lib.sr3_get_batch_invariant(self.ctx))
        _lib.check(min(n, 0))
        return n

    def conv_f8_supported(self, B: int, H: int, W: int, Cout: int, Cin: int) -> bool:
        """Does the 'f16f8' mode run a 3x3 / stride-1 conv of this shape with fp8 correction products on THIS engine —
        under its planning batch while the batch-invariant mode is on (sr3_conv_f8_supported itself describes the
        default plan)?"""
        P = self.batch_invariant()
        if P:
            return bool(conv_plan(B, H, W, Cin, Cout, 3, 1, 0, "f16f8", False, P)["f8"])
        return bool(self.lib.sr3_conv_f8_supported(B, H, W, Cout, Cin))

    def set_precision(self, name: str):
        """'f32': exact fp32 MFMA (default). 'f16x3': split-f16 operands, fp32-equivalent accuracy. 'f16f8': f16x3 with
        the correction products of the MFMA-bound convs on the fp8 matrix path (~6e-5 from the reference, faster)."""
        _lib.check(self.lib.sr3_set_precision(self.ctx, self.PRECISIONS[name]))
        self.precision = name

    def set_range_policy(self, strict: bool):
        """split-f16 mode, activation beyond the fp16 range: strict=True fails the call; False (default)
        finishes it in exact f32 and warns (`Sr3RangeWarning`)."""
        _lib.check(self.lib.sr3_set_range_policy(self.ctx, 1 if strict else 0))

    def fallback_calls(self) -> int:
        return int(self.lib.sr3_fallback_calls(self.ctx))

    def gn_wino_passes(self) -> int:
        """GroupNorm apply passes launched (or captured into a graph) in the form that writes the Winograd input transform of
        the conv behind them, since the engine was created; 0 under SR3_NO_GN_WINO=1 and outside the f32 mode."""
        return int(self.lib.sr3_gn_wino_passes(self.ctx))

    def wino_gemm_out_launches(self) -> int:
        """Three-pass Winograd convs this engine launched (or captured into a graph) in the form that runs the position GEMMs
        and the output transform in one kernel; 0 under SR3_NO_WINO_GEMM_OUT=1 and outside the f32 mode."""
        return int(self.lib.sr3_wino_gemm_out_launches(self.ctx))

    def conv_in_f32_launches(self) -> int:
        """Forwards this engine launched (or captured into a graph; op_conv_in_f32 calls included) whose first conv ran on
        conv_in_f32_kernel; 0 under SR3_NO_CONV_IN_F32=1 and outside the f32 mode."""
        return int(self.lib.sr3_conv_in_f32_launches(self.ctx))

    def up2_wino_launches(self) -> int:
        """Upsample convs this engine launched (or captured into a graph) as sub-pixel Winograd F(2x2, 2x2); 0 under
        SR3_NO_UP2_WINO=1 and outside the f32 mode."""
        return int(self.lib.sr3_up2_wino_launches(self.ctx))

    def wino_fused_rows_launches(self) -> int:
        """Three-pass Winograd convs this engine launched (or captured into a graph) on the one-pass kernel with 2 | 4 tile rows
        per block (the 32x32 and 16x16 levels); 0 under SR3_NO_WINO_FUSED_ROWS=1 and outside the f32 mode."""
        return int(self.lib.sr3_wino_fused_rows_launches(self.ctx))

    def gn_res1x1_launches(self) -> int:
        """block1 GroupNorm apply passes this engine launched (or captured into a graph) together with the block's 1x1
        res_conv, op_gn_res1x1 calls included; 0 under SR3_NO_GN_RES1X1=1 and outside the f32 mode."""
        return int(self.lib.sr3_gn_res1x1_launches(self.ctx))

    def step_graph_captures(self) -> int:
        """Sampler steps this engine captured into a graph since it was created: a step whose form and baked-in values
        were seen before replays its graph and adds nothing; 0 under SR3_NO_GRAPH=1."""
        return int(self.lib.sr3_step_graph_captures(self.ctx))

    def replay_calls(self) -> int:
        """Calls finished after replaying work whose in-place split-K wait had given up (SR3_OK_REPLAYED)."""
        return int(self.lib.sr3_replay_calls(self.ctx))

    def synchronize(self):
        _lib.check(self.lib.sr3_synchronize(self.ctx))

    def wait_for_stream(self, stream_handle: Optional[int]):
        """The library's stream waits (on the device) for the work enqueued so far on `stream_handle`."""
        _lib.check(self.lib.sr3_wait_for_stream(self.ctx, stream_handle or None))

    def stream_wait_for_engine(self, stream_handle: Optional[int]):
        """`stream_handle` waits (on the device) for the library work enqueued so far."""
        _lib.check(self.lib.sr3_stream_wait_for_ctx(self.ctx, stream_handle or None))

    def device_bytes(self) -> int:
        return int(self.lib.sr3_device_bytes(self.ctx))

    # ---- weights -------------------------------------------------------------------------
    def param_list(self) -> List[Tuple[str, Tuple[int, ...]]]:
        n = self.lib.sr3_num_params(self.ctx)
        out = []
        name = C.create_string_buffer(192)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(n):
            _lib.check(self.lib.sr3_param_info(self.ctx, i, name, 192, shape, C.byref(nd)))
            out.append((name.value.decode(), tuple(int(shape[k]) for k in range(nd.value))))
        return out

    def load_weight(self, name: str, host_array) -> None:
        h = _host_f32(host_array)
        shape = (C.c_int64 * max(1, h.ndim))(*h.shape)
        _lib.check(self.lib.sr3_load_weight(self.ctx, name.encode(), h.ctypes.data, shape, h.ndim))

    def load_state_dict(self, sd: Dict[str, np.ndarray], prefix: str = "") -> None:
        """Loads every parameter the library declares from `sd[prefix + name]` (numpy arrays)."""
        for name, _ in self.param_list():
            self.load_weight(name, sd[prefix + name])

    WEIGHT_LAYOUTS = {"plain": 0, "split": 1, "f8": 2, "wino": 3, "wino_frag": 4, "conv_in": 5, "final_mfma": 6,
                      "final_valu": 7, "fused_bias": 8, "ident": 9, "up_wino_frag": 10}

    def load_weights_device(self, items: Sequence[Tuple[str, object]]) -> int:
        """Refreshes the listed parameters from tensors that live on this engine's device: `items` is a list of
        (name, tensor), the tensors fp32, contiguous, in the reference layout (anything with `data_ptr()`, `shape`,
        `dtype`, `device`, `is_contiguous()`: torch tensors). Every kernel layout is rebuilt on the device with one host
        synchronisation for the whole list, and is the same bytes as `load_weight` makes. Returns the number refreshed."""
        items = list(items)
        n = len(items)
        if n == 0:
            return 0
        names = (C.c_char_p * n)()
        ptrs = (C.c_void_p * n)()
        shapes = (C.c_int64 * (4 * n))()
        ndims = (C.c_int * n)()
        for i, (name, t) in enumerate(items):
            dev = t.device
            if (str(t.dtype) != "torch.float32" or not t.is_contiguous() or dev.type != "cuda"
                    or (dev.index is not None and dev.index != self.device)):
                raise _lib.Sr3Error(f"{name}: load_weights_device needs a contiguous fp32 tensor on device {self.device} "
                                    f"(got {t.dtype}, {dev}); use load_weight for anything else")
            if len(t.shape) > 4:
                raise _lib.Sr3Error(f"{name}: more than 4 dims")
            names[i] = name.encode()
            ptrs[i] = t.data_ptr()
            ndims[i] = len(t.shape)
            for k, d in enumerate(t.shape):
                shapes[4 * i + k] = int(d)
        rc = self.lib.sr3_load_weights_dev(self.ctx, n, names, ptrs, shapes, ndims)
        _lib.check(min(rc, 0))
        return int(rc)

    def read_weight_layout(self, name: str, layout) -> Optional[np.ndarray]:
        """The bytes (uint8 array) of one kernel layout the engine keeps of a parameter (`WEIGHT_LAYOUTS`: a name or an
        id); None when the parameter has no such layout. For tests and tools."""
        lid = self.WEIGHT_LAYOUTS[layout] if isinstance(layout, str) else int(layout)
        size = int(self.lib.sr3_read_weight_layout(self.ctx, name.encode(), lid, None, 0))
        _lib.check(min(size, 0))
        if size == 0:
            return None
        out = np.empty(size, dtype=np.uint8)
        _lib.check(min(int(self.lib.sr3_read_weight_layout(self.ctx, name.encode(), lid, out.ctypes.data, size)), 0))
        return out

    def weight_unscale(self, name: str) -> float:
        """2^-k of the parameter's split-f16 copy (1.0 for parameters without one)."""
        v = float(self.lib.sr3_weight_unscale(self.ctx, name.encode()))
        if v == 0.0:
            _lib.check(-1)
        return v

    def weights_missing(self) -> int:
        return int(self.lib.sr3_weights_missing(self.ctx))

    # ---- UNet forward ---------------------------------------------------------------------
    def unet_forward(self, x_ptr: int, nl_ptr: int, B: int, H: int, W: int, out_ptr: int) -> None:
        _lib.check(self.lib.sr3_unet_forward(self.ctx, x_ptr, nl_ptr, B, H, W, out_ptr))

    # ---- denoising loss (GaussianDiffusion.p_losses, evaluation only) -----------
    LOSS_TYPES = {"l1": 0, "l2": 1}

    def denoise_loss(self, hr_ptr: int, cond_ptr: Optional[int], N: int, row_offset: int, level_ptr: int, s_ptr: int,
                     B: int, H: int, W: int, per_image_ptr: int, loss_type: str = "l1", noise_ptr: Optional[int] = None,
                     noise_per_source: bool = False, seed: int = 0, image_offset: int = 0,
                     x_noisy_ptr: Optional[int] = None, eps_ptr: Optional[int] = None) -> None:
        """Row b noises hr[(row_offset + b) % N] at level[b] (s[b] = float32 sqrt(1 - level^2)), runs the UNet on
        cat(cond, x_noisy) and leaves the summed |noise - eps| ('l1') or (noise - eps)^2 ('l2') of the row as fp64 at
        per_image_ptr [B] (sr3_denoise_loss; stream-ordered). noise_ptr None: device Philox (seed, image_offset + b)."""
        _lib.check(self.lib.sr3_denoise_loss(self.ctx, hr_ptr, cond_ptr or None, N, row_offset, level_ptr, s_ptr,
                                             noise_ptr or None, 1 if noise_per_source else 0, seed, image_offset, B, H, W,
                                             self.LOSS_TYPES[loss_type], per_image_ptr, x_noisy_ptr or None, eps_ptr or None))

    def q_sample(self, hr_ptr: int, N: int, row_offset: int, level_ptr: int, s_ptr: int, B: int, C: int, H: int, W: int,
                 out_ptr: int, noise_ptr: Optional[int] = None, noise_per_source: bool = False, seed: int = 0,
                 image_offset: int = 0) -> None:
        """x_noisy = level * hr + s * noise of the same rows into out_ptr [B,C,H,W] (sr3_op_q_sample; stream-ordered)."""
        _lib.check(self.lib.sr3_op_q_sample(self.ctx, hr_ptr, N, row_offset, level_ptr, s_ptr, noise_ptr or None,
                                            1 if noise_per_source else 0, seed, image_offset, B, C, H, W, out_ptr))

    # ---- sampler --------------------------------------------------------------------------
    def set_schedule(self, bufs: Dict[str, np.ndarray]) -> None:
        nl = _host_f32(bufs["noise_level"])
        T = nl.size - 1
        arrs = [nl] + [_host_f32(bufs[k]) for k in (
            "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
            "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")]
        for a in arrs[1:]:
            assert a.size == T
        _lib.check(self.lib.sr3_set_schedule(self.ctx, T, *[a.ctypes.data for a in arrs]))
        self.T = T

    def set_sampler_schedule(self, tables: Dict) -> None:
        """A sampler's per-step tables (samplers.sampler_tables): S steps from then on. "ddpm" tables go through
        sr3_set_schedule, the reference's loop exactly."""
        S = int(tables["S"])
        if tables.get("kind") == "ddpm":
            self.set_schedule({"noise_level": tables["noise_level"], "sqrt_recip_alphas_cumprod": tables["a"],
                               "sqrt_recipm1_alphas_cumprod": tables["b"], "posterior_log_variance_clipped": tables["logvar"],
                               "posterior_mean_coef1": tables["c1"], "posterior_mean_coef2": tables["c2"]})
            return
        nl = _host_f32(tables["noise_level"])
        arrs = [_host_f32(tables[k]) for k in ("a", "b", "c1", "c2", "c3", "sigma")]
        if nl.size != S + 1 or any(a.size != S for a in arrs):
            raise ValueError("sampler tables: noise_level needs S+1 entries, the coefficients S")
        _lib.check(self.lib.sr3_set_sampler_schedule(self.ctx, S, nl.ctypes.data, *[a.ctypes.data for a in arrs],
                                                     1 if tables["uses_history"] else 0))
        self.T = S

    def num_frames(self, start_step: Optional[int] = None) -> int:
        """Frames one sampling call writes: after every step i with i % (1 | S // 10) == 0, over all S steps or, with
        start_step, over the start_step steps of a warm start (sr3_num_frames_from)."""
        if start_step is None:
            n = self.lib.sr3_num_frames(self.ctx)
        else:
            n = self.lib.sr3_num_frames_from(self.ctx, int(start_step))
        if n < 0:
            _lib.check(n)
        return n

    def max_batch(self, H: int, W: int) -> int:
        """Largest batch one sample / unet_forward call takes at H x W (4 GiB per activation tensor)."""
        n = self.lib.sr3_max_batch(self.ctx, int(H), int(W))
        if n < 0:
            _lib.check(n)
        return n

    def sample(self, cond_ptr: Optional[int], B: int, H: int, W: int, out_ptr: int,
               noise_ptr: Optional[int] = None, seed: int = 0, image_offset: int = 0,
               frames_ptr: Optional[int] = None, init_ptr: Optional[int] = None, start_step: Optional[int] = None,
               noised: bool = True) -> None:
        """sr3_sample; with init_ptr ([B,C,H,W]) the warm start sr3_sample_from: the last start_step steps (None: all S)
        from that image, noised to noise_level[start_step] first unless noised is False. noise_ptr is then
        [start_step,B,C,H,W]."""
        if init_ptr is None:
            if start_step is not None:
                raise ValueError("start_step needs init_ptr: the image the loop starts from")
            _lib.check(self.lib.sr3_sample(self.ctx, cond_ptr or None, B, H, W, noise_ptr or None,
                                           seed, image_offset, out_ptr, frames_ptr or None))
            return
        s0 = self.T if start_step is None else int(start_step)
        _lib.check(self.lib.sr3_sample_from(self.ctx, cond_ptr or None, B, H, W, init_ptr, s0, 1 if noised else 0,
                                            noise_ptr or None, seed, image_offset, out_ptr, frames_ptr or None))

    def sample_begin(self, cond_ptr, B, H, W, init_noise_ptr=None, seed=0, image_offset=0):
        _lib.check(self.lib.sr3_sample_begin(self.ctx, cond_ptr or None, B, H, W,
                                             init_noise_ptr or None, seed, image_offset))

    def sample_begin_from(self, cond_ptr, B, H, W, init_ptr, start_step, noised=True, noise0_ptr=None, seed=0,
                          image_offset=0):
        """Step API of the warm start (sr3_sample_begin_from): the state before step start_step - 1, from init_ptr."""
        _lib.check(self.lib.sr3_sample_begin_from(self.ctx, cond_ptr or None, B, H, W, init_ptr, int(start_step),
                                                  1 if noised else 0, noise0_ptr or None, seed, image_offset))

    def sample_step(self, t: int, noise_ptr: Optional[int] = None):
        _lib.check(self.lib.sr3_sample_step(self.ctx, int(t), noise_ptr or None))

    def sample_end(self, out_ptr: int):
        _lib.check(self.lib.sr3_sample_end(self.ctx, out_ptr))

    def range_check(self) -> None:
        """Raises Sr3Error if a split-f16 store left the fp16 range since the last check."""
        _lib.check(self.lib.sr3_range_check(self.ctx))

    # ---- rolling batch: every row at its own position ---------------------------
    def rows_begin(self, B: int, H: int, W: int, seed: int = 0) -> None:
        """Opens a row session of B slots at H x W, all idle (sr3_rows_begin). Uses the sampler, arithmetic and dynamic
        threshold set on the engine; refuses the per-call LR consistency (set_lr_consistency: a session holds single rows,
        rows_lr_consistency), the feature cache and Dropout sampling. Every step runs at batch B whatever is live: a
        row's result is that of its row in a uniform call of B images. (In the batch-invariant mode rows_step takes a
        `batch` below B and rows_move compacts the live rows: the step then costs what `batch` images cost.)"""
        _lib.check(self.lib.sr3_rows_begin(self.ctx, int(B), int(H), int(W), int(seed) & (2 ** 64 - 1)))
        self._rows_slots = int(B)

    def rows_lr_consistency(self, lh: int, lw: int) -> None:
        """Arms the open session for LR images of lh x lw (sr3_rows_lr_consistency): right after rows_begin, before the
        first rows_admit. The rows admitted with an `lr` are then held to it, the others are not."""
        _lib.check(self.lib.sr3_rows_lr_consistency(self.ctx, int(lh), int(lw)))

    def rows_admit(self, row: int, cond_ptr: int, image_id: int, init_ptr: Optional[int] = None,
                   start_step: Optional[int] = None, noised: bool = True, noise0_ptr: Optional[int] = None,
                   lr: Optional[int] = None, lr_strength: float = 1.0) -> None:
        """One request into idle slot `row` (sr3_rows_admit): cond [Cc,H,W]; init_ptr None: from the start noise at the
        top; init [C,H,W] with start_step (None: S): the warm start, noised to noise_level[start_step] unless noised is
        False. noise0: the start noise / the z of q_sample, [C,H,W] (None: Philox draw 0 of image_id). lr: the device
        address of the row's LR image, fp32 [C,lh,lw] in [-1,1], in an armed session (sr3_rows_admit_lr; the library
        copies it), held at lr_strength in [0, 1]; None: the row is not held."""
        if init_ptr is None and start_step is not None and int(start_step) != self.T:
            raise ValueError("start_step needs init_ptr: the image the row starts from")
        s0 = self.T if start_step is None else int(start_step)
        if lr is None:
            _lib.check(self.lib.sr3_rows_admit(self.ctx, int(row), cond_ptr, init_ptr or None, s0, 1 if noised else 0,
                                               noise0_ptr or None, int(image_id) & (2 ** 64 - 1)))
            return
        _lib.check(self.lib.sr3_rows_admit_lr(self.ctx, int(row), cond_ptr, init_ptr or None, s0, 1 if noised else 0,
                                              noise0_ptr or None, int(image_id) & (2 ** 64 - 1), lr, float(lr_strength)))

    def rows_frames(self, row: int, frames_ptr: int, capacity: int) -> None:
        """After rows_admit, before the row's first step: the row writes its frames, [n,C,H,W] with n = num_frames(its
        start_step), to frames_ptr (sr3_rows_frames) — those of its row in the uniform call with frames."""
        _lib.check(self.lib.sr3_rows_frames(self.ctx, int(row), frames_ptr, int(capacity)))

    def rows_step(self, noise_ptrs: Optional[Sequence[Optional[int]]] = None, batch: Optional[int] = None) -> int:
        """One step of every live row at its own position (sr3_rows_step); noise_ptrs: one device address (or None)
        per slot, the [C,H,W] draw of that row's step. Returns the number of rows stepped (0: nothing was launched).
        batch (batch-invariant mode only): the step runs over slots [0, batch) alone (sr3_rows_step_batch) and costs
        what `batch` images cost; every live row must sit below it (rows_move). None: the whole session."""
        arr = None
        if noise_ptrs is not None:
            # (the library reads one entry per slot of the session)
            if len(noise_ptrs) != getattr(self, "_rows_slots", -1):
                raise ValueError(f"noise_ptrs needs one entry per slot of the session ({getattr(self, '_rows_slots', 0)}), "
                                 f"got {len(noise_ptrs)}")
            arr = (C.c_void_p * len(noise_ptrs))(*[p or None for p in noise_ptrs])
        if batch is None:
            n = int(self.lib.sr3_rows_step(self.ctx, arr))
        else:
            n = int(self.lib.sr3_rows_step_batch(self.ctx, arr, int(batch)))
        _lib.check(min(n, 0))
        return n

    def rows_move(self, src: int, dst: int) -> None:
        """Moves live slot `src` into idle slot `dst` (sr3_rows_move): state, packed copy, x0 history, LR image and the
        row's position, image id, strength and frames; `src` is left idle and zero. One launch, stream-ordered."""
        _lib.check(self.lib.sr3_rows_move(self.ctx, int(src), int(dst)))

    def rows_rows_run(self) -> int:
        """The sum of the batch over every row-session step this engine has launched (sr3_rows_rows_run)."""
        return int(self.lib.sr3_rows_rows_run(self.ctx))

    def read_history(self, B: int, H: int, W: int) -> np.ndarray:
        """The x0 history of the current workspace, float32 [B, C, H, W] (sr3_read_history). For tests."""
        a = np.empty((B, self.cfg.out_channel, H, W), dtype=np.float32)
        n = int(self.lib.sr3_read_history(self.ctx, a.ctypes.data))
        _lib.check(min(n, 0))
        assert n == a.size, (n, a.shape)
        return a

    def rows_position(self, row: int) -> int:
        """Steps left for the slot, -1 for an idle one (sr3_rows_position)."""
        n = int(self.lib.sr3_rows_position(self.ctx, int(row)))
        if n < -1:
            _lib.check(-1)
        return n

    def rows_retire(self, row: int, out_ptr: int) -> None:
        """Copies a finished row to out [C,H,W] and frees its slot (sr3_rows_retire)."""
        _lib.check(self.lib.sr3_rows_retire(self.ctx, int(row), out_ptr))

    def rows_drop(self, row: int) -> None:
        _lib.check(self.lib.sr3_rows_drop(self.ctx, int(row)))

    def rows_end(self) -> None:
        _lib.check(self.lib.sr3_rows_end(self.ctx))

    def philox_normal(self, seed: int, image: int, draw: int, n: int) -> np.ndarray:
        buf = self.buffer(n)
        _lib.check(self.lib.sr3_philox_normal(self.ctx, seed, image, draw, n, buf.ptr))
        return buf.download()

    def philox_normal_into(self, seed: int, image: int, draw: int, n: int, out_ptr: int) -> None:
        """Device Philox stream of (seed, image, draw) written to a device buffer (stream-ordered)."""
        _lib.check(self.lib.sr3_philox_normal(self.ctx, seed, image, draw, n, out_ptr))

    # ---- low-resolution consistency --------------------------------------------
    def set_lr_consistency(self, lr_ptr: Optional[int], N: int = 0, lh: int = 0, lw: int = 0, row_offset: int = 0,
                           strength: float = 1.0) -> None:
        """While set, every sampling step projects its x0 prediction onto the images whose bicubic downsample is the LR
        input: batch row b is held to lr[(row_offset + b) % N], lr fp32 [N,C,lh,lw] in [-1,1] on the device (it must
        outlive the calls). None or strength 0 turns it off (sr3_set_lr_consistency). Set before sample / sample_begin."""
        _lib.check(self.lib.sr3_set_lr_consistency(self.ctx, lr_ptr or None, int(N), int(lh), int(lw), int(row_offset),
                                                   float(strength) if lr_ptr else 0.0))

    LR_FORMS = {"auto": 0, "lds": 1, "scratch": 2}

    def lr_project(self, x_ptr: int, B: int, C_: int, H: int, W: int, lr_ptr: int, N: int, lh: int, lw: int,
                   row_offset: int = 0, strength: float = 1.0, form: str = "auto") -> None:
        """X <- X + strength * P_v (Y - A_v X A_h^T) P_h^T in place on x fp32 [B,C,H,W] (sr3_op_lr_project;
        stream-ordered). form: 'auto' | 'lds' (one block per plane) | 'scratch' (one launch per stage)."""
        _lib.check(self.lib.sr3_op_lr_project(self.ctx, x_ptr, B, C_, H, W, lr_ptr, N, lh, lw, int(row_offset), float(strength),
                                              self.LR_FORMS[form]))

    def lr_project_rows(self, x_ptr: int, B: int, C_: int, H: int, W: int, lr_ptr: int, lh: int, lw: int,
                        strengths: Sequence[float], live: Sequence[int], form: str = "auto") -> None:
        """The rows form of the projection (sr3_op_lr_project_rows): row b of x [B,C,H,W] against lr [B,C,lh,lw] at
        strengths[b] where live[b] and strengths[b] != 0; every other row is left alone."""
        st = np.ascontiguousarray(strengths, dtype=np.float32)
        lv = np.ascontiguousarray(live, dtype=np.int32)
        if st.shape != (B,) or lv.shape != (B,):
            raise ValueError(f"strengths and live need one entry per row ({B})")
        _lib.check(self.lib.sr3_op_lr_project_rows(self.ctx, x_ptr, B, C_, H, W, lr_ptr, lh, lw, st.ctypes.data,
                                                   lv.ctypes.data, self.LR_FORMS[form]))

    def lr_project_rows_np(self, x, lr, strengths, live, form: str = "auto") -> np.ndarray:
        """numpy convenience: x [B,C,H,W], lr [B,C,lh,lw] -> x with its live, held rows projected."""
        x, lr = _host_f32(x), _host_f32(lr)
        B, C_, H, W = x.shape
        _, _, lh, lw = lr.shape
        dx, dl = self.to_device(x), self.to_device(lr)
        self.lr_project_rows(dx.ptr, B, C_, H, W, dl.ptr, lh, lw, strengths, live, form)
        out = dx.download(x.shape)
        dx.free(); dl.free()
        return out

    def lr_residual(self, img_ptr: int, B: int, C_: int, H: int, W: int, lr_ptr: int, N: int, lh: int, lw: int,
                    row_offset: int, sumsq_ptr: int, maxabs_ptr: int) -> None:
        """Per row b: sum (A img - y)^2 -> fp64 [B] at sumsq_ptr, max |A img - y| -> fp32 [B] at maxabs_ptr, against
        lr[(row_offset + b) % N] (sr3_lr_residual; stream-ordered)."""
        _lib.check(self.lib.sr3_lr_residual(self.ctx, img_ptr, B, C_, H, W, lr_ptr, N, lh, lw, int(row_offset), sumsq_ptr,
                                            maxabs_ptr))

    def lr_project_np(self, x, lr, row_offset: int = 0, strength: float = 1.0, form: str = "auto") -> np.ndarray:
        """numpy convenience: x [B,C,H,W], lr [N,C,lh,lw] -> the projected x."""
        x, lr = _host_f32(x), _host_f32(lr)
        B, C_, H, W = x.shape
        N, _, lh, lw = lr.shape
        dx, dl = self.to_device(x), self.to_device(lr)
        self.lr_project(dx.ptr, B, C_, H, W, dl.ptr, N, lh, lw, row_offset, strength, form)
        out = dx.download(x.shape)
        dx.free(); dl.free()
        return out

    def lr_residual_np(self, img, lr, row_offset: int = 0) -> Dict[str, np.ndarray]:
        """numpy convenience: {"sumsq": float64 [B], "max_abs": float32 [B]} of img [B,C,H,W] against lr [N,C,lh,lw]."""
        img, lr = _host_f32(img), _host_f32(lr)
        B, C_, H, W = img.shape
        N, _, lh, lw = lr.shape
        di, dl = self.to_device(img), self.to_device(lr)
        ds, dm = self.buffer(2 * B), self.buffer(B)
        self.lr_residual(di.ptr, B, C_, H, W, dl.ptr, N, lh, lw, row_offset, ds.ptr, dm.ptr)
        out = {"sumsq": ds.download().view(np.float64).copy(), "max_abs": dm.download()}
        for b in (di, dl, ds, dm):
            b.free()
        return out

    # ---- feature cache: deep UNet features reused across sampler steps ---------------
    def set_feature_cache(self, interval: Optional[int] = None, depth: int = 1) -> None:
        """While set (interval > 1), only every interval-th step of a sampling call runs the whole UNet; the steps between
        run its `depth` top resolution levels on the deep feature of the last whole step (DeepCache; sr3_set_feature_cache).
        interval None (or <= 1) turns it off. depth is 1 .. len(channel_mults) - 1."""
        _lib.check(self.lib.sr3_set_feature_cache(self.ctx, 0 if interval is None else int(interval), int(depth)))

    def feature_cache_steps(self) -> Tuple[int, int]:
        """(whole, shallow) steps of the last sampling call, replayed ones included (sr3_feature_cache_steps)."""
        w, s = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.sr3_feature_cache_steps(self.ctx, C.byref(w), C.byref(s)))
        return int(w.value), int(s.value)

    def unet_forward_cached(self, x_ptr: int, nl_ptr: int, B: int, H: int, W: int, depth: int, out_ptr: int) -> None:
        _lib.check(self.lib.sr3_unet_forward_cached(self.ctx, x_ptr, nl_ptr, B, H, W, int(depth), out_ptr))

    # ---- train-mode Dropout ---------------------------------------------------
    # ---- dynamic thresholding of the x0 prediction ------------------------------
    def set_dynamic_threshold(self, ratio: Optional[float] = None, max_value: Optional[float] = None) -> None:
        """While set, every sampling step replaces the static clamp of its x0 prediction by clamp(x0, -s, s) / s with s the
        per-image `ratio`-quantile of |x0|, at least 1 and at most max_value (None: no bound). ratio None (or <= 0) turns it
        off (sr3_set_dynamic_threshold). Set before sample / sample_begin."""
        if ratio is None:
            _lib.check(self.lib.sr3_set_dynamic_threshold(self.ctx, 0.0, 1.0))
            return
        _lib.check(self.lib.sr3_set_dynamic_threshold(self.ctx, float(ratio), float("inf") if max_value is None else float(max_value)))

    def dynamic_threshold_launches(self) -> int:
        """Sampler steps issued in the thresholded form since the engine was created (sr3_dynamic_threshold_launches)."""
        return int(self.lib.sr3_dynamic_threshold_launches(self.ctx))

    def abs_quantile(self, x_ptr: int, B: int, n: int, ratio: float, max_value: Optional[float], lo_ptr: Optional[int],
                     hi_ptr: Optional[int], s_ptr: Optional[int]) -> None:
        """Per row of x fp32 [B,n]: the two order statistics of |x| around the ratio-quantile and s (sr3_op_abs_quantile;
        stream-ordered)."""
        _lib.check(self.lib.sr3_op_abs_quantile(self.ctx, x_ptr, int(B), int(n), float(ratio),
                                                float("inf") if max_value is None else float(max_value), lo_ptr or None,
                                                hi_ptr or None, s_ptr or None))

    def dynamic_threshold(self, x_ptr: int, B: int, n: int, ratio: float, max_value: Optional[float] = None,
                          s_ptr: Optional[int] = None) -> None:
        """x <- clamp(x, -s, s) / s in place on x fp32 [B,n] (sr3_op_dynamic_threshold; stream-ordered)."""
        _lib.check(self.lib.sr3_op_dynamic_threshold(self.ctx, x_ptr, int(B), int(n), float(ratio),
                                                     float("inf") if max_value is None else float(max_value), s_ptr or None))

    def op_abs_quantile(self, x, ratio: float, max_value: Optional[float] = None, misalign: bool = False) -> Dict[str, np.ndarray]:
        """numpy convenience: x [B, ...] -> {"lo", "hi", "s"}, fp32 [B] each. misalign: the device copy starts 4 bytes past
        a 16-byte boundary."""
        x = _host_f32(x)
        B = x.shape[0]
        n = x.size // B
        flat = x.reshape(-1)
        if misalign:
            flat = np.concatenate([np.zeros(1, np.float32), flat])
        dx, out = self.to_device(flat), self.buffer(3 * B)
        self.abs_quantile(dx.ptr + (4 if misalign else 0), B, n, ratio, max_value, out.ptr, out.ptr + 4 * B, out.ptr + 8 * B)
        r = out.download((3, B))
        dx.free(); out.free()
        return {"lo": r[0].copy(), "hi": r[1].copy(), "s": r[2].copy()}

    def op_dynamic_threshold(self, x, ratio: float, max_value: Optional[float] = None, misalign: bool = False):
        """numpy convenience: x [B, ...] -> (the thresholded x, s [B])."""
        x = _host_f32(x)
        B = x.shape[0]
        n = x.size // B
        flat = x.reshape(-1)
        if misalign:
            flat = np.concatenate([np.zeros(1, np.float32), flat])
        dx, ds = self.to_device(flat), self.buffer(B)
        self.dynamic_threshold(dx.ptr + (4 if misalign else 0), B, n, ratio, max_value, ds.ptr)
        got = dx.download()[1 if misalign else 0:].reshape(x.shape).copy()
        s = ds.download()
        dx.free(); ds.free()
        return got, s

    def set_dropout(self, enable: bool, seed: int = 0, image_offset: int = 0) -> None:
        """Train-mode Dropout (p = cfg.dropout) in front of every ResnetBlock.block2 conv, as the reference's UNet under
        .train(); off (the default) is the identity and launches exactly the kernels it always did. `seed` keys the Philox
        mask stream; `image_offset` is the global index of row 0 for unet_forward (sample / denoise_loss take their own)."""
        _lib.check(self.lib.sr3_set_dropout(self.ctx, 1 if enable else 0, int(seed) & (2 ** 64 - 1), int(image_offset)))

    def set_dropout_masks(self, masks_ptr: Optional[int], nbytes: int = 0) -> None:
        """Injected keep masks instead of Philox: one uint8 device buffer, the layers of dropout_layers() concatenated, each
        [B,C,H,W], nonzero = keep; nbytes must be dropout_mask_bytes(B, H, W). None returns to Philox. The buffer must
        outlive the calls that read it."""
        _lib.check(self.lib.sr3_set_dropout_masks(self.ctx, masks_ptr or None, int(nbytes) if masks_ptr else 0))

    def dropout_layers(self, H: int, W: int) -> List[Tuple[int, int, int]]:
        """(C, H, W) of every Dropout layer (one per ResnetBlock, execution order) for an H x W input."""
        n = C.c_int()
        _lib.check(self.lib.sr3_dropout_layers(self.ctx, int(H), int(W), C.byref(n), None))
        chw = (C.c_int * (3 * n.value))()
        _lib.check(self.lib.sr3_dropout_layers(self.ctx, int(H), int(W), C.byref(n), chw))
        return [(chw[3 * i], chw[3 * i + 1], chw[3 * i + 2]) for i in range(n.value)]

    def dropout_mask_bytes(self, B: int, H: int, W: int) -> int:
        n = int(self.lib.sr3_dropout_mask_bytes(self.ctx, int(B), int(H), int(W)))
        if n < 0:
            _lib.check(-1)
        return n

    def dropout_mask(self, seed: int, image: int, draw: int, layer: int, C_: int, H: int, W: int) -> np.ndarray:
        """The device's Philox keep mask of one image and layer as uint8 [C,H,W] (CPU twin: tests/dropout_ref.py)."""
        n = C_ * H * W
        buf = self.buffer((n + 3) // 4)
        _lib.check(self.lib.sr3_op_dropout_mask(self.ctx, int(seed) & (2 ** 64 - 1), int(image), int(draw), int(layer), C_, H, W,
                                                buf.ptr))
        out = np.empty(n, dtype=np.uint8)
        _lib.check(self.lib.sr3_synchronize(self.ctx))
        _lib.check(self.lib.sr3_memcpy_d2h(self.ctx, out.ctypes.data, buf.ptr, n))
        buf.free()
        return out.reshape(C_, H, W)

    def upload_bytes(self, a: np.ndarray) -> DeviceBuffer:
        """A uint8 host array in a library-owned device buffer (injected dropout masks for hosts without torch)."""
        h = np.ascontiguousarray(a, dtype=np.uint8).ravel()
        buf = self.buffer((h.size + 3) // 4)
        _lib.check(self.lib.sr3_memcpy_h2d(self.ctx, buf.ptr, h.ctypes.data, h.size))
        return buf

    # ---- pre-processing ---------------------------------------------------------------------
    def preprocess_bicubic(self, in_ptr: int, B: int, Hin: int, Win: int, Hout: int, Wout: int,
                           out_ptr: int, out_u8_ptr: Optional[int] = None) -> None:
        """uint8 HWC device images -> PIL-exact bicubic -> fp32 NCHW [-1,1] (sr3_preprocess_bicubic)."""
        _lib.check(self.lib.sr3_preprocess_bicubic(self.ctx, in_ptr, B, Hin, Win, Hout, Wout, out_ptr,
                                                   out_u8_ptr or None))

    def preprocess_bicubic_np(self, img_u8: np.ndarray, Hout: int, Wout: int):
        """numpy convenience: [B,H,W,3] uint8 -> (fp32 [B,3,Hout,Wout], uint8 [B,Hout,Wout,3])."""
        a = np.ascontiguousarray(img_u8, dtype=np.uint8)
        B, H, W, _ = a.shape
        nin, nout = a.size, B * Hout * Wout * 3
        din, dout, du8 = self.buffer((nin + 3) // 4), self.buffer(nout), self.buffer((nout + 3) // 4)
        _lib.check(self.lib.sr3_memcpy_h2d(self.ctx, din.ptr, a.ctypes.data, nin))
        self.preprocess_bicubic(din.ptr, B, H, W, Hout, Wout, dout.ptr, du8.ptr)
        u8 = np.empty(nout, dtype=np.uint8)
        _lib.check(self.lib.sr3_memcpy_d2h(self.ctx, u8.ctypes.data, du8.ptr, nout))
        return dout.download((B, 3, Hout, Wout)), u8.reshape(B, Hout, Wout, 3)

    # ---- measurement ------------------------------------------------------------------------
    # ---- post-processing ------------------------------------------------
    def postprocess_u8(self, sr_ptr: int, B: int, H: int, W: int, up: int = 224, blob: int = 112,
                       img_u8_ptr: Optional[int] = None, up_u8_ptr: Optional[int] = None,
                       images_ptr: Optional[int] = None, arcface_ptr: Optional[int] = None) -> None:
        _lib.check(self.lib.sr3_postprocess_u8(self.ctx, sr_ptr, B, H, W, up, blob, img_u8_ptr, up_u8_ptr,
                                               images_ptr, arcface_ptr))

    def postprocess_tensor_blob(self, sr_ptr: int, B: int, H: int, W: int, blob: int, arcface_ptr: int) -> None:
        _lib.check(self.lib.sr3_postprocess_tensor_blob(self.ctx, sr_ptr, B, H, W, blob, arcface_ptr))

    # ---- validation metrics ----------------------------------------------
    def metrics(self, sr_ptr: int, hr_ptr: int, B: int, N: int, row_offset: int, H: int, W: int,
                ssd_ptr: int, ssim_ptr: int) -> None:
        """Row b of sr fp32 [B,3,H,W] against hr[(row_offset + b) % N] (fp32 [N,3,H,W]): exact sum of squared uint8
        differences -> int64 [B] at ssd_ptr, SSIM -> fp64 [B] at ssim_ptr (sr3_metrics_psnr_ssim; stream-ordered)."""
        from .validation import gaussian_kernel
        taps = np.ascontiguousarray(gaussian_kernel(11, 1.5), dtype=np.float64)
        _lib.check(self.lib.sr3_metrics_psnr_ssim(self.ctx, sr_ptr, hr_ptr, B, N, row_offset, H, W,
                                                  taps.ctypes.data, ssd_ptr, ssim_ptr))

    def postprocess_np(self, sr: np.ndarray, up: int = 224, blob: int = 112) -> Dict[str, np.ndarray]:
        """Host-array convenience (tests): fp32 [B,3,H,W] -> dict(img_u8, up_u8, images, arcface,
        tensor_arcface)."""
        sr = _host_f32(sr)
        B, _, H, W = sr.shape
        S = up if up else H
        d_in = self.to_device(sr)
        sizes = {"img_u8": B * H * W * 3, "up_u8": B * S * S * 3}
        bufs = {k: self.buffer((n + 3) // 4) for k, n in sizes.items()}
        bufs["images"] = self.buffer(B * 3 * S * S)
        bufs["arcface"] = self.buffer(B * 3 * blob * blob)
        bufs["tensor_arcface"] = self.buffer(B * 3 * blob * blob)
        self.postprocess_u8(d_in.ptr, B, H, W, up, blob, bufs["img_u8"].ptr,
                            bufs["up_u8"].ptr if up else None, bufs["images"].ptr if up else None,
                            bufs["arcface"].ptr)
        self.postprocess_tensor_blob(d_in.ptr, B, H, W, blob, bufs["tensor_arcface"].ptr)
        out = {}
        for k, shape in (("img_u8", (B, H, W, 3)), ("up_u8", (B, S, S, 3))):
            if k == "up_u8" and not up:
                continue
            raw = bufs[k].download()
            out[k] = raw.view(np.uint8)[: sizes[k]].reshape(shape).copy()
        if up:
            out["images"] = bufs["images"].download((B, 3, S, S))
        out["arcface"] = bufs["arcface"].download((B, 3, blob, blob))
        out["tensor_arcface"] = bufs["tensor_arcface"].download((B, 3, blob, blob))
        for b in list(bufs.values()) + [d_in]:
            b.free()
        return out

    def profile_enable(self, on: bool):
        _lib.check(self.lib.sr3_profile_enable(self.ctx, 1 if on else 0))

    def profile_reset(self):
        _lib.check(self.lib.sr3_profile_reset(self.ctx))

    def profile_get(self) -> Dict[str, Dict[str, float]]:
        out = {}
        for i, fam in enumerate(_lib.FAMILIES):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            _lib.check(self.lib.sr3_profile_get(self.ctx, i, C.byref(ms), C.byref(n), C.byref(fl)))
            out[fam] = {"ms": ms.value, "launches": int(n.value), "flops": fl.value}
        return out

    def bench_conv(self, B, H, W, C0, C1, Cout, ks=3, stride=1, up2=0, mode=2, resid=0, chan_bias=0,
                   iters=10) -> float:
        ms, ams = C.c_float(), C.c_float()
        _lib.check(self.lib.sr3_bench_conv(self.ctx, B, H, W, C0, C1, Cout, ks, stride, up2, mode,
                                           resid, chan_bias, iters, C.byref(ms), C.byref(ams)))
        return ms.value, ams.value

    def profile_dump_csv(self, path: str):
        _lib.check(self.lib.sr3_profile_dump_csv(self.ctx, path.encode()))

    # ---- single ops (numpy in / numpy out; NHWC) --------------------------------------------
    def op_conv2d(self, x0, weight, bias=None, x1=None, stride=1, up2=False, gn_scale=None,
                  gn_shift=None, swish=False, chan_bias=None, resid=None, return_stats=False):
        """return_stats=True runs the conv as the engine runs it, with the fused GroupNorm statistics of its output offered
        (conv_plan(..., stats=True) names the kernel), and returns (out, stats): stats float64 [B, slices, Cout, 2] =
        {sum, sum of squares} per (image, slice, channel), NaN where no kernel wrote; None where the plan has none."""
        x0 = _host_f32(x0)
        B, H, W, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[-1]
        weight = _host_f32(weight)
        Cout, Cin, ks, _ = weight.shape
        assert Cin == C0 + C1
        pad = ks // 2
        Hv, Wv = (H * 2, W * 2) if up2 else (H, W)
        Ho, Wo = (Hv + 2 * pad - ks) // stride + 1, (Wv + 2 * pad - ks) // stride + 1
        d0 = self.to_device(x0)
        d1 = self.to_device(x1) if x1 is not None else None
        dsc = self.to_device(gn_scale) if gn_scale is not None else None
        dsh = self.to_device(gn_shift) if gn_shift is not None else None
        dcb = self.to_device(chan_bias) if chan_bias is not None else None
        drs = self.to_device(resid) if resid is not None else None
        out = self.buffer(B * Ho * Wo * Cout)
        bh = _host_f32(bias) if bias is not None else None
        args = (self.ctx, d0.ptr, C0, d1.ptr if d1 else None, C1, B, H, W, weight.ctypes.data,
                bh.ctypes.data if bh is not None else None, Cout, ks, stride, 1 if up2 else 0,
                dsc.ptr if dsc else None, dsh.ptr if dsh else None, 1 if swish else 0,
                dcb.ptr if dcb else None, drs.ptr if drs else None, out.ptr)
        if not return_stats:
            _lib.check(self.lib.sr3_op_conv2d(*args))
            return out.download((B, Ho, Wo, Cout))
        # (sized by the plan the call will take; the call fails if it takes another)
        slices = self.conv_plan(B, H, W, Cin, Cout, ks, stride, 1 if up2 else 0, stats=True)["stats_slices"]
        cap = max(1, B * slices * Cout * 2)
        st = self.buffer(cap * 2)
        got = C.c_int(-1)
        _lib.check(self.lib.sr3_op_conv2d_stats(*args, st.ptr, cap, C.byref(got)))
        o = out.download((B, Ho, Wo, Cout))
        if got.value == 0:
            return o, None
        assert got.value == slices, (got.value, slices)
        return o, st.download().view(np.float64).reshape(B, slices, Cout, 2)

    FUSED_SENTINEL = 0x7FC0FEED     # (a quiet NaN: what op_conv2d_fused fills `out` with before a twin-only call)

    def op_conv2d_fused(self, x0, weight, bias=None, x1=None, gn_scale=None, gn_shift=None, swish=False, chan_bias=None,
                        resid=None, in2=None, in2b=None, w2=None, b2=None, ident=False, twin=False, f32_out=True,
                        resid_split=False) -> dict:
        """The second launch of a ResnetBlock as the engine builds it (sr3_op_conv2d_fused): the 3x3 / stride 1 conv of
        op_conv2d(..., return_stats=True) plus
          in2 [B,H,W,C2a], in2b [B,H,W,C2b] (optional), w2 [Cout, C2a+C2b], b2 [Cout]: the res_conv as extra 1x1 K-steps;
          ident=True (split-f16): in2 is the block input, added through the identity K-steps (no w2);
          twin=True (split-f16): also the split-f16 twin of the output; f32_out=False: the twin alone;
          resid_split=True: resid holds the uint32 words of the split format.
        Returns a dict: out (float32 [B,H,W,Cout]; with f32_out=False the buffer as the call left it, filled with
        FUSED_SENTINEL words before), twin (uint32 words [B,H,W,Cout] or None), stats (float64 [B, slices, Cout, 2], NaN
        where no kernel wrote; None where the plan has none)."""
        def words(a):
            a = np.ascontiguousarray(a)
            return a.view(np.float32) if a.dtype == np.uint32 else _host_f32(a)

        x0 = _host_f32(x0)
        B, H, W, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[-1]
        weight = _host_f32(weight)
        Cout, Cin, ks, _ = weight.shape
        assert Cin == C0 + C1 and ks == 3
        dev = lambda a: self.to_device(_host_f32(a)) if a is not None else None
        ptr = lambda d: d.ptr if d is not None else None
        host = lambda a: _host_f32(a) if a is not None else None
        hptr = lambda a: a.ctypes.data if a is not None else None
        d0, d1, dsc, dsh, dcb, d2, d2b = dev(x0), dev(x1), dev(gn_scale), dev(gn_shift), dev(chan_bias), dev(in2), dev(in2b)
        drs = self.to_device(words(resid)) if resid is not None else None
        C2a = 0 if in2 is None else in2.shape[-1]
        C2b = 0 if in2b is None else in2b.shape[-1]
        bh, w2h, b2h = host(bias), host(w2), host(b2)
        if w2h is not None:
            assert w2h.reshape(Cout, -1).shape == (Cout, C2a + C2b), w2h.shape
        n = B * H * W * Cout
        if f32_out:
            out = self.buffer(n)
        else:
            out = self.to_device(np.full(n, self.FUSED_SENTINEL, dtype=np.uint32).view(np.float32))
        tw = self.buffer(n) if twin else None
        slices = self.conv_plan(B, H, W, Cin, Cout, 3, 1, 0, stats=True)["stats_slices"]
        cap = max(1, B * slices * Cout * 2)
        st = self.buffer(cap * 2)
        got = C.c_int(-1)
        flags = (1 if ident else 0) | (0 if f32_out else 2) | (4 if resid_split else 0)
        _lib.check(self.lib.sr3_op_conv2d_fused(
            self.ctx, d0.ptr, C0, ptr(d1), C1, B, H, W, weight.ctypes.data, hptr(bh), Cout, ptr(dsc), ptr(dsh),
            1 if swish else 0, ptr(dcb), ptr(drs), ptr(d2), C2a, ptr(d2b), C2b, hptr(w2h), hptr(b2h), flags, out.ptr,
            ptr(tw), st.ptr, cap, C.byref(got)))
        assert got.value in (0, slices), (got.value, slices)
        return {"out": out.download((B, H, W, Cout)),
                "twin": tw.download((B, H, W, Cout)).view(np.uint32) if tw else None,
                "stats": st.download().view(np.float64).reshape(B, slices, Cout, 2) if got.value else None}

    def op_conv_in(self, state, weight, bias=None, want_out=True, want_twin=True, want_stats=True) -> dict:
        """The UNet's first conv on the packed split-f16 state, as the split-f16 forward runs it (sr3_op_conv_in): state
        [B, H, W, Cin <= 8] fp32, weight OIHW [Cout, Cin, 3, 3]. Returns a dict: out (float32 [B, H, W, Cout]), twin (the
        uint16 halfs as stored, [B, H, W, Cout // 32, 2, 32]: per 32-channel chunk hi | lo), stats (float64
        [B, H*W // 256, Cout, 2], NaN where no kernel wrote) — each None when switched off — and packed (uint16
        [B, H+2, W+2, 2, 8]: per padded pixel 8 hi | 8 lo halfs)."""
        state = _host_f32(state)
        B, H, W, Cin = state.shape
        weight = _host_f32(weight)
        Cout = weight.shape[0]
        assert weight.shape == (Cout, Cin, 3, 3), weight.shape
        d = self.to_device(state.transpose(0, 3, 1, 2))
        bh = _host_f32(bias) if bias is not None else None
        n = B * H * W * Cout
        out = self.buffer(n) if want_out else None
        twin = self.buffer(n) if want_twin else None
        slices = max(1, H * W // 256)
        cap = B * slices * Cout * 2
        st = self.buffer(cap * 2) if want_stats else None
        packed = np.empty((B, H + 2, W + 2, 2, 8), dtype=np.uint16)
        got = C.c_int(-1)
        _lib.check(self.lib.sr3_op_conv_in(
            self.ctx, d.ptr, B, H, W, Cin, weight.ctypes.data, bh.ctypes.data if bh is not None else None, Cout,
            out.ptr if out else None, twin.ptr if twin else None, st.ptr if st else None, cap, C.byref(got),
            packed.ctypes.data))
        assert got.value == H * W // 256, got.value
        return {"out": out.download((B, H, W, Cout)) if out else None,
                "twin": twin.download().view(np.uint16).reshape(B, H, W, Cout // 32, 2, 32) if twin else None,
                "stats": st.download().view(np.float64).reshape(B, got.value, Cout, 2) if st else None,
                "packed": packed}

    def op_conv_in_f32(self, state, weight, bias=None, want_stats=True, stats_slots=None) -> dict:
        """The UNet's first conv as the exact-f32 forward runs it (sr3_op_conv_in_f32, conv_in_f32_kernel): state
        [B, H, W, Cin <= 8] fp32, weight OIHW [Cout, Cin, 3, 3]. Returns a dict: out (float32 [B, H, W, Cout]), stats
        (float64 [B, H*W // 256, Cout, 2]; None when switched off), slices (H*W // 256) and stats_raw (the whole statistics
        buffer as float64, stats_slots >= B * slices * Cout * 2 doubles when given: what lies behind the slices keeps the
        0xFF fill, NaN)."""
        state = _host_f32(state)
        B, H, W, Cin = state.shape
        weight = _host_f32(weight)
        Cout = weight.shape[0]
        assert weight.shape == (Cout, Cin, 3, 3), weight.shape
        d = self.to_device(state.transpose(0, 3, 1, 2))
        bh = _host_f32(bias) if bias is not None else None
        out = self.buffer(B * H * W * Cout)
        need = B * max(1, H * W // 256) * Cout * 2
        cap = need if stats_slots is None else int(stats_slots)
        st = self.buffer(cap * 2) if want_stats else None
        got = C.c_int(-1)
        _lib.check(self.lib.sr3_op_conv_in_f32(
            self.ctx, d.ptr, B, H, W, Cin, weight.ctypes.data, bh.ctypes.data if bh is not None else None, Cout,
            out.ptr, st.ptr if st else None, cap, C.byref(got)))
        assert got.value == H * W // 256, got.value
        raw = st.download().view(np.float64) if st else None
        return {"out": out.download((B, H, W, Cout)),
                "stats": raw[:B * got.value * Cout * 2].reshape(B, got.value, Cout, 2) if st else None,
                "slices": got.value, "stats_raw": raw}

    def op_final_conv(self, x, gn_scale, gn_shift, weight, bias, return_form=False):
        """The UNet's last layer as the forward runs it (sr3_op_final_conv): swish(x * gn_scale + gn_shift), zero padding,
        3x3 conv. x [B, H, W, C] fp32, gn_scale / gn_shift [B, C] (op_groupnorm_affine), weight OIHW [Cout, C, 3, 3]. The
        fp32 VALU kernel runs in f32, the MFMA kernel in split-f16 where the forward takes it; return_form adds which
        ("valu" | "mfma")."""
        x = _host_f32(x)
        B, H, W, Cc = x.shape
        weight, bias = _host_f32(weight), _host_f32(bias)
        Cout = weight.shape[0]
        assert weight.shape == (Cout, Cc, 3, 3) and bias.shape == (Cout,), (weight.shape, bias.shape)
        sc, sh = _host_f32(gn_scale), _host_f32(gn_shift)
        assert sc.shape == (B, Cc) and sh.shape == (B, Cc), (sc.shape, sh.shape)
        d, dsc, dsh = self.to_device(x), self.to_device(sc), self.to_device(sh)
        out = self.buffer(B * H * W * Cout)
        form = C.c_int(0)
        _lib.check(self.lib.sr3_op_final_conv(self.ctx, d.ptr, B, H, W, Cc, dsc.ptr, dsh.ptr, weight.ctypes.data,
                                              bias.ctypes.data, Cout, out.ptr, C.byref(form)))
        o = out.download((B, H, W, Cout))
        return (o, {1: "valu", 2: "mfma"}[form.value]) if return_form else o

    def read_packed_state(self):
        """(state, packed) of the current call's sampler state: state float32 [B, H+2, W+2, 8] (the 8 leading channels of
        the zero-bordered fp32 state), packed uint16 [B, H+2, W+2, 2, 8] (8 hi | 8 lo halfs per pixel); None when the
        call's shape keeps no packed state. For tests."""
        dims = (C.c_int * 3)()
        n = int(self.lib.sr3_read_packed_state(self.ctx, None, None, dims))
        _lib.check(min(n, 0))
        if n == 0:
            return None
        B, H, W = dims[0], dims[1], dims[2]
        assert n == B * (H + 2) * (W + 2), (n, B, H, W)
        state = np.empty((B, H + 2, W + 2, 8), dtype=np.float32)
        packed = np.empty((B, H + 2, W + 2, 2, 8), dtype=np.uint16)
        _lib.check(min(int(self.lib.sr3_read_packed_state(self.ctx, state.ctypes.data, packed.ctypes.data, dims)), 0))
        return state, packed

    def op_groupnorm_apply(self, x0, gamma, beta, groups=32, x1=None, stats0=None, stats1=None, mode=2, fmt=0,
                           in_split=0, route=0, want_raw=False):
        """The engine's GroupNorm apply pass over x0 ‖ x1 (NHWC; float32, or the uint32 words of the split-f16 format for an
        input named in in_split). stats0 / stats1: float64 partials [B, slices, C, 2] of x0 / x1 (None: the statistics
        kernel runs). mode 0 copy | 1 affine | 2 affine + Swish; fmt 0 fp32 | 1 split-f16 | 2 F8C; route 0 the engine's
        choice | 1 folded | 2 finalize + streaming rows. Returns a dict: out (float32 for fmt 0, else uint32 words), raw
        (want_raw), route (taken), range_flag."""
        def words(a):
            a = np.ascontiguousarray(a)
            return a.view(np.float32) if a.dtype == np.uint32 else _host_f32(a)

        def doubles(a):
            return self.to_device(np.ascontiguousarray(a, dtype=np.float64).view(np.float32))

        x0 = words(x0)
        B, H, W, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[-1]
        Cc = C0 + C1
        d0 = self.to_device(x0)
        d1 = self.to_device(words(x1)) if x1 is not None else None
        s0 = doubles(stats0) if stats0 is not None else None
        s1 = doubles(stats1) if stats1 is not None else None
        for st, Cs in ((stats0, C0), (stats1, C1)):
            assert st is None or (st.ndim == 4 and st.shape[0] == B and st.shape[2:] == (Cs, 2)), st.shape
        g, b = _host_f32(gamma), _host_f32(beta)
        assert g.size == Cc and b.size == Cc
        out = self.buffer(B * H * W * Cc)
        raw = self.buffer(B * H * W * Cc) if want_raw else None
        took, flag = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.sr3_op_groupnorm_apply(
            self.ctx, d0.ptr, C0, d1.ptr if d1 else None, C1, B, H, W, groups, g.ctypes.data, b.ctypes.data,
            s0.ptr if s0 else None, stats0.shape[1] if stats0 is not None else 0,
            s1.ptr if s1 else None, stats1.shape[1] if stats1 is not None else 0,
            mode, fmt, in_split, route, out.ptr, raw.ptr if raw else None, C.byref(took), C.byref(flag)))
        res = {"out": out.download((B, H, W, Cc)), "route": took.value, "range_flag": bool(flag.value)}
        if fmt:
            res["out"] = res["out"].view(np.uint32)
        if want_raw:
            r = raw.download((B, H, W, Cc))
            res["raw"] = r.view(np.uint32) if fmt else r
        return res

    def bench_gn_res1x1(self, B, H, W, C0, C1, Cout, iters=20, groups=32):
        """(ms of the apply pass + 1x1 conv pair, ms of finalize + gn_res1x1_kernel, route of the pair's apply pass) for one
        block shape on random data (sr3_bench_gn_res1x1)."""
        pair, one, route = C.c_float(0), C.c_float(0), C.c_int(0)
        _lib.check(self.lib.sr3_bench_gn_res1x1(self.ctx, B, H, W, C0, C1, Cout, groups, iters, C.byref(pair), C.byref(one),
                                                C.byref(route)))
        return pair.value, one.value, route.value

    def op_gn_res1x1(self, x, gamma, beta, w2, groups=32, skip=None, sentinel=-12345.0, want_pair=False):
        """block1's GroupNorm + Swish pass and the block's 1x1 res_conv in one kernel (f32 mode) over NHWC x ‖ skip; w2
        [Cout, C0 + C1]. Returns a dict: act [B, H+2, W+2, C] (border = sentinel), res [B, H, W, Cout] and, with
        want_pair, res_pair: the same product from the 1x1 side launch the kernel replaces in the engine."""
        x = _host_f32(x)
        B, H, W, C0 = x.shape
        C1 = 0 if skip is None else skip.shape[-1]
        Cc = C0 + C1
        w2 = _host_f32(w2)
        Cout = w2.shape[0]
        assert w2.size == Cout * Cc
        g, b = _host_f32(gamma), _host_f32(beta)
        assert g.size == Cc and b.size == Cc
        d0 = self.to_device(x)
        d1 = self.to_device(_host_f32(skip)) if skip is not None else None
        act = self.buffer(B * (H + 2) * (W + 2) * Cc)
        res = self.buffer(B * H * W * Cout)
        pair = self.buffer(B * H * W * Cout) if want_pair else None
        _lib.check(self.lib.sr3_op_gn_res1x1(
            self.ctx, d0.ptr, C0, d1.ptr if d1 else None, C1, B, H, W, groups, g.ctypes.data, b.ctypes.data, w2.ctypes.data,
            Cout, float(sentinel), act.ptr, res.ptr, pair.ptr if pair else None))
        out = {"act": act.download((B, H + 2, W + 2, Cc)), "res": res.download((B, H, W, Cout))}
        if want_pair:
            out["res_pair"] = pair.download((B, H, W, Cout))
        return out

    def op_groupnorm_affine(self, x0, gamma, beta, groups=32, x1=None):
        x0 = _host_f32(x0)
        B, H, W, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[-1]
        C = C0 + C1
        d0 = self.to_device(x0)
        d1 = self.to_device(x1) if x1 is not None else None
        sc, sh = self.buffer(B * C), self.buffer(B * C)
        g, b = _host_f32(gamma), _host_f32(beta)
        _lib.check(self.lib.sr3_op_groupnorm_affine(
            self.ctx, d0.ptr, C0, d1.ptr if d1 else None, C1, B, H, W, groups, g.ctypes.data,
            b.ctypes.data, sc.ptr, sh.ptr))
        return sc.download((B, C)), sh.download((B, C))

    def op_attention(self, qkv, streaming: bool = False, twin: bool = False, f32_out: bool = True):
        """streaming=True runs the online-softmax core at any N (otherwise it runs only above 1024 tokens). twin=True
        (split-f16 core only, sr3_op_attention_twin) returns (out, twin): twin the uint32 words of the split-f16 copy of the
        result; f32_out=False writes the twin alone and returns (None, twin)."""
        qkv = _host_f32(qkv)
        B, N, C3 = qkv.shape
        d = self.to_device(qkv)
        n = B * N * (C3 // 3)
        out = self.buffer(n) if f32_out else None
        if twin:
            assert not streaming
            tw = self.buffer(n)
            _lib.check(self.lib.sr3_op_attention_twin(self.ctx, d.ptr, B, N, C3 // 3, out.ptr if out else None, tw.ptr,
                                                      0 if f32_out else 1))
            return (out.download((B, N, C3 // 3)) if out else None), tw.download((B, N, C3 // 3)).view(np.uint32)
        fn = self.lib.sr3_op_attention_stream if streaming else self.lib.sr3_op_attention
        _lib.check(fn(self.ctx, d.ptr, B, N, C3 // 3, out.ptr))
        return out.download((B, N, C3 // 3))

    def op_noise_embed(self, noise_level) -> Tuple[np.ndarray, np.ndarray]:
        nl = _host_f32(noise_level).ravel()
        B = nl.size
        total = self.lib.sr3_chan_bias_total(self.ctx)
        d = self.to_device(nl)
        te, cb = self.buffer(B * self.cfg.inner_channel), self.buffer(B * total)
        _lib.check(self.lib.sr3_op_noise_embed(self.ctx, d.ptr, B, te.ptr, cb.ptr))
        return te.download((B, self.cfg.inner_channel)), cb.download((B, total))

    # ---- numpy conveniences (NCHW in / out) ---------------------------------------------------
    def unet_forward_np(self, x, noise_level) -> np.ndarray:
        x = _host_f32(x)
        B, _, H, W = x.shape
        dx, dn = self.to_device(x), self.to_device(np.asarray(noise_level).ravel())
        out = self.buffer(B * self.cfg.out_channel * H * W)
        self.unet_forward(dx.ptr, dn.ptr, B, H, W, out.ptr)
        return out.download((B, self.cfg.out_channel, H, W))

    def unet_forward_cached_np(self, x, noise_level, depth: int = 1) -> np.ndarray:
        """The shallow forward of `depth` on what the last unet_forward_np of the same shape left in the workspace."""
        x = _host_f32(x)
        B, _, H, W = x.shape
        dx, dn = self.to_device(x), self.to_device(np.asarray(noise_level).ravel())
        out = self.buffer(B * self.cfg.out_channel * H * W)
        self.unet_forward_cached(dx.ptr, dn.ptr, B, H, W, depth, out.ptr)
        return out.download((B, self.cfg.out_channel, H, W))

    def sample_np(self, cond, noise=None, seed=0, image_offset=0, frames=False, shape=None, init=None, start_step=None,
                  noised=True):
        """cond [B,Cc,H,W] (or None with shape=(B,C,H,W)); noise [T,B,C,H,W] or None (Philox). init [B,C,H,W] with
        start_step: the warm start (Engine.sample); noise is then [start_step,B,C,H,W]."""
        C_ = self.cfg.out_channel
        if cond is not None:
            cond = _host_f32(cond)
            B, _, H, W = cond.shape
            dc = self.to_device(cond)
        else:
            B, _, H, W = shape
            dc = None
        dn = self.to_device(noise) if noise is not None else None
        di = self.to_device(init) if init is not None else None
        out = self.buffer(B * C_ * H * W)
        nf = self.num_frames(start_step if init is not None else None)
        fr = self.buffer(nf * B * C_ * H * W) if frames else None
        self.sample(dc.ptr if dc else None, B, H, W, out.ptr, dn.ptr if dn else None, seed,
                    image_offset, fr.ptr if fr else None, init_ptr=di.ptr if di else None, start_step=start_step,
                    noised=noised)
        o = out.download((B, C_, H, W))
        if frames:
            return o, fr.download((nf, B, C_, H, W))
        return o

    def rows_np(self, requests, slots: int, seed: int = 0, on_step=None, elastic: bool = False, ladder=None):
        """numpy convenience (tests): a whole row session. requests: dicts with cond [Cc,H,W], image_id, and optionally
        at (the earliest session step the request may be admitted at, default 0), init [C,H,W] with start_step and
        noised, noise [s0,C,H,W] (slab 0 the start noise / the z of q_sample, slab k the draw of step t = s0 - k) and
        slot (a slot of its own; default: the lowest free one), lr [C,lh,lw] with lr_strength (the row is held to it: the
        session is armed for the size of the first lr among the requests) and frames True (the row's frames come back with
        its image). A request enters once `at` steps have run and a slot is
        free; finished rows retire after every step. on_step(k) runs after step k, with the session open (read-backs).
        Returns (images in request order, trace): trace[k] = the request index per slot (None: idle) during step k; the
        entry of a request with frames is (image, frames [n,C,H,W]). elastic (batch-invariant mode): before each step
        the live rows are compacted by rolling.elastic_plan over `ladder` (default rolling.default_ladder(slots)) and the
        step runs at the batch it names; returns (images, trace, batches) with the batch of every step (0 for an empty
        one), the trace taken after the moves."""
        from .rolling import check_ladder, elastic_plan
        if elastic:
            if not self.batch_invariant():
                raise ValueError("elastic=True needs the batch-invariant mode: call set_batch_invariant first")
            ladder = check_ladder(ladder, slots)
        batches = []
        C_ = self.cfg.out_channel
        H, W = np.asarray(requests[0]["cond"]).shape[-2:]
        self.rows_begin(slots, H, W, seed)
        lrs = [np.asarray(rq["lr"]).shape[-2:] for rq in requests if rq.get("lr") is not None]
        fbufs = [None] * slots
        keep, held = [], [None] * slots         # device buffers of the live rows; request index per slot
        pos0 = [0] * slots
        out = [None] * len(requests)
        obuf = self.buffer(C_ * H * W)
        waiting = list(range(len(requests)))
        trace, k = [], 0
        try:
            if lrs:
                self.rows_lr_consistency(*lrs[0])
            while waiting or any(h is not None for h in held):
                for i in list(waiting):
                    rq = requests[i]
                    if int(rq.get("at", 0)) > k:
                        continue
                    free = [s for s in range(slots) if held[s] is None]
                    s = rq.get("slot", free[0] if free else None)
                    if s is None or held[s] is not None:
                        continue
                    dc = self.to_device(rq["cond"])
                    di = self.to_device(rq["init"]) if rq.get("init") is not None else None
                    nz = _host_f32(rq["noise"]) if rq.get("noise") is not None else None
                    dn = [self.to_device(z) for z in nz] if nz is not None else None
                    s0 = int(rq.get("start_step", self.T)) if di is not None else self.T
                    dl = self.to_device(rq["lr"]) if rq.get("lr") is not None else None
                    self.rows_admit(s, dc.ptr, rq["image_id"], di.ptr if di else None, s0 if di else None,
                                    bool(rq.get("noised", True)), dn[0].ptr if dn else None,
                                    lr=dl.ptr if dl else None, lr_strength=float(rq.get("lr_strength", 1.0)))
                    if dl is not None:
                        dl.free()               # (the library holds its own copy)
                    if rq.get("frames"):
                        nf = self.num_frames(s0)
                        fbufs[s] = (self.buffer(nf * C_ * H * W), nf)
                        self.rows_frames(s, fbufs[s][0].ptr, nf)
                    keep.append((dc, di, dn))
                    held[s], pos0[s] = (i, dn), s0
                    waiting.remove(i)
                if all(h is None for h in held):    # nothing admissible yet: an empty step of the session clock
                    assert self.rows_step() == 0
                    trace.append([None] * slots)
                    batches.append(0)
                    k += 1
                    continue
                batch = None
                if elastic:
                    moves, batch = elastic_plan([h is not None for h in held], ladder)
                    for a, b in moves:
                        self.rows_move(a, b)
                        held[b], pos0[b], fbufs[b] = held[a], pos0[a], fbufs[a]
                        held[a], fbufs[a] = None, None
                batches.append(slots if batch is None else batch)
                ptrs = None
                if any(h is not None and h[1] is not None for h in held):
                    ptrs = []
                    for s in range(slots):
                        dn = held[s][1] if held[s] is not None else None
                        p = self.rows_position(s)
                        # slab index of step t = p - 1 in a run of pos0 steps: pos0 - t (none for t == 0)
                        ptrs.append(dn[pos0[s] - (p - 1)].ptr if dn is not None and p > 1 else None)
                self.rows_step(ptrs, batch)
                trace.append([h[0] if h is not None else None for h in held])
                if on_step is not None:
                    on_step(k)
                k += 1
                for s in range(slots):
                    if held[s] is not None and self.rows_position(s) == 0:
                        self.rows_retire(s, obuf.ptr)
                        out[held[s][0]] = obuf.download((C_, H, W)).copy()
                        if fbufs[s] is not None:
                            fb, nf = fbufs[s]
                            out[held[s][0]] = (out[held[s][0]], fb.download((nf, C_, H, W)).copy())
                            fb.free()
                            fbufs[s] = None
                        held[s] = None
        finally:
            self.rows_end()
            for dc, di, dn in keep:
                for b in [dc, di] + (dn or []):
                    if b is not None:
                        b.free()
            obuf.free()
        return (out, trace, batches) if elastic else (out, trace)
