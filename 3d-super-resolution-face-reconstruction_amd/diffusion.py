"""`GaussianDiffusion`: the reference's sampler API (model/sr/sr3_modules/diffusion.py:66-225)
over libsr3hip. The whole p_sample_loop — T UNet evaluations and the DDPM update — runs inside
the HIP library; this class only holds the schedule buffers (for state_dict parity) and moves
pointers. The denoising loss (q_sample, p_losses, forward: diffusion.py:275-318) is EVALUATED on the device
(sr3_denoise_loss); backward passes and the *_learn members stay out of scope.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import nn

from . import samplers as _samplers
from . import schedule as _schedule
from ._lib import Sr3Error


class DictTensor:
    """The reference's wrapper of a batch dict (diffusion.py:323-344), which callers pass through DataParallel."""

    def __init__(self, data):
        self.data = data

    def to(self, device):
        self.data = {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in self.data.items()}
        return self

    def __getitem__(self, key):
        return self.data[key]

    def __setitem__(self, key, value):
        self.data[key] = value

    def keys(self):
        return self.data.keys()

    def items(self):
        return self.data.items()

    def __repr__(self):
        return str(self.data)


def draw_levels(sqrt_alphas_cumprod_prev, T: int, b: int):
    """The host draws of p_losses (diffusion.py:287-294), the reference's own two np.random calls in its order: one
    timestep t in [1, T], then b continuous levels, uniform between sqrt_alphas_cumprod_prev[t-1] and [t]. Returns
    (t, float32 [b]); the cast is torch.FloatTensor's. The same np.random.seed gives the reference's levels."""
    t = np.random.randint(1, T + 1)
    lv = np.random.uniform(sqrt_alphas_cumprod_prev[t - 1], sqrt_alphas_cumprod_prev[t], size=b)
    return int(t), np.asarray(lv, dtype=np.float32)


def noise_coefficient(levels) -> np.ndarray:
    """s = sqrt(1 - a^2) of q_sample (diffusion.py:281) for fp32 levels a: the reference's expression
    `(1 - a**2).sqrt()` with every operation a correctly rounded fp32 one (numpy: product, difference, square root), which
    is what the reference gets on the GPU. torch's vectorised CPU sqrt is not used: it is 1 ulp off on some hosts."""
    a = np.ascontiguousarray(np.asarray(levels, dtype=np.float32).reshape(-1))
    return np.sqrt(np.float32(1) - a * a)


def lr_to_tensor(lr) -> torch.Tensor:
    """The LR images the consistency projection holds a sample to, as fp32 [N,3,l,l] in [-1,1]: an fp32 NCHW tensor is
    taken as it is (the dataset's `LR` entry), uint8 [N,l,l,3] (HWC crops) is mapped as the dataset maps them, ToTensor and
    min_max (-1, 1): (u8 / 255) * 2 - 1 in fp32 (datasets/util.py:76-83)."""
    lr = torch.as_tensor(lr)
    if lr.dtype == torch.uint8:
        if lr.dim() != 4 or lr.shape[-1] != 3:
            raise RuntimeError(f"uint8 LR images must be [N,l,l,3], got {tuple(lr.shape)}")
        x = lr.to(torch.float32) / 255.0
        return (x * 2.0 + (-1.0)).permute(0, 3, 1, 2).contiguous()
    if lr.dtype != torch.float32 or lr.dim() != 4:
        raise RuntimeError(f"LR images must be fp32 [N,C,l,l] in [-1,1] or uint8 [N,l,l,3], got {lr.dtype} {tuple(lr.shape)}")
    return lr.contiguous()


class GaussianDiffusion(nn.Module):
    def __init__(self, denoise_fn, image_size, channels=3, loss_type="l1", conditional=True,
                 schedule_opt=None):
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.denoise_fn = denoise_fn
        self.loss_type = loss_type
        self.conditional = conditional
        self.num_timesteps = 0
        self._sched_np = None
        self._sched_pushed = None   # engine id the schedule was pushed to
        self._sampler = ("ddpm", None, 0.0)   # set_sampler(); not part of state_dict()
        self._lr = None                       # set_lr_consistency(): (fp32 [N,C,lh,lw], strength); not part of state_dict()
        self._start = None                    # set_start(): (strength | None, step | None, init, noised); not part of state_dict()
        self._dyn = None                      # set_dynamic_threshold(): (ratio, max_value | None); not part of state_dict()
        self._fc = None                       # set_feature_cache(): (interval, depth); not part of state_dict()

    # ---- reference surface that is configuration only -----------------------------------------
    def set_loss(self, device=None):
        """diffusion.py:85-91: selects the summed L1 ('l1') or L2 ('l2') loss that p_losses evaluates. Like the
        reference's, a model on which set_loss was never called has no loss function (there p_losses fails on the missing
        attribute; here it raises NotImplementedError, as it did before the loss existed)."""
        if self.loss_type not in ("l1", "l2"):
            raise NotImplementedError()
        self.loss_func = self.loss_type

    def set_new_noise_schedule(self, schedule_opt, device=None):
        """diffusion.py:93-142. `device` may be 0, a list of ids (the reference's form), a
        torch.device or None (= where the denoiser lives)."""
        if isinstance(device, (list, tuple)):
            device = device[0]
        if device is None:
            device = next(self.denoise_fn.parameters()).device
        bufs = _schedule.schedule_buffers(schedule_opt)
        self.sqrt_alphas_cumprod_prev = bufs["sqrt_alphas_cumprod_prev"]
        self.num_timesteps = int(bufs["betas"].shape[0])
        for name in _schedule.BUFFER_NAMES:
            t = torch.tensor(bufs[name], dtype=torch.float32, device=device)
            if name in self._buffers:
                self._buffers[name] = t
            else:
                self.register_buffer(name, t)
        self._sched_np = bufs
        self._sched_pushed = None

    def set_sampler(self, kind="ddpm", steps=None, eta=0.0):
        """Sampling algorithm of every sampling entry point (super_resolution, sample, p_sample_loop, sample_batch,
        super_resolution_batch; validation.validate_batch and the dist.sharded_* helpers through them), DESIGN.md §3.5:

          "ddpm"      the reference's ancestral loop over all T steps (default)
          "ddim"      DDIM over `steps` (S) of the schedule's levels; eta = 0 deterministic, eta = 1 with S = T is DDPM
          "dpmpp_2m"  DPM-Solver++(2M), deterministic, second order

        steps=None means S = T. The setting survives set_new_noise_schedule (the tables are re-derived from the new
        schedule) and adds nothing to state_dict(). p_sample / p_mean_variance / q_posterior stay the reference's
        single DDPM step whatever the setting."""
        # (without a schedule yet, S <= T is checked when the tables are derived)
        _samplers.check_sampler(kind, steps, eta, self.num_timesteps if self._sched_np is not None else None)
        self._sampler = (kind, None if steps is None or kind == "ddpm" else int(steps), float(eta))
        self._sched_pushed = None

    def set_start(self, strength=None, *, step=None, init="cond", noised=True) -> None:
        """Warm start of every sampling entry point: instead of pure noise at the top of the schedule,
        a call starts from its own conditioning image, forward-diffused (q_sample, diffusion.py:275-282) to an
        intermediate level, and runs only the last s0 of its S steps — the reference's own p_sample steps (:183-215), s0
        UNet evaluations instead of S.

          strength  in (0, 1]: s0 = max(1, round(strength * S)), re-derived whenever S changes (set_sampler,
                    set_new_noise_schedule); 1.0 runs every step, from q_sample at the top level rather than pure noise
          step      s0 itself, in [1, S] (checked against the S of the moment at every call)
          init      "cond": every call starts from its own x_in — super_resolution, sample_batch, p_sample_loop,
                    validation.validate_batch (samples x images), mc-dropout runs and the dist.sharded_* helpers pick it
                    up with no further plumbing. Raises for the unconditional model, which has no such image. An
                    explicit start image is a per-call argument (sample_batch(init=...)).
          noised    False: the image is taken as the state itself (it already sits at that level)

        Both None turns it off: every call is then bit for bit what it was. Like set_sampler, the setting survives
        set_new_noise_schedule and set_sampler, adds nothing to state_dict(), and leaves p_sample alone. Sample quality at
        a given strength is a property of the checkpoint and is not established here."""
        if strength is None and step is None:
            self._start = None
            return
        if strength is not None and step is not None:
            raise ValueError("give strength or step, not both")
        if init != "cond":
            raise ValueError(f"init must be 'cond' (an explicit image is passed per call: sample_batch(init=...)), got {init!r}")
        if not self.conditional:
            raise ValueError("init='cond' needs a conditional model: the unconditional one has no conditioning image")
        if strength is not None:
            strength = float(strength)
            if not 0.0 < strength <= 1.0:       # (also refuses NaN)
                raise ValueError(f"strength must lie in (0, 1], got {strength}")
        else:
            if isinstance(step, bool) or int(step) != step:
                raise ValueError(f"step must be an integer, got {step!r}")
            step = int(step)
            S = self.num_sampling_steps if self._sched_np is not None or self._sampler[1] is not None else None
            if step < 1 or (S is not None and step > S):
                raise ValueError(f"step must lie in [1, S] (S = {S} sampling steps), got {step}")
        self._start = (strength, step, "cond", bool(noised))

    @staticmethod
    def start_steps(S: int, strength=None, step=None) -> int:
        """s0 of a warm start over S steps: max(1, round(strength * S)), or `step` checked against [1, S]."""
        if strength is not None:
            strength = float(strength)
            if not 0.0 < strength <= 1.0:
                raise ValueError(f"strength must lie in (0, 1], got {strength}")
            return max(1, min(int(S), int(round(strength * int(S)))))
        if isinstance(step, bool) or int(step) != step or not 1 <= int(step) <= int(S):
            raise ValueError(f"step must be an integer in [1, S] (S = {int(S)} sampling steps), got {step!r}")
        return int(step)

    def set_lr_consistency(self, lr, strength: float = 1.0) -> None:
        """Keeps every sample consistent with its low-resolution input: each step of every sampling
        entry point projects its x0 prediction onto the images whose antialiased bicubic downsample — the reference's
        degradation, datasets/tool/prepare_data.py:37-47 — is the LR image, so the result provably downsamples to it
        (strength 1; 0 < strength < 1 moves that fraction of the way) and only what the LR image cannot see is left to
        the network. lr: fp32 [N,3,l,l] in [-1,1] (the dataset's `LR` entry) or uint8 [N,l,l,3] (lr_to_tensor); batch
        row b is held to lr[(image_offset + b) % N], so samples x images batches, chunks and shards pass the images once.
        None (or strength 0) turns it off: the sampler is then bit for bit what it was. The setting survives set_sampler
        and set_new_noise_schedule and adds nothing to state_dict(). p_sample stays the reference's single step."""
        if lr is None or float(strength) == 0.0:
            self._lr = None
            return
        if not 0.0 < float(strength) <= 1.0:
            raise ValueError(f"strength must lie in [0, 1], got {strength}")
        t = lr_to_tensor(lr)
        if t.shape[1] != self.channels:
            raise RuntimeError(f"LR images need {self.channels} channels, got {tuple(t.shape)}")
        self._lr = (t, float(strength))

    def _arm_lr(self, eng, dev, H: int, W: int, row_offset: int):
        """Puts the engine's consistency setting in the state the next sampling call needs; returns the LR tensor on the
        device (the caller keeps it alive until the call is enqueued and ordered)."""
        if self._lr is None:
            if getattr(eng, "_lr_on", False):
                eng.set_lr_consistency(None)
                eng._lr_on = False
            return None
        t, strength = self._lr
        if t.device != dev:
            t = t.to(dev)
            self._lr = (t, strength)
        N, _, lh, lw = t.shape
        if lh >= H or lw >= W:
            raise RuntimeError(f"LR images of {lh}x{lw} cannot constrain samples of {H}x{W}")
        eng.set_lr_consistency(t.data_ptr(), N, lh, lw, int(row_offset), strength)
        eng._lr_on = True
        return t

    def set_dynamic_threshold(self, ratio=None, max_value=None) -> None:
        """Dynamic thresholding of the x0 prediction in every sampling entry point (Imagen, Saharia et
        al. 2022, §2.3): each step replaces the reference's x_recon.clamp_(-1., 1.) (diffusion.py:175-176) by
        clamp(x0, -s, s) / s, with s the `ratio`-quantile of |x0| over the C*H*W values of each image (exact, linear
        interpolation between the two order statistics), never below 1 and never above max_value. With s = 1 that is the
        static clamp bit for bit. The few-step samplers (set_sampler "ddim" / "dpmpp_2m", set_start) are where it
        matters: their early x0 predictions lie far outside [-1, 1].

          ratio      in (0, 1]; None turns the feature off: the sampler is then bit for bit what it was
          max_value  >= 1, the cap on s; None means no bound

        The statistic is per image, so chunks, shards and image offsets change nothing. The setting survives set_sampler
        and set_new_noise_schedule, adds nothing to state_dict(), and leaves p_sample — the reference's single step —
        alone. Sample quality with it on a trained checkpoint is not established here."""
        if ratio is None:
            if max_value is not None:
                raise ValueError("max_value needs a ratio (ratio=None turns the feature off)")
            self._dyn = None
            return
        ratio = float(ratio)
        if not 0.0 < ratio <= 1.0:              # (also refuses NaN)
            raise ValueError(f"ratio must lie in (0, 1], got {ratio}")
        if max_value is not None:
            max_value = float(max_value)
            if not max_value >= 1.0:
                raise ValueError(f"max_value must be >= 1 (None: no bound), got {max_value}")
        self._dyn = (ratio, max_value)

    def _arm_dyn(self, eng) -> None:
        """Puts the engine's threshold setting in the state the next sampling call needs (next to _arm_lr)."""
        want = self._dyn
        if getattr(eng, "_dyn_set", None) != want:
            eng.set_dynamic_threshold(*(want if want is not None else (None, None)))
            eng._dyn_set = want

    def set_feature_cache(self, interval=None, depth: int = 1) -> None:
        """Reuses the deep UNet features across the steps of every sampling entry point (DeepCache, Ma,
        Fang, Wang 2023; training-free): only every `interval`-th step of a call runs the whole UNet (unet.py:235-265), the
        steps between run its `depth` top resolution levels on the feature the deep part produced at the last whole step.
        The sampler, the schedule, the noise draws and the weights stay what they are.

          interval  an integer >= 1; None (or 1) turns the feature off: the sampler is then bit for bit what it was
          depth     resolution levels kept fresh, an integer in [1, len(channel_mults) - 1]

        It covers sample_batch, super_resolution*, refine and interpolate in every sampler (set_sampler, set_start), with
        set_lr_consistency and set_dynamic_threshold. The first step of every call is whole, so chunks and shards, each a
        call of its own, behave alike. The setting survives set_sampler and set_new_noise_schedule, adds nothing to
        state_dict(), and leaves p_sample — the reference's single step — alone. Sample quality with it on a trained
        checkpoint is not established here."""
        n_levels = len(self.denoise_fn.cfg.channel_mults)
        if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 1 <= int(depth) <= n_levels - 1:
            raise ValueError(f"depth must be an integer in [1, {n_levels - 1}] (resolution levels kept fresh), got {depth!r}")
        if interval is None:
            self._fc = None
            return
        if isinstance(interval, bool) or not isinstance(interval, (int, np.integer)) or int(interval) < 1:
            raise ValueError(f"interval must be an integer >= 1 (None: off), got {interval!r}")
        self._fc = (int(interval), int(depth)) if int(interval) > 1 else None

    def _arm_fc(self, eng) -> None:
        """Puts the engine's feature-cache setting in the state the next sampling call needs (next to _arm_dyn)."""
        want = self._fc
        if getattr(eng, "_fc_set", None) != want:
            eng.set_feature_cache(*(want if want is not None else (None, 1)))
            eng._fc_set = want

    def set_batch_invariant(self, on: bool = True, plan_batch: int = 64) -> None:
        """Batch-invariant mode (UNet.set_batch_invariant): an image's bytes no longer depend on the batch
        it ran in. Honoured by sample_batch, super_resolution_batch, refine, p_losses, validate_batch, rolling() — a
        session inherits the setting, changing it inside one is refused — and dist.sharded_super_resolution: the same
        request gives the same bytes served alone, in a chunk, in a slot or on another rank. Off by default."""
        self.denoise_fn.set_batch_invariant(on, plan_batch)

    def set_dropout_sampling(self, on: bool, seed: Optional[int] = None) -> None:
        """Opt in to sampling the UNet's Dropout as the reference does under .train() (unet.py:81-91; model 3 samples
        with the SR model in train mode, model/sr3d/model.py:234-249). While on, in train() mode and with cfg.dropout >
        0, these run with dropout: denoise_fn(x, level), p_losses / forward, p_sample, super_resolution, sample,
        sample_batch (and what is built on them). A fresh dropout seed comes from torch's generator per call unless
        `seed` pins it; chunks of one call share the seed and pass their image offset, so masks follow the GLOBAL image
        index. In eval() dropout is always the identity. DESIGN.md §3.7."""
        self.denoise_fn.set_dropout_sampling(on, seed)

    def set_dropout_masks(self, masks) -> None:
        """Injected keep masks (UNet.set_dropout_masks) for p_losses, denoise_fn and p_sample; the whole-loop entry points
        refuse them (one buffer cannot hold every step's masks)."""
        self.denoise_fn.set_dropout_masks(masks)

    def tie_weights(self, ref_netG: nn.Module) -> None:
        """UNet.tie_weights through the `denoise_fn.` prefix: this model's UNet shares the nn.Parameter objects of
        `ref_netG.denoise_fn.*` (the reference GaussianDiffusion a trainer optimises) and refreshes its kernel layouts on
        the device whenever they change."""
        prefix = "denoise_fn."
        theirs = {k[len(prefix):]: v for k, v in ref_netG.named_parameters() if k.startswith(prefix)}
        self.denoise_fn.tie_weights(theirs)

    @property
    def num_sampling_steps(self) -> int:
        """S: UNet evaluations of one sampling call (num_timesteps = T for the default "ddpm" sampler)."""
        kind, steps, _ = self._sampler
        return self.num_timesteps if steps is None else int(steps)

    @property
    def num_steps_run(self) -> int:
        """UNet evaluations one sampling call actually runs: s0 under set_start, else S."""
        if self._start is None:
            return self.num_sampling_steps
        return self.start_steps(self.num_sampling_steps, self._start[0], self._start[1])

    def _engine(self):
        eng = self.denoise_fn.engine()
        if self._sched_np is None:
            raise Sr3Error("set_new_noise_schedule() has not been called")
        # like the reference, sample with whatever the registered buffers hold now (a checkpoint's
        # load_state_dict may have replaced them, diffusion.py:144-162 reads self.<buffer>[t]); the
        # noise levels come from the config-derived float64 array (diffusion.py:108-109,166-167)
        sig = (id(eng), self._sampler) + tuple((self._buffers[k].data_ptr(), self._buffers[k]._version)
                                               for k in _schedule.ENGINE_BUFFERS)
        if self._sched_pushed != sig:
            bufs = {"noise_level": self._sched_np["noise_level"]}
            for k in _schedule.ENGINE_BUFFERS:
                bufs[k] = self._buffers[k].detach().to("cpu", torch.float32).numpy()
            kind, steps, eta = self._sampler
            if kind == "ddpm":
                eng.set_schedule(bufs)
                levels = bufs["noise_level"]
            else:
                bufs["sqrt_alphas_cumprod_prev"] = self._sched_np["sqrt_alphas_cumprod_prev"]
                tables = _samplers.sampler_tables(bufs, kind, steps, eta)
                eng.set_sampler_schedule(tables)
                levels = tables["noise_level"]
            self._levels_pushed = np.asarray(levels, dtype=np.float32)    # [S+1]: the state before step t-1 sits at [t]
            self._sched_pushed = sig
        return eng

    def _ddpm_engine(self):
        """The engine with the reference's DDPM schedule (p_sample: one reference step whatever set_sampler chose)."""
        if self._sampler[0] == "ddpm":
            return self._engine()
        keep = self._sampler
        try:
            self._sampler = ("ddpm", None, 0.0)
            return self._engine()
        finally:
            self._sampler = keep

    # ---- sampling ------------------------------------------------------------------------------
    @staticmethod
    def _draw_seed() -> int:
        # one draw from torch's global generator: torch.manual_seed() makes sampling reproducible,
        # as with the reference's torch.randn calls (the streams themselves differ: Philox on device)
        return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())

    @staticmethod
    def chunk_plan(B: int, limit: int):
        """Equal chunks for a batch above the per-call limit: (n_chunks, chunk) with n_chunks * chunk >= B and the
        fewest chunks; the last one is PADDED to `chunk` images (rows discarded) so that every chunk runs the same
        workspace, the same captured graph and the same kernels (the tile rule depends on the batch)."""
        if B <= limit:
            return 1, B
        n = -(-B // limit)
        return n, -(-B // n)

    @torch.no_grad()
    def sample_batch(self, x_in, continous=False, noise: Optional[torch.Tensor] = None,
                     seed: Optional[int] = None, image_offset: int = 0, max_chunk: Optional[int] = None,
                     init: Optional[torch.Tensor] = None, start=None, noised: Optional[bool] = None):
        """p_sample_loop for a whole batch (diffusion.py:189-215).

        x_in: conditioning [B,3,H,W] (conditional) or a shape tuple (unconditional, :193-201).
        noise: optional [S,B,C,H,W] tensor replacing the RNG (slab 0 = initial image, slab k = the
        randn_like of step t=S-k; S = num_sampling_steps, = T for the default sampler). Returns [B,C,H,W], or
        (final, frames [n,B,C,H,W]) if continous.

        Batches above the library's per-call limit (4 GiB per activation tensor: ~250 images at 128x128) — the
        reference's validation loop is 15 samples x N images (lib/trainer_temp.py:441-446), BASELINE configs[3] is 512
        images — run as equal chunks, one sr3_sample call each; Philox streams stay keyed by the GLOBAL image index
        (image_offset + row), so the noise does not depend on the chunking. max_chunk lowers the limit (tests). The
        arithmetic does, by default: the library plans every launch from the batch of the call, so the chunk size moves
        an image by fp32 round-off in f32 / f16x3 and by up to about 1e-4 in f16f8, where it also decides which convs take
        the fp8 products. Under set_batch_invariant() the result is bit-equal whatever the chunking, in every arithmetic.

        Warm start: init [B,C,H,W] is an explicit start image and overrides set_start; it is chunked,
        and its last chunk padded, like x_in. start: a strength in (0, 1] (float) or s0 itself (int); None takes
        set_start's, or S without one. noised (None: set_start's, or True): False takes the image as the state itself.
        The call runs steps t = s0-1 .. 0; noise is then [s0,B,C,H,W] (slab 0 = the z of q_sample, slab k = the draw of
        step t = s0-k) and there are len(schedule.frame_steps(S, s0)) frames.
        """
        eng = self._engine()
        if self.conditional:
            x = x_in.to(torch.float32).contiguous()
            B, _, H, W = x.shape
            dev = x.device
        else:
            B, _, H, W = tuple(x_in)
            dev, x = next(self.denoise_fn.parameters()).device, None
        C = self.channels
        T = self.num_sampling_steps
        # the start of this call: (image, s0, noised) or None (pure noise at the top: the library's sr3_sample)
        s0, x_init = None, None
        if init is not None:
            x_init = init.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(x_init.shape) != (B, C, H, W):
                raise RuntimeError(f"init must be {(B, C, H, W)}, got {tuple(x_init.shape)}")
            if start is None:
                s0 = self.num_steps_run
            elif isinstance(start, float):
                s0 = self.start_steps(T, strength=start)
            else:
                s0 = self.start_steps(T, step=start)
            if noised is None:
                noised = self._start[3] if self._start is not None else True
        elif start is not None or noised is not None:
            raise ValueError("start / noised describe an explicit start image: pass init (or use set_start)")
        elif self._start is not None:
            if x is None or x.shape[1] != C:
                raise RuntimeError("set_start(init='cond') needs a conditioning image with the channels of the result")
            x_init, s0, noised = x, self.num_steps_run, self._start[3]
        n_run = T if s0 is None else s0
        n_frames = eng.num_frames(s0) if continous else 0
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
        frames = None
        if continous:
            frames = torch.empty((n_frames, B, C, H, W), dtype=torch.float32, device=dev)
        if noise is not None:
            noise = noise.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(noise.shape) != (n_run, B, C, H, W):
                raise RuntimeError(f"noise must be {(n_run, B, C, H, W)}, got {tuple(noise.shape)}")
        if seed is None:
            seed = self._draw_seed()
        limit = eng.max_batch(H, W)
        if max_chunk is not None:
            limit = max(1, min(limit, int(max_chunk)))
        n_chunks, chunk = self.chunk_plan(B, limit)
        self.denoise_fn.arm_dropout(eng)            # (one dropout seed per call; the chunks pass their image offset)

        def run(xc, b, oc, nc, off, fc, ic):
            ptr = lambda t: t.data_ptr() if t is not None else None
            if ic is None:
                eng.sample(ptr(xc), b, H, W, oc.data_ptr(), ptr(nc), seed, off, ptr(fc))
            else:
                eng.sample(ptr(xc), b, H, W, oc.data_ptr(), ptr(nc), seed, off, ptr(fc), init_ptr=ic.data_ptr(),
                           start_step=s0, noised=bool(noised))

        if n_chunks == 1:
            self.denoise_fn.ready()
            self._arm_lr(eng, dev, H, W, image_offset)
            self._arm_dyn(eng)
            self._arm_fc(eng)
            run(x, B, out, noise, image_offset, frames, x_init)
            self.denoise_fn.finish()
            return (out, frames) if continous else out

        def rows(t, a, b, dim):
            """rows [a, b) of `t` along `dim`, padded to `chunk` rows by repeating the last one, contiguous"""
            part = t.narrow(dim, a, b - a)
            if b - a < chunk:
                last = part.narrow(dim, b - a - 1, 1)
                part = torch.cat([part] + [last] * (chunk - (b - a)), dim=dim)
            return part.contiguous()

        for k in range(n_chunks):
            a, b = k * chunk, min(B, (k + 1) * chunk)
            xc = rows(x, a, b, 0) if x is not None else None
            nc = rows(noise, a, b, 1) if noise is not None else None
            ic = None
            if x_init is not None:
                ic = xc if x_init is x else rows(x_init, a, b, 0)
            whole = b - a == chunk
            oc = out[a:b] if whole else torch.empty((chunk, C, H, W), dtype=torch.float32, device=dev)
            fc = torch.empty((frames.shape[0], chunk, C, H, W), dtype=torch.float32, device=dev) if continous else None
            self.denoise_fn.ready()
            self._arm_lr(eng, dev, H, W, image_offset + a)
            self._arm_dyn(eng)
            self._arm_fc(eng)
            run(xc, chunk, oc, nc, image_offset + a, fc, ic)
            self.denoise_fn.finish()
            if not whole:
                out[a:b] = oc[: b - a]
            if continous:
                frames[:, a:b] = fc[:, : b - a]
        return (out, frames) if continous else out

    def rolling(self, slots: Optional[int] = None, seed: Optional[int] = None, shape=None, lr_size=None,
                elastic: bool = False, ladder=None):
        """A `rolling.RollingSampler` on this model: single-image requests served through `slots` batch
        rows, each at its own position of the schedule, so a request takes a free slot while the others are mid-trajectory.
        It uses the model's sampler (set_sampler), arithmetic, range policy and dynamic threshold as they stand now. Every
        step runs at batch `slots`, so a request is byte for byte its row of a uniform call of `slots` images —
        super_resolution_batch(x, seed=seed, image_offset=image_id)[0] with x of `slots` rows, or refine(...) with a
        strength — whatever shared the batch and wherever it sat. Against a call at ANOTHER batch size (the B = 1 call, say)
        it differs, by default, as any two batch sizes differ: the conv dispatch depends on the batch (fp32 round-off in
        f32 / f16x3, 1e-5 in f16f8, whose fp8 path runs only from 32 or 64 images on). Under
        set_batch_invariant() a request is its B = 1 call byte for byte; a session inherits that setting and holds it
        (changing it inside one is refused), and `slots` must lie within the mode's maximum batch (planned for one image,
        plan_batch=1, that is 16 images at 128x128 with the yml UNet: a 64-slot session is refused there). slots None:
        min(64, the per-call limit at `shape` = (H, W), default image_size). LR consistency is per request here: submit(..., lr=image) holds that request to its LR image (fp32
        [C,l,l] or uint8 [l,l,3], lr_to_tensor) as set_lr_consistency holds a batch, a request without one is not held; the
        session is armed for the LR size when it begins — by lr_size=(lh, lw), or by the first request carrying an lr.
        submit(..., continous=True) makes poll return what super_resolution(x, continous=True) returns for one image:
        the conditioning image followed by the request's frames. The per-call set_lr_consistency, the feature cache and
        Dropout sampling do not follow single rows: the session refuses them, naming the setting. elastic=True (needs
        set_batch_invariant(): ValueError otherwise): a step runs over the live rows only, at the smallest batch of
        `ladder` (default rolling.default_ladder(slots)) that covers them, the rows compacted by one-launch moves where
        that lowers the batch; a lightly loaded session then pays for the rows it holds, not for its slots, and every
        request is still its B = 1 call byte for byte (`batch_trace`, `moves`). Use as a context manager, or close() it."""
        from .rolling import RollingSampler
        if not self.conditional:
            raise Sr3Error("rolling() needs a conditional model: the unconditional one has no per-request input")
        if self._lr is not None:
            raise Sr3Error("rolling(): set_lr_consistency is on and holds rows to one image offset per call; turn it off")
        if self._fc is not None:
            raise Sr3Error("rolling(): set_feature_cache is on and counts whole and shallow steps per call; turn it off")
        if self.denoise_fn.dropout_live():
            raise Sr3Error("rolling(): Dropout sampling (set_dropout_sampling) is on and keys its masks per call; turn it off")
        if elastic and not self.denoise_fn.batch_invariant:
            raise ValueError("rolling(elastic=True) needs the batch-invariant mode: call set_batch_invariant() first")
        eng = self._engine()
        self.denoise_fn.arm_dropout(eng)
        dev = next(self.denoise_fn.parameters()).device
        self._arm_lr(eng, dev, 0, 0, 0)
        self._arm_dyn(eng)
        self._arm_fc(eng)
        if slots is None:
            H, W = shape if shape is not None else (self.image_size, self.image_size)
            slots = min(64, eng.max_batch(int(H), int(W)))
        C = self.channels

        def alloc(r):
            return torch.empty((C,) + tuple(r.cond.shape[-2:]), dtype=torch.float32, device=r.cond.device)

        def alloc_frames(r, n):
            return torch.empty((n, C) + tuple(r.cond.shape[-2:]), dtype=torch.float32, device=r.cond.device)

        def to_lr(lr):
            t = torch.as_tensor(lr)
            t = lr_to_tensor(t if t.dim() == 4 else t[None])
            if t.shape[0] != 1 or t.shape[1] != C:
                raise RuntimeError(f"one LR image of {C} channels per request, got {tuple(t.shape)}")
            return t[0].to(dev).contiguous()

        def deliver(r):
            # p_sample_loop's ret_img for one image: the conditioning image, then its frames
            return torch.cat([r.cond.to(torch.float32)[None], r.frames], dim=0) if r.continous else r.out

        return RollingSampler(eng, int(slots), self.num_sampling_steps, self._draw_seed() if seed is None else int(seed),
                              precision=getattr(eng, "precision", "f32"), strict=self.denoise_fn.strict_range,
                              start_steps=lambda S, strength: self.start_steps(S, strength=strength), alloc=alloc,
                              ready=self.denoise_fn.ready, finish=self.denoise_fn.finish, lr_size=lr_size, to_lr=to_lr,
                              alloc_frames=alloc_frames, deliver=deliver, elastic=elastic, ladder=ladder)

    @torch.no_grad()
    def p_sample_loop(self, x_in, continous=False, noise=None, seed=None):
        """Reference return convention (diffusion.py:212-215): `ret_img` = cat([x_in, frames...])
        if continous else `ret_img[-1]` — the LAST image of the batch, shape [C,H,W]."""
        if not continous:
            return self.sample_batch(x_in, False, noise, seed)[-1]
        if seed is None:
            seed = self._draw_seed()
        out, frames = self.sample_batch(x_in, True, noise, seed)
        if self.conditional:
            first = x_in.to(torch.float32)
        elif noise is not None:
            # unconditional branch: ret_img starts with the initial noise image (diffusion.py:193-201,
            # `img = torch.randn(shape); ret_img = img`) = slab 0 of the injected noise
            first = noise[0].to(device=out.device, dtype=torch.float32)
        else:
            # device RNG: the initial image is draw 0 of every image's Philox stream
            # (init_state_kernel); regenerate it from the same (seed, image index) keys
            first = torch.empty_like(out)
            eng, n = self._engine(), out[0].numel()
            self.denoise_fn.ready()
            for i in range(out.shape[0]):
                eng.philox_normal_into(seed, i, 0, n, first[i].data_ptr())
            self.denoise_fn.finish()
        return torch.cat([first, frames.reshape(-1, *frames.shape[2:])], dim=0)

    @torch.no_grad()
    def sample(self, batch_size=1, continous=False):
        s = self.image_size
        return self.p_sample_loop((batch_size, self.channels, s, s), continous)

    @torch.no_grad()
    def super_resolution(self, x_in, continous=False):
        return self.p_sample_loop(x_in, continous)

    @torch.no_grad()
    def super_resolution_batch(self, x_in, noise=None, seed=None, image_offset=0, max_chunk=None, init=None, start=None,
                               noised=None):
        """Throughput entry point: every image of the batch, [B,3,H,W] (any B: see sample_batch, also for the warm
        start's init / start / noised)."""
        return self.sample_batch(x_in, False, noise, seed, image_offset, max_chunk, init=init, start=start, noised=noised)

    @torch.no_grad()
    def refine(self, x_in, img, strength, noise=None, seed=None, image_offset=0, max_chunk=None, noised=True):
        """Refines an existing image — the result of a cheaper run or of a previous cascade stage — under the
        conditioning x_in: img [B,C,H,W] is forward-diffused to the level of `strength` (a float in (0, 1], or s0 as an
        int) and the last s0 steps run from there. super_resolution_batch(x_in, init=img, start=strength)."""
        return self.super_resolution_batch(x_in, noise, seed, image_offset, max_chunk, init=img, start=strength, noised=noised)

    @torch.no_grad()
    def interpolate(self, x1, x2, t=None, lam=0.5, x_in=None, noise=None, noise2=None, seed=None):
        """The `interpolate` member of the reference's ddpm variant (model/sr/ddpm_modules/diffusion.py:243-257): both
        images are noised with independent noise (q_sample on the device), mixed as (1 - lam) * xt1 + lam * xt2, and the
        last t steps of the loop, i = t-1 .. 0, run from the mix (an un-noised start with s0 = t). No new device code.

        The level convention is this class's: the mix is the state before step t-1, so both images are noised to
        sqrt_alphas_cumprod_prev[t] (entry t of the S-step level table under a few-step sampler) — the level step t-1
        feeds the UNet. That is ONE index below the ddpm variant's, whose q_sample(t) noises with sqrt_alphas_cumprod[t] =
        sqrt_alphas_cumprod_prev[t+1] before the same steps t-1 .. 0. t=None is S-1, the variant's default.

        x_in: the conditioning ([B,Cc,H,W]) of the conditional model. noise: optional [t,B,C,H,W]; slab 0 noises x1 (and is
        the unread slab 0 of the loop), slab k is the draw of step t-k. noise2: optional [B,C,H,W] noising x2. Without
        them the two q_sample draws are torch.randn_like (as the reference's) and the loop draws from Philox under `seed`."""
        self._engine()
        S = self.num_sampling_steps
        s0 = self.start_steps(S, step=S - 1 if t is None else t)
        if self.conditional and x_in is None:
            raise RuntimeError("the conditional model interpolates under a conditioning image: pass x_in")
        x1 = x1.to(torch.float32).contiguous()
        x2 = x2.to(device=x1.device, dtype=torch.float32).contiguous()
        if x1.shape != x2.shape:
            raise RuntimeError(f"x1 {tuple(x1.shape)} and x2 {tuple(x2.shape)} differ in shape")
        level = torch.full((x1.shape[0],), float(self._levels_pushed[s0]), dtype=torch.float32)
        xt1 = self.q_sample(x1, level, None if noise is None else noise[0])
        xt2 = self.q_sample(x2, level, noise2)
        mix = (1.0 - float(lam)) * xt1 + float(lam) * xt2
        cond = x_in if self.conditional else tuple(x1.shape)
        return self.sample_batch(cond, False, noise, seed, init=mix, start=s0, noised=False)

    @torch.no_grad()
    def p_sample(self, x, t, clip_denoised=True, condition_x=None, noise=None):
        """One reverse step (diffusion.py:182-187) on the device."""
        if not clip_denoised:
            raise NotImplementedError("clip_denoised=False is never used by the reference")
        eng = self._ddpm_engine()
        x = x.to(torch.float32).contiguous()
        B, _, H, W = x.shape
        cond = condition_x.to(torch.float32).contiguous() if condition_x is not None else None
        if noise is None and t > 0:
            noise = torch.randn_like(x)
        nz = noise.to(torch.float32).contiguous() if (noise is not None and t > 0) else None
        out = torch.empty_like(x)
        self.denoise_fn.arm_dropout(eng)

        def one_step():
            self.denoise_fn.ready()
            if getattr(eng, "_lr_on", False):       # (the reference's single step: never projected)
                eng.set_lr_consistency(None)
                eng._lr_on = False
            if getattr(eng, "_dyn_set", None) is not None:      # (nor thresholded)
                eng.set_dynamic_threshold(None)
                eng._dyn_set = None
            eng.sample_begin(cond.data_ptr() if cond is not None else None, B, H, W, x.data_ptr(), 0, 0)
            eng.sample_step(int(t), nz.data_ptr() if nz is not None else None)
            eng.sample_end(out.data_ptr())

        # The step API cannot replay inside the library (the caller owns the noise); this facade still holds x, cond and
        # noise, so it finishes the step like sr3_sample would: an in-place split-K wait that gave up -> the same step again
        # (the library has switched to its non-waiting conv path); an out-of-range step -> one arithmetic down, f16f8 ->
        # f16x3 -> exact f32 (the reference computes in fp32 and has no range limit, unet.py:235-265).
        import warnings
        from ._lib import Sr3RangeWarning, Sr3ReplayWarning
        prev = getattr(eng, "precision", "f32")
        ladder = {"f16f8": ["f16x3", "f32"], "f16x3": ["f32"], "f32": []}[prev]
        try:
            for attempt in range(8):
                try:
                    one_step()
                    break
                except Sr3Error as e:
                    msg = str(e)
                    if "repeat the call" in msg and attempt == 0:
                        warnings.warn(Sr3ReplayWarning(f"p_sample(t={int(t)}) repeated: {e}"), stacklevel=2)
                        continue
                    if "range" not in msg or not ladder or self.denoise_fn.strict_range:
                        raise
                    nxt = ladder.pop(0)
                    eng.set_precision(nxt)
                    warnings.warn(Sr3RangeWarning(f"p_sample(t={int(t)}) recomputed in {nxt}: {e}"), stacklevel=2)
        finally:
            if getattr(eng, "precision", prev) != prev:
                eng.set_precision(prev)
        self.denoise_fn.finish()
        return out

    # ---- small closed-form members kept for API completeness (diffusion.py:144-180) -------------
    def predict_start_from_noise(self, x_t, t, noise):
        return self.sqrt_recip_alphas_cumprod[t] * x_t - self.sqrt_recipm1_alphas_cumprod[t] * noise

    def q_posterior(self, x_start, x_t, t):
        mean = self.posterior_mean_coef1[t] * x_start + self.posterior_mean_coef2[t] * x_t
        return mean, self.posterior_log_variance_clipped[t]

    @torch.no_grad()
    def p_mean_variance(self, x, t, clip_denoised: bool, condition_x=None):
        B = x.shape[0]
        nl = torch.full((B, 1), float(np.float32(self.sqrt_alphas_cumprod_prev[t + 1])),
                        dtype=torch.float32, device=x.device)
        inp = torch.cat([condition_x, x], dim=1) if condition_x is not None else x
        x_recon = self.predict_start_from_noise(x, t, self.denoise_fn(inp, nl))
        if clip_denoised:
            x_recon.clamp_(-1.0, 1.0)
        return self.q_posterior(x_recon, x, t)

    # ---- the denoising loss, evaluated on the device ---------------------------
    def _loss_rows(self, hr, sr, levels, loss_type, noise=None, noise_per_source=False, seed=0, image_offset=0,
                   row_offset=0, max_chunk=None, want=()):
        """sr3_denoise_loss over `len(levels)` rows: row b noises hr[(row_offset + b) % N] at levels[b]. levels: fp32
        CPU tensor. noise: [rows,C,H,W] (or [N,C,H,W] with noise_per_source) or None (Philox keyed by image_offset + row,
        or + source image). Rows above the per-call limit run as equal chunks (chunk_plan; the last one padded, its
        extra rows discarded). Returns {"per_image": fp64 [rows]} plus "x_noisy" / "eps" [rows,C,H,W] if named in want."""
        eng = self._engine()
        dev = hr.device
        N, C, H, W = hr.shape
        R = int(levels.numel())
        levels = levels.to("cpu", torch.float32).reshape(-1).contiguous()
        s = torch.from_numpy(noise_coefficient(levels.numpy()))
        out = {"per_image": torch.empty(R, dtype=torch.float64, device=dev)}
        for k in want:
            out[k] = torch.empty((R, C, H, W), dtype=torch.float32, device=dev)
        limit = eng.max_batch(H, W)
        if max_chunk is not None:
            limit = max(1, min(limit, int(max_chunk)))
        n_chunks, chunk = self.chunk_plan(R, limit)
        self.denoise_fn.arm_dropout(eng)            # (one dropout seed per call; the chunks pass their image offset)

        def padded(t, a, b):
            part = t[a:b]
            if b - a < chunk:
                part = torch.cat([part] + [part[-1:]] * (chunk - (b - a)), dim=0)
            return part.contiguous()

        for k in range(n_chunks):
            a, b = k * chunk, min(R, (k + 1) * chunk)
            whole = b - a == chunk
            lv, sv = padded(levels, a, b).to(dev), padded(s, a, b).to(dev)
            nz = None
            if noise is not None:
                nz = noise if noise_per_source else padded(noise, a, b)
            bufs = {name: (t[a:b] if whole else torch.empty((chunk,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev))
                    for name, t in out.items()}
            self.denoise_fn.ready()
            eng.denoise_loss(hr.data_ptr(), sr.data_ptr() if sr is not None else None, N, row_offset + a,
                             lv.data_ptr(), sv.data_ptr(), chunk, H, W, bufs["per_image"].data_ptr(), loss_type,
                             nz.data_ptr() if nz is not None else None, noise_per_source, seed,
                             image_offset if noise_per_source else image_offset + a,
                             bufs["x_noisy"].data_ptr() if "x_noisy" in bufs else None,
                             bufs["eps"].data_ptr() if "eps" in bufs else None)
            self.denoise_fn.finish()
            if not whole:
                for name, t in out.items():
                    t[a:b] = bufs[name][: b - a]
        return out

    def _loss_inputs(self, x_in):
        if getattr(self, "loss_func", None) is None:
            raise NotImplementedError("no loss function: call set_loss(device) first (reference diffusion.py:85-91)")
        if next(self.denoise_fn.parameters()).device.type != "cuda":
            raise NotImplementedError("the denoising loss is evaluated by the HIP library only: p_losses has no CPU "
                                      "implementation (move the model to the GPU)")
        dev = next(self.denoise_fn.parameters()).device
        if x_in["HR"].device != dev:        # the library reads raw device addresses: a host tensor must never reach it
            raise RuntimeError(f"x_in['HR'] is on {x_in['HR'].device}: it must be on the model's device ({dev})")
        hr = x_in["HR"].to(torch.float32).contiguous()
        sr = x_in["SR"].to(device=hr.device, dtype=torch.float32).contiguous() if self.conditional else None
        if hr.dim() != 4 or hr.shape[1] != self.channels or (sr is not None and sr.shape[0] != hr.shape[0]):
            raise RuntimeError(f"expected HR [B, {self.channels}, H, W] and SR with the same B, got {tuple(hr.shape)}"
                               + (f" and {tuple(sr.shape)}" if sr is not None else ""))
        return hr, sr

    @torch.no_grad()
    def q_sample(self, x_start, continuous_sqrt_alpha_cumprod, noise=None):
        """diffusion.py:275-282 on the device, bit-equal to the reference expression on the same fp32 inputs (with
        sqrt(1 - a^2) formed as noise_coefficient does).
        continuous_sqrt_alpha_cumprod: one level per image (any shape with B entries). noise=None draws one
        torch.randn_like, as the reference does."""
        dev = next(self.denoise_fn.parameters()).device
        if dev.type != "cuda" or x_start.device != dev:     # (raw device addresses cross into the library)
            raise RuntimeError(f"x_start is on {x_start.device} and the model on {dev}: both must be on the same GPU")
        x = x_start.to(torch.float32).contiguous()
        B, C, H, W = x.shape
        lv = continuous_sqrt_alpha_cumprod.detach().to("cpu", torch.float32).reshape(-1)
        if lv.numel() != B:
            raise RuntimeError(f"need one level per image ({B}), got {lv.numel()}")
        nz = (torch.randn_like(x) if noise is None else noise.to(device=x.device, dtype=torch.float32)).contiguous()
        sv = torch.from_numpy(noise_coefficient(lv.numpy())).to(x.device)
        lv = lv.contiguous().to(x.device)
        out = torch.empty_like(x)
        eng = self.denoise_fn.engine()
        self.denoise_fn.ready()
        eng.q_sample(x.data_ptr(), B, 0, lv.data_ptr(), sv.data_ptr(), B, C, H, W, out.data_ptr(), nz.data_ptr())
        self.denoise_fn.finish()
        return out

    @torch.no_grad()
    def p_losses(self, x_in, noise=None, sr_out=False, seed: Optional[int] = None, image_offset: int = 0,
                 max_chunk: Optional[int] = None):
        """The reference's denoising loss (diffusion.py:284-313), EVALUATED on the device: no gradient is formed and
        the result carries no grad_fn (backward passes are out of scope).

        x_in: {'HR': [B,C,H,W], 'SR': [B,C,H,W]}. The timestep and the B noise levels are drawn on the host with the
        reference's own np.random calls (draw_levels), so np.random.seed reproduces the reference's levels. noise: the
        [B,C,H,W] tensor the reference would draw; None draws it on the device from Philox (the sampler's generator,
        not torch.randn) under `seed` (None: a fresh one from torch's generator, as sample_batch draws one), keyed by
        image_offset + row. Dropout is the identity unless set_dropout_sampling(True) opted in: without it,
        in train() mode with dropout > 0 this differs from the reference's stochastic forward, and one UserWarning per
        object says so; with it the block2 masks are sampled on the device.

        Returns the SUM over the batch — L1Loss / MSELoss(reduction='sum'), callers divide by b*c*h*w themselves — as a
        0-dim fp32 tensor on the input's device; the fp64 per-image sums stay on self.last_loss_per_image. Batches above
        the library's per-call limit run as chunks (max_chunk lowers it). sr_out=True returns
        super_resolution(x_in['SR']) — the reference's ret_img[-1] — without the forward the reference runs and
        discards first."""
        if sr_out:
            return self.super_resolution(x_in["SR"])
        hr, sr = self._loss_inputs(x_in)
        if (self.training and float(self.denoise_fn.cfg.dropout) > 0 and not self.denoise_fn.dropout_live()
                and not getattr(self, "_warned_dropout", False)):
            import warnings
            warnings.warn("p_losses in train() mode: the library evaluates the UNet with dropout as the identity "
                          f"(dropout={self.denoise_fn.cfg.dropout} is not sampled); the loss is the eval() loss",
                          UserWarning, stacklevel=2)
            self._warned_dropout = True
        B = hr.shape[0]
        _, levels = draw_levels(self.sqrt_alphas_cumprod_prev, self.num_timesteps, B)
        if noise is not None:
            noise = noise.to(device=hr.device, dtype=torch.float32).contiguous()
            if tuple(noise.shape) != tuple(hr.shape):
                raise RuntimeError(f"noise must be {tuple(hr.shape)}, got {tuple(noise.shape)}")
        elif seed is None:
            seed = self._draw_seed()
        res = self._loss_rows(hr, sr, torch.from_numpy(levels), self.loss_func, noise=noise, seed=seed or 0,
                              image_offset=image_offset, max_chunk=max_chunk)
        self.last_loss_per_image = res["per_image"]
        return res["per_image"].sum().to(torch.float32)

    def forward(self, x, sr_out=False, *args, **kwargs):
        """diffusion.py:315-318: unwraps a DictTensor and evaluates p_losses."""
        if isinstance(x, DictTensor):
            x = x.data
        return self.p_losses(x, sr_out=sr_out, *args, **kwargs)

    # ---- training members: out of scope --------------------------------------------
    def super_resolution_learn(self, *args, **kwargs):
        raise NotImplementedError("differentiable sampling (*_learn) needs a backward pass: out of scope")

    p_sample_loop_learn = super_resolution_learn
