"""numpy restatement of the feature cache (DeepCache, Ma, Fang, Wang 2023) over the public functions of
the CPU oracle (oracle/sr3_oracle.py): the whole forward that also returns what a later shallow forward needs, the
shallow forward of a depth, and the sampling loops that run a whole forward every `interval`-th step. Test
infrastructure: the module split is derived here from unet_plan, independently of csrc/sr3_api.hip; the loops run in
fp32 in the operation order of oracle.p_sample and of fast_sampler_ref.sample_loop. Not a test module (no test_ prefix)."""
import numpy as np

import fast_sampler_ref
import sr3_oracle as oracle

F32 = np.float32


def max_depth(cfg):
    return len(cfg.channel_mults) - 1


def split(cfg, depth):
    """(fresh_downs, skipped, fresh_ups): the module triples of unet_plan a shallow forward of `depth` runs in front of
    the jump, the ones it jumps over (the last of them produced the cached tensor), and the ones it runs behind it."""
    if not 1 <= depth <= max_depth(cfg):
        raise ValueError(f"depth {depth} outside [1, {max_depth(cfg)}]")
    downs, mid, ups = oracle.unet_plan(cfg)
    rb = cfg.res_blocks
    n_down = 1 + depth * rb + (depth - 1)
    n_up = depth * (rb + 1) + (depth - 1)
    return downs[:n_down], downs[n_down:] + mid + ups[:len(ups) - n_up], ups[len(ups) - n_up:]


def forward(sd, cfg, x_nchw, noise_level, depth=None, cache=None, prefix=""):
    """cache None: the whole UNet.forward (oracle.unet_forward's operations in its order) -> (eps, cache), where cache
    maps the prefix of every Upsample module to its output (NHWC) — what a shallow forward of any depth reads.
    cache given: the shallow forward of `depth` on it -> (eps, cache); feats is empty at its end."""
    g = cfg.norm_groups
    x = np.ascontiguousarray(np.transpose(np.asarray(x_nchw, dtype=F32), (0, 2, 3, 1)))
    temb = oracle.noise_level_mlp(sd, prefix, np.asarray(noise_level, dtype=F32).reshape(-1), cfg.inner_channel)

    def res(p, x, attn):
        x = oracle.resnet_block(sd, prefix + p + ".res_block", x, temb, g)
        return oracle.self_attention(sd, prefix + p + ".attn", x, g) if attn else x

    if cache is None:
        downs, mid, ups = oracle.unet_plan(cfg)
        skipped, out = [], {}
    else:
        downs, skipped, ups = split(cfg, depth)
        mid, out = [], cache
    feats = []
    for kind, p, attn in downs:
        if kind == "conv":
            x = oracle.conv2d(x, sd[prefix + p + ".weight"], sd[prefix + p + ".bias"])
        elif kind == "down":
            x = oracle.conv2d(x, sd[prefix + p + ".conv.weight"], sd[prefix + p + ".conv.bias"], stride=2)
        else:
            x = res(p, x, attn)
        feats.append(x)
    for kind, p, attn in mid:
        x = res(p, x, attn)
    if skipped:
        kind, p, _ = skipped[-1]
        assert kind == "up", (kind, p)
        x = cache[p]
    for kind, p, attn in ups:
        if kind == "up":
            x = oracle.conv2d(oracle.upsample_nearest2(x), sd[prefix + p + ".conv.weight"], sd[prefix + p + ".conv.bias"])
            if cache is None:
                out[p] = x
        else:
            x = res(p, np.concatenate([x, feats.pop()], axis=-1), attn)
    assert not feats, len(feats)
    x = oracle.block(sd, prefix + "final_conv", x, g)
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2))), out


class CachedEps:
    """eps of step k = 0, 1, ... of one sampling call: whole when k % interval == 0, else shallow on the last whole
    step's cache. interval None or <= 1: every step is whole."""

    def __init__(self, sd, cfg, interval, depth):
        self.sd, self.cfg, self.depth = sd, cfg, depth
        self.interval = interval if interval and interval > 1 else 1
        self.k, self.cache, self.whole, self.shallow = 0, None, 0, 0

    def __call__(self, inp, nl):
        if self.k % self.interval == 0:
            eps, self.cache = forward(self.sd, self.cfg, inp, nl)
            self.whole += 1
        else:
            eps, _ = forward(self.sd, self.cfg, inp, nl, self.depth, self.cache)
            self.shallow += 1
        self.k += 1
        return eps


def sample_loop(sd, cfg, sched, cond, noise, interval=None, depth=1):
    """oracle.p_sample_loop (DDPM, T steps, noise [T,B,C,H,W]) with the feature cache: the operations of oracle.p_sample
    in their order, eps from CachedEps. Returns (final, frames)."""
    T = int(sched["betas"].shape[0])
    si = 1 | (T // 10)
    eps_fn = CachedEps(sd, cfg, interval, depth)
    x = np.asarray(noise[0], dtype=F32)
    B = x.shape[0]
    frames = []
    for k, t in enumerate(reversed(range(T))):
        nl = np.full((B,), F32(sched["sqrt_alphas_cumprod_prev"][t + 1]), dtype=F32)
        inp = np.concatenate([cond, x], axis=1) if cond is not None else x
        eps = eps_fn(inp, nl)
        x0 = sched["sqrt_recip_alphas_cumprod"][t] * x - sched["sqrt_recipm1_alphas_cumprod"][t] * eps
        x0 = np.clip(x0, -1.0, 1.0).astype(F32)
        mean = sched["posterior_mean_coef1"][t] * x0 + sched["posterior_mean_coef2"][t] * x
        if t > 0:
            sigma = np.exp(F32(0.5) * sched["posterior_log_variance_clipped"][t]).astype(F32)
            x = (mean + noise[k + 1] * sigma).astype(F32)
        else:
            x = mean.astype(F32)
        if t % si == 0:
            frames.append(x.copy())
    return x, np.stack(frames, axis=0)


def fast_sample_loop(sd, cfg, sched_opt, cond, noise, kind, S, eta=0.0, interval=None, depth=1, coefs=None):
    """fast_sampler_ref.sample_loop (its coefficients, its operation order) with the feature cache."""
    co = coefs if coefs is not None else fast_sampler_ref.coefficients(sched_opt, kind, S, eta)
    si = 1 | (S // 10)
    eps_fn = CachedEps(sd, cfg, interval, depth)
    x = np.asarray(noise[0], dtype=F32)
    B = x.shape[0]
    hist = None
    frames = []
    for k, i in enumerate(reversed(range(S))):
        c = co[i]
        inp = np.concatenate([cond, x], axis=1) if cond is not None else x
        eps = eps_fn(inp, np.full((B,), c["nl"], dtype=F32))
        x0 = np.clip(F32(c["a"]) * x - F32(c["b"]) * eps, -1.0, 1.0).astype(F32)
        v = F32(c["c1"]) * x0 + F32(c["c2"]) * x
        if hist is not None and c["c3"] != 0.0:
            v = v + F32(c["c3"]) * hist
        if c["sigma"] != 0.0:
            v = v + np.asarray(noise[k + 1], dtype=F32) * F32(c["sigma"])
        hist = x0
        x = v.astype(F32)
        if i % si == 0:
            frames.append(x.copy())
    return x, np.stack(frames, axis=0)
