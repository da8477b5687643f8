"""numpy restatement of the sampler's warm start over the CPU oracle: the reference's q_sample
(model/sr/sr3_modules/diffusion.py:275-282) of a start image, then the last s0 steps of a loop — the reference's p_sample
(oracle.p_sample) or a few-step sampler (fast_sampler_ref.coefficients, whose first step here is the first-order one).
Test infrastructure, shared by test_warm_start_host.py and test_gpu_warm_start.py. Not a test module (no test_ prefix)."""
import numpy as np

from conftest import cfg_from_meta, load_golden, pkg      # (first: conftest puts oracle/ on sys.path)

import fast_sampler_ref as fsr
import sr3_oracle as oracle

F32 = np.float32
synth = pkg("synth")


def q_sample(init, level, z):
    """level * init + sqrt(1 - level^2) * z with every operation a correctly rounded fp32 one (diffusion.py:279-282 as
    torch evaluates it: two products and a sum, the coefficient from a product, a difference and a square root)."""
    a = F32(level)
    s = np.sqrt(F32(1) - a * a)
    return (a * np.asarray(init, F32) + s * np.asarray(z, F32)).astype(F32)


def ddpm_tail(sd, cfg, sched, cond, state, noise, s0, T):
    """oracle.p_sample over reversed(range(s0)) from `state`; noise [s0,...]: slab k is the draw of step s0 - k (slab 0 is
    the z of q_sample: not read here). Returns frames [n,B,C,H,W] after the steps i with i % (1 | T // 10) == 0."""
    si = 1 | (T // 10)
    x, frames = np.asarray(state, F32), []
    for i in reversed(range(s0)):
        x = oracle.p_sample(sd, cfg, sched, x, i, cond, noise[s0 - i] if i > 0 else None)
        if i % si == 0:
            frames.append(x.copy())
    return np.stack(frames, axis=0)


def fast_tail(sd, cfg, sched_opt, cond, state, noise, kind, S, s0, eta=0.0):
    """The last s0 steps of fast_sampler_ref.sample_loop from `state`. The first step has no x0 history: for
    "dpmpp_2m" it is the first-order step, whose weight of x0 is c1 + c3 (= alpha_t (1 - e^-h), formed here in float64)."""
    co = [dict(c) for c in fsr.coefficients(sched_opt, kind, S, eta)]
    first = co[s0 - 1]
    first["c1"], first["c3"] = first["c1"] + first["c3"], 0.0
    si = 1 | (S // 10)
    x = np.asarray(state, F32)
    B = x.shape[0]
    hist, frames = None, []
    for i in reversed(range(s0)):
        c = co[i]
        inp = np.concatenate([cond, x], axis=1) if cond is not None else x
        eps = oracle.unet_forward(sd, cfg, inp, np.full((B,), c["nl"], dtype=F32))
        x0 = np.clip(F32(c["a"]) * x - F32(c["b"]) * eps, -1.0, 1.0).astype(F32)
        v = F32(c["c1"]) * x0 + F32(c["c2"]) * x
        if hist is not None and c["c3"] != 0.0:
            v = v + F32(c["c3"]) * hist
        if c["sigma"] != 0.0:
            v = v + np.asarray(noise[s0 - i], dtype=F32) * F32(c["sigma"])
        hist = x0
        x = v.astype(F32)
        if i % si == 0:
            frames.append(x.copy())
    return x, np.stack(frames, axis=0)


_FIXTURE = None


def fixture():
    """warm_start_tiny.npz with its regenerated inputs, loaded once and shared (read-only) by the tests: dict(meta, cfg,
    sd, cond, img, noise [T,B,3,r,r], cases {(s0, tag): (state_sub, frames_sub)})."""
    global _FIXTURE
    if _FIXTURE is None:
        g = load_golden("warm_start_tiny.npz")
        m = g["meta"]
        B, r, T = m["B"], m["r"], m["schedule"]["n_timestep"]
        cfg = cfg_from_meta(m)
        f = {"meta": m, "cfg": cfg, "sd": synth.synth_state_dict(cfg, m["seed"]),
             "cond": synth.synth_cond(B, r, m["l"], m["seed"]), "img": synth.synth_cond(B, r, m["img_l"], m["img_seed"]),
             "noise": synth.synth_noise(T, B, 3, r, r, m["noise_seed"]),
             "cases": {(s0, tag): (g[f"s{s0}.{tag}.state_sub"], g[f"s{s0}.{tag}.frames_sub"])
                       for s0 in m["start_steps"] for tag in m["inits"]}}
        for v in (f["cond"], f["img"], f["noise"]):
            v.setflags(write=False)
        _FIXTURE = f
    return _FIXTURE
