"""numpy restatement of the few-step samplers (DDIM, DPM-Solver++(2M)) over the CPU oracle's UNet
(oracle/sr3_oracle.unet_forward). Test infrastructure: the coefficients are derived here again, step by step in
float64 from the beta schedule, independently of the package's samplers.py; the loop runs in fp32 in the operation
order of the HIP update kernel. Not a test module (no test_ prefix)."""
import math

import numpy as np

import sr3_oracle as oracle

F32 = np.float32


def levels(T, S):
    return [j * T // S for j in range(S + 1)]


def coefficients(sched_opt, kind, S, eta=0.0):
    """Per step index i (S-1 .. 0): dict(nl, a, b, c1, c2, c3, sigma) as float64 / fp32 table values."""
    betas = oracle.make_beta_schedule(sched_opt["schedule"], sched_opt["n_timestep"], sched_opt["linear_start"],
                                      sched_opt["linear_end"])
    T = len(betas)
    abar = [1.0] + list(np.cumprod(1.0 - np.asarray(betas, np.float64)))
    sched = oracle.noise_schedule(sched_opt)
    K = levels(T, S)

    def lam(k):
        return 0.5 * math.log(abar[k]) - 0.5 * math.log(1.0 - abar[k])

    out = []
    for i in range(S):
        s, t = K[i + 1], K[i]
        al_s, al_t = math.sqrt(abar[s]), math.sqrt(abar[t])
        sg_s, sg_t = math.sqrt(1.0 - abar[s]), math.sqrt(1.0 - abar[t])
        c3 = 0.0
        if kind == "ddim":
            var = eta * eta * (1.0 - abar[t]) / (1.0 - abar[s]) * (1.0 - abar[s] / abar[t])
            d = math.sqrt(max(1.0 - abar[t] - var, 0.0))
            sigma = math.sqrt(var)
            c1, c2 = al_t - d * al_s / sg_s, d / sg_s
        elif kind == "dpmpp_2m":
            sigma = 0.0
            if t == 0:
                c1, c2 = 1.0, 0.0
            else:
                h = lam(t) - lam(s)
                phi = -math.expm1(-h)            # 1 - e^{-h}
                c2 = sg_t / sg_s
                if i == S - 1:
                    c1 = al_t * phi
                else:
                    r = (lam(s) - lam(K[i + 2])) / h
                    c1 = al_t * phi * (1.0 + 0.5 / r)
                    c3 = -al_t * phi * 0.5 / r
        else:
            raise ValueError(kind)
        out.append({"nl": F32(sched["sqrt_alphas_cumprod_prev"][s]),
                    "a": sched["sqrt_recip_alphas_cumprod"][s - 1], "b": sched["sqrt_recipm1_alphas_cumprod"][s - 1],
                    "c1": c1, "c2": c2, "c3": c3, "sigma": sigma})
    return out


def sample_loop(sd, cfg, sched_opt, cond, noise, kind, S, eta=0.0, coefs=None):
    """The loop of sr3_sample with the RNG replaced by `noise` [S,B,C,H,W] (slab 0 = the initial image, slab k = the
    noise of step i = S-k). Returns (final [B,C,H,W], frames [n,B,C,H,W]); frames follow i % (1 | S // 10) == 0.
    coefs: the per-step list of coefficients() to use instead (a test may edit it)."""
    co = coefs if coefs is not None else coefficients(sched_opt, kind, S, eta)
    si = 1 | (S // 10)
    x = np.asarray(noise[0], dtype=F32)
    B = x.shape[0]
    hist = None
    frames = []
    for k, i in enumerate(reversed(range(S))):
        c = co[i]
        inp = np.concatenate([cond, x], axis=1) if cond is not None else x
        eps = oracle.unet_forward(sd, cfg, inp, np.full((B,), c["nl"], dtype=F32))
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
