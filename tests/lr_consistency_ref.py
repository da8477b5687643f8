"""float64 restatement of the low-resolution consistency projection and of a projected sampler chain.
Test infrastructure: the operators are derived here again from Pillow's published precompute_coeffs (real weights, before
the fixed-point rounding) and numpy's solver, independently of the library's Cholesky; the chain runs the CPU oracle's
UNet (oracle/sr3_oracle.unet_forward) and the update in float64 from the fp32 table values. Not a test module."""
import math

import numpy as np

import fast_sampler_ref as fast
import sr3_oracle as oracle
from pil_bicubic import bicubic_filter

F32 = np.float32


def real_coeffs(in_size, out_size):
    """A [out, in] float64: the normalised real weights of Resample.c precompute_coeffs for the bicubic filter, and the
    bounds [out, 2] (first input, count) they occupy."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    A = np.zeros((out_size, in_size), dtype=np.float64)
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic_filter((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        A[xx, xmin:xmin + xmax] = [v / ww if ww != 0.0 else v for v in w]
        bounds[xx] = (xmin, xmax)
    return A, bounds


def operators(l, r):
    """(A [l,r], P [r,l]) float64 with P = A^T (A A^T)^-1."""
    A, _ = real_coeffs(r, l)
    return A, np.linalg.solve(A @ A.T, A).T


def downsample(img, lh, lw):
    """A_v img A_h^T per plane in float64: img [..., H, W] -> [..., lh, lw]."""
    img = np.asarray(img, dtype=np.float64)
    Av, _ = real_coeffs(img.shape[-2], lh)
    Ah, _ = real_coeffs(img.shape[-1], lw)
    return Av @ img @ Ah.T


def project(x, lr, row_offset=0, strength=1.0):
    """X + strength * P_v (Y - A_v X A_h^T) P_h^T in float64; row b is held to lr[(row_offset + b) % N]."""
    x, lr = np.asarray(x, dtype=np.float64), np.asarray(lr, dtype=np.float64)
    B, N = x.shape[0], lr.shape[0]
    Av, Pv = operators(lr.shape[-2], x.shape[-2])
    Ah, Ph = operators(lr.shape[-1], x.shape[-1])
    y = lr[[(row_offset + b) % N for b in range(B)]]
    return x + strength * (Pv @ (y - Av @ x @ Ah.T) @ Ph.T)


def residual(img, lr, row_offset=0):
    """{"sumsq": [B], "max_abs": [B]} of A img - y in float64."""
    lr = np.asarray(lr, dtype=np.float64)
    B, N = img.shape[0], lr.shape[0]
    d = downsample(img, lr.shape[-2], lr.shape[-1]) - lr[[(row_offset + b) % N for b in range(B)]]
    return {"sumsq": (d * d).reshape(B, -1).sum(1), "max_abs": np.abs(d).reshape(B, -1).max(1)}


def ddpm_coefficients(sched_opt):
    """The per-step values of the reference's loop (oracle.p_sample) in the form of fast.coefficients."""
    s = oracle.noise_schedule(sched_opt)
    T = int(s["betas"].shape[0])
    return [{"nl": F32(s["sqrt_alphas_cumprod_prev"][t + 1]), "a": s["sqrt_recip_alphas_cumprod"][t],
             "b": s["sqrt_recipm1_alphas_cumprod"][t], "c1": s["posterior_mean_coef1"][t], "c2": s["posterior_mean_coef2"][t],
             "c3": 0.0, "sigma": float(np.exp(F32(0.5) * s["posterior_log_variance_clipped"][t]).astype(F32)) if t > 0 else 0.0}
            for t in range(T)]


def sample_loop(sd, cfg, sched_opt, cond, noise, kind, S=None, eta=0.0, lr=None, row_offset=0, strength=1.0, coefs=None):
    """The loop of sr3_sample with the projection between the x0 prediction and the posterior update (lr None: without),
    the RNG replaced by `noise` [S,B,C,H,W] as in fast.sample_loop; kind "ddpm" runs all T steps. The UNet is the fp32
    oracle; everything around it is float64 over the fp32 table values. Returns (final, frames) as float64."""
    co = coefs if coefs is not None else (ddpm_coefficients(sched_opt) if kind == "ddpm" else fast.coefficients(sched_opt, kind, S, eta))
    S = len(co)
    si = 1 | (S // 10)
    x = np.asarray(noise[0], dtype=np.float64)
    B = x.shape[0]
    hist = None
    frames = []

    def f(v):
        return float(F32(v))

    for k, i in enumerate(reversed(range(S))):
        c = co[i]
        xf = x.astype(F32)
        inp = np.concatenate([cond, xf], axis=1) if cond is not None else xf
        eps = oracle.unet_forward(sd, cfg, inp, np.full((B,), c["nl"], dtype=F32)).astype(np.float64)
        x0 = np.clip(f(c["a"]) * x - f(c["b"]) * eps, -1.0, 1.0)
        if lr is not None:
            x0 = project(x0, lr, row_offset, strength)
        v = f(c["c1"]) * x0 + f(c["c2"]) * x
        if hist is not None and c["c3"] != 0.0:
            v = v + f(c["c3"]) * hist
        if c["sigma"] != 0.0:
            v = v + np.asarray(noise[k + 1], dtype=np.float64) * f(c["sigma"])
        hist = x0
        x = v
        if i % si == 0:
            frames.append(x.copy())
    return x, np.stack(frames, axis=0)
