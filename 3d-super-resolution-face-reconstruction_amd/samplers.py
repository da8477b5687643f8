"""Few-step samplers over an SR3 noise schedule: the per-step tables of
sr3_set_sampler_schedule, computed on the host in float64 and cast to fp32 once.

SR3's UNet is conditioned on the continuous noise level sqrt(alpha_bar) (reference
model/sr/sr3_modules/diffusion.py:284-296 draws it between table entries in training), so a sampler may
visit any subset of the schedule's levels:

  "ddpm"      the reference's ancestral loop (S = T only): the registered buffers as they are
  "ddim"      deterministic at eta = 0 (Song et al. 2021); eta = 1, S = T is the DDPM posterior
  "dpmpp_2m"  DPM-Solver++(2M), data prediction (Lu et al. 2022): second order, one UNet call per step
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

KINDS = ("ddpm", "ddim", "dpmpp_2m")


def sampler_levels(T: int, S: int) -> np.ndarray:
    """K_j = floor(j T / S), j = 0..S: K_0 = 0, K_S = T, strictly increasing (S <= T)."""
    return (np.arange(S + 1, dtype=np.int64) * int(T)) // int(S)


def check_sampler(kind: str, steps, eta: float, T: Optional[int]) -> Optional[int]:
    """Validates a sampler setting against a schedule of T steps (None: not known yet); returns S."""
    if kind not in KINDS:
        raise ValueError(f"unknown sampler {kind!r}: one of {', '.join(KINDS)}")
    if steps is not None and (isinstance(steps, bool) or int(steps) != steps):
        raise ValueError(f"steps must be an integer, got {steps!r}")
    S = T if steps is None else int(steps)
    if S is not None and (S < 1 or (T is not None and S > T)):
        raise ValueError(f"steps must lie in [1, T] for a schedule of T = {T} steps, got {S}")
    eta = float(eta)
    if not np.isfinite(eta) or eta < 0.0:
        raise ValueError(f"eta must be >= 0, got {eta}")
    if kind != "ddim" and eta != 0.0:
        raise ValueError(f"eta applies to the 'ddim' sampler only, not {kind!r}")
    if kind == "ddpm" and T is not None and S != T:
        raise ValueError(f"the 'ddpm' sampler runs every step of the schedule (steps = {T}), got {S}")
    return S


def sampler_tables(bufs: Dict[str, np.ndarray], kind: str = "ddpm", steps=None, eta: float = 0.0) -> Dict:
    """bufs: schedule.schedule_buffers(...) (or the same keys). Returns {"S", "kind", "uses_history",
    "noise_level" [S+1], "a", "b", "c1", "c2", "c3", "sigma" [S]} (fp32, indexed by the step index i = S-1 .. 0).
    "ddpm" returns the reference's buffers instead of c3 / sigma: "noise_level", "a", "b", "c1", "c2" and "logvar",
    which Engine.set_sampler_schedule passes to sr3_set_schedule unchanged."""
    sqrt_prev = np.asarray(bufs["sqrt_alphas_cumprod_prev"], dtype=np.float64)    # sqrt(abar(k)), k = 0..T
    T = int(sqrt_prev.size - 1)
    S = check_sampler(kind, steps, eta, T)
    f4 = np.float32
    if kind == "ddpm":       # the reference's buffers for sr3_set_schedule (the library derives sigma from logvar)
        return {"S": T, "uses_history": False, "kind": kind,
                "logvar": np.asarray(bufs["posterior_log_variance_clipped"], dtype=f4),
                "noise_level": np.asarray(bufs["noise_level"], dtype=f4),
                "a": np.asarray(bufs["sqrt_recip_alphas_cumprod"], dtype=f4),
                "b": np.asarray(bufs["sqrt_recipm1_alphas_cumprod"], dtype=f4),
                "c1": np.asarray(bufs["posterior_mean_coef1"], dtype=f4),
                "c2": np.asarray(bufs["posterior_mean_coef2"], dtype=f4)}
    K = sampler_levels(T, S)
    abar = sqrt_prev * sqrt_prev
    abar[0] = 1.0
    s_lv, t_lv = K[1:], K[:-1]                 # step i goes from level K[i+1] down to K[i]
    ab_s, ab_t = abar[s_lv], abar[t_lv]
    al_s, al_t = sqrt_prev[s_lv], sqrt_prev[t_lv]
    sg_s, sg_t = np.sqrt(1.0 - ab_s), np.sqrt(1.0 - ab_t)
    c3 = np.zeros(S)
    if kind == "ddim":
        sig = eta * np.sqrt((1.0 - ab_t) / (1.0 - ab_s)) * np.sqrt(np.maximum(1.0 - ab_s / ab_t, 0.0))
        d = np.sqrt(np.maximum(1.0 - ab_t - sig * sig, 0.0))
        c1 = al_t - d * al_s / sg_s
        c2 = d / sg_s
    else:
        sig = np.zeros(S)
        c1, c2 = np.ones(S), np.zeros(S)       # the last step (t = 0) is x' = x0: lambda_0 = inf is never formed
        with np.errstate(divide="ignore"):
            lam = np.log(sqrt_prev) - 0.5 * np.log1p(-abar)            # lambda_k, k = 1..T (inf at k = 0)
        for i in range(1, S):                  # t = K[i] > 0
            s, t = K[i + 1], K[i]
            h = lam[t] - lam[s]
            em = np.expm1(-h)
            c2[i] = sg_t[i] / sg_s[i]
            if i == S - 1:                     # the first step of the call: first order
                c1[i] = -al_t[i] * em
            else:
                r = (lam[s] - lam[K[i + 2]]) / h
                c1[i] = -al_t[i] * em * (1.0 + 1.0 / (2.0 * r))
                c3[i] = al_t[i] * em / (2.0 * r)
    return {"S": S, "uses_history": kind == "dpmpp_2m", "kind": kind,
            "noise_level": sqrt_prev[K].astype(f4),
            "a": np.asarray(bufs["sqrt_recip_alphas_cumprod"], dtype=f4)[s_lv - 1],
            "b": np.asarray(bufs["sqrt_recipm1_alphas_cumprod"], dtype=f4)[s_lv - 1],
            "c1": c1.astype(f4), "c2": c2.astype(f4), "c3": c3.astype(f4), "sigma": sig.astype(f4)}
