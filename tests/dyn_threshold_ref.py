"""numpy restatement of the dynamic thresholding of the sampler's x0 prediction: the order statistics
by a sort of the integer keys, the fp32 expressions with every operation rounded by itself (numpy's float32 arithmetic),
and a sampler loop whose eps comes from a callback, in the operation order of the HIP update kernels. Test
infrastructure, independent of the library's radix select. Not a test module (no test_ prefix)."""
import math

import numpy as np

F32 = np.float32


def keys(x):
    """The bit patterns of |x| as unsigned integers: a total order (-0 = +0, denormals kept, NaN above inf)."""
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def plan(ratio, n):
    """(k, k2, frac) of the fp32 ratio over n values: pos = (double)ratio * (n - 1), k = min(floor(pos), n - 1),
    k2 = min(k + 1, n - 1), frac = (float)(pos - k)."""
    pos = float(F32(ratio)) * (n - 1)
    k = min(int(math.floor(pos)), n - 1)
    return k, min(k + 1, n - 1), F32(pos - k)


def select(x, ratio, max_value=None):
    """x [B, ...]: per image {"lo", "hi", "s_raw", "s"} as fp32 [B]."""
    x = np.ascontiguousarray(x, dtype=F32)
    B = x.shape[0]
    srt = np.sort(keys(x).reshape(B, -1), axis=1)
    k, k2, frac = plan(ratio, srt.shape[1])
    lo = np.ascontiguousarray(srt[:, k]).view(F32)
    hi = np.ascontiguousarray(srt[:, k2]).view(F32)
    with np.errstate(all="ignore"):
        s_raw = (lo + (frac * (hi - lo)).astype(F32)).astype(F32)
    cap = F32(np.inf if max_value is None else max_value)
    s = np.fmin(np.fmax(s_raw, F32(1.0)), cap).astype(F32)      # (fmaxf / fminf: a NaN s_raw gives 1)
    return {"lo": lo, "hi": hi, "s_raw": s_raw, "s": s}


def apply(x, s):
    """clamp(x, -s, s) / s per image in fp32 (fmaxf / fminf / a correctly rounded division)."""
    x = np.ascontiguousarray(x, dtype=F32)
    sb = np.asarray(s, dtype=F32).reshape((-1,) + (1,) * (x.ndim - 1))
    with np.errstate(all="ignore"):
        return (np.fmin(np.fmax(x, -sb), sb) / sb).astype(F32)


def threshold(x, ratio, max_value=None):
    """(thresholded x, s [B])."""
    s = select(x, ratio, max_value)["s"]
    return apply(x, s), s


def sample_loop(eps_fn, co, noise, ratio=None, max_value=None, project=None, history="thresholded"):
    """The loop of sr3_sample in fp32, statement for statement as the update kernels run it. eps_fn(x, nl) -> eps
    [B,C,H,W] for the state x and the step's noise level; co: the per-step coefficient dicts (nl, a, b, c1, c2, c3, sigma)
    of fast_sampler_ref.coefficients / lr_consistency_ref.ddpm_coefficients, indexed by step i (the loop runs i = S-1 .. 0);
    noise [S,B,C,H,W]: slab 0 the initial image, slab k the draw of step i = S-k. ratio None: the static clamp.
    project(x0) -> x0: the low-resolution projection, after the threshold. history "clamped": what a library that kept the
    static clamp's x0 in the dpmpp_2m history would compute (a test shows the difference).
    Returns {"final", "states" [S,B,C,H,W] (the state after every step), "s" [S,B], "x0" [S,B,C,H,W]}."""
    S = len(co)
    x = np.asarray(noise[0], dtype=F32)
    hist = None
    states, ss, x0s = [], [], []
    for k, i in enumerate(reversed(range(S))):
        c = co[i]
        eps = np.asarray(eps_fn(x, c["nl"]), dtype=F32)
        raw = (F32(c["a"]) * x - F32(c["b"]) * eps).astype(F32)
        if ratio is None:
            x0, s = np.fmin(np.fmax(raw, F32(-1.0)), F32(1.0)).astype(F32), np.ones(x.shape[0], F32)
        else:
            x0, s = threshold(raw, ratio, max_value)
        keep = x0 if history == "thresholded" else np.fmin(np.fmax(raw, F32(-1.0)), F32(1.0)).astype(F32)
        if project is not None:
            x0 = np.asarray(project(x0), dtype=F32)
            keep = x0
        v = (F32(c["c1"]) * x0 + F32(c["c2"]) * x).astype(F32)
        if hist is not None and c["c3"] != 0.0:
            v = (v + F32(c["c3"]) * hist).astype(F32)
        if c["sigma"] != 0.0:
            v = (v + np.asarray(noise[k + 1], dtype=F32) * F32(c["sigma"])).astype(F32)
        hist = keep
        x = v
        states.append(x.copy())
        ss.append(s)
        x0s.append(x0)
    return {"final": x, "states": np.stack(states), "s": np.stack(ss), "x0": np.stack(x0s)}
