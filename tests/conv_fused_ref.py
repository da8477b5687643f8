"""float64 side of test_gpu_conv_fused.py (TEST INFRASTRUCTURE, not collected by pytest): the data of one case of the
ResnetBlock's second launch and its reference

    conv3x3_f64(act(x), w) + [in2 ‖ in2b] @ w2^T + b + b2 + chan_bias + resid          (every operand widened to float64)

Data: x, in2, in2b, biases and residual ~ N(0,1); w ~ N(0,1) / sqrt(9 Cin); w2 ~ N(0,1) / sqrt(C2a + C2b). Large batches
repeat three distinct images, so the float64 conv runs on three; image B-1 is a copy of image 0 in every input.
"""
import numpy as np

import gn_stats_ref as gn


def images(B):
    """index of the distinct image behind each batch entry: image B-1 is image 0, the middle one differs, and from B = 5
    on three distinct images take turns in between."""
    idx = np.arange(B) % 3
    idx[0], idx[B // 2], idx[-1] = 0, 1, 0
    if B <= 2:
        idx[:] = 0
    return idx


def conv3x3_f64(x, w):
    """3x3 / stride 1 / padding 1 on NHWC x, w OIHW, in float64."""
    B, H, W, C = x.shape
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    w64 = w.astype(np.float64)
    out = np.zeros((B * H * W, w.shape[0]), np.float64)
    for dy in range(3):
        for dx in range(3):
            out += np.ascontiguousarray(xp[:, dy:dy + H, dx:dx + W, :]).reshape(-1, C) @ np.ascontiguousarray(w64[:, :, dy, dx].T)
    return out.reshape(B, H, W, -1)


def exact_split(v):
    """float32 values -> (the uint32 words of the split format, the float64 values hi + lo those words stand for)."""
    words = gn.pack_format(v, 1)
    hi, lo = gn.split_halves(words)
    return words, hi + lo


def case_data(shape, term, gnorm=False, resid=True, seed=0):
    """Distinct-image tensors of one case (first axis: the distinct images) and the float64 reference `want`.
    term: (C2a, C2b) of the 1x1 term, "ident" (in2 = a block input of Cout channels, added as it is), or None."""
    B, H, W, Cin, Cout = shape
    idx = images(B)
    nd = int(idx.max()) + 1
    rs = np.random.RandomState((B * 7919 + H * 131 + W * 17 + Cin * 3 + Cout + seed) & 0xFFFFFFF)
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    d = {"idx": idx, "nd": nd}
    d["x"] = f32(nd, H, W, Cin) * 2 + 0.5 if gnorm else f32(nd, H, W, Cin)
    d["w"] = f32(Cout, Cin, 3, 3) / np.float32(np.sqrt(9 * Cin))
    d["b"], d["cb"] = f32(Cout), f32(nd, Cout)
    d["resid"] = f32(nd, H, W, Cout) if resid else None
    d["gamma"], d["beta"] = 1 + 0.1 * f32(Cin), 0.1 * f32(Cin)
    d["in2"] = d["in2b"] = d["w2"] = d["b2"] = None
    if term == "ident":
        d["in2"] = f32(nd, H, W, Cout)
    elif term is not None:
        C2a, C2b = term
        d["in2"] = f32(nd, H, W, C2a)
        d["in2b"] = f32(nd, H, W, C2b) if C2b else None
        d["w2"] = f32(Cout, C2a + C2b) / np.float32(np.sqrt(C2a + C2b))
        d["b2"] = f32(Cout)
    d["want"] = reference(d, gnorm)
    return d


def reference(d, gnorm=False, resid64=None):
    """float64 reference of the data d (resid64: the residual's values where they are not d["resid"] itself)."""
    xin = gn.group_norm64(d["x"], d["gamma"], d["beta"], 32, swish=True) if gnorm else d["x"]
    want = conv3x3_f64(xin, d["w"]) + d["b"].astype(np.float64) + d["cb"].astype(np.float64)[:, None, None, :]
    if d["w2"] is not None:
        cat = d["in2"] if d["in2b"] is None else np.concatenate([d["in2"], d["in2b"]], -1)
        want += cat.astype(np.float64) @ d["w2"].astype(np.float64).T + d["b2"].astype(np.float64)
    elif d["in2"] is not None:
        want += d["in2"].astype(np.float64)
    if resid64 is not None:
        want += resid64
    elif d["resid"] is not None:
        want += d["resid"].astype(np.float64)
    return want
