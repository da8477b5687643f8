"""float64 model of the fp8-correction conv (conv3x3_halo_h3<..., F8C = true>, csrc/kernels_conv.hip) evaluated on the
kernel's OWN quantised operands (TEST INFRASTRUCTURE, not collected by pytest; used by test_f8c_ref_host.py,
test_gpu_f8c_model.py and the `f8c` mode of emulate_operand_formats.py):

    out = 2^-k * sum over taps, channels (xh * wh + xl8 * wh8 + xh8 * wl8) + bias + chan_bias + resid

  activations (store8<2>, csrc/kernels_misc.hip; gn_stats_ref.pack_format(g, 2)), per 32-channel chunk
      32 hi halfs | 32 x e4m3(lo * 2^SR3_F8_XL) | 32 x e4m3(g * 2^SR3_F8_XH)       hi = fp16(g), lo = g - hi in fp32
  weights (split_conv_weight_k, then make_f8_weights_kernel), per 32-channel chunk of a [tap][Cout][Cin] row
      32 hi halfs | 32 x e4m3(clamp(hi * 2^SR3_F8_WH)) | 32 x e4m3(clamp(lo * 2^SR3_F8_WL))     of v = w * 2^k
  the powers of two come back through the block scales of v_mfma_scale_f32_32x32x64_f8f6f4.

A correct kernel differs from this model by its fp32 accumulation order only; chain_roundoff measures that on the CPU and
BAR = 3 x that is what test_gpu_f8c_model.py holds the kernel to (the factor: the kernel's chain is not the emulated one —
two register sets, the MFMA's internal order, the epilogue's fp32 adds)."""
import functools

import numpy as np

import conv_fused_ref as cref
import gn_stats_ref as gn
from edge_conv_ref import split_scale_exponent          # k = 11 - e with max|w| = f * 2^e, f in [0.5, 1); 0 for zeros
from gn_stats_ref import SR3_F8_WH, SR3_F8_WL, SR3_F8_XH, SR3_F8_XL      # csrc/sr3_internal.h, restated in one place

SPLIT_F8_MAX = 448.0                                 # csrc/sr3_internal.h
BAR_FACTOR, BAR_LIMIT = 3.0, 1.5e-5

# every OCP e4m3 byte as a float64 (bias 7; exponent field 0: subnormals m * 2^-9; 0x7F / 0xFF: NaN, never written)
_m, _e = np.arange(256) & 7, (np.arange(256) >> 3) & 15
E4M3 = np.where(_e == 0, _m * 2.0 ** -9, (8 + _m) * 2.0 ** (_e - 10.0)) * np.where(np.arange(256) & 128, -1.0, 1.0)
E4M3[[0x7F, 0xFF]] = np.nan


def e4m3_decode(b):
    return E4M3[np.asarray(b, np.uint8)]


def pack_weight(w):
    """OIHW (or [Cout, Cin] of a 1x1) -> the packed rows [taps * Cout, Cin] (pack_conv_weight), Cin a multiple of 32."""
    w = np.asarray(w, np.float32)
    Cout, Cin = w.shape[:2]
    assert Cin % 32 == 0
    return np.ascontiguousarray(w.reshape(Cout, Cin, -1).transpose(2, 0, 1)).reshape(-1, Cin)


def weight_split(packed, k=None):
    """split_scale_exponent / split_conv_weight_k on packed rows [rows, CinPad]: v = w * 2^k in fp32, hi = fp16(v),
    lo = fp16(v - hi). Returns (k, hi, lo, the uint8 bytes of the `split` layout: per 32-channel chunk 32 hi | 32 lo halfs)."""
    packed = np.ascontiguousarray(packed, np.float32)
    assert packed.ndim == 2 and packed.shape[1] % 32 == 0
    if k is None:
        k = split_scale_exponent(packed)
    with np.errstate(over="ignore", under="ignore"):
        v = packed * np.float32(2.0 ** k)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    both = np.concatenate([hi.reshape(-1, 32), lo.reshape(-1, 32)], axis=1)
    return k, hi, lo, np.ascontiguousarray(both).view(np.uint8).reshape(-1)


def weight_f8c_bytes(split_bytes):
    """make_f8_weights_kernel: the bytes of the `f8` layout from those of the `split` layout."""
    h = np.ascontiguousarray(split_bytes, np.uint8).view(np.float16).reshape(-1, 64).astype(np.float32)
    cl = lambda v: np.clip(v, -SPLIT_F8_MAX, SPLIT_F8_MAX)
    h8 = gn.e4m3_bytes(cl(h[:, :32] * np.float32(2.0 ** SR3_F8_WH)))
    l8 = gn.e4m3_bytes(cl(h[:, 32:] * np.float32(2.0 ** SR3_F8_WL)))
    hi_b = np.ascontiguousarray(split_bytes, np.uint8).reshape(-1, 128)[:, :64]
    return np.ascontiguousarray(np.concatenate([hi_b, h8, l8], axis=1)).reshape(-1)


def unpack_f8c_act(words):
    """uint32 words of activation format 2 [..., C] -> float64 (xh, xl8, xh8) of the same shape, the scales taken out."""
    C = words.shape[-1]
    b = np.ascontiguousarray(words, np.uint32).view(np.uint8).reshape(-1, C // 32, 128)
    xh = np.ascontiguousarray(b[..., :64]).view(np.float16).astype(np.float64)
    xl8 = e4m3_decode(b[..., 64:96]) * 2.0 ** -SR3_F8_XL
    xh8 = e4m3_decode(b[..., 96:]) * 2.0 ** -SR3_F8_XH
    return tuple(a.reshape(words.shape) for a in (xh, xl8, xh8))


def unpack_f8c_weight(f8_bytes, shape):
    """uint8 bytes of the weights' `f8` layout -> float64 (wh, wh8, wl8) of `shape` ([rows, CinPad]), the scales taken out."""
    b = np.ascontiguousarray(f8_bytes, np.uint8).reshape(-1, 128)
    wh = np.ascontiguousarray(b[:, :64]).view(np.float16).astype(np.float64)
    wh8 = e4m3_decode(b[:, 64:96]) * 2.0 ** -SR3_F8_WH
    wl8 = e4m3_decode(b[:, 96:]) * 2.0 ** -SR3_F8_WL
    return tuple(a.reshape(shape) for a in (wh, wh8, wl8))


def _oihw(wt):
    """[9 * Cout, Cin] packed rows -> OIHW"""
    Cin = wt.shape[-1]
    return wt.reshape(3, 3, -1, Cin).transpose(2, 3, 0, 1)


def term_k(w, term):
    """The 2^k the launch splits w with: its own, the common one of prepare_fused (w2), or the identity steps' k <= 15."""
    k = split_scale_exponent(w)
    if term is not None and term.get("w2") is not None:
        return min(k, split_scale_exponent(term["w2"]))
    return min(k, 15) if term is not None else k


def operands(g, w, k=None, f16x3=False):
    """The conv's operands as float64: xh, xl8, xh8 [B, H, W, C]; wh, wh8, wl8 [9 * Cout, C] (scaled by 2^k); k.
    f16x3: the two lo operands as the halfs of the plain split format (three f16 products) instead of e4m3."""
    g = np.ascontiguousarray(g, np.float32)
    assert np.abs(g).max() <= SPLIT_F8_MAX
    packed = pack_weight(w)
    k, hi, lo, sb = weight_split(packed, k)
    if f16x3:
        xh, xl = gn.split_halves(gn.pack_format(g, 1))
        return {"xh": xh, "xl8": xl, "xh8": xh, "wh": hi.astype(np.float64), "wh8": hi.astype(np.float64),
                "wl8": lo.astype(np.float64), "k": k}
    xh, xl8, xh8 = unpack_f8c_act(gn.pack_format(g, 2))
    wh, wh8, wl8 = unpack_f8c_weight(weight_f8c_bytes(sb), packed.shape)
    return {"xh": xh, "xl8": xl8, "xh8": xh8, "wh": wh, "wh8": wh8, "wl8": wl8, "k": k}


def conv_operands(o):
    """2^-k * sum (xh * wh + xl8 * wh8 + xh8 * wl8) of an operand set, float64 [B, H, W, Cout]."""
    acc = cref.conv3x3_f64(o["xh"], _oihw(o["wh"])) + cref.conv3x3_f64(o["xl8"], _oihw(o["wh8"])) + \
        cref.conv3x3_f64(o["xh8"], _oihw(o["wl8"]))
    return acc * 2.0 ** -o["k"]


def term64(term, k, Cout):
    """What sr3_op_conv2d_fused adds to the accumulator, times 2^-k (float64 [B, H, W, Cout]): the 1x1 K-steps stay f16x3
    inside an F8C launch — in2 / in2b in the plain split format against w2 split with the launch's k — or the identity
    K-steps ((in2_hi + in2_lo) * fp16(2^k))."""
    cat = term["in2"] if term.get("in2b") is None else np.concatenate([term["in2"], term["in2b"]], -1)
    ih, il = gn.split_halves(gn.pack_format(cat, 1))
    if term.get("w2") is None:
        assert cat.shape[-1] == Cout and k <= 15
        return ih + il
    _, h2, l2, _ = weight_split(pack_weight(term["w2"]), k)
    h2, l2 = h2.astype(np.float64), l2.astype(np.float64)
    return (ih @ h2.T + il @ h2.T + ih @ l2.T) * 2.0 ** -k


def conv_f8c_model(g0, w, bias=None, g1=None, chan_bias=None, resid=None, term=None, f16x3=False):
    """The model of the module docstring on g = g0 ‖ g1, the fp32 NHWC tensor the apply pass formats (zero-padded by 1).
    term: {"in2", "in2b" (optional), "w2", "b2"} or {"in2"} alone for the identity K-steps."""
    g = g0 if g1 is None else np.concatenate([g0, g1], -1)
    k = term_k(w, term)
    out = conv_operands(operands(g, w, k, f16x3))
    if term is not None:
        out += term64(term, k, w.shape[0])
    if bias is not None or (term is not None and term.get("b2") is not None):
        b = np.zeros(w.shape[0], np.float32) if bias is None else np.asarray(bias, np.float32)
        if term is not None and term.get("b2") is not None:
            b = b + np.asarray(term["b2"], np.float32)          # prepare_fused pre-adds the two biases in fp32
        out += b.astype(np.float64)
    if chan_bias is not None:
        out += np.asarray(chan_bias, np.float64)[:, None, None, :]
    if resid is not None:
        out += np.asarray(resid, np.float64)
    return out


def chain_roundoff(g, w, term=None):
    """The model of image g[0] accumulated as ONE fp32 chain: tap-major, per 32-channel chunk the first 16-channel f16
    K-step, the fp8 pair of the whole chunk, the second f16 K-step (the kernel's issue order); every partial product sum
    exact (float64), the running sum rounded to fp32 after each; scaled by 2^-k at the end. Returns max |chain - model|.
    term (as in conv_f8c_model): the chain goes on through the 1x1 K-steps, three f16 products per 16 channels."""
    o = operands(g[:1], w, term_k(w, term))
    H, W, C = o["xh"].shape[1:]
    pad = lambda a: np.pad(a[0], ((1, 1), (1, 1), (0, 0)))
    xh, xl8, xh8 = pad(o["xh"]), pad(o["xl8"]), pad(o["xh8"])
    wt = {n: o[n].reshape(9, -1, C) for n in ("wh", "wh8", "wl8")}
    acc = np.zeros((H * W, wt["wh"].shape[1]), np.float32)
    add = lambda p: (acc.astype(np.float64) + p).astype(np.float32)
    for t in range(9):
        dy, dx = divmod(t, 3)
        win = lambda a: a[dy:dy + H, dx:dx + W].reshape(H * W, C)
        a_h, a_l8, a_h8 = win(xh), win(xl8), win(xh8)
        for c in range(0, C, 32):
            s0, s1, s = slice(c, c + 16), slice(c + 16, c + 32), slice(c, c + 32)
            acc = add(a_h[:, s0] @ wt["wh"][t][:, s0].T)
            acc = add(a_l8[:, s] @ wt["wh8"][t][:, s].T + a_h8[:, s] @ wt["wl8"][t][:, s].T)
            acc = add(a_h[:, s1] @ wt["wh"][t][:, s1].T)
    want = conv_operands(o)[0].reshape(H * W, -1)
    if term is not None:
        k, Cout = o["k"], acc.shape[1]
        cat = term["in2"] if term.get("in2b") is None else np.concatenate([term["in2"], term["in2b"]], -1)
        ih, il = (a[0].reshape(H * W, -1) for a in gn.split_halves(gn.pack_format(cat[:1], 1)))
        if term.get("w2") is None:
            h2, l2 = np.eye(Cout) * 2.0 ** k, np.zeros((Cout, Cout))
        else:
            h2, l2 = (a.astype(np.float64) for a in weight_split(pack_weight(term["w2"]), k)[1:3])
        for c in range(0, ih.shape[1], 16):
            s = slice(c, c + 16)
            for a, b in ((il, h2), (ih, l2), (ih, h2)):
                acc = add(a[:, s] @ b[:, s].T)
        want = want + term64({n: (v[:1] if n in ("in2", "in2b") and v is not None else v) for n, v in term.items()}, k,
                             Cout)[0].reshape(H * W, -1)
    chain = acc.astype(np.float64) * 2.0 ** -o["k"]
    return float(np.abs(chain - want).max())


# ---- the cases of test_gpu_f8c_model.py (b): (B, H, W, C0, C1, Cout) ----------------------------------------------------------
CASES = [
    (16, 32, 32, 32, 0, 512),        # smallest batch that plans F8C; one chunk per tap: 9 halo K-steps
    (64, 32, 32, 96, 0, 128),        # a single N tile; an odd chunk count through the two register sets
    (128, 8, 16, 64, 0, 512),        # one tile is one whole image
    (128, 16, 8, 32, 32, 512),       # W = 8: 16 image rows per tile; the second chunk comes from in1
    (128, 4, 32, 32, 0, 512),        # four-row images
    (48, 12, 32, 64, 0, 512),        # three tiles per image
    (24, 24, 32, 32, 64, 512),       # unequal concat halves; six tiles per image
    (64, 16, 16, 512, 512, 512),     # the deepest K the yml UNet has: 288 halo K-steps
]
KINDS = ("normal", "wide", "neighbours")
NEIGHBOUR_SCALE = 100.0


def case_id(case):
    return "x".join(map(str, case))


@functools.lru_cache(maxsize=None)
def case_data(case, kind="normal"):
    """Three distinct images of one case (first axis), `idx` the distinct image behind each batch entry
    (conv_fused_ref.images: first = last, the middle one differs). normal: x ~ N(0, 1); wide: x * exp(U(-12, 5)) held inside
    +-SPLIT_F8_MAX with a few elements exactly at the limit; neighbours: the middle image scaled by 100, inside the limit.
    w ~ N(0, 1) / sqrt(9 Cin); bias, chan_bias, resid ~ N(0, 1)."""
    B, H, W, C0, C1, Cout = case
    C = C0 + C1
    rs = np.random.RandomState((B * 7919 + H * 131 + W * 17 + C0 * 5 + C1 * 3 + Cout) & 0xFFFFFFF)
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    x = f32(3, H, W, C)
    d = {"idx": cref.images(B), "w": f32(Cout, C, 3, 3) / np.float32(np.sqrt(9 * C)), "b": f32(Cout), "cb": f32(3, Cout),
         "resid": f32(3, H, W, Cout)}
    assert d["idx"].max() == 2
    if kind == "wide":
        x = x * np.exp(rs.uniform(-12, 5, x.shape)).astype(np.float32)
        x = np.clip(x, -SPLIT_F8_MAX, SPLIT_F8_MAX)
        flat = x.reshape(-1)
        at = rs.choice(flat.size, 8, replace=False)
        flat[at] = np.float32(SPLIT_F8_MAX) * np.where(np.arange(8) & 1, -1, 1).astype(np.float32)
    elif kind == "neighbours":
        x[1] = np.clip(x[1] * np.float32(NEIGHBOUR_SCALE), -SPLIT_F8_MAX, SPLIT_F8_MAX)
    else:
        assert kind == "normal"
    d["x"] = np.ascontiguousarray(x)
    d["x0"], d["x1"] = np.ascontiguousarray(x[..., :C0]), (np.ascontiguousarray(x[..., C0:]) if C1 else None)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case_refs(case, kind="normal"):
    """(model, exact float64 conv) of the case's three images, both with the bias; computed once per session."""
    d = case_data(case, kind)
    model = conv_f8c_model(d["x"], d["w"], d["b"])
    exact = cref.conv3x3_f64(d["x"], d["w"]) + d["b"].astype(np.float64)
    model.setflags(write=False)
    exact.setflags(write=False)
    return model, exact


@functools.lru_cache(maxsize=None)
def bar(case):
    """BAR(case) = 3 x chain_roundoff on the first image of the case's standard-normal data."""
    d = case_data(case, "normal")
    return BAR_FACTOR * chain_roundoff(d["x"], d["w"])
