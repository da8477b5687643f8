"""numpy references for the kernels of csrc/kernels_edge.hip (not collected on its own): the UNet's first conv on the packed
split-f16 state (conv_in_kernel, pack_state_kernel) and its last layer GroupNorm -> Swish -> Conv3x3 (final_conv_kernel,
final_conv_mfma_kernel). Used by test_edge_conv_ref_host.py (CPU) and test_gpu_edge_convs.py / test_gpu_packed_state.py.

  conv_in64 / final_conv64   the operation in float64: what the kernels are held to
  pack16                     the packed operand format: (f16(v), f16(v - f16(v)))
  emulate_split              the kernels' arithmetic restated: both operands split into hi / lo f16, the weights scaled by
                             2^k first (split_scale_exponent: max|w| 2^k in [1024, 2048)), three products xl*wh + xh*wl +
                             xh*wh, fp32 accumulation, * 2^-k, + bias. drop="x_lo" / "w_lo" leaves one correction product
                             out: the size of the mistake a test bar has to see.
  final_conv_f32             the VALU form restated in plain fp32

Error bars (test_gpu_edge_convs.py): per case 8 x the error of the restatement against float64 on the case's
own data. The margin of 8 covers what the restatements do not reproduce: the MFMA's accumulation order inside a 32-deep
K-step (the restatement adds tap by tap through BLAS), the fma of the affine, and Swish on v_exp_f32 / v_rcp_f32 (1 ulp
each) against numpy's exp and division. The bar is never taken from the kernels' results; bar_condition() checks that it
stays at most 1/20 of the error either dropped correction product makes on the same data.

The case lists live here so that the CPU test checks the bars on exactly the data the GPU test runs.
"""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
MARGIN = 8.0            # bar = MARGIN x (restatement - float64)
SEPARATION = 20.0       # bar <= (dropped correction product - float64) / SEPARATION


# ---- the operations in float64 -----------------------------------------------------------------------------------------
def conv3x3(x, w, dtype):
    """3x3 / stride 1 / zero padding 1 conv of NHWC x with OIHW w, every product and sum in `dtype`, tap by tap."""
    x, w = np.asarray(x, dtype=dtype), np.asarray(w, dtype=dtype)
    B, H, W, C = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B * H * W, w.shape[0]), dtype=dtype)
    for dy in range(3):
        for dx in range(3):
            out += np.ascontiguousarray(xp[:, dy:dy + H, dx:dx + W, :]).reshape(-1, C) @ np.ascontiguousarray(w[:, :, dy, dx].T)
    return out.reshape(B, H, W, -1)


def conv_in64(state, w, bias=None):
    """downs.0 in float64: state [B,H,W,Cin] NHWC, w OIHW."""
    out = conv3x3(state, w, F64)
    return out if bias is None else out + np.asarray(bias, dtype=F64)


def swish(v):
    with np.errstate(over="ignore"):
        return v / (1 + np.exp(-v))


def activate(x, scale, shift, dtype):
    """swish(x * scale[b, c] + shift[b, c]) in `dtype` (the folded GroupNorm affine per (image, channel))."""
    x = np.asarray(x, dtype=dtype)
    v = x * np.asarray(scale, dtype=dtype)[:, None, None, :] + np.asarray(shift, dtype=dtype)[:, None, None, :]
    return swish(v).astype(dtype)


def final_conv64(x, scale, shift, w, bias):
    """final_conv in float64: affine -> Swish -> zero padding AFTER the activation -> 3x3 (the padded pixels contribute 0,
    not swish(shift))."""
    return conv3x3(activate(x, scale, shift, F64), w, F64) + np.asarray(bias, dtype=F64)


def final_conv_f32(x, scale, shift, w, bias):
    """The VALU kernel restated: fp32 affine, fp32 Swish, fp32 products and sums."""
    return conv3x3(activate(x, scale, shift, F32), w, F32) + np.asarray(bias, dtype=F32)


def gn_affine64(x, gamma, beta, groups, eps=1e-5):
    """GroupNorm folded into scale[b,c] = rstd gamma[c], shift[b,c] = beta[c] - mean rstd gamma[c] (float64 statistics,
    fp32 results): what op_groupnorm_affine returns, for the CPU side."""
    B, H, W, C = x.shape
    xg = x.astype(F64).reshape(B, H * W, groups, C // groups)
    mean, var = xg.mean(axis=(1, 3)), xg.var(axis=(1, 3))
    rstd = np.repeat(1 / np.sqrt(var + eps), C // groups, axis=1)
    mean = np.repeat(mean, C // groups, axis=1)
    scale = rstd * gamma.astype(F64)
    return scale.astype(F32), (beta.astype(F64) - mean * scale).astype(F32)


# ---- the operand formats -------------------------------------------------------------------------------------------------
def pack16(v):
    """(hi, lo) float16: hi = f16(v), lo = f16(v - f32(hi)), round to nearest even like the kernels' conversions."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(F32)).astype(np.float16)
    return hi, lo


def split_scale_exponent(w):
    """k with max|w| * 2^k in [1024, 2048) (csrc/kernels_conv.hip split_scale_exponent); 0 for an all-zero tensor."""
    mx = F32(np.abs(np.asarray(w, dtype=F32)).max())
    if not mx > 0:
        return 0
    return 11 - int(np.frexp(mx)[1])


def emulate_split(act, w, bias=None, drop=None):
    """The split-f16 kernels' arithmetic on an activated NHWC fp32 input: see the module docstring."""
    assert drop in (None, "x_lo", "w_lo")
    k = split_scale_exponent(w)
    ws = np.asarray(w, dtype=F32) * F32(2.0 ** k)                  # exact: a power of two
    xh, xl = (a.astype(F32) for a in pack16(act))
    wh, wl = (a.astype(F32) for a in pack16(ws))
    acc = conv3x3(xh, wh, F32)
    if drop != "x_lo":
        acc = acc + conv3x3(xl, wh, F32)
    if drop != "w_lo":
        acc = acc + conv3x3(xh, wl, F32)
    out = acc * F32(2.0 ** -k)
    return out if bias is None else out + np.asarray(bias, dtype=F32)


def errors(want, restated, dropped):
    """(bar, restatement error, smallest dropped-product error): all max |. - want| over the case."""
    e = float(np.abs(restated - want).max())
    d = min(float(np.abs(x - want).max()) for x in dropped)
    return MARGIN * e, e, d


# ---- the cases -------------------------------------------------------------------------------------------------------------
# conv_in (B, H, W, Cin, Cout): one block with whole-row M-tiles on the tiny config's width | blocks end at image ends |
# two M-tiles per row | waves straddle rows (64 pixels over 48-pixel rows) | unconditional (channels 3..7 zero) | no zero
# channel | more blocks (520) than the 512 persistent ones: blocks loop
CONV_IN_SHAPES = [(1, 16, 16, 6, 32), (3, 16, 16, 6, 64), (2, 8, 32, 6, 64), (1, 16, 48, 6, 64), (2, 16, 16, 3, 64),
                  (2, 16, 16, 8, 32), (520, 16, 16, 6, 64)]
# final_conv (B, H, W): ragged 32x4 (VALU) and 32x8 (MFMA) blocks, odd sizes, exact fits; 2 x 8 x 64 makes the last halo
# M-tile (pixels 336..339 of 340, lanes clamped) part of two blocks per image
FINAL_SHAPES = [(2, 6, 20), (1, 9, 33), (3, 4, 32), (1, 16, 16), (2, 8, 64)]
FINAL_VALU = [(s, C, Co) for s in FINAL_SHAPES for C in (64, 128, 256) for Co in (1, 2, 3, 4)]
FINAL_MFMA = [(s, C, 3) for s in FINAL_SHAPES for C in (64, 128)]


def image_index(B):
    """The distinct image behind each batch row: image B-1 is always a copy of image 0; up to 3 distinct images."""
    nd = max(1, min(B - 1, 3))
    idx = np.arange(B) % nd
    idx[B - 1] = 0
    return idx


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def conv_in_case(shape):
    """Data and references of one conv_in case, computed once and read-only: state [nd,H,W,Cin] (the distinct images),
    idx [B], w, bias, want (float64 [nd,...]), bar, emu_err, dropped_err."""
    B, H, W, Cin, Cout = shape
    rs = np.random.RandomState(1000 + sum(shape))
    idx = image_index(B)
    nd = int(idx.max()) + 1
    state = rs.standard_normal((nd, H, W, Cin)).astype(F32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(F32)
    bias = (0.1 * rs.standard_normal(Cout)).astype(F32)
    want = conv_in64(state, w, bias)
    bar, e, d = errors(want, emulate_split(state, w, bias), [emulate_split(state, w, bias, drop=k) for k in ("x_lo", "w_lo")])
    _ro(state, idx, w, bias, want)
    return {"state": state, "idx": idx, "w": w, "bias": bias, "want": want, "bar": bar, "emu_err": e, "dropped_err": d}


@functools.lru_cache(maxsize=None)
def final_case(shape, C, Cout):
    """Data of one final_conv case (read-only): x [nd,H,W,C], idx, gamma, beta (around +2: swish(shift) is far from 0, so
    padding applied before the activation would show at every border), w, bias. The GroupNorm affine comes from the GPU in
    the GPU test and from gn_affine64 here, so the references are functions of it: final_refs()."""
    B, H, W = shape
    rs = np.random.RandomState(2000 + 7 * sum(shape) + C + Cout)
    idx = image_index(B)
    nd = int(idx.max()) + 1
    x = (1.5 * rs.standard_normal((nd, H, W, C)) + 0.3).astype(F32)
    gamma = (1 + 0.1 * rs.standard_normal(C)).astype(F32)
    beta = (2 + 0.1 * rs.standard_normal(C)).astype(F32)
    w = (rs.standard_normal((Cout, C, 3, 3)) / np.sqrt(9 * C)).astype(F32)
    bias = (0.1 * rs.standard_normal(Cout)).astype(F32)
    _ro(x, idx, gamma, beta, w, bias)
    return {"x": x, "idx": idx, "gamma": gamma, "beta": beta, "w": w, "bias": bias}


def final_refs(case, scale, shift, form):
    """want (float64), bar, restatement error and (MFMA form) the smallest dropped-product error for the case's distinct
    images under the affine scale / shift [nd, C]. form "valu": the plain fp32 restatement; "mfma": emulate_split on the
    fp32 activation."""
    x, w, bias = case["x"], case["w"], case["bias"]
    want = final_conv64(x, scale, shift, w, bias)
    if form == "valu":
        e = float(np.abs(final_conv_f32(x, scale, shift, w, bias) - want).max())
        return {"want": want, "bar": MARGIN * e, "emu_err": e, "dropped_err": None}
    act = activate(x, scale, shift, F32)
    bar, e, d = errors(want, emulate_split(act, w, bias), [emulate_split(act, w, bias, drop=k) for k in ("x_lo", "w_lo")])
    return {"want": want, "bar": bar, "emu_err": e, "dropped_err": d}


def bar_condition(bar, dropped_err):
    """The bar separates a correct kernel from one that lost a correction product by a factor of SEPARATION."""
    return bar * SEPARATION <= dropped_err
