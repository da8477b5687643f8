"""numpy restatements shared by test_gpu_conv_stats.py, test_gpu_gn_consumers.py and test_gn_formats_host.py (TEST
INFRASTRUCTURE, not collected by pytest):

  - the apply pass's output formats (csrc/kernels_misc.hip: store8<0|1|2>), bit for bit;
  - fp64 GroupNorm statistics partials in the ConvParams::stats layout [B][slices][C][2], built from a tensor itself;
  - the float64 GroupNorm (+ Swish) the consumers are held to.
"""
import numpy as np
import torch

SR3_F8_XH, SR3_F8_XL = 0, 11        # csrc/sr3_internal.h
SR3_F8_WH, SR3_F8_WL = -3, 9        # csrc/sr3_internal.h (the weights' side: tests/f8c_ref.py)


def e4m3_bytes(v):
    """OCP e4m3 (bias 7, no infinities), round to nearest even, of float32 values inside +-448 -> uint8."""
    v = np.ascontiguousarray(v, np.float32)
    assert np.all(np.abs(v) <= 448.0), "e4m3 packer: keep values inside +-448 (beyond it the hardware conversion is NaN)"
    return torch.from_numpy(v).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def pack_format(g, fmt):
    """float32 [..., C] (C a multiple of 32) -> the uint32 words store8<fmt> writes for it, same shape. Per 32-channel
    chunk (128 bytes): fmt 1 = 32 hi halfs | 32 lo halfs; fmt 2 = 32 hi halfs | 32 x e4m3(lo * 2^11) | 32 x e4m3(g).
    hi = fp16(g) (RNE), lo = fp16(g - hi), the difference taken in fp32 (it is exact there)."""
    g = np.ascontiguousarray(g, np.float32)
    if fmt == 0:
        return g.view(np.uint32)
    C = g.shape[-1]
    assert C % 32 == 0
    g3 = g.reshape(-1, C // 32, 32)
    with np.errstate(over="ignore"):
        hi = g3.astype(np.float16)
    lof = g3 - hi.astype(np.float32)
    hi_b = hi.view(np.uint8).reshape(-1, C // 32, 64)
    if fmt == 1:
        rest = [lof.astype(np.float16).view(np.uint8).reshape(-1, C // 32, 64)]
    else:
        rest = [e4m3_bytes(lof * np.float32(2.0 ** SR3_F8_XL)), e4m3_bytes(g3 * np.float32(2.0 ** SR3_F8_XH))]
    words = np.ascontiguousarray(np.concatenate([hi_b] + rest, axis=-1)).view(np.uint32)
    return words.reshape(g.shape)


def split_halves(words):
    """uint32 words of format 1 -> (hi, lo) as float64 arrays of the same shape."""
    C = words.shape[-1]
    h = np.ascontiguousarray(words).view(np.float16).reshape(-1, C // 32, 64)
    return (h[..., :32].astype(np.float64).reshape(words.shape), h[..., 32:].astype(np.float64).reshape(words.shape))


def chunk_bounds(rs, n, slices):
    """`slices` contiguous, non-empty, unequal chunks of range(n) -> their boundaries [0, ..., n]."""
    assert 1 <= slices <= n
    cuts = np.sort(rs.choice(np.arange(1, n), size=slices - 1, replace=False)) if slices > 1 else np.zeros(0, int)
    return np.concatenate([[0], cuts, [n]]).astype(int)


def partials(x, bounds):
    """fp64 {sum, sum of squares} per (image, slice, channel) of x [B, H, W, C] over the pixel chunks `bounds`."""
    B, H, W, C = x.shape
    v = x.reshape(B, H * W, C).astype(np.float64)
    out = np.empty((B, len(bounds) - 1, C, 2), np.float64)
    for s in range(len(bounds) - 1):
        seg = v[:, bounds[s]:bounds[s + 1]]
        out[:, s, :, 0] = seg.sum(axis=1)
        out[:, s, :, 1] = (seg * seg).sum(axis=1)
    return out


def group_norm64(x, gamma, beta, groups, eps=1e-5, swish=False):
    """torch.nn.GroupNorm (biased variance, eps inside the root) (+ Swish) in float64 on NHWC x."""
    B, H, W, C = x.shape
    xg = x.astype(np.float64).reshape(B, H * W, groups, C // groups)
    mean = xg.mean(axis=(1, 3), keepdims=True)
    var = ((xg - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    y = ((xg - mean) / np.sqrt(var + eps)).reshape(B, H, W, C) * gamma.astype(np.float64) + beta.astype(np.float64)
    return y / (1.0 + np.exp(-y)) if swish else y
