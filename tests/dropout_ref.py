"""CPU twin of the device's Dropout mask stream and a mask-aware wrapper of the aten oracle — TEST INFRASTRUCTURE ONLY.

The mask stream (csrc/sr3_internal.h: dropout_fields8 / dropout_apply8), restated over
oracle/philox.py::philox4x32_10:

    one Philox4x32-10 evaluation serves the 8 consecutive channels c .. c+7 of pixel (y, x) of a [C][H][W] layer
    key     = the dropout seed (low word, high word)
    counter = (octet = (y*W + x)*(C/8) + c/8,  ((layer+1) << 24) | draw,  image low word,  image high word)
    channel c + j takes the 16-bit field (r[j >> 1] >> (16 * (j & 1))) & 0xffff and is kept iff field >= thr
    thr     = round-half-even(p * 65536); the kept values are multiplied by s = float32(1.0 / (1.0 - p))

`image` is the GLOBAL image index (image_offset + batch row); `layer` the 0-based ordinal of the ResnetBlock in
execution order downs -> mid -> ups; `draw` = T - t in step t of the sampler, 0 in the forward and the loss.

The wrapper (`masked`) multiplies the activated input of every ResnetBlock.block2 conv of oracle/sr3_oracle_aten.py by
a given keep mask times s, the reference's train-mode Block (model/sr/sr3_modules/unet.py:81-91) — without touching
oracle/.
"""
from __future__ import annotations

import contextlib
from typing import List, Sequence

import numpy as np

import philox
import sr3_oracle_aten as aten

MAX_LAYERS = 254
MAX_DRAW = 1 << 24


def threshold(p: float) -> int:
    """round-half-even(p * 65536) — Python's round() on the exact double product, the device host's nearbyint()."""
    return int(round(float(p) * 65536.0))


def scale(p: float) -> np.float32:
    """float32(1.0 / (1.0 - p)): the division in double, rounded once (what torch.nn.Dropout multiplies by)."""
    return np.float32(1.0 / (1.0 - float(p)))


def counter_c1(layer: int, draw: int) -> int:
    if not 0 <= layer < MAX_LAYERS:
        raise ValueError(f"layer {layer} outside [0, {MAX_LAYERS})")
    if not 0 <= draw < MAX_DRAW:
        raise ValueError(f"draw {draw} does not fit 24 bits")
    return ((layer + 1) << 24) | draw


def fields(seed: int, image: int, draw: int, layer: int, C: int, H: int, W: int) -> np.ndarray:
    """The 16-bit fields of one image's layer as uint32 [C][H][W]."""
    assert C % 8 == 0
    C8 = C // 8
    octet = np.arange(H * W * C8, dtype=np.uint32)
    n = octet.size
    u32 = lambda v: np.full(n, v & 0xffffffff, dtype=np.uint32)
    r = philox.philox4x32_10(octet, u32(counter_c1(layer, draw)), u32(image), u32(image >> 32),
                             seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    r = np.stack([np.asarray(w, dtype=np.uint32) for w in r], axis=1)            # [octet][4]
    f = np.empty((n, 8), dtype=np.uint32)
    for j in range(8):
        f[:, j] = (r[:, j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xffff)
    # octet = pix * C8 + c8, channel = c8 * 8 + j  ->  [pix][C] -> [C][H][W]
    return np.ascontiguousarray(f.reshape(H * W, C).T).reshape(C, H, W)


def mask(seed: int, image: int, draw: int, layer: int, C: int, H: int, W: int, p: float) -> np.ndarray:
    """uint8 [C][H][W], 1 = keep: what sr3_op_dropout_mask dumps."""
    return (fields(seed, image, draw, layer, C, H, W) >= threshold(p)).astype(np.uint8)


def batch_masks(seed: int, image_offset: int, draw: int, layers: Sequence[Sequence[int]], B: int, p: float) -> List[np.ndarray]:
    """One uint8 [B][C][H][W] per layer of `layers` = [(C, H, W), ...] (Engine.dropout_layers)."""
    return [np.stack([mask(seed, image_offset + b, draw, l, C, H, W, p) for b in range(B)])
            for l, (C, H, W) in enumerate(layers)]


def concat(masks: Sequence[np.ndarray]) -> np.ndarray:
    """The injected-mask buffer: the layers concatenated in layer order, each NCHW."""
    return np.concatenate([np.ascontiguousarray(m, dtype=np.uint8).ravel() for m in masks])


def pack(masks: Sequence[np.ndarray]) -> np.ndarray:
    return np.packbits(concat(masks))


def unpack(bits: np.ndarray, shapes: Sequence[Sequence[int]]) -> List[np.ndarray]:
    """Inverse of pack(): shapes = the [B, C, H, W] of every layer."""
    total = sum(int(np.prod(s)) for s in shapes)
    flat = np.unpackbits(np.asarray(bits, dtype=np.uint8))[:total]
    out, o = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[o:o + n].reshape(s).copy())
        o += n
    return out


@contextlib.contextmanager
def masked(masks: Sequence[np.ndarray], p: float):
    """While active, one aten.unet_forward evaluates the train-mode UNet: the k-th `.block2` of the forward multiplies
    its activated input by masks[k] * s (keep ? h * s : 0; unet.py:81-91). Exactly len(masks) block2 calls must happen
    per `with` block (several forwards: pass their masks concatenated)."""
    import torch
    import torch.nn.functional as F

    s = float(scale(p))
    it = iter(masks)
    used = [0]
    orig = aten.block

    def block(sd, pfx, x, groups):
        if not pfx.endswith(".block2"):
            return orig(sd, pfx, x, groups)
        h = aten.swish(F.group_norm(x, groups, sd[pfx + ".block.0.weight"], sd[pfx + ".block.0.bias"], eps=1e-5))
        m = torch.from_numpy(np.ascontiguousarray(next(it))).to(h.dtype)
        assert tuple(m.shape) == tuple(h.shape), (pfx, tuple(m.shape), tuple(h.shape))
        used[0] += 1
        h = h * (m * torch.tensor(s, dtype=torch.float32).to(h.dtype))
        return F.conv2d(h, sd[pfx + ".block.3.weight"], sd[pfx + ".block.3.bias"], padding=1)

    aten.block = block
    try:
        yield
    finally:
        aten.block = orig
    assert used[0] == len(masks), (used[0], len(masks))
