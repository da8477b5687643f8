"""Single 3x3 convs at the edges of the dispatch gates (sr3_op_conv2d runs a conv as the engine would run it for the
shape): the Winograd gates in exact f32, the x-halo split-K and F8C gates in the f16 modes. The library is asked which
kernel it runs (Engine.conv_plan: the plan launch_conv itself switches on). Every image of the batch against a float64
numpy conv.

Data as in tests/test_gpu_ops.py: N(0,1) inputs, N(0,1) / sqrt(9 Cin) weights, N(0,1) bias; every other case adds the
FeatureWiseAffine bias (chan_bias) and a residual. Bars: 2e-5 absolute in f32 and f16x3 (test_conv2d's bar; that test
holds a K = 9216 Winograd conv to it), 2e-4 in f16f8 (tests/test_gpu_f16f8.py). Image B-1 is a copy of image 0: the two
output rows must be bit-identical.

Gate arithmetic (csrc/kernels_conv.hip, conv_plan):
  three-pass Winograd: H, W even, H*W <= 1024, Cin >= 128, Cin % 32 == 0, Cout % 64 == 0, B*H/2*W/2 >= 1024 tiles
  one-pass Winograd:   H*W >= 4096, H even, W % 64 == 0, Cin >= 64, Cin % 32 == 0, Cout % 64 == 0,
                       B * H/2 * W/64 * Cout/64 >= 1024 blocks
  F8C:                 128 <= H*W <= 1024, H*W % 128 == 0, Cout % 128 == 0, M/128 * Cout/128 >= 512 tiles"""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")


@pytest.fixture(scope="module")
def eng():
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    e.load_state_dict(synth.synth_state_dict(e.cfg, 11))
    yield e
    e.close()


def conv3x3_f64(x, w, b):
    """3x3 / stride 1 / padding 1 on NHWC x, w OIHW, everything widened to float64."""
    B, H, W, C = x.shape
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    w64 = w.astype(np.float64)
    out = np.zeros((B * H * W, w.shape[0]), np.float64)
    for dy in range(3):
        for dx in range(3):
            out += np.ascontiguousarray(xp[:, dy:dy + H, dx:dx + W, :]).reshape(-1, C) @ np.ascontiguousarray(w64[:, :, dy, dx].T)
    return (out + b.astype(np.float64)).reshape(B, H, W, -1)


def _case_data(case, extras):
    B, H, W, Cin, Cout = case
    rs = np.random.RandomState((B * 7919 + H * 131 + W * 17 + Cin + Cout) & 0xFFFFFFF)
    x = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    cb = rs.standard_normal((B, Cout)).astype(np.float32) if extras else None
    resid = rs.standard_normal((B, H, W, Cout)).astype(np.float32) if extras else None
    x[B - 1] = x[0]                       # the same image at batch positions 0 and B-1
    if extras:
        cb[B - 1], resid[B - 1] = cb[0], resid[0]
    want = conv3x3_f64(x, w, b)
    if extras:
        want = want + cb.astype(np.float64)[:, None, None, :] + resid.astype(np.float64)
    return x, w, b, cb, resid, want


def _run(eng, prec, x, w, b, cb, resid):
    eng.set_precision(prec)
    try:
        return eng.op_conv2d(x, w, b, chan_bias=cb, resid=resid)
    finally:
        eng.set_precision("f32")


# (B, H, W, Cin, Cout), the form the Winograd gates give it in exact f32
F32_CASES = [
    ((16, 16, 16, 128, 64), "three-pass"),      # exactly WINO_MIN_TILES tiles
    ((15, 16, 16, 128, 64), "direct"),          # 960 tiles: just below
    ((8, 16, 64, 160, 192), "three-pass"),      # H*W = 1024 non-square, Cin = 160 (five K chunks), Cout = 192 (three 64-channel blocks)
    ((43, 14, 14, 256, 128), "three-pass"),     # 49 tiles per image: one statistics-free output slice, ragged M tiles
    ((171, 6, 10, 128, 64), "three-pass"),
    ((4, 2, 512, 128, 64), "three-pass"),       # one tile row, exactly 1024 tiles
    ((5, 32, 32, 288, 192), "three-pass"),      # Cin = 288 (nine K chunks)
    ((16, 16, 18, 128, 64), "three-pass"),      # W = 18: even, 9 tiles per row
    ((1, 128, 128, 64, 512), "one-pass"),       # exactly WINO_FUSED_MIN_BLOCKS blocks from one image
    ((11, 192, 64, 64, 64), "one-pass"),        # 1056 blocks, one strip per tile row
    ((12, 192, 64, 64, 64), "one-pass"),
    ((10, 192, 64, 64, 64), "direct"),          # 960 blocks: just below
    ((8, 64, 128, 96, 128), "one-pass"),        # Cin = 96 (three K chunks), exactly 1024 blocks
    ((3, 64, 128, 96, 128), "direct"),          # 384 blocks
    ((4, 70, 64, 64, 512), "one-pass"),         # 35 tile rows (odd)
    ((2, 70, 64, 64, 512), "direct"),           # 560 blocks
    ((16, 17, 16, 128, 64), "direct"),          # odd H
    ((16, 16, 17, 128, 64), "direct"),          # odd W
    ((64, 64, 96, 64, 64), "direct"),           # W % 64 != 0
]


WINO_KERNELS = {"one-pass": "wino_one_pass", "three-pass": "wino_three_pass"}


def wino_form(B, H, W, Cin, Cout):
    """The Winograd gates of csrc/kernels_conv.hip restated (wino_shape, wino_fused_shape)."""
    if H * W >= 4096 and H % 2 == 0 and W % 64 == 0 and Cin >= 64 and Cin % 32 == 0 and Cout % 64 == 0 \
            and B * (H // 2) * (W // 64) * (Cout // 64) >= 1024:
        return "one-pass"
    if H % 2 == 0 and W % 2 == 0 and H * W <= 1024 and Cin >= 128 and Cin % 32 == 0 and Cout % 64 == 0 \
            and B * (H // 2) * (W // 2) >= 1024:
        return "three-pass"
    return "direct"


@pytest.mark.parametrize("idx", range(len(F32_CASES)), ids=["x".join(map(str, c)) + "-" + f for c, f in F32_CASES])
def test_conv_f32_at_winograd_gates(eng, idx):
    case, form = F32_CASES[idx]
    assert wino_form(*case) == form
    kernel = eng.conv_plan(*case, precision="f32")["kernel"]
    assert kernel == WINO_KERNELS[form] if form != "direct" else kernel.startswith("generic_"), kernel
    x, w, b, cb, resid, want = _case_data(case, extras=idx % 2 == 1)
    got = _run(eng, "f32", x, w, b, cb, resid)
    B = case[0]
    err = np.abs(got - want).reshape(B, -1).max(1)
    print(f"{case} [{form}{', chan_bias + resid' if idx % 2 else ''}]: max abs err {err.max():.2e} (image {int(err.argmax())})")
    assert got.shape == want.shape
    assert err.max() <= 2e-5, err
    np.testing.assert_array_equal(got[0], got[B - 1])


# (B, H, W, Cin, Cout), does conv_f8_supported take it, the kernel and split-K form f16x3 runs (f16f8: the F8C kernel
# where conv_f8_supported, else the same)
F16_CASES = [
    ((64, 16, 32, 256, 512), True, "halo_128x128_seg32", "none"),   # non-square 16x32 level, 1024 tiles of 128x128
    ((63, 32, 32, 256, 256), True, "halo_128x128_seg32", "none"),   # 504 M-tiles x 2: 1008 tiles, odd batch
    ((128, 4, 32, 512, 512), True, "halo_128x128_seg32", "none"),   # H*W = 128 (one tile per image), exactly 512 tiles
    ((64, 4, 32, 512, 512), False, "halo_128x64", "none"),          # 256 tiles of 128x128: the 128x64 x-halo tile
    # H*W = 64 < 128: in-place split-K of the x-halo tile (rows of 8 pixels), 17 K chunks, 72 tiles
    ((36, 8, 8, 544, 512), False, "halo_128x128_seg8", "inplace_halo"),
]


@pytest.mark.parametrize("idx", range(len(F16_CASES)), ids=["x".join(map(str, c)) + ("-f8" if f else "-nof8") for c, f, _, _ in F16_CASES])
def test_conv_f16_at_halo_and_f8_gates(eng, idx):
    case, f8, kernel, split = F16_CASES[idx]
    B, H, W, Cin, Cout = case
    assert eng.conv_f8_supported(B, H, W, Cout, Cin) == f8
    p3, p8 = eng.conv_plan(*case, precision="f16x3"), eng.conv_plan(*case, precision="f16f8")
    assert (p3["kernel"], p3["split"], p3["f8"]) == (kernel, split, False), p3
    assert (p8["kernel"], p8["split"], p8["f8"]) == (("halo_f8c", "none", True) if f8 else (kernel, split, False)), p8
    x, w, b, cb, resid, want = _case_data(case, extras=idx % 2 == 1)
    got3 = _run(eng, "f16x3", x, w, b, cb, resid)
    got8 = _run(eng, "f16f8", x, w, b, cb, resid)
    e3 = np.abs(got3 - want).reshape(B, -1).max(1)
    e8 = np.abs(got8 - want).reshape(B, -1).max(1)
    print(f"{case} [{'F8C' if f8 else 'no F8C'}{', chan_bias + resid' if idx % 2 else ''}]: f16x3 {e3.max():.2e}  f16f8 {e8.max():.2e}")
    assert e3.max() <= 2e-5, e3
    assert e8.max() <= 2e-4, e8
    if f8:
        assert e8.max() > 2 * e3.max(), "the fp8 path was not taken (error as small as f16x3's)"
    else:
        np.testing.assert_array_equal(got8, got3)       # no F8C for this shape: f16f8 runs the f16x3 kernel
    np.testing.assert_array_equal(got3[0], got3[B - 1])
    np.testing.assert_array_equal(got8[0], got8[B - 1])
