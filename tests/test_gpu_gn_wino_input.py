"""The GroupNorm apply pass that writes the Winograd input transform of the three-pass conv behind it
(gn_wino_input_kernel; ConvParams::u_ready): copy, affine and affine + Swish in front of single convs (sr3_op_conv2d runs
a conv as the engine would run it for the shape) against a float64 numpy reference — affine, x * sigmoid(x), zero
padding, 3x3 conv — and bit for bit against the two passes it replaces, which a child process with SR3_NO_GN_WINO=1 runs
(the switch is read once per process, as SR3_NO_WINOGRAD in tests/test_gpu_winograd.py).

Data as in tests/test_gpu_ops.py: N(0,1) inputs, N(0,1) / sqrt(9 Cin) weights, per-(image, channel) scale 1 + 0.1 N and
shift 0.1 N; every other case adds the FeatureWiseAffine bias (chan_bias) and a residual. Image B-1 is a copy of image 0.
Bars (test_gpu_ops.py holds op_conv2d to the same): 3e-5 absolute with GroupNorm (+ Swish), 2e-5 for the plain copy.
Engine.gn_wino_passes() tells which route ran."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")

# (B, H, W, Cin, Cout), channels of x0 (the rest is x1)
CASES = [
    ((16, 16, 16, 128, 64), 128),       # exactly 1024 tiles
    ((16, 16, 16, 128, 64), 96),        # x0 ‖ x1 = 96 + 32: the concat boundary is off a 64-channel block
    ((171, 6, 10, 128, 64), 128),       # 5 tiles per row, 3 tile rows
    ((4, 2, 512, 128, 64), 128),        # one tile row: window rows 0 and 3 are both border
    ((43, 14, 14, 256, 128), 256),      # 49 tiles per image
    ((8, 16, 64, 160, 192), 160),       # Cin is not a multiple of 64
]
MODES = ("copy", "affine", "swish")
BAR = {"copy": 2e-5, "affine": 3e-5, "swish": 3e-5}
DIRECT_CASE = (15, 16, 16, 128, 64)     # 960 tiles: the direct kernel, two passes
FWD_B, FWD_HW = 4, 32                   # sweep config D: its 32x32 level is three-pass (exactly 1024 tiles), 16x16 and 8x8 direct


def case_data(ci):
    (B, H, W, Cin, Cout), _ = CASES[ci]
    rs = np.random.RandomState(1000 + ci)
    x = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    sc = (1 + 0.1 * rs.standard_normal((B, Cin))).astype(np.float32)
    sh = (0.1 * rs.standard_normal((B, Cin))).astype(np.float32)
    cb = rs.standard_normal((B, Cout)).astype(np.float32)
    resid = rs.standard_normal((B, H, W, Cout)).astype(np.float32)
    for a in (x, sc, sh, cb, resid):
        a[B - 1] = a[0]                 # the same image at batch positions 0 and B-1
    return x, w, b, sc, sh, cb, resid


def run_case(eng, ci, mode, data=None, scale_shift=None):
    """One op_conv2d call of case ci; every other (case, mode) pair carries chan_bias + resid."""
    _, c0 = CASES[ci]
    x, w, b, sc, sh, cb, resid = data if data is not None else case_data(ci)
    if scale_shift is not None:
        sc, sh = scale_shift
    extras = (ci * len(MODES) + MODES.index(mode)) % 2 == 1
    x1 = np.ascontiguousarray(x[..., c0:]) if c0 < x.shape[-1] else None
    return eng.op_conv2d(np.ascontiguousarray(x[..., :c0]), w, b, x1=x1,
                         gn_scale=None if mode == "copy" else sc, gn_shift=None if mode == "copy" else sh,
                         swish=mode == "swish", chan_bias=cb if extras else None, resid=resid if extras else None), extras


def border_scale_shift():
    (B, _, _, Cin, _), _ = CASES[0]
    return np.zeros((B, Cin), np.float32), np.full((B, Cin), 3.0, np.float32)


def forward_input():
    cfg = synth.sweep_unet_config("D")
    x, nl = synth.synth_unet_input(cfg, FWD_B, FWD_HW, FWD_HW, 3)
    return cfg, x, nl


def reference(data, mode, extras, scale_shift=None):
    x, w, b, sc, sh, cb, resid = data
    if scale_shift is not None:
        sc, sh = scale_shift
    B, H, W, C = x.shape
    a = x.astype(np.float64)
    if mode != "copy":
        a = a * sc.astype(np.float64)[:, None, None, :] + sh.astype(np.float64)[:, None, None, :]
    if mode == "swish":
        a = a / (1.0 + np.exp(-a))
    ap = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))        # the border is zero, not the activation of anything
    w64 = w.astype(np.float64)
    out = np.zeros((B * H * W, w.shape[0]), np.float64)
    for dy in range(3):
        for dx in range(3):
            out += np.ascontiguousarray(ap[:, dy:dy + H, dx:dx + W, :]).reshape(-1, C) @ np.ascontiguousarray(w64[:, :, dy, dx].T)
    out = (out + b.astype(np.float64)).reshape(B, H, W, -1)
    if extras:
        out = out + cb.astype(np.float64)[:, None, None, :] + resid.astype(np.float64)
    return out


def child_main(path):
    """Everything the tests compare across the switch, in the order the tests run it."""
    Engine = pkg("engine").Engine
    e = Engine(synth.tiny_unet_config(), 0)
    out = {}
    for ci in range(len(CASES)):
        data = case_data(ci)
        for mode in MODES:
            out[f"c{ci}_{mode}"] = run_case(e, ci, mode, data)[0]
    out["border"] = run_case(e, 0, "swish", scale_shift=border_scale_shift())[0]
    out["passes_ops"] = np.int64(e.gn_wino_passes())
    e.close()
    cfg, x, nl = forward_input()
    e = Engine(cfg, 0)
    e.load_state_dict(synth.synth_state_dict(cfg, 21))
    out["forward"] = e.unet_forward_np(x, nl)
    out["passes_forward"] = np.int64(e.gn_wino_passes())
    e.close()
    np.savez(path, **out)


@pytest.fixture(scope="module")
def eng():
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fused():
    """op_conv2d outputs of this process (the fused route), filled by the tests below and compared with the child's."""
    return {}


@pytest.fixture(scope="module")
def two_pass(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gn_wino") / "two_pass.npz")
    env = dict(os.environ)
    env["SR3_NO_GN_WINO"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    z = np.load(path)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("ci", range(len(CASES)), ids=["x".join(map(str, c)) + f"-x0_{c0}" for c, c0 in CASES])
def test_fused_pass_against_float64(eng, fused, ci):
    (B, H, W, Cin, Cout), _ = CASES[ci]
    assert eng.conv_plan(B, H, W, Cin, Cout, precision="f32")["kernel"] == "wino_three_pass"
    data = case_data(ci)
    for mode in MODES:
        n0 = eng.gn_wino_passes()
        got, extras = run_case(eng, ci, mode, data)
        assert eng.gn_wino_passes() == n0 + 1
        fused[f"c{ci}_{mode}"] = got
        err = np.abs(got - reference(data, mode, extras)).reshape(B, -1).max(1)
        print(f"{CASES[ci]} {mode}{' + chan_bias + resid' if extras else ''}: max abs err {err.max():.2e} (image {int(err.argmax())})")
        assert err.max() <= BAR[mode], err
        np.testing.assert_array_equal(got[0], got[B - 1])


def test_border_pixels_are_zero_not_activated(eng, fused):
    """scale 0, shift 3: every in-image activation is swish(3) = 2.86; an activated border pixel would add 2.86 * (a
    border tap's weights) to the edge outputs, far beyond the bar."""
    data = case_data(0)
    ss = border_scale_shift()
    n0 = eng.gn_wino_passes()
    got, extras = run_case(eng, 0, "swish", data, scale_shift=ss)
    assert eng.gn_wino_passes() == n0 + 1
    fused["border"] = got
    err = np.abs(got - reference(data, "swish", extras, scale_shift=ss))
    print(f"border case: max abs err {err.max():.2e}")
    assert err.max() <= BAR["swish"]


def test_other_routes_leave_the_counter(eng):
    B, H, W, Cin, Cout = DIRECT_CASE
    assert eng.conv_plan(B, H, W, Cin, Cout, precision="f32")["kernel"].startswith("generic_")
    rs = np.random.RandomState(7)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    sc = (1 + 0.1 * rs.standard_normal((16, Cin))).astype(np.float32)
    sh = (0.1 * rs.standard_normal((16, Cin))).astype(np.float32)
    x = rs.standard_normal((16, H, W, Cin)).astype(np.float32)
    n0 = eng.gn_wino_passes()
    eng.op_conv2d(x[:B], w, gn_scale=sc[:B], gn_shift=sh[:B], swish=True)       # 960 tiles: direct
    assert eng.gn_wino_passes() == n0
    eng.set_precision("f16x3")
    try:
        eng.op_conv2d(x, w, gn_scale=sc, gn_shift=sh, swish=True)               # the first shape, split-f16
    finally:
        eng.set_precision("f32")
    assert eng.gn_wino_passes() == n0
    eng.op_conv2d(x, w, gn_scale=sc, gn_shift=sh, swish=True)                   # ... and in f32: fused
    assert eng.gn_wino_passes() == n0 + 1


def test_bit_identical_to_the_two_passes(eng, fused, two_pass):
    assert int(two_pass["passes_ops"]) == 0 and int(two_pass["passes_forward"]) == 0
    for ci in range(len(CASES)):
        for mode in MODES:
            k = f"c{ci}_{mode}"
            if k not in fused:          # (this test selected alone)
                fused[k] = run_case(eng, ci, mode)[0]
            assert np.array_equal(fused[k], two_pass[k]), k
    if "border" not in fused:
        fused["border"] = run_case(eng, 0, "swish", scale_shift=border_scale_shift())[0]
    assert np.array_equal(fused["border"], two_pass["border"])


def test_unet_forward_mixes_fused_and_two_pass_levels(two_pass):
    cfg, x, nl = forward_input()
    e = pkg("engine").Engine(cfg, 0)
    try:
        e.load_state_dict(synth.synth_state_dict(cfg, 21))
        assert e.conv_plan(FWD_B, 32, 32, 128, 128, stats=True)["kernel"] == "wino_three_pass"
        assert e.conv_plan(FWD_B, 16, 16, 256, 256, stats=True)["kernel"].startswith("generic_")
        assert e.conv_plan(FWD_B, 8, 8, 512, 512, stats=True)["kernel"].startswith("generic_")
        got = e.unet_forward_np(x, nl)
        passes = e.gn_wino_passes()
    finally:
        e.close()
    print(f"sweep config D, B = {FWD_B}, {FWD_HW}x{FWD_HW}: {passes} fused passes")
    assert passes > 0
    assert np.isfinite(got).all()
    assert np.array_equal(got, two_pass["forward"])


if __name__ == "__main__":
    child_main(sys.argv[1])
