"""The second form of the three-pass Winograd plan (wino_gemm_out_kernel: the 16 position GEMMs and the output transform in
one kernel, M never stored) against the two kernels it replaces, bit for bit, and against a float64 numpy conv.

The form is chosen by conv_plan (ConvPlan::wino_gemm_out) where enough blocks of 64 tiles x 64 | 128 channels fill the
chip; the switches are read once per process, so two child processes of this file run the same calls:
  "off"     SR3_NO_WINO_GEMM_OUT=1: position GEMMs + wino_output_kernel everywhere (the counter stays 0)
  "forced"  SR3_WINO_GEMM_OUT_FORCE=1: the new kernel on every shape its preconditions admit, whatever the tuning gate says
and the pytest process runs them under the default gate. Engine.wino_gemm_out_launches() tells which form ran.

Data as in tests/test_gpu_conv_gates.py: N(0,1) inputs, N(0,1) / sqrt(9 Cin) weights, N(0,1) bias; every other case adds
the FeatureWiseAffine bias (chan_bias) and a residual. Image B-1 is a copy of image 0. Bars: 2e-5 absolute against float64
(test_gpu_conv_gates.py), fused statistics 1e-9 relative against the fp64 sums of the call's own stored output
(test_gpu_conv_stats.py). Across the switch outputs AND statistics are bit-equal: the kernel adds the statistics in
wino_output_kernel's order.

Gate arithmetic (csrc/kernels_conv.hip, wino_gemm_out_bn): bn = 128 if Cout % 128 == 0 else 64; statistics slices of 16 or
32 tiles (or none requested) are the preconditions; the tuning gate adds ceil(tiles / 64) * Cout / bn >=
WINO_GEMM_OUT_MIN_BLOCKS and Cin <= WINO_GEMM_OUT_MAX_CIN."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")

MIN_BLOCKS, MAX_CIN = 256, 256          # WINO_GEMM_OUT_MIN_BLOCKS, WINO_GEMM_OUT_MAX_CIN (csrc/sr3_internal.h)

# (B, H, W, Cin, Cout), slices of the fused GroupNorm statistics the call asks for (return_stats=True), 0 = a plain call
CASES = [
    ((16, 16, 16, 128, 64), 0),         # exactly 1024 tiles, one 64-channel block, 4 K-steps per position
    ((8, 16, 64, 160, 192), 0),         # five K chunks, three channel blocks, non-square
    ((64, 8, 8, 128, 128), 1),          # a block spans four images and four slices; chan_bias changes inside a block
    ((43, 14, 14, 256, 128), 0),        # 49 tiles per image (7x7, no power of two), 2107 tiles: ragged last block
    ((171, 6, 10, 128, 64), 0),         # 3x5 tiles per image
    ((5, 32, 32, 288, 192), 0),         # nine K chunks
    ((4, 32, 32, 128, 256), 16),        # 16 slices of 16 tiles per image, exactly 1024 tiles
    ((64, 32, 32, 128, 128), 8),        # 256 blocks of 64 tiles x 128 channels: the default gate takes it; 32-tile slices
]
IDS = ["x".join(map(str, c)) + ("-stats" if s else "") for c, s in CASES]
GN_CASE = 0                             # the case that also runs behind the GroupNorm pass that writes U
DIRECT_CASE = (15, 16, 16, 128, 64)     # 960 tiles: the direct kernel
FWD_B, FWD_HW = 40, 32                  # sweep config D: convs with the fused 1x1 term (res_conv) at its 32x32 level


def gate(case, stats_slices, forced):
    """wino_gemm_out_bn restated: True where the new kernel runs."""
    B, H, W, Cin, Cout = case
    tpi = (H // 2) * (W // 2)
    if stats_slices and tpi // stats_slices not in (16, 32):
        return False
    bn = 128 if Cout % 128 == 0 else 64
    return forced or (-(-B * tpi // 64) * (Cout // bn) >= MIN_BLOCKS and Cin <= MAX_CIN)


def case_data(ci):
    (B, H, W, Cin, Cout), _ = CASES[ci]
    rs = np.random.RandomState(4000 + ci)
    x = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    cb = rs.standard_normal((B, Cout)).astype(np.float32)
    resid = rs.standard_normal((B, H, W, Cout)).astype(np.float32)
    for a in (x, cb, resid):
        a[B - 1] = a[0]                 # the same image at batch positions 0 and B-1
    return x, w, b, cb, resid


def run_case(eng, ci, data=None):
    """The op_conv2d call of case ci -> (out, stats or None, launches of the new kernel); odd cases carry chan_bias + resid."""
    x, w, b, cb, resid = data if data is not None else case_data(ci)
    extras = ci % 2 == 1
    n0 = eng.wino_gemm_out_launches()
    kw = dict(chan_bias=cb if extras else None, resid=resid if extras else None)
    out, st = eng.op_conv2d(x, w, b, return_stats=True, **kw) if CASES[ci][1] else (eng.op_conv2d(x, w, b, **kw), None)
    return out, st, eng.wino_gemm_out_launches() - n0


def gn_data():
    (B, _, _, Cin, _), _ = CASES[GN_CASE]
    rs = np.random.RandomState(77)
    return (1 + 0.1 * rs.standard_normal((B, Cin))).astype(np.float32), (0.1 * rs.standard_normal((B, Cin))).astype(np.float32)


def run_gn_case(eng):
    """-> (out, GroupNorm passes that wrote U, launches of the new kernel)"""
    x, w, b, cb, resid = case_data(GN_CASE)
    sc, sh = gn_data()
    g0, n0 = eng.gn_wino_passes(), eng.wino_gemm_out_launches()
    out = eng.op_conv2d(x, w, b, gn_scale=sc, gn_shift=sh, swish=True, chan_bias=cb, resid=resid)
    return out, eng.gn_wino_passes() - g0, eng.wino_gemm_out_launches() - n0


def run_other_routes(eng):
    """launches of the new kernel by a direct-kernel shape and by the first shape in f16x3"""
    rs = np.random.RandomState(7)
    B, H, W, Cin, Cout = DIRECT_CASE
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    x = rs.standard_normal((16, H, W, Cin)).astype(np.float32)
    n0 = eng.wino_gemm_out_launches()
    eng.op_conv2d(x[:B], w)
    n1 = eng.wino_gemm_out_launches()
    eng.set_precision("f16x3")
    try:
        eng.op_conv2d(x, w)
    finally:
        eng.set_precision("f32")
    return n1 - n0, eng.wino_gemm_out_launches() - n1


def run_forward():
    cfg = synth.sweep_unet_config("D")
    x, nl = synth.synth_unet_input(cfg, FWD_B, FWD_HW, FWD_HW, 3)
    e = pkg("engine").Engine(cfg, 0)
    try:
        e.load_state_dict(synth.synth_state_dict(cfg, 21))
        n0 = e.wino_gemm_out_launches()
        out = e.unet_forward_np(x, nl)
        return out, e.wino_gemm_out_launches() - n0, e.fallback_calls()
    finally:
        e.close()


def child_main(path):
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    out = {}
    for ci in range(len(CASES)):
        o, st, n = run_case(e, ci)
        out[f"c{ci}"], out[f"n{ci}"] = o, np.int64(n)
        if st is not None:
            out[f"s{ci}"] = st
    o, g, n = run_gn_case(e)
    out["gn"], out["gn_passes"], out["gn_n"] = o, np.int64(g), np.int64(n)
    out["other"] = np.array(run_other_routes(e), np.int64)
    e.close()
    o, n, fb = run_forward()
    out["forward"], out["forward_n"], out["forward_fallback"] = o, np.int64(n), np.int64(fb)
    np.savez(path, **out)


def _child(tmp_path_factory, name, env_add):
    path = str(tmp_path_factory.mktemp("wino_gemm_out") / (name + ".npz"))
    env = dict(os.environ)
    env.pop("SR3_NO_WINO_GEMM_OUT", None)
    env.pop("SR3_WINO_GEMM_OUT_FORCE", None)
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    z = np.load(path)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def off(tmp_path_factory):
    return _child(tmp_path_factory, "off", {"SR3_NO_WINO_GEMM_OUT": "1"})


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    return _child(tmp_path_factory, "forced", {"SR3_WINO_GEMM_OUT_FORCE": "1"})


@pytest.fixture(scope="module")
def eng():
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    yield e
    e.close()


_want = {}


def want_f64(ci):
    """float64 numpy conv of case ci (computed once)"""
    if ci not in _want:
        x, w, b, cb, resid = case_data(ci)
        B, H, W, C = x.shape
        xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
        w64 = w.astype(np.float64)
        out = np.zeros((B * H * W, w.shape[0]), np.float64)
        for dy in range(3):
            for dx in range(3):
                out += np.ascontiguousarray(xp[:, dy:dy + H, dx:dx + W, :]).reshape(-1, C) @ np.ascontiguousarray(w64[:, :, dy, dx].T)
        out = (out + b.astype(np.float64)).reshape(B, H, W, -1)
        if ci % 2 == 1:
            out = out + cb.astype(np.float64)[:, None, None, :] + resid.astype(np.float64)
        _want[ci] = out
    return _want[ci]


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_bit_equal_to_gemm_plus_output_kernel(eng, off, forced, ci):
    case, sl = CASES[ci]
    stats = sl > 0
    plan = eng.conv_plan(*case, precision="f32", stats=stats)
    assert plan["kernel"] == "wino_three_pass" and (not stats or plan["stats_slices"] == sl)
    assert int(off[f"n{ci}"]) == 0
    # forced: the new kernel wherever its preconditions hold
    new_forced = gate(case, sl, True)
    assert int(forced[f"n{ci}"]) == int(new_forced)
    # this process: the default gate
    got, st, n = run_case(eng, ci)
    new_default = gate(case, sl, False)
    tiles = case[0] * (case[1] // 2) * (case[2] // 2)
    print(f"{case}{' + stats, %d slices' % sl if stats else ''}: {tiles} tiles; forced gate: {'new kernel' if new_forced else 'GEMM + output kernel'}; "
          f"default gate: {'new kernel' if new_default else 'GEMM + output kernel'} ({n} launches)")
    assert n == int(new_default)
    assert np.array_equal(forced[f"c{ci}"], off[f"c{ci}"])
    assert np.array_equal(got, off[f"c{ci}"])
    if stats:
        assert st is not None and f"s{ci}" in off and f"s{ci}" in forced
        assert np.isfinite(off[f"s{ci}"]).all()
        assert np.array_equal(forced[f"s{ci}"], off[f"s{ci}"])
        assert np.array_equal(st, off[f"s{ci}"])


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_against_float64(eng, forced, ci):
    (B, H, W, Cin, Cout), sl = CASES[ci]
    stats = sl > 0
    got = forced[f"c{ci}"]
    want = want_f64(ci)
    assert got.shape == want.shape
    err = np.abs(got - want).reshape(B, -1).max(1)
    print(f"{CASES[ci][0]}{' + chan_bias + resid' if ci % 2 else ''} [{int(forced[f'n{ci}'])} launches of the new kernel]: "
          f"max abs err {err.max():.2e} (image {int(err.argmax())})")
    assert err.max() <= 2e-5, err
    np.testing.assert_array_equal(got[0], got[B - 1])
    if stats:
        st = forced[f"s{ci}"]                           # [B, slices, Cout, 2]
        assert st.shape == (B, sl, Cout, 2) and np.isfinite(st).all()
        # slice s of image n = the run of th * tw / slices consecutive tiles (row-major), four pixels each
        g = got.astype(np.float64).reshape(B, H // 2, 2, W // 2, 2, Cout).transpose(0, 1, 3, 2, 4, 5)
        g = g.reshape(B, sl, -1, Cout)                  # [image][slice][tiles per slice x 4 pixels][channel]
        s1, s2 = g.sum(2), (g * g).sum(2)
        r1 = np.abs(st[..., 0] - s1).max() / np.abs(s1).max()
        r2 = np.abs(st[..., 1] - s2).max() / np.abs(s2).max()
        print(f"  statistics, {sl} slices: sum {r1:.1e}, sum of squares {r2:.1e} relative")
        assert r1 <= 1e-9 and r2 <= 1e-9
        np.testing.assert_array_equal(st[0], st[B - 1])


def test_behind_the_groupnorm_pass_that_writes_u(eng, off, forced):
    assert int(forced["gn_passes"]) == 1 and int(forced["gn_n"]) == 1
    assert int(off["gn_passes"]) == 1 and int(off["gn_n"]) == 0
    assert np.array_equal(forced["gn"], off["gn"])
    got, g, n = run_gn_case(eng)                        # the default gate: 16 blocks, GEMM + output kernel
    assert g == 1 and n == int(gate(CASES[GN_CASE][0], 0, False))
    assert np.array_equal(got, off["gn"])
    # float64: affine, x * sigmoid(x), zero padding, conv (bar of tests/test_gpu_gn_wino_input.py with Swish)
    x, w, b, cb, resid = case_data(GN_CASE)
    sc, sh = gn_data()
    a = x.astype(np.float64) * sc.astype(np.float64)[:, None, None, :] + sh.astype(np.float64)[:, None, None, :]
    a = a / (1.0 + np.exp(-a))
    B, H, W, C = x.shape
    ap = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))
    want = np.zeros((B * H * W, w.shape[0]), np.float64)
    for dy in range(3):
        for dx in range(3):
            want += ap[:, dy:dy + H, dx:dx + W, :].reshape(-1, C) @ w[:, :, dy, dx].T.astype(np.float64)
    want = (want + b).reshape(B, H, W, -1) + cb.astype(np.float64)[:, None, None, :] + resid
    err = np.abs(forced["gn"] - want).max()
    print(f"behind gn_wino_input_kernel: max abs err {err:.2e}")
    assert err <= 3e-5


def test_unet_forward_with_the_fused_1x1_term(off, forced):
    """Config D's ResnetBlocks with a res_conv run the 1x1 conv first, into the output; the new kernel adds it as the residual."""
    assert int(off["forward_n"]) == 0
    print(f"sweep config D, B = {FWD_B}, {FWD_HW}x{FWD_HW}: {int(forced['forward_n'])} launches of the new kernel (forced)")
    assert int(forced["forward_n"]) > 0
    assert int(forced["forward_fallback"]) == 0 and int(off["forward_fallback"]) == 0
    assert np.isfinite(forced["forward"]).all()
    assert np.array_equal(forced["forward"], off["forward"])
    got, n, fb = run_forward()                          # the default gate
    print(f"  default gate: {n} launches")
    assert fb == 0
    assert np.array_equal(got, off["forward"])


def test_other_routes_leave_the_counter(eng, off, forced):
    assert tuple(forced["other"]) == (0, 0) and tuple(off["other"]) == (0, 0)
    B, H, W, Cin, Cout = DIRECT_CASE
    assert eng.conv_plan(B, H, W, Cin, Cout, precision="f32")["kernel"].startswith("generic_")
    assert run_other_routes(eng) == (0, 0)


if __name__ == "__main__":
    child_main(sys.argv[1])
