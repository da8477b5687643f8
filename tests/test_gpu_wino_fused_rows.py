"""The one-pass exact-f32 Winograd kernel with R = 2 | 4 tile rows per block (wino_fused_kernel<R>: the 32x32 and 16x16
levels) against a float64 numpy conv, its fused GroupNorm statistics against the fp64 sums of the call's own stored output,
and the three-pass forms it replaces against the bits of the parent commit's library.

The form is an unexported field of the three-pass plan (ConvPlan::wino_fused_rows); the switches are read once per process,
so two child processes of this file run the same calls:
  "forced"  SR3_WINO_FUSED_ROWS_FORCE=1: the new form wherever its preconditions hold (the tuning constants lifted, nothing else)
  "off"     SR3_NO_WINO_FUSED_ROWS=1: the parent's launches everywhere (the counter stays 0)
Engine.wino_fused_rows_launches() tells which form ran.

Shapes (B, H, W, Cin, Cout): the smallest that still have a three-pass plan (at least 1024 tiles, Cin at least 128).
  (4, 32, 32, 128, 64)    R = 2, the smallest 32x32 case
  (4, 32, 32, 160, 192)   five K-steps, three channel blocks
  (4, 32, 32, 128, 256)   16 statistics slices per image: two per block
  (8, 16, 32, 128, 64)    non-square
  (16, 16, 16, 128, 64)   R = 4
  (8, 64, 16, 128, 128)   R = 4, tall
  (6, 30, 32, 128, 64)    15 tile rows: outside the preconditions (H % 2R), three-pass also when forced
Each runs plain (bias only) and with bias + residual + FeatureWiseAffine bias + statistics; the first also behind the
GroupNorm + Swish pass, which then writes the zero-bordered activated tensor instead of U.

Bars: 2e-5 absolute against float64 on O(1) data (tests/test_gpu_conv_gates.py: N(0,1) inputs, N(0,1) / sqrt(9 Cin) weights,
N(0,1) bias), 3e-5 behind GroupNorm + Swish (tests/test_gpu_gn_wino_input.py), statistics 1e-9 relative per slice
(tests/test_gpu_conv_stats.py). The UNet forwards compare forced against off at 1e-4, the fixture tests' bar. The two forms
fold A^T M A in different orders and are not bit-equal: the largest difference is printed, as a record.

tests/golden/wino_fused_rows_parent.json holds sha256 digests of outputs and statistics recorded from a build of the PARENT
commit (no atomics, fixed summation orders: the bits do not depend on the machine): every case under
SR3_NO_WINO_FUSED_ROWS=1, and the shape outside the preconditions under FORCE, must give exactly those. To record again,
build the older commit elsewhere and run
    SR3_LIB=/path/to/older/libsr3hip.so python tests/test_gpu_wino_fused_rows.py record OUT.json
never from the tree under test."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, pkg

synth = pkg("synth")
engine = pkg("engine")

GOLDEN_FILE = os.path.join(GOLDEN, "wino_fused_rows_parent.json")
MIN_BLOCKS = {2: 2048, 4: 0}             # WINO_FUSED_ROWS_MIN_BLOCKS, _16 (csrc/sr3_internal.h); 0: never by default
SWITCHES = ("SR3_NO_WINO_FUSED_ROWS", "SR3_WINO_FUSED_ROWS_FORCE")

TABLE = [(4, 32, 32, 128, 64), (4, 32, 32, 160, 192), (4, 32, 32, 128, 256), (8, 16, 32, 128, 64), (16, 16, 16, 128, 64),
         (8, 64, 16, 128, 128), (6, 30, 32, 128, 64)]
OUTSIDE = [TABLE[6]]
VARIANTS = [False, True]                 # plain | bias + residual + FeatureWiseAffine bias + statistics
GN_SHAPE = TABLE[0]
DEFAULT_CASE = (64, 32, 32, 128, 256)    # exactly MIN_BLOCKS[2] blocks: the default gate takes it (three distinct images)
FWD = {"tiny": (2, 32), "D": (16, 32)}   # config -> (B, H = W); D: R = 2 at its 32x32 level, R = 4 at 16x16, 8x8 direct


def _id(shape, extras):
    return "x".join(map(str, shape)) + ("-extras" if extras else "")


def gate(shape, stats, forced):
    """wino_fused_rows (csrc/kernels_conv.hip) restated from the exported plan: tile rows per block, 0 = a parent's form"""
    B, H, W, Cin, Cout = shape
    plan = engine.conv_plan(B, H, W, Cin, Cout, precision="f32", stats=stats)
    R = {32: 2, 16: 4}.get(W, 0)
    if plan["kernel"] != "wino_three_pass" or R == 0 or H % (2 * R) or Cin % 32 or Cout % 64:
        return 0
    bpi = (H // 2) * (W // 2) // 32
    if stats and (plan["stats_slices"] <= 0 or plan["stats_slices"] % bpi or plan["stats_slices"] // bpi not in (1, 2, 4)):
        return 0
    if forced:
        return R
    return R if MIN_BLOCKS[R] > 0 and B * bpi * (Cout // 64) >= MIN_BLOCKS[R] else 0


def _images(B):
    if B <= 16:
        return np.arange(B)
    idx = np.arange(B) % 3
    idx[0], idx[B // 2], idx[-1] = 0, 1, 2
    return idx


def case_data(shape):
    B, H, W, Cin, Cout = shape
    rs = np.random.RandomState(5000 + B + 3 * H + 5 * W + 7 * Cin + 11 * Cout)
    idx = _images(B)
    nd = int(idx.max()) + 1
    x = rs.standard_normal((nd, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    cb = rs.standard_normal((nd, Cout)).astype(np.float32)
    resid = rs.standard_normal((nd, H, W, Cout)).astype(np.float32)
    return idx, x, w, b, cb, resid


def gn_data(shape):
    rs = np.random.RandomState(77)
    B, Cin = shape[0], shape[3]
    return (1 + 0.1 * rs.standard_normal((B, Cin))).astype(np.float32), (0.1 * rs.standard_normal((B, Cin))).astype(np.float32)


def run_case(eng, shape, extras, gn=False, count=True):
    """-> (out, statistics or None, launches of the new form, GroupNorm passes that wrote U)"""
    idx, x, w, b, cb, resid = case_data(shape)
    n0, g0 = (eng.wino_fused_rows_launches(), eng.gn_wino_passes()) if count else (0, 0)
    eng.set_precision("f32")
    kw = {}
    if gn:
        kw["gn_scale"], kw["gn_shift"] = gn_data(shape)
        kw["swish"] = True
    if extras:
        out, st = eng.op_conv2d(x[idx], w, b, chan_bias=cb[idx], resid=resid[idx], return_stats=True, **kw)
    else:
        out, st = eng.op_conv2d(x[idx], w, b, **kw), None
    n, g = (eng.wino_fused_rows_launches() - n0, eng.gn_wino_passes() - g0) if count else (0, 0)
    return out, st, n, g


_want = {}


def want_f64(shape, extras, gn=False):
    """float64 conv3x3 of the distinct images (computed once per shape and prologue)"""
    idx, x, w, b, cb, resid = case_data(shape)
    key = (shape, gn)
    if key not in _want:
        a = x.astype(np.float64)
        if gn:
            sc, sh = gn_data(shape)
            a = a * sc.astype(np.float64)[:, None, None, :] + sh.astype(np.float64)[:, None, None, :]
            a = a / (1.0 + np.exp(-a))
        nd, H, W, C = a.shape
        ap = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))
        out = np.zeros((nd * H * W, w.shape[0]))
        for dy in range(3):
            for dx in range(3):
                out += np.ascontiguousarray(ap[:, dy:dy + H, dx:dx + W, :]).reshape(-1, C) @ w[:, :, dy, dx].T.astype(np.float64)
        _want[key] = out.reshape(nd, H, W, -1) + b.astype(np.float64)
    out = _want[key][idx]
    if extras:
        out = out + cb.astype(np.float64)[idx][:, None, None, :] + resid.astype(np.float64)[idx]
    return out


def digests(out, st):
    d = {"out": hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()}
    if st is not None:
        d["stats"] = hashlib.sha256(np.ascontiguousarray(st).tobytes()).hexdigest()
    return d


def run_forward(name):
    cfg = synth.tiny_unet_config() if name == "tiny" else synth.sweep_unet_config(name)
    B, hw = FWD[name]
    x, nl = synth.synth_unet_input(cfg, B, hw, hw, 5)
    e = engine.Engine(cfg, 0)
    try:
        e.load_state_dict(synth.synth_state_dict(cfg, 31))
        n0 = e.wino_fused_rows_launches()
        out = e.unet_forward_np(x, nl.reshape(-1))
        return out, e.wino_fused_rows_launches() - n0, e.fallback_calls()
    finally:
        e.close()


def child_main(path):
    e = engine.Engine(synth.tiny_unet_config(), 0)
    out = {}
    for shape in TABLE:
        for extras in VARIANTS:
            k = _id(shape, extras)
            o, st, n, _ = run_case(e, shape, extras)
            out["o:" + k], out["n:" + k] = o, np.int64(n)
            if st is not None:
                out["s:" + k] = st
    o, _, n, g = run_case(e, GN_SHAPE, True, gn=True)
    out["gn"], out["gn_n"], out["gn_passes"] = o, np.int64(n), np.int64(g)
    e.close()
    for name in FWD:
        o, n, fb = run_forward(name)
        out["fwd_" + name], out["fwd_" + name + "_n"], out["fwd_" + name + "_fb"] = o, np.int64(n), np.int64(fb)
    np.savez(path, **out)


def _child(tmp_path_factory, name, env_add):
    path = str(tmp_path_factory.mktemp("wino_fused_rows") / (name + ".npz"))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    z = np.load(path)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def off(tmp_path_factory):
    return _child(tmp_path_factory, "off", {"SR3_NO_WINO_FUSED_ROWS": "1"})


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    return _child(tmp_path_factory, "forced", {"SR3_WINO_FUSED_ROWS_FORCE": "1"})


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN_FILE) as f:
        return json.load(f)["cases"]


def test_the_table_reaches_every_path():
    """host only: what the forced gate admits, what the default gate leaves alone"""
    for s in TABLE:
        for stats in (False, True):
            assert engine.conv_plan(*s, precision="f32", stats=stats)["kernel"] == "wino_three_pass", s
    takes = {s: [gate(s, st, True) for st in (False, True)] for s in TABLE}
    assert [takes[s] for s in TABLE[:6]] == [[2, 2], [2, 2], [2, 2], [2, 2], [4, 4], [4, 4]], takes
    assert takes[TABLE[6]] == [0, 0]
    spb = {s: engine.conv_plan(*s, precision="f32", stats=True)["stats_slices"] * 128 // (s[1] * s[2]) for s in TABLE[:6] + [DEFAULT_CASE]}
    assert spb[DEFAULT_CASE] == 1 and set(spb[s] for s in TABLE[:6]) == {2}, spb     # whole-block slices and two per block
    assert not any(gate(s, True, False) for s in TABLE)        # the default gate leaves them alone
    B, H, W, Cin, Cout = DEFAULT_CASE
    assert B * (H * W // 128) * (Cout // 64) == MIN_BLOCKS[2] and gate(DEFAULT_CASE, True, False) == 2
    with open(GOLDEN_FILE) as f:
        have = set(json.load(f)["cases"])
    assert have == {_id(s, x) for s in TABLE for x in VARIANTS}


def test_default_gate_keeps_the_routes_of_the_existing_tests():
    """host only: no shape that tests/test_gpu_wino_gemm_out.py, test_gpu_gn_wino_input.py, test_gpu_conv_stats.py and
    test_gpu_dropout.py run (they count gn_wino_passes() / wino_gemm_out_launches() under the default gate) changes route"""
    import test_gpu_conv_stats as cs
    import test_gpu_gn_wino_input as gw
    import test_gpu_wino_gemm_out as go
    shapes = [c for c, _ in go.CASES] + [go.DIRECT_CASE] + [c for c, _ in gw.CASES] + [gw.DIRECT_CASE]
    shapes += [tuple(c[1][:5]) for c in cs.CASES if c[0] == "f32" and len(c[1]) == 5]
    # the UNet forwards of those files: sweep config D (128 / 256 / 512 channels at 32x32 / 16x16 / 8x8) at B <= 40
    for B in (2, 4, go.FWD_B):
        shapes += [(B, 32, 32, ci, 128) for ci in (128, 256)] + [(B, 16, 16, ci, 256) for ci in (128, 256, 384, 512)]
    assert (64, 32, 32, 128, 128) in shapes                     # 1024 blocks: stays on wino_gemm_out_kernel
    for s in shapes:
        for stats in (False, True):
            assert gate(s, stats, False) == 0, s


def _check_against_f64(shape, extras, out, st, what, gn=False):
    B, H, W, Cin, Cout = shape
    want = want_f64(shape, extras, gn)
    bar = 3e-5 if gn else 2e-5
    assert out.shape == want.shape == (B, H, W, Cout)
    err = np.abs(out - want).max()
    msg = f"{_id(shape, extras)}{' behind GroupNorm + Swish' if gn else ''} [{what}]: max abs err {err:.2e} (bar {bar:.0e})"
    assert err <= bar, msg
    if st is not None:
        sl = engine.conv_plan(B, H, W, Cin, Cout, precision="f32", stats=True)["stats_slices"]
        assert st.shape == (B, sl, Cout, 2) and np.isfinite(st).all()
        # slice s of image n = the run of th * tw / slices consecutive tiles (row-major), four pixels each
        g = out.astype(np.float64).reshape(B, H // 2, 2, W // 2, 2, Cout).transpose(0, 1, 3, 2, 4, 5).reshape(B, sl, -1, Cout)
        s1, s2 = g.sum(2), (g * g).sum(2)
        r1 = np.abs(st[..., 0] - s1).max() / np.abs(s1).max()
        r2 = np.abs(st[..., 1] - s2).max() / np.abs(s2).max()
        msg += f"; statistics, {sl} slices of {H * W // sl} pixels: sum {r1:.1e}, sum of squares {r2:.1e} relative (bar 1e-9)"
        print(msg)
        assert r1 <= 1e-9 and r2 <= 1e-9
    else:
        print(msg)


@pytest.mark.gpu
@pytest.mark.parametrize("extras", VARIANTS, ids=["plain", "extras"])
@pytest.mark.parametrize("shape", TABLE, ids=lambda s: "x".join(map(str, s)))
def test_forced_against_float64(forced, off, shape, extras):
    k = _id(shape, extras)
    n = int(forced["n:" + k])
    assert n == int(gate(shape, extras, True) > 0), (k, n)
    assert n == (0 if shape in OUTSIDE else 1), f"{k}: wino_fused_rows_launches"
    _check_against_f64(shape, extras, forced["o:" + k], forced.get("s:" + k), "wino_fused_kernel<R>" if n else "three-pass")
    print(f"  largest |forced - off| (a record, no bar): {np.abs(forced['o:' + k] - off['o:' + k]).max():.2e}")


@pytest.mark.gpu
def test_behind_the_groupnorm_pass(forced, off):
    """forced: the apply pass writes the zero-bordered activated tensor (no pass writes U); off: the pass that writes U"""
    assert int(forced["gn_n"]) == 1 and int(forced["gn_passes"]) == 0
    assert int(off["gn_n"]) == 0 and int(off["gn_passes"]) == 1
    _check_against_f64(GN_SHAPE, True, forced["gn"], None, "wino_fused_kernel<2>", gn=True)
    _check_against_f64(GN_SHAPE, True, off["gn"], None, "three-pass", gn=True)
    print(f"  largest |forced - off| (a record, no bar): {np.abs(forced['gn'] - off['gn']).max():.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TABLE, ids=lambda s: "x".join(map(str, s)))
def test_switch_gives_back_the_parents_bits(off, forced, gold, shape):
    for extras in VARIANTS:
        k = _id(shape, extras)
        assert int(off["n:" + k]) == 0, k
        assert digests(off["o:" + k], off.get("s:" + k)) == gold[k], f"{k}: SR3_NO_WINO_FUSED_ROWS=1 differs from the parent's library"
        if shape in OUTSIDE:
            # outside the preconditions: the parent's form also when forced, counter unchanged, the parent's bits
            assert int(forced["n:" + k]) == 0, k
            assert digests(forced["o:" + k], forced.get("s:" + k)) == gold[k], f"{k}: forced, outside the preconditions"


@pytest.mark.gpu
def test_default_gate_in_this_process():
    """the pytest process runs under the default gate: a small shape stays on the parent's form, MIN_BLOCKS blocks do not"""
    e = engine.Engine(synth.tiny_unet_config(), 0)
    try:
        for shape in (TABLE[0], TABLE[4], DEFAULT_CASE):
            out, st, n, _ = run_case(e, shape, True)
            assert n == int(gate(shape, True, False) > 0), (shape, n)
            _check_against_f64(shape, True, out, st, "default gate: " + ("wino_fused_kernel<R>" if n else "three-pass"))
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FWD))
def test_unet_forward_forced_against_off(off, forced, name):
    B, hw = FWD[name]
    a, b = forced["fwd_" + name], off["fwd_" + name]
    # (the tiny configuration has no conv of 128 input channels: no three-pass plan, the forced forward is the parent's)
    assert int(off["fwd_" + name + "_n"]) == 0 and (int(forced["fwd_" + name + "_n"]) > 0) == (name == "D")
    assert int(off["fwd_" + name + "_fb"]) == 0 and int(forced["fwd_" + name + "_fb"]) == 0
    assert np.isfinite(a).all() and a.shape == b.shape
    err = np.abs(a - b).max()
    print(f"config {name}, B = {B}, {hw}x{hw}: {int(forced['fwd_' + name + '_n'])} convs on wino_fused_kernel<R>; "
          f"max |forced - off| = {err:.2e} (bar 1e-4), max |off| = {np.abs(b).max():.2f}")
    assert err <= 1e-4


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child_main(sys.argv[2])
    else:
        # records the golden file from the library SR3_LIB names (a build of the commit before the change)
        assert sys.argv[1] == "record" and os.environ.get("SR3_LIB"), "record from another build of the library: set SR3_LIB"
        e = engine.Engine(synth.tiny_unet_config(), 0)
        rec = {}
        for shape in TABLE:
            for extras in VARIANTS:
                out, st, _, _ = run_case(e, shape, extras, count=False)
                rec[_id(shape, extras)] = digests(out, st)
        e.close()
        with open(sys.argv[2], "w") as f:
            json.dump({"recorded_with": "libsr3hip.so of the parent commit, RandomState inputs of case_data", "cases": rec}, f, indent=1)
            f.write("\n")
