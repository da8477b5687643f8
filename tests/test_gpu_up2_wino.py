"""The exact-f32 Upsample conv (nearest x2 + conv3x3) as sub-pixel Winograd F(2x2, 2x2) (wino_up2_kernel) against a float64
numpy conv, its fused GroupNorm statistics against the fp64 sums of the call's own stored output, and the phase form it
replaces against the bits of the parent commit's library.

The form is an unexported field of the conv plan (ConvPlan::up2_wino); the switches are read once per process, so two child
processes of this file run the same calls:
  "forced"  SR3_UP2_WINO_FORCE=1: the new kernel wherever its preconditions hold (the tuning constant lifted, nothing else)
  "off"     SR3_NO_UP2_WINO=1: four sub-pixel phase convs on the direct kernel everywhere (the counter stays 0)
Engine.up2_wino_launches() tells which form ran.

Shapes (B, H_low, W_low, Cin, Cout): the smallest at which each path of the kernel can go wrong.
  (2, 4, 64, 32, 32)     R = 1 (one strip per block), one K-step, one channel block
  (1, 2, 128, 96, 64)    two strips per tile row, odd step count, two channel blocks
  (3, 4, 32, 64, 96)     R = 2 (two tile rows per block)
  (2, 8, 16, 160, 32)    R = 4 and five K-steps -- but the direct plan of this shape is a split-K plan, which is outside the
                         kernel's preconditions (the exported plan's split columns must stay what they are): it runs the
                         phase form also when forced, and is one of the "outside" shapes below
  (64, 8, 16, 160, 96)   so this one stands in for it: R = 4, five K-steps, unsplit (three distinct images repeated)
  (1, 24, 16, 32, 64)    several R = 4 blocks per image
  (1, 4, 128, 64, 32)    128-pixel statistics slices at a width of 128: one block runs the two strips of a slice pair
Each runs with and without bias and with and without statistics. The direct plans of these shapes have statistics slices of
128 low-resolution pixels (tile 128x32) or of 64 (tile 64x64); the kernel writes either. gate() restates the preconditions
(csrc/kernels_conv.hip, up2_wino_rows) from the exported plan.

Bars: 2e-5 absolute against float64 on O(1) data (tests/test_gpu_conv_stats.py: N(0,1) inputs, N(0,1) / sqrt(9 Cin) weights,
N(0,1) bias), statistics 1e-9 relative per slice (the same file's bar). The UNet forwards compare forced against off at 1e-4,
the fixture tests' bar. The measured maxima are printed.

tests/golden/up2_direct_parent.json holds sha256 digests of outputs and statistics recorded from a build of the PARENT commit
(the direct kernel has no atomics and a fixed summation order, so the bits do not depend on the machine): every shape
under SR3_NO_UP2_WINO=1, and the shapes outside the preconditions under FORCE, must give exactly those. To record again,
build the older commit elsewhere and run
    SR3_LIB=/path/to/older/libsr3hip.so python tests/test_gpu_up2_wino.py record OUT.json
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

GOLDEN_FILE = os.path.join(GOLDEN, "up2_direct_parent.json")
MIN_BLOCKS = 512                         # UP2_WINO_MIN_BLOCKS (csrc/sr3_internal.h)

TABLE = [(2, 4, 64, 32, 32), (1, 2, 128, 96, 64), (3, 4, 32, 64, 96), (2, 8, 16, 160, 32), (64, 8, 16, 160, 96), (1, 24, 16, 32, 64),
         (1, 4, 128, 64, 32)]
# outside the preconditions: low-resolution width 8 and 24, Cout = 48, a shape the plan splits (also TABLE[3])
OUTSIDE = [(2, 8, 8, 32, 32), (2, 8, 24, 32, 32), (2, 8, 16, 32, 48), (1, 8, 16, 512, 32)]
VARIANTS = [(True, True), (True, False), (False, True), (False, False)]          # (bias, statistics)
DEFAULT_CASE = (64, 16, 16, 32, 128)     # exactly MIN_BLOCKS blocks: the default gate takes it
BORDER = [0, 2, 5]                       # TABLE rows (R = 1, 2, 4) that also run the border-only input
FWD = {"tiny": (2, 32), "D": (8, 64)}    # config -> (B, H = W): every Upsample conv of the forward meets the preconditions


def _id(shape, bias, stats):
    return "x".join(map(str, shape)) + ("-bias" if bias else "") + ("-stats" if stats else "")


def gate(shape, stats, forced):
    """up2_wino_rows restated from the exported plan: True where wino_up2_kernel runs"""
    B, H, W, Cin, Cout = shape
    R = {16: 4, 32: 2}.get(W, 1 if W % 64 == 0 else 0)
    if R == 0 or H % (2 * R) or Cin % 32 or Cout % 32:
        return False
    plan = engine.conv_plan(B, H, W, Cin, Cout, 3, 1, 1, precision="f32", stats=stats)
    if plan["split"] != "none":
        return False
    if stats:
        tm = plan["tile"][0]
        if tm not in (64, 128) or plan["stats_slices"] != 4 * (H * W // tm) or (tm == 128 and W > 64 and W % 128):
            return False
    return forced or B * (H * W // 128) * (Cout // 32) >= MIN_BLOCKS


def _images(B):
    if B <= 3:
        return np.arange(B)
    idx = np.arange(B) % 3
    idx[0], idx[B // 2], idx[-1] = 0, 1, 2
    return idx


def case_data(shape, border=False):
    B, H, W, Cin, Cout = shape
    rs = np.random.RandomState(2000 + B + 3 * H + 5 * W + 7 * Cin + 11 * Cout + (1 if border else 0))
    idx = _images(B)
    xd = rs.standard_normal((int(idx.max()) + 1, H, W, Cin)).astype(np.float32)
    if border:
        xd[:, 1:-1, 1:-1, :] = 0
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    return idx, xd, w, b


def run_case(eng, shape, bias, stats, border=False, count=True):
    """-> (out, statistics or None, launches of the new kernel)"""
    idx, xd, w, b = case_data(shape, border)
    n0 = eng.up2_wino_launches() if count else 0
    eng.set_precision("f32")
    if stats:
        out, st = eng.op_conv2d(xd[idx], w, b if bias else None, up2=True, return_stats=True)
    else:
        out, st = eng.op_conv2d(xd[idx], w, b if bias else None, up2=True), None
    return out, st, (eng.up2_wino_launches() - n0) if count else 0


_want = {}


def want_f64(shape, bias, border=False):
    """float64 nearest x2 + conv3x3 of the distinct images (computed once per shape)"""
    key = (shape, border)
    idx, xd, w, b = case_data(shape, border)
    if key not in _want:
        nd, H, W, C = xd.shape
        up = np.pad(xd.astype(np.float64).repeat(2, 1).repeat(2, 2), ((0, 0), (1, 1), (1, 1), (0, 0)))
        out = np.zeros((nd * 4 * H * W, w.shape[0]))
        for dy in range(3):
            for dx in range(3):
                out += np.ascontiguousarray(up[:, dy:dy + 2 * H, dx:dx + 2 * W, :]).reshape(-1, C) @ w[:, :, dy, dx].T.astype(np.float64)
        _want[key] = out.reshape(nd, 2 * H, 2 * W, -1)
    return _want[key][idx] + (b.astype(np.float64) if bias else 0.0)


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
        n0 = e.up2_wino_launches()
        out = e.unet_forward_np(x, nl.reshape(-1))
        return out, e.up2_wino_launches() - n0, e.fallback_calls()
    finally:
        e.close()


def child_main(path):
    e = engine.Engine(synth.tiny_unet_config(), 0)
    out = {}
    for shape in TABLE + OUTSIDE:
        for bias, stats in VARIANTS:
            k = _id(shape, bias, stats)
            o, st, n = run_case(e, shape, bias, stats)
            out["o:" + k], out["n:" + k] = o, np.int64(n)
            if st is not None:
                out["s:" + k] = st
    for ti in BORDER:
        o, _, n = run_case(e, TABLE[ti], False, False, border=True)
        out[f"border{ti}"], out[f"border{ti}_n"] = o, np.int64(n)
    e.close()
    for name in FWD:
        o, n, fb = run_forward(name)
        out["fwd_" + name], out["fwd_" + name + "_n"], out["fwd_" + name + "_fb"] = o, np.int64(n), np.int64(fb)
    np.savez(path, **out)


def _child(tmp_path_factory, name, env_add):
    path = str(tmp_path_factory.mktemp("up2_wino") / (name + ".npz"))
    env = {k: v for k, v in os.environ.items() if k not in ("SR3_NO_UP2_WINO", "SR3_UP2_WINO_FORCE")}
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    z = np.load(path)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def off(tmp_path_factory):
    return _child(tmp_path_factory, "off", {"SR3_NO_UP2_WINO": "1"})


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    return _child(tmp_path_factory, "forced", {"SR3_UP2_WINO_FORCE": "1"})


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN_FILE) as f:
        return json.load(f)["cases"]


def test_the_table_reaches_every_path():
    """host only: which rows the forced gate admits, and what they reach"""
    takes = {s: [gate(s, st, True) for st in (False, True)] for s in TABLE + OUTSIDE}
    assert all(all(takes[s]) for i, s in enumerate(TABLE) if i != 3), takes
    assert not any(any(takes[s]) for s in OUTSIDE + [TABLE[3]]), takes
    assert engine.conv_plan(*TABLE[3], 3, 1, 1, precision="f32")["split"] != "none"
    assert engine.conv_plan(*OUTSIDE[3], 3, 1, 1, precision="f32")["split"] != "none"
    tiles = {s: engine.conv_plan(*s, 3, 1, 1, precision="f32", stats=True)["tile"][0] for s in TABLE}
    assert set(tiles.values()) == {64, 128}, tiles            # both statistics layouts
    assert not any(gate(s, True, False) for s in TABLE)        # the default gate leaves them alone
    B, H, W, Cin, Cout = DEFAULT_CASE
    assert B * (H * W // 128) * (Cout // 32) == MIN_BLOCKS and gate(DEFAULT_CASE, True, False)
    with open(GOLDEN_FILE) as f:
        have = set(json.load(f)["cases"])
    assert have == {_id(s, b, st) for s in TABLE + OUTSIDE for b, st in VARIANTS}


def _check_against_f64(shape, bias, stats, out, st, what):
    B, H, W, Cin, Cout = shape
    want = want_f64(shape, bias)
    assert out.shape == want.shape == (B, 2 * H, 2 * W, Cout)
    err = np.abs(out - want).max()
    msg = f"{_id(shape, bias, stats)} [{what}]: max abs err {err:.2e} (bar 2e-5)"
    assert err <= 2e-5, msg
    if stats:
        sl = engine.conv_plan(B, H, W, Cin, Cout, 3, 1, 1, precision="f32", stats=True)["stats_slices"]
        assert st is not None and st.shape == (B, sl, Cout, 2) and np.isfinite(st).all()
        # slice ph * (sl / 4) + k = pixels [k * tm, (k + 1) * tm) of phase image ph = (py, px), row-major over the low resolution
        g = out.astype(np.float64).reshape(B, H, 2, W, 2, Cout).transpose(0, 2, 4, 1, 3, 5).reshape(B, sl, -1, Cout)
        s1, s2 = g.sum(2), (g * g).sum(2)
        r1 = np.abs(st[..., 0] - s1).max() / np.abs(s1).max()
        r2 = np.abs(st[..., 1] - s2).max() / np.abs(s2).max()
        msg += f"; statistics, {sl} slices of {4 * H * W // sl} pixels: sum {r1:.1e}, sum of squares {r2:.1e} relative (bar 1e-9)"
        print(msg)
        assert r1 <= 1e-9 and r2 <= 1e-9
    else:
        print(msg)


@pytest.mark.gpu
@pytest.mark.parametrize("bias, stats", VARIANTS, ids=["bias-stats", "bias", "stats", "plain"])
@pytest.mark.parametrize("shape", TABLE, ids=lambda s: "x".join(map(str, s)))
def test_forced_against_float64(forced, shape, bias, stats):
    k = _id(shape, bias, stats)
    n = int(forced["n:" + k])
    assert n == int(gate(shape, stats, True)), (k, n)
    if shape != TABLE[3]:
        assert n == 1, f"{k}: up2_wino_launches did not rise"
    _check_against_f64(shape, bias, stats, forced["o:" + k], forced.get("s:" + k), "wino_up2_kernel" if n else "phase convs")


@pytest.mark.gpu
@pytest.mark.parametrize("ti", BORDER)
def test_border_only_input(forced, ti):
    """zero except on the outermost rows and columns: only the border windows of every phase contribute"""
    shape = TABLE[ti]
    assert int(forced[f"border{ti}_n"]) == 1
    out, want = forced[f"border{ti}"], want_f64(shape, False, border=True)
    err = np.abs(out - want).max()
    print(f"{'x'.join(map(str, shape))}, border-only input: max abs err {err:.2e} (bar 2e-5)")
    assert err <= 2e-5
    assert np.abs(want).max() > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TABLE + OUTSIDE, ids=lambda s: "x".join(map(str, s)))
def test_switch_gives_back_the_parents_bits(off, forced, gold, shape):
    for bias, stats in VARIANTS:
        k = _id(shape, bias, stats)
        assert int(off["n:" + k]) == 0, k
        assert digests(off["o:" + k], off.get("s:" + k)) == gold[k], f"{k}: SR3_NO_UP2_WINO=1 differs from the parent's library"
        if shape in OUTSIDE or shape == TABLE[3]:
            # outside the preconditions: the phase form also when forced, counter unchanged, the parent's bits
            assert int(forced["n:" + k]) == 0, k
            assert digests(forced["o:" + k], forced.get("s:" + k)) == gold[k], f"{k}: forced, outside the preconditions"


@pytest.mark.gpu
def test_default_gate_in_this_process():
    """the pytest process runs under the default gate: a small shape stays on the phase form, MIN_BLOCKS blocks do not"""
    e = engine.Engine(synth.tiny_unet_config(), 0)
    try:
        for shape in (TABLE[0], DEFAULT_CASE):
            out, st, n = run_case(e, shape, True, True)
            assert n == int(gate(shape, True, False)), (shape, n)
            _check_against_f64(shape, True, True, out, st, "default gate: " + ("wino_up2_kernel" if n else "phase convs"))
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FWD))
def test_unet_forward_forced_against_off(off, forced, name):
    B, hw = FWD[name]
    a, b = forced["fwd_" + name], off["fwd_" + name]
    assert int(off["fwd_" + name + "_n"]) == 0 and int(forced["fwd_" + name + "_n"]) > 0
    assert int(off["fwd_" + name + "_fb"]) == 0 and int(forced["fwd_" + name + "_fb"]) == 0
    assert np.isfinite(a).all() and a.shape == b.shape
    err = np.abs(a - b).max()
    print(f"config {name}, B = {B}, {hw}x{hw}: {int(forced['fwd_' + name + '_n'])} Upsample convs on wino_up2_kernel; "
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
        for shape in TABLE + OUTSIDE:
            for bias, stats in VARIANTS:
                out, st, _ = run_case(e, shape, bias, stats, count=False)
                rec[_id(shape, bias, stats)] = digests(out, st)
        e.close()
        with open(sys.argv[2], "w") as f:
            json.dump({"recorded_with": "libsr3hip.so of the parent commit, RandomState inputs of case_data", "cases": rec}, f, indent=1)
            f.write("\n")
