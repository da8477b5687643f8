"""The LDS stages of wino_fused_kernel<2 | 4> and wino_up2_kernel<2 | 4> hold each of the block's 2R + 2 distinct padded
input rows once (tile row tr reads its four window rows from stage row 2 tr on) instead of four rows per tile row. The
arithmetic is untouched, so the first check is the bits: sha256 of outputs and statistics against
tests/golden/wino_stage_rows_parent.json, recorded from a build of the PARENT commit (no atomics, fixed summation orders:
the bits do not depend on the machine). To record again, build the older commit elsewhere and run
    SR3_LIB=/path/to/older/libsr3hip.so python tests/test_gpu_wino_stage_rows.py record OUT.json
never from the tree under test.

Both forms are unexported fields of the conv plan whose switches are read once per process, so one child process of this
file runs every case under SR3_WINO_FUSED_ROWS_FORCE=1 and SR3_UP2_WINO_FORCE=1 (the tuning constants lifted, nothing else);
Engine.wino_fused_rows_launches() and Engine.up2_wino_launches() tell which kernel ran.

Cases (B, H, W, Cin, Cout); H, W of the low resolution for the Upsample convs.
  wino_fused_kernel<R> is a form of the three-pass plan, which starts at 1024 tiles and Cin = 128 (wino_shape), and FORCE
  lifts the form's own tuning constants only. The four shapes the change was specified with
      (2, 4, 32, 32, 64)  (2, 8, 32, 96, 128)  (2, 8, 16, 32, 64)  (2, 16, 16, 160, 64)
  therefore run the direct kernel (test_what_each_case_reaches asserts it; a single K-step cannot be reached through
  the op at all: nk = 4 is the form's shortest loop). They stay, with every check below, and next to each stands the same
  geometry with B and Cin raised to that floor, which does reach the kernel:
      R = 2  (32, 4, 32, 128, 64)    one group of two tile rows per image; nk = 4
             (16, 8, 32, 160, 128)   two groups, so a row shared inside a block and a row shared between blocks both
                                     occur; nk = 5 (ends on the other stage); two channel blocks
      R = 4  (32, 8, 16, 128, 64)    one group of four tile rows; nk = 4
             (16, 16, 16, 160, 64)   two groups; nk = 5
  wino_up2_kernel<R> (widths of tests/test_gpu_up2_wino.py: 32 -> R = 2, 16 -> R = 4):
      R = 2  (3, 8, 32, 96, 96)      two groups, nk = 3              (2, 4, 32, 32, 32)   a single K-step: the DMA of the
      R = 4  (2, 16, 16, 96, 64)     two groups, nk = 3              (2, 8, 16, 32, 32)   next stage switched off at once
Each runs plain (no bias) and with everything its epilogue has: bias + residual + FeatureWiseAffine bias + statistics
(wino_up2_kernel has no residual: its gate leaves such a conv to the phase form). The two-group shapes of
wino_fused_kernel<R> also run behind the GroupNorm + Swish pass. The last image of every batch is a copy of image 0.

Checks per case: the parent's digests; float64 at 2e-5 absolute on O(1) data (N(0,1) inputs, N(0,1) / sqrt(9 Cin) weights,
N(0,1) bias: tests/test_gpu_conv_gates.py), 3e-5 behind GroupNorm + Swish (tests/test_gpu_gn_wino_input.py); statistics
against the fp64 sums of the call's own stored output at 1e-9 relative (tests/test_gpu_conv_stats.py); image B - 1
bit-identical to image 0; a second call gives the same bits.

The default gate (no switch set) takes the 16x16 level from 1024 blocks on up to Cin = 512: (64, 16, 16, 512, 512), three
distinct images replicated, runs in the pytest process, plain and behind GroupNorm + Swish: wino_fused_rows_launches() rises by
one, gn_wino_passes() does not rise (the pass writes the activated tensor, not U), the float64 bars hold; half the blocks
and Cin = 768 stay on the three-pass form. Under SR3_NO_WINO_FUSED_ROWS=1 (a second child) the counter stays and the bits
are the parent's (the golden file's "off" entries, recorded with that switch set)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, pkg

import test_gpu_up2_wino as up2
import test_gpu_wino_fused_rows as rows

synth = pkg("synth")
engine = pkg("engine")

GOLDEN_FILE = os.path.join(GOLDEN, "wino_stage_rows_parent.json")
FORCE = {"SR3_WINO_FUSED_ROWS_FORCE": "1", "SR3_UP2_WINO_FORCE": "1"}
SWITCHES = tuple(FORCE) + ("SR3_NO_WINO_FUSED_ROWS", "SR3_NO_UP2_WINO")

# (form, tile rows per block the case reaches (0: the direct kernel), shape)
AS_SPECIFIED = [("fused", 0, (2, 4, 32, 32, 64)), ("fused", 0, (2, 8, 32, 96, 128)),
                ("fused", 0, (2, 8, 16, 32, 64)), ("fused", 0, (2, 16, 16, 160, 64))]
SHAPES = AS_SPECIFIED + [
    ("fused", 2, (32, 4, 32, 128, 64)), ("fused", 2, (16, 8, 32, 160, 128)),
    ("fused", 4, (32, 8, 16, 128, 64)), ("fused", 4, (16, 16, 16, 160, 64)),
    ("up2", 2, (3, 8, 32, 96, 96)), ("up2", 2, (2, 4, 32, 32, 32)),
    ("up2", 4, (2, 16, 16, 96, 64)), ("up2", 4, (2, 8, 16, 32, 32)),
]
GN_SHAPES = [(16, 8, 32, 160, 128), (16, 16, 16, 160, 64)]
# (form, R, shape, everything the epilogue has, behind GroupNorm + Swish)
# under the default gate: exactly WINO_FUSED_ROWS_MIN_BLOCKS_16 = 1024 blocks at WINO_FUSED_ROWS_MAX_CIN_16 = 512 input channels
# (the smallest shape the gate takes), plain and behind GroupNorm + Swish; half the blocks, and a Cin above the range
DEFAULT_SHAPE, FEWER_BLOCKS, DEEPER_K = (64, 16, 16, 512, 512), (32, 16, 16, 512, 512), (64, 16, 16, 768, 512)
DEFAULT_CASES = [("fused", 4, DEFAULT_SHAPE, True, False), ("fused", 4, DEFAULT_SHAPE, True, True)]
CASES = [(f, R, s, full, False) for f, R, s in SHAPES for full in (False, True)] + [("fused", {32: 2, 16: 4}[s[2]], s, True, True) for s in GN_SHAPES]


def _id(case):
    form, R, shape, full, gn = case
    return f"{form}{R}-" + "x".join(map(str, shape)) + ("-all" if full else "-none") + ("-gn" if gn else "")


def takes(case):
    """tile rows per block of the form under test for this call when forced (the gates of the two files this one imports)"""
    form, R, shape, full, gn = case
    if form == "fused":
        return rows.gate(shape, full, True)
    return {16: 4, 32: 2}.get(shape[2], 1) if up2.gate(shape, full, True) else 0


def _images(B):
    """distinct images 0 .. nd - 1 repeated; the last image of the batch is image 0 again"""
    nd = max(1, min(B - 1, 3))
    idx = np.arange(B) % nd
    idx[-1] = 0
    return idx


def case_data(shape):
    B, H, W, Cin, Cout = shape
    rs = np.random.RandomState(9300 + 2 * B + 3 * H + 5 * W + 7 * Cin + 11 * Cout)
    idx = rows._images(B) if B == 64 else _images(B)      # (B = 64: three distinct images, placed as that file places them)
    nd = int(idx.max()) + 1
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    x = f32(nd, H, W, Cin)
    w = f32(Cout, Cin, 3, 3) / np.float32(np.sqrt(Cin * 9))
    b, cb = f32(Cout), f32(nd, Cout)
    resid = f32(nd, H, W, Cout)
    sc = (1 + np.float32(0.1) * f32(nd, Cin)).astype(np.float32)
    sh = (np.float32(0.1) * f32(nd, Cin)).astype(np.float32)
    return idx, x, w, b, cb, resid, sc, sh


def run_case(eng, case):
    """-> (out, statistics or None, launches of wino_fused_kernel<R > 1>, launches of wino_up2_kernel)"""
    form, R, shape, full, gn = case
    idx, x, w, b, cb, resid, sc, sh = case_data(shape)
    n0, u0 = eng.wino_fused_rows_launches(), eng.up2_wino_launches()
    eng.set_precision("f32")
    kw = {"up2": True} if form == "up2" else {}
    if gn:
        kw.update(gn_scale=sc[idx], gn_shift=sh[idx], swish=True)
    if full:
        if form == "fused":
            kw["resid"] = resid[idx]
        out, st = eng.op_conv2d(x[idx], w, b, chan_bias=cb[idx], return_stats=True, **kw)
    else:
        out, st = eng.op_conv2d(x[idx], w, **kw), None
    return out, st, eng.wino_fused_rows_launches() - n0, eng.up2_wino_launches() - u0


_want = {}


def want_f64(case):
    """float64 conv3x3 (behind nearest x2 for the Upsample convs) of the distinct images, computed once per shape and prologue"""
    form, R, shape, full, gn = case
    idx, x, w, b, cb, resid, sc, sh = case_data(shape)
    key = (form, shape, gn)
    if key not in _want:
        a = x.astype(np.float64)
        if gn:
            a = a * sc.astype(np.float64)[:, None, None, :] + sh.astype(np.float64)[:, None, None, :]
            a = a / (1.0 + np.exp(-a))
        if form == "up2":
            a = a.repeat(2, 1).repeat(2, 2)
        nd, H, W, C = a.shape
        ap = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))
        out = np.zeros((nd * H * W, w.shape[0]))
        for dy in range(3):
            for dx in range(3):
                out += np.ascontiguousarray(ap[:, dy:dy + H, dx:dx + W, :]).reshape(-1, C) @ w[:, :, dy, dx].T.astype(np.float64)
        _want[key] = out.reshape(nd, H, W, -1)
    out = _want[key][idx]
    if full:
        out = out + b.astype(np.float64) + cb.astype(np.float64)[idx][:, None, None, :]
        if form == "fused":
            out = out + resid.astype(np.float64)[idx]
    return out


def digests(out, st):
    d = {"out": hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()}
    if st is not None:
        d["stats"] = hashlib.sha256(np.ascontiguousarray(st).tobytes()).hexdigest()
    return d


def child_main(path):
    e = engine.Engine(synth.tiny_unet_config(), 0)
    rec = {}
    for c in CASES:
        k = _id(c)
        out, st, n, u = run_case(e, c)
        out2, st2, _, _ = run_case(e, c)
        rec["o:" + k], rec["n:" + k], rec["u:" + k] = out, np.int64(n), np.int64(u)
        rec["again:" + k] = np.bool_(digests(out, st) == digests(out2, st2))
        if st is not None:
            rec["s:" + k] = st
    e.close()
    np.savez(path, **rec)


def child_off_main(path):
    e = engine.Engine(synth.tiny_unet_config(), 0)
    rec = {}
    for c in DEFAULT_CASES:
        g0 = e.gn_wino_passes()
        out, st, n, _ = run_case(e, c)
        rec[_id(c)] = dict(digests(out, st), fused_rows_launches=n, gn_wino_passes=e.gn_wino_passes() - g0)
    e.close()
    with open(path, "w") as f:
        json.dump(rec, f)


def _run(mode, path, env_add):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])


def run_child(path):
    _run("child", path, FORCE)
    z = np.load(path)
    return {k: z[k] for k in z.files}


def run_child_off(path):
    _run("child_off", path, {"SR3_NO_WINO_FUSED_ROWS": "1"})
    with open(path) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    return run_child(str(tmp_path_factory.mktemp("wino_stage_rows") / "forced.npz"))


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_what_each_case_reaches():
    """host only: the forced gates take every case with the R it is listed under; the shapes as specified have no
    three-pass plan, so no switch brings them to wino_fused_kernel<R>"""
    for c in CASES + DEFAULT_CASES:
        assert takes(c) == c[1], (_id(c), takes(c))
    for form, R, s in AS_SPECIFIED:
        for stats in (False, True):
            assert engine.conv_plan(*s, precision="f32", stats=stats)["kernel"] != "wino_three_pass", s
    for form, R, (B, H, W, Cin, Cout) in SHAPES[len(AS_SPECIFIED):]:
        groups = H // (2 * R)                    # groups of R tile rows per image
        assert groups in (1, 2) and W == {2: 32, 4: 16}[R]
    reach = lambda form, R: [s for f, r, s in SHAPES if (f, r) == (form, R)]
    for form in ("fused", "up2"):
        for R in (2, 4):
            g = sorted(s[1] // (2 * R) for s in reach(form, R))
            assert g == [1, 2], (form, R, g)     # a single group, and two: shared rows inside and between blocks
            nks = sorted(s[3] // 32 for s in reach(form, R))
            assert nks[0] == (1 if form == "up2" else 4) and nks[1] % 2 == 1, (form, R, nks)
    assert any(s[4] // 64 == 2 for s in reach("fused", 2))      # two channel blocks
    B, H, W, Cin, Cout = DEFAULT_SHAPE
    assert B * (H * W // 128) * (Cout // 64) == 1024
    with open(GOLDEN_FILE) as f:
        g = json.load(f)
    assert set(g["cases"]) == {_id(c) for c in CASES} and set(g["off"]) == {_id(c) for c in DEFAULT_CASES}


def _check_float64_and_statistics(case, out, st):
    form, R, shape, full, gn = case
    B, H, W, Cin, Cout = shape
    k = _id(case)
    s = 2 if form == "up2" else 1
    assert out.shape == (B, s * H, s * W, Cout) and np.isfinite(out).all() and (st is None or full)
    assert R == 0 or (st is not None) == full, k
    want = want_f64(case)
    bar = 3e-5 if gn else 2e-5
    err = np.abs(out - want).max()
    msg = f"{k}: max abs err {err:.2e} (bar {bar:.0e})"
    if st is not None:
        sl = engine.conv_plan(B, H, W, Cin, Cout, 3, 1, int(form == "up2"), precision="f32", stats=True)["stats_slices"]
        assert st.shape == (B, sl, Cout, 2) and np.isfinite(st).all(), (k, st.shape, sl)
        o64 = out.astype(np.float64)
        if form == "up2":   # slice ph * (sl / 4) + j: a run of low-resolution pixels of phase image ph = (py, px), row-major
            g = o64.reshape(B, H, 2, W, 2, Cout).transpose(0, 2, 4, 1, 3, 5).reshape(B, sl, -1, Cout)
        elif R:             # slice j: a run of consecutive 2x2 tiles (row-major), four pixels each
            g = o64.reshape(B, H // 2, 2, W // 2, 2, Cout).transpose(0, 1, 3, 2, 4, 5).reshape(B, sl, -1, Cout)
        else:               # the direct kernel: a run of consecutive pixels
            g = o64.reshape(B, sl, -1, Cout)
        s1, s2 = g.sum(2), (g * g).sum(2)
        r1 = np.abs(st[..., 0] - s1).max() / np.abs(s1).max()
        r2 = np.abs(st[..., 1] - s2).max() / np.abs(s2).max()
        msg += f"; statistics, {sl} slices: sum {r1:.1e}, sum of squares {r2:.1e} relative (bar 1e-9)"
    print(msg)
    assert err <= bar, msg
    if st is not None:
        assert r1 <= 1e-9 and r2 <= 1e-9, msg


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bits_of_the_parent_and_float64(forced, gold, case):
    form, R, shape, full, gn = case
    B = shape[0]
    k = _id(case)
    out, st = forced["o:" + k], forced.get("s:" + k)
    want_launches = (0, 0) if R == 0 else ((1, 0) if form == "fused" else (0, 1))
    assert (int(forced["n:" + k]), int(forced["u:" + k])) == want_launches, k
    _check_float64_and_statistics(case, out, st)
    assert out[B - 1].tobytes() == out[0].tobytes(), f"{k}: image {B - 1} is a copy of image 0"
    if st is not None:
        assert st[B - 1].tobytes() == st[0].tobytes(), f"{k}: statistics of image {B - 1}"
    assert bool(forced["again:" + k]), f"{k}: a second call gave other bits"
    assert digests(out, st) == gold["cases"][k], f"{k}: differs from the parent commit's library"


@pytest.mark.gpu
def test_default_gate_takes_the_16x16_level():
    e = engine.Engine(synth.tiny_unet_config(), 0)
    try:
        for case in DEFAULT_CASES:
            g0 = e.gn_wino_passes()
            out, st, n, _ = run_case(e, case)
            assert n == 1, f"{_id(case)}: wino_fused_rows_launches rose by {n}"
            assert e.gn_wino_passes() == g0, f"{_id(case)}: a GroupNorm pass wrote U"
            _check_float64_and_statistics(case, out, st)
        for shape in (FEWER_BLOCKS, DEEPER_K):
            _, _, n, _ = run_case(e, ("fused", 0, shape, False, False))
            assert n == 0, (shape, n)
    finally:
        e.close()


@pytest.mark.gpu
def test_switched_off_the_default_case_gives_the_parents_bits(tmp_path_factory, gold):
    got = run_child_off(str(tmp_path_factory.mktemp("wino_stage_rows") / "off.json"))
    for case in DEFAULT_CASES:
        k = _id(case)
        # (the pass in front of a three-pass conv writes U, with or without GroupNorm: one per call)
        assert got[k]["fused_rows_launches"] == 0 and got[k]["gn_wino_passes"] == 1, (k, got[k])
        assert {x: got[k][x] for x in ("out", "stats")} == gold["off"][k], f"{k}: SR3_NO_WINO_FUSED_ROWS=1 differs from the parent's library"


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child_main(sys.argv[2])
    elif sys.argv[1] == "child_off":
        child_off_main(sys.argv[2])
    else:
        # records the golden file from the library SR3_LIB names (a build of the commit before the change)
        assert sys.argv[1] == "record" and os.environ.get("SR3_LIB"), "record from another build of the library: set SR3_LIB"
        got = run_child(sys.argv[2] + ".tmp.npz")
        os.remove(sys.argv[2] + ".tmp.npz")
        rec = {}
        for c in CASES:
            k = _id(c)
            want_launches = 0 if c[1] == 0 else 1
            assert int(got["n:" + k]) + int(got["u:" + k]) == want_launches and bool(got["again:" + k]), k
            rec[k] = digests(got["o:" + k], got.get("s:" + k))
            print(k, rec[k], flush=True)
        off = run_child_off(sys.argv[2] + ".tmp.json")
        os.remove(sys.argv[2] + ".tmp.json")
        off = {k: {x: v[x] for x in ("out", "stats")} for k, v in off.items()}
        with open(sys.argv[2], "w") as f:
            json.dump({"recorded_with": "libsr3hip.so of the parent commit, RandomState inputs of case_data; off: under SR3_NO_WINO_FUSED_ROWS=1",
                       "cases": rec, "off": off}, f, indent=1)
            f.write("\n")
