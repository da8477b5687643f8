"""The LDS-DMA lane offsets of the one-pass Winograd kernels, held across the K loop instead of recomputed per K-step, on the
instantiations that no digest covered yet: wino_fused_kernel<2> and <4> (the 32x32 and 16x16 levels) and wino_up2_kernel<1 | 2 | 4>
(wino_fused_kernel<1>: tests/test_gpu_wino_fused_kloop.py). A wrong offset, a wrong switch for "no next stage" or for the
instructions past a stage's last changes what a stage holds, so the check is the bits: sha256 of output and statistics
against tests/golden/wino_dma_offsets_parent.json, recorded from a build of the commit BEFORE the offsets were hoisted
(no atomics, fixed summation orders: the bits do not depend on the machine). To record it again, build the older commit
elsewhere and run
    SR3_LIB=/path/to/older/libsr3hip.so python tests/test_gpu_wino_dma_offsets.py OUT.json
never from the tree under test.

Both forms are unexported fields of the conv plan whose switches are read once per process, so one child process of this file
runs every case under SR3_WINO_FUSED_ROWS_FORCE=1 and SR3_UP2_WINO_FORCE=1 (the tuning constants lifted, nothing else);
Engine.wino_fused_rows_launches() and Engine.up2_wino_launches() tell that the form under test ran, and the width fixes R.

Cases (B, H, W, Cin, Cout), the smallest shapes of tests/test_gpu_wino_fused_rows.py and tests/test_gpu_up2_wino.py that reach
each instantiation, two loop lengths nk = Cin / 32 each:
  wino_fused_kernel<2>   (4, 32, 32, 128, 64)   nk = 4     (4, 32, 32, 160, 192)  nk = 5, three channel blocks
  wino_fused_kernel<4>   (16, 16, 16, 128, 64)  nk = 4     (16, 16, 16, 160, 64)  nk = 5
      (R > 1 is a form of the three-pass plan, which starts at Cin = 128: nk = 4 is its shortest loop and nk = 2 cannot be
      reached; the odd length ends on the other stage)
  wino_up2_kernel<1>     (1, 4, 128, 64, 32)    nk = 2: the first step is also the one before the last; the block runs two
                                                strips one after the other, so the held offsets serve two descriptors
                         (1, 2, 128, 96, 64)    nk = 3
  wino_up2_kernel<2>     (3, 4, 32, 64, 96)     nk = 2     (3, 4, 32, 96, 96)     nk = 3  (34 of the 36 DMA slots live)
  wino_up2_kernel<4>     (1, 24, 16, 64, 64)    nk = 2     (1, 24, 16, 96, 64)    nk = 3
Each runs plain (no bias) and with everything its epilogue has: bias + residual + FeatureWiseAffine bias + statistics
(wino_up2_kernel has no residual: its gate leaves such a conv to the phase form).
"""
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

GOLDEN_FILE = os.path.join(GOLDEN, "wino_dma_offsets_parent.json")
FORCE = {"SR3_WINO_FUSED_ROWS_FORCE": "1", "SR3_UP2_WINO_FORCE": "1"}
SWITCHES = tuple(FORCE) + ("SR3_NO_WINO_FUSED_ROWS", "SR3_NO_UP2_WINO")

# (form, R, shape)
SHAPES = [
    ("fused", 2, (4, 32, 32, 128, 64)), ("fused", 2, (4, 32, 32, 160, 192)),
    ("fused", 4, (16, 16, 16, 128, 64)), ("fused", 4, (16, 16, 16, 160, 64)),
    ("up2", 1, (1, 4, 128, 64, 32)), ("up2", 1, (1, 2, 128, 96, 64)),
    ("up2", 2, (3, 4, 32, 64, 96)), ("up2", 2, (3, 4, 32, 96, 96)),
    ("up2", 4, (1, 24, 16, 64, 64)), ("up2", 4, (1, 24, 16, 96, 64)),
]
CASES = [(form, R, shape, full) for form, R, shape in SHAPES for full in (False, True)]


def _id(case):
    form, R, shape, full = case
    return f"{form}{R}-" + "x".join(map(str, shape)) + ("-all" if full else "-none")


def takes(case):
    """tile rows per block of the form under test for this call when forced (the gates of the two files this one imports)"""
    form, R, shape, full = case
    if form == "fused":
        return rows.gate(shape, full, True)
    return {16: 4, 32: 2}.get(shape[2], 1) if up2.gate(shape, full, True) else 0


def run_case(eng, case):
    """-> (out, statistics or None, launches of wino_fused_kernel<R > 1>, launches of wino_up2_kernel)"""
    form, R, (B, H, W, Cin, Cout), full = case
    rs = np.random.RandomState(7100 + 2 * B + 3 * H + 5 * W + 7 * Cin + 11 * Cout)
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    x = f32(B, H, W, Cin)
    w = f32(Cout, Cin, 3, 3) / np.float32(np.sqrt(Cin * 9))
    b, cb, resid = f32(Cout), f32(B, Cout), f32(B, H, W, Cout)
    n0, u0 = eng.wino_fused_rows_launches(), eng.up2_wino_launches()
    eng.set_precision("f32")
    kw = {"up2": True} if form == "up2" else {}
    if full:
        if form == "fused":
            kw["resid"] = resid
        out, st = eng.op_conv2d(x, w, b, chan_bias=cb, return_stats=True, **kw)
    else:
        out, st = eng.op_conv2d(x, w, **kw), None
    return out, st, eng.wino_fused_rows_launches() - n0, eng.up2_wino_launches() - u0


def digests(out, st):
    d = {"out": hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()}
    if st is not None:
        d["stats"] = hashlib.sha256(np.ascontiguousarray(st).tobytes()).hexdigest()
    return d


def child_main(path):
    e = engine.Engine(synth.tiny_unet_config(), 0)
    rec = {}
    for c in CASES:
        out, st, n, u = run_case(e, c)
        rec[_id(c)] = dict(digests(out, st), fused_rows_launches=n, up2_launches=u, finite=bool(np.isfinite(out).all()),
                           shape=list(out.shape), has_stats=st is not None)
    e.close()
    with open(path, "w") as f:
        json.dump(rec, f)


def run_child(path):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(FORCE)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    with open(path) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    return run_child(str(tmp_path_factory.mktemp("wino_dma_offsets") / "forced.json"))


def test_every_case_reaches_its_instantiation():
    """host only: the forced gates take every case with the R it is listed under, both loop lengths per instantiation"""
    for c in CASES:
        assert takes(c) == c[1], (_id(c), takes(c))
    for form, R in {(f, r) for f, r, _ in SHAPES}:
        nks = sorted(s[3] // 32 for f, r, s in SHAPES if (f, r) == (form, R))
        assert len(nks) == 2 and nks[0] % 2 == 0 and nks[1] % 2 == 1, (form, R, nks)
        assert nks[0] == (2 if form == "up2" else 4)
    with open(GOLDEN_FILE) as f:
        assert set(json.load(f)["cases"]) == {_id(c) for c in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_bits_of_the_parent(forced, case):
    form, R, (B, H, W, Cin, Cout), full = case
    got = forced[_id(case)]
    assert (got["fused_rows_launches"], got["up2_launches"]) == ((1, 0) if form == "fused" else (0, 1)), got
    s = 2 if form == "up2" else 1
    assert got["shape"] == [B, s * H, s * W, Cout] and got["finite"] and got["has_stats"] == full, got
    with open(GOLDEN_FILE) as f:
        gold = json.load(f)["cases"][_id(case)]
    assert {k: got[k] for k in gold} == gold, f"{_id(case)}: differs from the library before the offsets were hoisted"


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child_main(sys.argv[2])
    else:
        # records the golden file from the library SR3_LIB names (a build of the commit before the change)
        assert os.environ.get("SR3_LIB"), "record from another build of the library: set SR3_LIB"
        got = run_child(sys.argv[1] + ".tmp")
        os.remove(sys.argv[1] + ".tmp")
        rec = {}
        for c in CASES:
            g = got[_id(c)]
            assert g["fused_rows_launches"] + g["up2_launches"] == 1 and g["finite"], (_id(c), g)
            rec[_id(c)] = {k: g[k] for k in ("out", "stats") if k in g}
            print(_id(c), rec[_id(c)], flush=True)
        with open(sys.argv[1], "w") as f:
            json.dump({"recorded_with": "libsr3hip.so of the parent commit, RandomState inputs of run_case", "cases": rec}, f, indent=1)
            f.write("\n")
