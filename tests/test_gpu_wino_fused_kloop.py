"""The K loop of the one-pass exact-f32 Winograd conv (wino_fused_kernel) at every loop length and block layout that can
go wrong when its loads move: the schedule of the loop may change, the bits it computes may not.

Cases (B, H, W, Cin, Cout), each asserted on the host to take the wino_one_pass plan:
  (32, 64, 64,  64,  64)   exactly 1024 blocks, nk = 2: the first iteration is also the one before the last
  (16, 64, 64,  96, 128)   nk = 3: odd stage parity at the end, two channel blocks
  ( 8, 64, 128, 160, 128)  nk = 5, two strips per tile row
  ( 4, 70, 64,  64, 512)   35 tile rows, eight channel blocks sharing a strip
  (32, 64, 64, 384,  64)   nk = 12, the deep loop
All run with bias + residual + FeatureWiseAffine bias + fused statistics (sr3_op_conv2d_stats); the first and the third
also with none of them (the same body behind sr3_op_conv2d: without a statistics buffer there is nothing to pass the
other entry point; the plan is asserted for that call too).

Two checks per case:
  1. out against a float64 conv (+ the epilogue terms) at 2e-5, the bar of test_gpu_conv_stats.py for this class; the
     statistics per (image, channel) against the fp64 sums of the call's own stored output to 1e-9 of sum|v| / sum v^2.
     The measured maxima are printed.
  2. sha256 of the output bytes and of the statistics bytes against tests/golden/wino_fused_kloop_parent.json, recorded
     from a build of the commit BEFORE the K loop was rescheduled (the kernel has no atomics and a fixed summation
     order, so the bits do not depend on the machine). To record it again, build the older commit elsewhere and run
         SR3_LIB=/path/to/older/libsr3hip.so python tests/test_gpu_wino_fused_kloop.py OUT.json
     never from the tree under test.

Large batches repeat three distinct images (first, middle and last differ), so the float64 conv runs on three.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, pkg

synth = pkg("synth")
engine = pkg("engine")

GOLDEN_FILE = os.path.join(GOLDEN, "wino_fused_kloop_parent.json")

# (shape, with bias + residual + FeatureWiseAffine bias + statistics)
CASES = [
    ((32, 64, 64, 64, 64), True),
    ((32, 64, 64, 64, 64), False),
    ((16, 64, 64, 96, 128), True),
    ((8, 64, 128, 160, 128), True),
    ((8, 64, 128, 160, 128), False),
    ((4, 70, 64, 64, 512), True),
    ((32, 64, 64, 384, 64), True),
]


def _id(case):
    shape, full = case
    return "x".join(map(str, shape)) + ("-all" if full else "-none")


def _images(B):
    if B <= 3:
        return np.arange(B)
    idx = np.arange(B) % 3
    idx[0], idx[B // 2], idx[-1] = 0, 1, 2
    return idx


def conv64(x, w):
    """float64 nn.Conv2d(3, padding=1) on NHWC x, w OIHW."""
    x, w = x.astype(np.float64), w.astype(np.float64)
    B, H, W, C = x.shape
    O = w.shape[0]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B * H * W, O))
    for dy in range(3):
        for dx in range(3):
            out += np.ascontiguousarray(xp[:, dy:dy + H, dx:dx + W, :]).reshape(-1, C) @ w[:, :, dy, dx].T
    return out.reshape(B, H, W, O)


def _gate(B, H, W, Cin, Cout):
    return (H * W >= 4096 and W % 64 == 0 and Cin >= 64 and Cin % 32 == 0 and Cout % 64 == 0
            and B * (H // 2) * (W // 64) * (Cout // 64) >= 1024)


def run_case(eng, case):
    """-> (out, stats or None, distinct inputs for the reference)"""
    (B, H, W, Cin, Cout), full = case
    rs = np.random.RandomState(1900 + B + H + W + Cin + Cout)
    idx = _images(B)
    nd = int(idx.max()) + 1
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    xd = f32(nd, H, W, Cin)
    w = f32(Cout, Cin, 3, 3) / np.float32(np.sqrt(Cin * 9))
    b, cbd, rd = f32(Cout), f32(nd, Cout), f32(nd, H, W, Cout)
    eng.set_precision("f32")
    if full:
        out, st = eng.op_conv2d(xd[idx], w, b, chan_bias=cbd[idx], resid=rd[idx], return_stats=True)
    else:
        out, st = eng.op_conv2d(xd[idx], w), None
    return out, st, (idx, nd, xd, w, b, cbd, rd)


def digests(out, st):
    d = {"out": hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()}
    if st is not None:
        d["stats"] = hashlib.sha256(np.ascontiguousarray(st).tobytes()).hexdigest()
    return d


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(synth.tiny_unet_config(), 0)
    e.load_state_dict(synth.synth_state_dict(e.cfg, 11))
    yield e
    e.close()


def test_every_case_takes_the_one_pass_plan():
    for (B, H, W, Cin, Cout), full in CASES:
        assert _gate(B, H, W, Cin, Cout)
        d = engine.conv_plan(B, H, W, Cin, Cout, precision="f32", stats=full)
        assert d["kernel"] == "wino_one_pass" and (d["stats_slices"] > 0 or not full), (_id(((B, H, W, Cin, Cout), full)), d)
    B, H, W, Cin, Cout = CASES[0][0]
    assert B * (H // 2) * (W // 64) * (Cout // 64) == 1024
    with open(GOLDEN_FILE) as f:
        assert set(json.load(f)["cases"]) == {_id(c) for c in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_wino_fused_kloop(eng, case):
    (B, H, W, Cin, Cout), full = case
    plan = engine.conv_plan(B, H, W, Cin, Cout, precision="f32", stats=full)
    assert plan["kernel"] == "wino_one_pass" and _gate(B, H, W, Cin, Cout), plan
    out, st, (idx, nd, xd, w, b, cbd, rd) = run_case(eng, case)

    # 1. float64 conv, and the statistics against the stored output
    want = conv64(xd, w)
    if full:
        want = want + b.astype(np.float64) + cbd[:, None, None, :].astype(np.float64) + rd
    err = max(np.abs(out[idx == k] - want[k]).max() for k in range(nd))
    print(f"{_id(case)}: conv err {err:.2e} (bar 2e-5)", end="")
    assert out.shape == (B, H, W, Cout)
    assert err < 2e-5
    if full:
        assert st is not None and st.shape == (B, plan["stats_slices"], Cout, 2) and not np.isnan(st).any()
        v = out.reshape(B, H * W, Cout).astype(np.float64)
        a1, a2 = np.abs(v).sum(1), (v * v).sum(1)
        d1, d2 = np.abs(st[..., 0].sum(1) - v.sum(1)), np.abs(st[..., 1].sum(1) - a2)
        print(f"  totals: S1 {np.max(d1 / a1):.1e} S2 {np.max(d2 / a2):.1e} (rel, bar 1e-9)", end="")
        assert np.all(d1 <= 1e-9 * a1) and np.all(d2 <= 1e-9 * a2)
    print()

    # 2. the bits of the build before the loop was rescheduled
    with open(GOLDEN_FILE) as f:
        gold = json.load(f)["cases"][_id(case)]
    assert digests(out, st) == gold


if __name__ == "__main__":
    # records the golden file from the library SR3_LIB names (a build of the commit before the change)
    assert os.environ.get("SR3_LIB"), "record from another build of the library: set SR3_LIB"
    e = engine.Engine(synth.tiny_unet_config(), 0)
    e.load_state_dict(synth.synth_state_dict(e.cfg, 11))
    rec = {}
    for c in CASES:
        out, st, _ = run_case(e, c)
        rec[_id(c)] = digests(out, st)
        print(_id(c), rec[_id(c)], flush=True)
    e.close()
    with open(sys.argv[1], "w") as f:
        json.dump({"recorded_with": "libsr3hip.so of the parent commit, RandomState inputs of run_case", "cases": rec}, f, indent=1)
        f.write("\n")
