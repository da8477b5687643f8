"""block1's GroupNorm + Swish pass and the block's 1x1 res_conv in one kernel (csrc/kernels_gn_res.hip, sr3_op_gn_res1x1)
against the two launches it replaces, in the same process, bit for bit:
  act   sr3_op_groupnorm_apply, mode 2, format 0, on both routes (the statistics come from the streaming statistics kernel
        either way; the folded route finalizes them inside the apply launch)
  res   the 1x1 conv. In the engine it is the side launch of conv2's Winograd plan: launch_conv on a ConvParams without a
        partial-sum buffer, which therefore never splits K. sr3_op_conv2d offers that buffer, and for two of the shapes below
        (few tiles, five and six K-steps) its plan is an in-place split-K of two slices, whose sums are added in another
        order than one ascending chain. So `res` must equal sr3_op_conv2d wherever that op's plan is unsplit, and the
        side launch itself (op_gn_res1x1(want_pair=True): the ConvParams launch_conv_wino builds) at EVERY shape.
and against a float64 restatement at the suite's bars: 3e-5 behind GroupNorm + Swish (tests/test_gpu_gn_wino_input.py),
2e-5 for the conv on N(0,1) data with N(0,1) / sqrt(Cin) weights (tests/test_gpu_conv_gates.py).

Cases (B, H, W, C0, C1, Cout); the kernel's tile is 128 pixels x 64 | 128 output channels, 32 channels per K-step (nk):
  (1, 8, 16, 64, 0, 64)     one tile that is a whole image; no skip; nk = 2
  (2, 16, 8, 32, 32, 64)    the x / skip seam between the two K-steps; a tile spanning sixteen image rows
  (3, 16, 16, 64, 32, 128)  nk = 3: the ring ends on the other stage; two Cout tiles and nk not divisible by them; 3 images
  (2, 16, 16, 96, 64, 256)  nk = 5; seam not at a power of two; four Cout tiles
  (2, 32, 32, 128, 64, 64)  several tiles per image; nk = 6
  (4, 64, 64, 32, 32, 512)  512 blocks of 128 output channels: the wide tile (taken from 512 blocks on), four Cout tiles
  (1, 8, 16, 48, 16, 64)    C0 = 48: refused by the gate, nothing launched
Image B-1 is a copy of image 0 (B > 1).

The engine: two child processes run the same forwards, SR3_GN_RES1X1_FORCE=1 against SR3_NO_GN_RES1X1=1 (switches are read
once per process). The gate needs a Winograd plan for conv2 and a conv1 that reads the plain activated tensor; the tiny
config and sweep config D at B = 2 have no Winograd conv at all (under 1024 tiles), so there the counter stays 0 and the
forwards are trivially the same launches. D at B = 4 with SR3_WINO_FUSED_ROWS_FORCE=1 in both children (its 32x32 level
then runs conv1 on the tile-row form, which reads the activated tensor) is the smallest forward that reaches the kernel:
three blocks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import pkg

synth = pkg("synth")
engine = pkg("engine")

CASES = [(1, 8, 16, 64, 0, 64), (2, 16, 8, 32, 32, 64), (3, 16, 16, 64, 32, 128), (2, 16, 16, 96, 64, 256),
         (2, 32, 32, 128, 64, 64), (4, 64, 64, 32, 32, 512)]
REFUSED = (1, 8, 16, 48, 16, 64)
BN = {CASES[0]: 64, CASES[1]: 64, CASES[2]: 64, CASES[3]: 64, CASES[4]: 64, CASES[5]: 128}    # gn_res1x1_bn
SENTINEL = -12345.0
BAR_ACT, BAR_RES = 3e-5, 2e-5
SWITCHES = ("SR3_NO_GN_RES1X1", "SR3_GN_RES1X1_FORCE", "SR3_WINO_FUSED_ROWS_FORCE", "SR3_NO_WINO_FUSED_ROWS")
# name -> (config, B, H = W, environment of both children, blocks that take the kernel when forced)
FWD = {"tiny": ("tiny", 2, 16, {}, 0), "D": ("D", 2, 32, {}, 0), "D4rows": ("D", 4, 32, {"SR3_WINO_FUSED_ROWS_FORCE": "1"}, 3)}


def _id(case):
    return "x".join(map(str, case))


def case_data(case):
    B, H, W, C0, C1, Cout = case
    rs = np.random.RandomState(9000 + B + 3 * H + 5 * W + 7 * C0 + 11 * C1 + 13 * Cout)
    C = C0 + C1
    x = rs.standard_normal((B, H, W, C)).astype(np.float32)
    x[B - 1] = x[0]
    gamma = (1 + 0.1 * rs.standard_normal(C)).astype(np.float32)
    beta = (0.1 * rs.standard_normal(C)).astype(np.float32)
    w2 = (rs.standard_normal((Cout, C)) / np.sqrt(C)).astype(np.float32)
    x0 = np.ascontiguousarray(x[..., :C0])
    x1 = np.ascontiguousarray(x[..., C0:]) if C1 else None
    return x, x0, x1, gamma, beta, w2


def reference_f64(case, groups=32):
    x, _, _, gamma, beta, w2 = case_data(case)
    B, H, W, C = x.shape
    a = x.astype(np.float64).reshape(B, H * W, groups, C // groups)
    mean = a.mean(axis=(1, 3), keepdims=True)
    var = a.var(axis=(1, 3), keepdims=True)
    a = ((a - mean) / np.sqrt(var + 1e-5)).reshape(B, H, W, C) * gamma.astype(np.float64) + beta.astype(np.float64)
    act = a / (1.0 + np.exp(-a))
    res = (x.astype(np.float64).reshape(-1, C) @ w2.astype(np.float64).T).reshape(B, H, W, -1)
    return act, res


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(synth.tiny_unet_config(), 0)
    e.set_precision("f32")
    yield e
    e.close()


def test_the_cases_reach_what_they_name():
    """host only: tiles, K-steps and the gate's answer for every case"""
    for case in CASES:
        B, H, W, C0, C1, Cout = case
        g = engine.gn_res1x1_gate(B, H, W, C0, C1, Cout)
        assert (H * W) % 128 == 0 and C0 % 32 == 0 and C1 % 32 == 0 and Cout % 64 == 0, case
        blocks128 = (B * H * W // 128) * (Cout // 128) if Cout % 128 == 0 else 0
        assert BN[case] == (128 if blocks128 >= 512 else 64), case
    nk = [(c[3] + c[4]) // 32 for c in CASES]
    tiles_n = [c[5] // BN[c] for c in CASES]
    assert nk == [2, 2, 3, 5, 6, 2] and tiles_n == [1, 1, 2, 4, 1, 4]
    assert [c[1] * c[2] // 128 for c in CASES] == [1, 1, 2, 2, 8, 32]           # tiles per image
    assert not engine.gn_res1x1_gate(*REFUSED)["valid"]
    # sr3_op_conv2d's own plan of the 1x1 splits K at exactly the two deep-K shapes with few tiles
    split = [engine.conv_plan(c[0], c[1], c[2], c[3] + c[4], c[5], ks=1)["splits"] > 1 for c in CASES]
    assert split == [False, False, False, True, True, False], split


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_one_pass_equals_the_two_launches(eng, case):
    B, H, W, C0, C1, Cout = case
    x, x0, x1, gamma, beta, w2 = case_data(case)
    n0 = eng.gn_res1x1_launches()
    got = eng.op_gn_res1x1(x0, gamma, beta, w2, skip=x1, sentinel=SENTINEL, want_pair=True)
    assert eng.gn_res1x1_launches() == n0 + 1
    act, res = got["act"], got["res"]
    interior = act[:, 1:-1, 1:-1, :]
    # the border of act still holds the sentinel: the kernel writes interior pixels only
    border = np.ones(act.shape[:3], bool)
    border[:, 1:-1, 1:-1] = False
    assert np.all(act[border] == np.float32(SENTINEL))
    assert not np.any(interior == np.float32(SENTINEL)) and not np.any(res == np.float32(SENTINEL))

    # the two launches it replaces, bit for bit
    for route in (2, 1):
        two = eng.op_groupnorm_apply(x0, gamma, beta, x1=x1, mode=2, fmt=0, route=route)
        assert two["route"] == route
        assert np.array_equal(interior.view(np.uint32), two["out"].view(np.uint32)), f"act differs from the apply pass on route {route}"
    assert np.array_equal(res.view(np.uint32), got["res_pair"].view(np.uint32)), "res differs from the 1x1 side launch"
    conv = eng.op_conv2d(x0, w2.reshape(Cout, C0 + C1, 1, 1), None, x1=x1)
    if engine.conv_plan(B, H, W, C0 + C1, Cout, ks=1)["splits"] == 1:
        assert np.array_equal(res.view(np.uint32), conv.view(np.uint32)), "res differs from sr3_op_conv2d"

    # float64
    act64, res64 = reference_f64(case)
    e_act, e_res, e_conv = np.abs(interior - act64).max(), np.abs(res - res64).max(), np.abs(conv - res64).max()
    print(f"{_id(case)}: max abs error act {e_act:.3g} res {e_res:.3g} (sr3_op_conv2d {e_conv:.3g})")
    assert e_act <= BAR_ACT and e_res <= BAR_RES and e_conv <= BAR_RES

    # a second call gives the same bits; image B-1 is image 0
    again = eng.op_gn_res1x1(x0, gamma, beta, w2, skip=x1, sentinel=SENTINEL)
    assert np.array_equal(again["act"].view(np.uint32), act.view(np.uint32))
    assert np.array_equal(again["res"].view(np.uint32), res.view(np.uint32))
    if B > 1:
        assert np.array_equal(act[B - 1].view(np.uint32), act[0].view(np.uint32))
        assert np.array_equal(res[B - 1].view(np.uint32), res[0].view(np.uint32))


@pytest.mark.gpu
def test_the_gate_refuses_48_channels(eng):
    x, x0, x1, gamma, beta, w2 = case_data(REFUSED)
    n0 = eng.gn_res1x1_launches()
    with pytest.raises(pkg("_lib").Sr3Error, match="refused by the gate"):
        eng.op_gn_res1x1(x0, gamma, beta, w2, skip=x1)
    assert eng.gn_res1x1_launches() == n0


@pytest.mark.gpu
def test_split_f16_mode_is_refused():
    e = engine.Engine(synth.tiny_unet_config(), 0)
    try:
        e.set_precision("f16x3")
        x, x0, x1, gamma, beta, w2 = case_data(CASES[0])
        with pytest.raises(pkg("_lib").Sr3Error, match="refused by the gate"):
            e.op_gn_res1x1(x0, gamma, beta, w2, skip=x1)
    finally:
        e.close()


# ---- the engine: forced against off, in child processes ----------------------------------------------------------------
def run_forward(name, precision="f32"):
    cfg_name, B, hw, _, _ = FWD[name]
    cfg = synth.tiny_unet_config() if cfg_name == "tiny" else synth.sweep_unet_config(cfg_name)
    x, nl = synth.synth_unet_input(cfg, B, hw, hw, 9)
    e = engine.Engine(cfg, 0)
    try:
        e.set_precision(precision)
        e.load_state_dict(synth.synth_state_dict(cfg, 41))
        n0 = e.gn_res1x1_launches()
        out = e.unet_forward_np(x, nl.reshape(-1))
        return out, e.gn_res1x1_launches() - n0, e.fallback_calls()
    finally:
        e.close()


def child_main(path, names):
    out = {}
    for name in names:
        o, n, fb = run_forward(name)
        out["fwd_" + name], out["n_" + name], out["fb_" + name] = o, np.int64(n), np.int64(fb)
        if name == "D4rows":
            o, n, fb = run_forward(name, "f16x3")
            out["n16_" + name] = np.int64(n)
    np.savez(path, **out)


def _children(tmp_path_factory, switch):
    """one child per distinct environment: the forwards that share it run in one process"""
    groups = {}
    for name, (_, _, _, env_add, _) in FWD.items():
        groups.setdefault(tuple(sorted(env_add.items())), []).append(name)
    got = {}
    for env_add, names in groups.items():
        path = str(tmp_path_factory.mktemp("gn_res1x1") / ("_".join(names) + ".npz"))
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(dict(env_add))
        env.update(switch)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", path] + names, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        z = np.load(path)
        got.update({k: z[k] for k in z.files})
    return got


@pytest.fixture(scope="module")
def off(tmp_path_factory):
    return _children(tmp_path_factory, {"SR3_NO_GN_RES1X1": "1"})


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    return _children(tmp_path_factory, {"SR3_GN_RES1X1_FORCE": "1"})


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FWD))
def test_forward_forced_equals_off(off, forced, name):
    want_n = FWD[name][4]
    assert int(off["n_" + name]) == 0
    assert int(forced["n_" + name]) == want_n, (name, int(forced["n_" + name]))
    assert int(off["fb_" + name]) == 0 and int(forced["fb_" + name]) == 0
    a, b = off["fwd_" + name], forced["fwd_" + name]
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: max abs difference {np.abs(a - b).max():.3g}"


@pytest.mark.gpu
def test_forward_reaches_the_kernel_only_in_f32(forced):
    assert int(forced["n_D4rows"]) > 0
    assert int(forced["n16_D4rows"]) == 0        # the split-f16 arithmetic launches what it launched before


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "child":
        child_main(sys.argv[2], sys.argv[3:])
    else:
        sys.exit("usage: test_gpu_gn_res1x1.py child OUT.npz NAME...")
