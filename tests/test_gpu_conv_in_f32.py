"""conv_in_f32_kernel (csrc/kernels_edge.hip): the first conv of the exact-f32 UNet on a kernel of its own, through the
forward's launcher and gate (sr3_op_conv_in_f32) and through whole forwards.

Single op, against float64 (numpy, computed here from the inputs). Two bars on max |gpu - float64|:
  * 2e-5 on O(1) data, the bar the project holds its exact-f32 convs to (tests/test_gpu_wino_fused_kloop.py and siblings);
  * at most twice the error of the GENERIC kernel on the same case (op_conv2d on the state and weights zero-padded to 32
    input channels: the launch the forward made before this kernel). Both add the same 9 * Cin fp32 products in fp32, in
    different orders, so neither is expected to be the more exact one.
Statistics: {sum, sum of squares} of the stored fp32 values per (image, 256-pixel block, channel) against fp64 sums of the
output read back, 1e-9 relative to sum |v| resp. sum v^2 of the slice (the kernel adds the same values in fp64 in another
order); slices_out == H*W/256; what lies behind the slices keeps the 0xFF fill.

Forward level: f32 forwards of the tiny config and of sweep config A (Cout 32: the NT = 2 instantiation, 48x80) at their
fixtures' sizes within tests/test_gpu_unet.py's TOL, the launch counter going up by one per forward; under
SR3_NO_CONV_IN_F32=1 (a child process) the counter stays 0 and the same TOL holds; a two-step DDPM sample run eagerly
(SR3_NO_GRAPH=1, a child process) and with captured steps returns the same bytes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import cfg_from_meta, load_golden, pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
Sr3Error = pkg("_lib").Sr3Error

BAR = 2e-5              # exact-f32 convs on O(1) data
STATS_REL = 1e-9
TOL = 1e-4              # tests/test_gpu_unet.py
GRID = 512              # CONV_IN_F32_GRID (csrc/sr3_internal.h): the launcher's persistent grid

# (B, H, W, Cin, Cout)
SHAPES = [
    (1, 16, 16, 6, 64),             # one block; an M-tile is one image row
    (3, 16, 16, 6, 64),             # blocks ending at image ends
    (2, 8, 32, 6, 32),              # NT = 2; an M-tile is half a row
    (2, 16, 48, 3, 64),             # waves straddle 48-pixel rows; three blocks per image; Cin 3
    (1, 32, 32, 8, 64),             # all eight channels live
    (GRID + 1, 16, 16, 6, 64),      # one block more than the persistent grid: the block loop wraps
]


def _sid(s):
    return "x".join(map(str, s))


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def conv_f64(state, w, bias):
    """3x3 / stride 1 / zero padding in float64: state [B, H, W, Cin], w OIHW -> [B, H, W, Cout]"""
    B, H, W, Cin = state.shape
    xp = np.zeros((B, H + 2, W + 2, Cin), np.float64)
    xp[:, 1:-1, 1:-1] = state
    w64 = w.astype(np.float64)
    out = np.zeros((B, H, W, w.shape[0]), np.float64)
    for dy in range(3):
        for dx in range(3):
            out += xp[:, dy:dy + H, dx:dx + W] @ w64[:, :, dy, dx].T
    if bias is not None:
        out += bias.astype(np.float64)
    return out


@functools.lru_cache(maxsize=None)
def case(shape):
    """state, weights (scaled by 1 / sqrt(9 Cin)), bias and the float64 results with and without bias; never written again"""
    B, H, W, Cin, Cout = shape
    rs = np.random.RandomState(B * 1000 + H * 10 + Cin)
    state = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    bias = rs.standard_normal(Cout).astype(np.float32)
    want = {False: conv_f64(state, w, None), True: conv_f64(state, w, bias)}
    for a in (state, w, bias, want[False], want[True]):
        a.setflags(write=False)
    return state, w, bias, want


def pad32(state, w):
    """the generic launch's operands: input channels zero-padded to 32, as the forward's state tensor and packed weights are"""
    B, H, W, Cin = state.shape
    s = np.zeros((B, H, W, 32), np.float32)
    s[..., :Cin] = state
    wp = np.zeros((w.shape[0], 32, 3, 3), np.float32)
    wp[:, :Cin] = w
    return s, wp


@pytest.fixture(scope="module")
def eng():
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    yield e
    e.close()


def check_against_f64(eng, tag, state, w, bias, want):
    """runs the new kernel and the generic one on the same inputs; both bars; returns the new kernel's result"""
    n0 = eng.conv_in_f32_launches()
    r = eng.op_conv_in_f32(state, w, bias, want_stats=False)
    assert eng.conv_in_f32_launches() == n0 + 1
    generic = eng.op_conv2d(*pad32(state, w), bias)
    assert eng.conv_in_f32_launches() == n0 + 1              # the generic path is not the new kernel
    err, err_g = float(np.abs(r["out"] - want).max()), float(np.abs(generic - want).max())
    print(f"conv_in_f32 {tag}: max |gpu - f64| {err:.3e}   generic kernel {err_g:.3e}   (bars {BAR:.0e}, 2 x generic)")
    assert r["out"].shape == want.shape and np.isfinite(r["out"]).all()
    assert err < BAR, err
    assert err <= 2 * err_g, (err, err_g)
    return r


@pytest.mark.parametrize("with_stats", [False, True], ids=["nostats", "stats"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_against_float64(eng, shape, with_bias, with_stats):
    B, H, W, Cin, Cout = shape
    state, w, bias, want = case(shape)
    b = bias if with_bias else None
    r = check_against_f64(eng, f"{_sid(shape)} bias={int(with_bias)}", state, w, b, want[with_bias])
    if not with_stats:
        assert r["stats"] is None
        return
    slices = H * W // 256
    need = B * slices * Cout * 2
    rs = eng.op_conv_in_f32(state, w, b, want_stats=True, stats_slots=need + 2 * Cout)
    out, st = rs["out"], rs["stats"]
    assert np.array_equal(_bits(out), _bits(r["out"]))       # the statistics change nothing of the output
    assert rs["slices"] == slices and st.shape == (B, slices, Cout, 2)
    assert not np.isnan(st).any(), f"{int(np.isnan(st).any(axis=(2, 3)).sum())} of {B * slices} (image, slice) rows hold the fill"
    v = out.reshape(B, slices, 256, Cout).astype(np.float64)
    e1 = np.abs(st[..., 0] - v.sum(2)) / np.abs(v).sum(2)
    e2 = np.abs(st[..., 1] - (v * v).sum(2)) / (v * v).sum(2)
    print(f"  stats S1 {e1.max():.1e} S2 {e2.max():.1e} (relative, bar {STATS_REL:.0e})")
    assert e1.max() <= STATS_REL and e2.max() <= STATS_REL
    tail = rs["stats_raw"][need:]
    assert tail.size == 2 * Cout and np.all(_bits(tail) == np.uint64(0xFFFFFFFFFFFFFFFF)), "slots behind the slices were written"


def test_borders(eng):
    """zero except the four corner pixels and one edge pixel: every live window hangs over the zero border"""
    shape = (2, 16, 32, 6, 64)
    B, H, W, Cin, Cout = shape
    rs = np.random.RandomState(5)
    state = np.zeros((B, H, W, Cin), np.float32)
    for y, x in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H - 1, 7)]:
        state[:, y, x] = rs.standard_normal((B, Cin))
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    bias = rs.standard_normal(Cout).astype(np.float32)
    want = conv_f64(state, w, bias)
    r = check_against_f64(eng, "borders " + _sid(shape), state, w, bias, want)
    # a pixel whose window holds no live input is its bias, exactly
    live = np.abs(conv_f64(np.abs(state), np.ones_like(w), None)).max(-1) > 0
    assert live.sum() == B * (4 * 4 + 6) and np.array_equal(r["out"][~live], np.broadcast_to(bias, r["out"][~live].shape))


def test_independent_of_batch_and_grid(eng):
    """image i of a B = 5 call is the B = 1 call on that image, byte for byte: output and statistics"""
    shape = (5, 16, 32, 6, 64)
    state, w, bias, _ = case(shape)
    whole = eng.op_conv_in_f32(state, w, bias)
    for i in range(shape[0]):
        one = eng.op_conv_in_f32(state[i:i + 1], w, bias)
        assert np.array_equal(_bits(one["out"][0]), _bits(whole["out"][i])), i
        assert np.array_equal(_bits(one["stats"][0]), _bits(whole["stats"][i])), i


@pytest.mark.parametrize("shape", [(1, 16, 16, 9, 64), (1, 16, 16, 6, 48), (1, 16, 16, 6, 128), (1, 32, 24, 6, 64), (1, 8, 16, 6, 64)],
                         ids=_sid)
def test_refuses_what_the_gate_refuses(eng, shape):
    B, H, W, Cin, Cout = shape
    n0 = eng.conv_in_f32_launches()
    with pytest.raises(Sr3Error, match=r"Cin <= 8, Cout 32 \| 64, W % 16 == 0, H\*W % 256 == 0"):
        eng.op_conv_in_f32(np.zeros((B, H, W, Cin), np.float32), np.zeros((Cout, Cin, 3, 3), np.float32))
    assert eng.conv_in_f32_launches() == n0


@pytest.mark.parametrize("prec", ["f16x3", "f16f8"])
def test_refuses_a_split_precision(eng, prec):
    state, w, bias, _ = case(SHAPES[0])
    eng.set_precision(prec)
    try:
        with pytest.raises(Sr3Error, match="exact-f32 arithmetic only"):
            eng.op_conv_in_f32(state, w, bias)
    finally:
        eng.set_precision("f32")


# ---- forward level ---------------------------------------------------------------------------------------------------------
SCHED = {"schedule": "linear", "n_timestep": 2, "linear_start": 1e-4, "linear_end": 2e-2}


def forward_inputs(name):
    g = load_golden(name)
    m = g["meta"]
    cfg = cfg_from_meta(m)
    if "x" in g:
        x, nl = g["x"], g["noise_level"]
    else:
        x, nl = synth.synth_unet_input(cfg, m["B"], *m["r"], m["seed"])
    return cfg, m["seed"], x, nl, g["eps"]


def run_forwards():
    """name -> (eps, launches of the new kernel by two forwards, fallback calls)"""
    res = {}
    for name in ("unet_tiny.npz", "unet_cfgA.npz"):
        cfg, seed, x, nl, _ = forward_inputs(name)
        e = pkg("engine").Engine(cfg, 0)
        try:
            e.load_state_dict(synth.synth_state_dict(cfg, seed))
            e.set_precision("f32")
            n0 = e.conv_in_f32_launches()
            eps = e.unet_forward_np(x, nl)
            n1 = e.conv_in_f32_launches()
            again = e.unet_forward_np(x, nl)
            assert np.array_equal(_bits(again), _bits(eps))
            res[name] = (eps, (n1 - n0, e.conv_in_f32_launches() - n1), e.fallback_calls())
        finally:
            e.close()
    return res


def run_sample():
    """a two-step f32 DDPM sample of the tiny config -> (images, graph captures, launches counted)"""
    cfg = synth.tiny_unet_config()
    e = pkg("engine").Engine(cfg, 0)
    try:
        e.load_state_dict(synth.synth_state_dict(cfg, 123))
        e.set_precision("f32")
        with np.errstate(divide="ignore", invalid="ignore"):
            e.set_schedule(pkg("schedule").schedule_buffers(SCHED))
        B, r, T = 2, 16, SCHED["n_timestep"]
        out = e.sample_np(synth.synth_cond(B, r, 8, 123), synth.synth_noise(T, B, 3, r, r, 123))
        return out, e.step_graph_captures(), e.conv_in_f32_launches()
    finally:
        e.close()


def child_main(what, path):
    if what == "forwards":
        res = run_forwards()
        np.savez(path, **{n: r[0] for n, r in res.items()}, **{n + ".n": np.array(r[1] + (r[2],), np.int64) for n, r in res.items()})
    else:
        out, captures, launches = run_sample()
        np.savez(path, out=out, n=np.array([captures, launches], np.int64))


def _child(tmp_path, what, env_add):
    path = str(tmp_path / (what + ".npz"))
    env = dict(os.environ)
    for k in ("SR3_NO_CONV_IN_F32", "SR3_NO_GRAPH"):
        env.pop(k, None)
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    z = np.load(path)
    return {k: z[k] for k in z.files}


def test_forwards_reach_the_kernel():
    for name, (eps, launches, fallbacks) in run_forwards().items():
        err = float(np.abs(eps - forward_inputs(name)[4]).max())
        print(f"{name} [f32]: max abs err vs reference {err:.3e}; launches per forward {launches}")
        assert err < TOL and launches == (1, 1) and fallbacks == 0, (name, err, launches, fallbacks)


def test_forwards_with_the_switch_set(tmp_path):
    z = _child(tmp_path, "forwards", {"SR3_NO_CONV_IN_F32": "1"})
    for name in ("unet_tiny.npz", "unet_cfgA.npz"):
        err = float(np.abs(z[name] - forward_inputs(name)[4]).max())
        print(f"{name} [f32, SR3_NO_CONV_IN_F32=1]: max abs err vs reference {err:.3e}; counters {z[name + '.n']}")
        assert err < TOL and z[name + ".n"].tolist() == [0, 0, 0], (name, err, z[name + ".n"])


def test_captured_step_equals_the_eager_step(tmp_path):
    eager = _child(tmp_path, "sample", {"SR3_NO_GRAPH": "1"})
    out, captures, launches = run_sample()
    assert eager["n"][0] == 0 and eager["n"][1] >= SCHED["n_timestep"], eager["n"]        # every step launched, none captured
    assert captures >= 1 and launches >= 1, (captures, launches)                          # the kernel is inside a captured step
    assert np.isfinite(out).all() and np.array_equal(_bits(out), _bits(eager["out"]))


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
