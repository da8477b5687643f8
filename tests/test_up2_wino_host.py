"""The Upsample conv as sub-pixel Winograd F(2x2, 2x2), host side (no GPU):

  1. a float64 numpy model of the transforms and of the indexing wino_up2_kernel uses (csrc/sr3_internal.h at
     make_up2_wino_weights) against nearest x2 + conv3x3: bar 1e-12 (the arithmetic is float64 and the transforms hold
     0 and +-1 only; the sums run over 9 * Cin terms of O(1): ~1e-15 expected);
  2. make_up2_wino_weights through sr3_wino_weights_host(frag = 2): every word is float32 of the fp64 sum, from 0.0 in
     (dy, dx) order, of the original taps G g G^T selects, in the layout [phase][position][CinPad/8][Cout][8];
  3. the exported conv plan of Upsample shapes is the same row with the switches unset, with SR3_NO_UP2_WINO=1 and with
     SR3_UP2_WINO_FORCE=1 (the new form is an unexported field of the plan): one child process per setting, since the
     switches are read once per process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import pkg

G = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
BT = np.array([[1.0, -1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, -1.0]])
AT = np.array([[1.0, 1.0, 0.0], [0.0, 1.0, -1.0]])
# taps of the 3x3 kernel that position i of phase p adds along one axis: G (g0, g1) = (g0, g0 + g1, g1) with the phase
# taps (g0, g1) = (w0, w1 + w2) for p = 0 and (w0 + w1, w2) for p = 1
TAPS = {0: [(0,), (0, 1, 2), (1, 2)], 1: [(0, 1), (0, 1, 2), (2,)]}


def upsample_conv_f64(x, w):
    """nearest x2 + zero-padded 3x3 conv; x [H, W, Cin], w [Cout, Cin, 3, 3] -> [2H, 2W, Cout], float64"""
    H, W, _ = x.shape
    up = np.pad(x.astype(np.float64).repeat(2, 0).repeat(2, 1), ((1, 1), (1, 1), (0, 0)))
    out = np.zeros((2 * H, 2 * W, w.shape[0]))
    for dy in range(3):
        for dx in range(3):
            out += up[dy:dy + 2 * H, dx:dx + 2 * W] @ w[:, :, dy, dx].astype(np.float64).T
    return out


def phase_taps(w, py, px):
    """the 2x2 taps of phase (py, px) over the padded low-resolution rows (y + py, y + py + 1): [2, 2, Cout, Cin]"""
    w = w.astype(np.float64)
    rows = [w[:, :, 0], w[:, :, 1] + w[:, :, 2]] if py == 0 else [w[:, :, 0] + w[:, :, 1], w[:, :, 2]]     # each [Cout, Cin, 3]
    g = np.zeros((2, 2) + w.shape[:2])
    for r, row in enumerate(rows):
        g[r, 0], g[r, 1] = (row[..., 0], row[..., 1] + row[..., 2]) if px == 0 else (row[..., 0] + row[..., 1], row[..., 2])
    return g


@pytest.mark.parametrize("H, W, Cin, Cout", [(8, 8, 5, 3), (4, 10, 3, 4)], ids=["8x8", "4x10"])
def test_transform_and_indexing_model(H, W, Cin, Cout):
    rs = np.random.default_rng(H * 100 + W)
    x = rs.standard_normal((H, W, Cin))
    w = rs.standard_normal((Cout, Cin, 3, 3))
    want = upsample_conv_f64(x, w)
    xp = np.pad(x, ((1, 1), (1, 1), (0, 0)))
    got = np.full_like(want, np.nan)
    for py in range(2):
        for px in range(2):
            V = np.einsum("ia,abok,jb->ijok", G, phase_taps(w, py, px), G)          # G g G^T: [3, 3, Cout, Cin]
            for ti in range(H // 2):
                for tj in range(W // 2):
                    d = xp[2 * ti + py:2 * ti + py + 3, 2 * tj + px:2 * tj + px + 3]   # [3, 3, Cin]
                    U = np.einsum("ia,abk,jb->ijk", BT, d, BT)
                    M = np.einsum("ijok,ijk->ijo", V, U)
                    Y = np.einsum("ai,ijo,bj->abo", AT, M, AT)
                    for a in range(2):
                        for b in range(2):
                            got[2 * (2 * ti + a) + py, 2 * (2 * tj + b) + px] = Y[a, b]
    err = np.abs(got - want).max()
    print(f"{H}x{W}, {Cin} -> {Cout}: max abs difference {err:.2e}")
    assert not np.isnan(got).any()
    assert err <= 1e-12


@pytest.fixture(scope="module")
def lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib_mod.load()


@pytest.mark.parametrize("cin", [32, 64])
def test_make_up2_wino_weights(lib, cin):
    cout = 32
    rs = np.random.default_rng(cin)
    packed = rs.standard_normal((9, cout, cin), dtype=np.float32)                 # [dy * 3 + dx][Cout][CinPad]
    dst = np.full(36 * cout * cin, np.nan, np.float32)
    assert lib.sr3_wino_weights_host(packed.ctypes.data, cout, cin, 2, dst.ctypes.data) == 0
    got = dst.reshape(4, 9, cin // 8, cout, 8)
    want = np.empty((4, 9, cout, cin), np.float32)
    for py in range(2):
        for px in range(2):
            for i in range(3):
                for j in range(3):
                    acc = np.zeros((cout, cin), np.float64)                       # from 0.0, in (dy, dx) order
                    for dy in TAPS[py][i]:
                        for dx in TAPS[px][j]:
                            acc = acc + packed[dy * 3 + dx].astype(np.float64)
                    want[py * 2 + px, i * 3 + j] = acc.astype(np.float32)         # rounded once
    want = want.reshape(4, 9, cout, cin // 8, 8).transpose(0, 1, 3, 2, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and the sums are G g G^T of the phase taps (the model above), to rounding
    w = packed.reshape(3, 3, cout, cin).transpose(2, 3, 0, 1)
    for py in range(2):
        for px in range(2):
            V = np.einsum("ia,abok,jb->ijok", G, phase_taps(w, py, px), G).reshape(9, cout, cin)
            have = got[py * 2 + px].transpose(0, 2, 1, 3).reshape(9, cout, cin)
            assert np.abs(have - V).max() <= 2.0 ** -22 * max(1.0, np.abs(V).max())


# B, H, W (low resolution), Cin, Cout: the step's Upsample convs, shapes the new form never takes, small forced-only shapes
PLAN_SHAPES = [(64, 8, 8, 512, 512), (64, 16, 16, 512, 512), (64, 32, 32, 256, 256), (64, 64, 64, 128, 128), (4, 64, 64, 128, 128),
               (2, 4, 64, 32, 32), (1, 2, 128, 96, 64), (3, 4, 32, 64, 96), (2, 8, 16, 160, 32), (1, 24, 16, 32, 64),
               (2, 8, 24, 32, 32), (2, 8, 16, 32, 48), (1, 8, 8, 512, 512)]


def _plans():
    engine = pkg("engine")
    rows = []
    for B, H, W, Cin, Cout in PLAN_SHAPES:
        for prec in ("f32", "f16x3"):
            for stats in (False, True):
                rows.append(engine.conv_plan(B, H, W, Cin, Cout, 3, 1, 1, precision=prec, stats=stats))
    return rows


def test_exported_plan_does_not_depend_on_the_switches(lib, tmp_path):
    got = {}
    for name, env_add in (("unset", {}), ("off", {"SR3_NO_UP2_WINO": "1"}), ("forced", {"SR3_UP2_WINO_FORCE": "1"})):
        env = {k: v for k, v in os.environ.items() if k not in ("SR3_NO_UP2_WINO", "SR3_UP2_WINO_FORCE")}
        env.update(env_add)
        path = str(tmp_path / (name + ".json"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        with open(path) as f:
            got[name] = json.load(f)
    assert len(got["unset"]) == 4 * len(PLAN_SHAPES)
    assert got["off"] == got["unset"] and got["forced"] == got["unset"]
    for row in got["unset"]:
        assert row["phases"] == 4 and not row["kernel"].startswith("wino")
    # the f32 rows of the step's three large Upsample convs keep the direct plan's statistics layout: 4 phases x HW / 128
    for i, (B, H, W, Cin, Cout) in enumerate(PLAN_SHAPES[1:4], start=1):
        row = got["unset"][4 * i + 1]
        assert row["split"] == "none" and row["stats_slices"] == 4 * (H * W // 128), row


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    with open(sys.argv[1], "w") as f:
        json.dump(_plans(), f)
