"""Weight layouts of the exact-f32 Winograd convs (no GPU): the one-pass kernel's fragment-major copy
[16][CinPad/8][Cout][8] holds, element by element, the values of the three-pass layout [16][Cout][CinPad]
(make_wino_weights), and those are G g G^T of the packed [9][Cout][CinPad] weights rounded once to fp32."""
import os

import numpy as np
import pytest

from conftest import pkg

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])


@pytest.fixture(scope="module")
def lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib_mod.load()


def _layout(lib, packed, cout, cin, frag):
    dst = np.full(16 * cout * cin, np.nan, np.float32)
    rc = lib.sr3_wino_weights_host(packed.ctypes.data, cout, cin, frag, dst.ctypes.data)
    assert rc == 0
    return dst


@pytest.mark.parametrize("cout, cin", [(64, 64), (64, 192), (128, 384), (32, 8)])
def test_frag_layout_matches_make_wino_weights(lib, cout, cin):
    rs = np.random.default_rng(cout * 1000 + cin)
    packed = rs.standard_normal((9, cout, cin), dtype=np.float32)         # [dy * 3 + dx][Cout][CinPad]
    std = _layout(lib, packed, cout, cin, 0).reshape(16, cout, cin)
    frag = _layout(lib, packed, cout, cin, 1).reshape(16, cin // 8, cout, 8)
    want = std.reshape(16, cout, cin // 8, 8).transpose(0, 2, 1, 3)
    assert np.array_equal(frag, want)
    # G g G^T in fp64, rounded once
    ref = np.einsum("ai,ijkc,bj->abkc", G, packed.reshape(3, 3, cout, cin).astype(np.float64), G).reshape(16, cout, cin)
    assert np.abs(std.astype(np.float64) - ref).max() <= 2 ** -22 * max(1.0, np.abs(ref).max())


def test_frag_layout_rejects_bad_cin(lib):
    packed = np.zeros(9 * 4 * 12, np.float32)
    dst = np.zeros(16 * 4 * 12, np.float32)
    assert lib.sr3_wino_weights_host(packed.ctypes.data, 4, 12, 1, dst.ctypes.data) != 0
