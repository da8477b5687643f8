"""The numpy packers of the apply pass's output formats (tests/gn_stats_ref.py) against hand-written vectors: the GPU
tests compare the kernels' words with these packers bit for bit, so the packers themselves are pinned here. No GPU."""
import numpy as np

import gn_stats_ref as ref


def _chunk(vals):
    g = np.zeros((1, 32), np.float32)
    g[0, :len(vals)] = vals
    return g


def _fmt1(vals):
    w = ref.pack_format(_chunk(vals), 1).view(np.uint16).reshape(64)
    return w[:len(vals)].tolist(), w[32:32 + len(vals)].tolist()


def _fmt2(vals):
    b = ref.pack_format(_chunk(vals), 2).view(np.uint8).reshape(128)
    return b[:64].view(np.uint16)[:len(vals)].tolist(), b[64:64 + len(vals)].tolist(), b[96:96 + len(vals)].tolist()


def test_fp16_hi_rounds_to_nearest_even_and_lo_takes_the_rest():
    vals = [1.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -12, 65504.0, 0.0]
    hi, lo = _fmt1(vals)
    #          1.0     tie -> even (1.0)  tie -> even (1 + 2^-9)  the same, negative  below the tie  largest half  zero
    assert hi == [0x3C00, 0x3C00, 0x3C02, 0xBC00, 0x3C00, 0x7BFF, 0x0000]
    assert lo == [0x0000, 0x1000, 0x9000, 0x9000, 0x0C00, 0x0000, 0x0000]


def test_fp16_subnormals():
    vals = [2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -15 + 2.0 ** -26]
    hi, lo = _fmt1(vals)
    # smallest subnormal | tie 0 / 2^-24 -> 0, and the rest (2^-25) ties to 0 again | tie 1 / 2 ulp -> 2, rest -2^-25 -> -0
    # smallest normal | largest subnormal | 2^-15 = 0x0200 with a rest of 2^-26 that rounds to 0
    assert hi == [0x0001, 0x0000, 0x0002, 0x0400, 0x03FF, 0x0200]
    assert lo == [0x0000, 0x0000, 0x8000, 0x0000, 0x0000, 0x0000]


def test_e4m3_of_hi_and_of_scaled_lo():
    vals = [448.0, -448.0, 1.0, 1.0625, 1.1875, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -6, 1 + 2.0 ** -11, 0.0]
    hi, l8, h8 = _fmt2(vals)
    assert hi[0] == 0x5F00 and hi[1] == 0xDF00 and hi[2] == 0x3C00
    # +-448 = 1.75 * 2^8: S.1111.110 | 1.0 = 0.0111.000 | ties 1.0625 -> 1.0, 1.1875 -> 1.25 (even mantissas)
    # subnormals: 2^-9 = 0x01, 2^-10 ties to 0, 1.5 * 2^-9 ties to 2 * 2^-9; 2^-6 = smallest normal
    assert h8 == [0x7E, 0xFE, 0x38, 0x38, 0x3A, 0x01, 0x00, 0x02, 0x08, 0x38, 0x00]
    # lo * 2^11: only 1 + 2^-11 leaves a rest among these (2^-11 -> 1.0 = 0x38)
    assert l8 == [0, 0, 0, 0, 0, 0, 0, 0, 0, 0x38, 0]


def test_e4m3_of_lo_subnormals_and_sign():
    # hi = 1.0 (ties to even below 1 + 2^-11), rest r: r * 2^11 = 2^-9 (smallest e4m3 subnormal), 2^-10 (ties to 0),
    # and a negative rest: 1 - 2^-13 -> hi = 1.0 (fp16 spacing below 1 is 2^-11), rest -2^-13 -> -0.25 = 1.01101.000 -> 0xA8
    vals = [1 + 2.0 ** -20, 1 + 2.0 ** -21, 1 - 2.0 ** -13]
    hi, l8, h8 = _fmt2(vals)
    assert hi == [0x3C00, 0x3C00, 0x3C00]
    assert l8 == [0x01, 0x00, 0xA8]
    assert h8 == [0x38, 0x38, 0x38]


def test_chunk_layout_and_round_trip():
    rs = np.random.RandomState(0)
    g = (rs.standard_normal((2, 3, 64)) * 5).astype(np.float32)
    w1 = ref.pack_format(g, 1)
    assert w1.shape == g.shape and w1.dtype == np.uint32
    hi, lo = ref.split_halves(w1)
    assert np.abs(hi + lo - g).max() <= 2.0 ** -21 * np.abs(g).max()
    # the second chunk of a pixel starts 128 bytes after the first
    b = w1.view(np.uint8).reshape(2, 3, 2, 128)
    assert np.array_equal(b[1, 2, 1, :64].view(np.float16), g[1, 2, 32:].astype(np.float16))
    w2 = ref.pack_format(g, 2).view(np.uint8).reshape(2, 3, 2, 128)
    assert np.array_equal(w2[..., :64], b[..., :64])            # the hi halfs are the same in both formats
    assert np.array_equal(ref.pack_format(g, 0), g.view(np.uint32))


def test_partials_add_up():
    rs = np.random.RandomState(1)
    x = rs.standard_normal((2, 5, 7, 8)).astype(np.float32)
    b = ref.chunk_bounds(rs, 35, 7)
    assert b[0] == 0 and b[-1] == 35 and np.all(np.diff(b) > 0) and len(b) == 8
    p = ref.partials(x, b)
    assert p.shape == (2, 7, 8, 2)
    np.testing.assert_allclose(p[..., 0].sum(1), x.astype(np.float64).sum((1, 2)), rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(p[..., 1].sum(1), (x.astype(np.float64) ** 2).sum((1, 2)), rtol=1e-13)
