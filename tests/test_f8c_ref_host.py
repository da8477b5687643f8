"""CPU side of test_gpu_f8c_model.py: the float64 model of the fp8-correction conv's operand formats (tests/f8c_ref.py) is
held to the packers it inverts, to the figures the formats predict, and to the defects it is there to see. No GPU.

BAR(case) = 3 x chain_roundoff (one sequential fp32 chain against the float64 model, first image of the case), max abs:

  (16, 32, 32, 32, 0, 512) 3.00e-6    (64, 32, 32, 96, 0, 128) 4.46e-6    (128, 8, 16, 64, 0, 512) 3.89e-6
  (128, 16, 8, 32, 32, 512) 3.85e-6   (128, 4, 32, 32, 0, 512) 2.19e-6    (48, 12, 32, 64, 0, 512) 4.09e-6
  (24, 24, 32, 32, 64, 512) 5.32e-6   (64, 16, 16, 512, 512, 512) 1.37e-5     (condition: every one <= 1.5e-5)

Discrimination: an operand defect put into the model, the case it is paired with, how far it moves the model and how far
the defective model is from the exact float64 conv (the 2e-4 of test_gpu_f16f8.py / test_gpu_conv_fused.py is measured
against that, and a correct kernel already sits ~5e-5 from it):

  defect                                                     case                         BAR     vs model  vs exact  2e-4 bar
  w_lo8 lost for 4 channels of one tap                       (128, 8, 16, 64, 0, 512)     3.9e-6  1.8e-4    1.7e-4    passes
  w_hi8 truncated instead of round-to-nearest-even           (64, 32, 32, 96, 0, 128)     4.5e-6  7.3e-5    6.3e-5    passes
  x_hi8 = e4m3(fp16(g)) instead of e4m3(g)                   (128, 4, 32, 32, 0, 512)     2.2e-6  1.8e-5    5.4e-5    passes
  w_lo8 * x_hi8 lost for one tap of one 32-channel chunk     (128, 8, 16, 64, 0, 512)     3.9e-6  2.9e-4    2.9e-4    fails
  x_lo8 of one lane's 8 channels lost on every tap           (48, 12, 32, 64, 0, 512)     4.1e-6  3.9e-4    4.0e-4    fails
  fp8 bytes of an image's row 0 from the previous image      (48, 12, 32, 64, 0, 512)     4.1e-6  1.0e-3    1.0e-3    fails
  block scale off by 2x in one chunk (x_lo8 * w_hi8)         (24, 24, 32, 32, 64, 512)    5.3e-6  6.0e-4    6.3e-4    fails
  w_lo8 lost for one output column in 128                    (64, 32, 32, 96, 0, 128)     4.5e-6  6.9e-4    7.1e-4    fails
  w_lo8 lost for 4 channels of one tap                       (64, 16, 16, 512, 512, 512)  1.4e-5  4.6e-5    6.3e-5    passes
  w_lo8 lost for one output column in 128                    (64, 16, 16, 512, 512, 512)  1.4e-5  5.7e-4    5.8e-4    fails

A localised defect weighs by 1 / sqrt(9 Cin) of these data (w ~ N(0, 1) / sqrt(9 Cin)): the first rows are larger here, at
Cin 64, than at the Cin 256 of the issue's table, and smaller at Cin 1024; three of them sit within 1e-5 of where a correct
kernel does against the exact conv (4.5e-5 .. 5.8e-5): no bar on that distance separates them from it.
"""
import numpy as np
import pytest
import torch

import conv_fused_ref as cref
import f8c_ref as f8
import gn_stats_ref as gn
from conftest import pkg

engine = pkg("engine")


# ---- decoders -----------------------------------------------------------------------------------------------------------------
def test_e4m3_table_is_the_format():
    b = np.arange(256, dtype=np.uint8)
    t = torch.from_numpy(b).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    ok = ~np.isnan(t)
    assert ok.sum() == 254 and np.array_equal(np.isnan(f8.E4M3), ~ok)
    assert np.array_equal(f8.E4M3[ok], t[ok]) and np.array_equal(np.signbit(f8.E4M3[ok]), np.signbit(t[ok]))
    assert f8.E4M3[0x7E] == 448.0 and f8.E4M3[0x01] == 2.0 ** -9 and f8.E4M3[0x08] == 2.0 ** -6
    assert np.array_equal(gn.e4m3_bytes(f8.E4M3[ok].astype(np.float32)), b[ok])          # every value encodes to its own byte


def test_activation_decoder_inverts_the_packer():
    rs = np.random.RandomState(0)
    g = (rs.standard_normal((2, 5, 7, 96)) * np.exp(rs.uniform(-14, 5, (2, 5, 7, 96)))).astype(np.float32)
    g = np.clip(g, -f8.SPLIT_F8_MAX, f8.SPLIT_F8_MAX)
    words = gn.pack_format(g, 2)
    xh, xl8, xh8 = f8.unpack_f8c_act(words)
    assert xh.shape == xl8.shape == xh8.shape == g.shape
    hi = g.astype(np.float16)
    lof = g - hi.astype(np.float32)
    assert np.array_equal(xh, hi.astype(np.float64))
    # re-encoding the decoded values gives the packer's bytes back, chunk by chunk
    b = words.view(np.uint8).reshape(-1, 3, 128)
    assert np.array_equal(gn.e4m3_bytes((xl8 * 2.0 ** f8.SR3_F8_XL).astype(np.float32)).reshape(-1, 3, 32), b[..., 64:96])
    assert np.array_equal(gn.e4m3_bytes((xh8 * 2.0 ** f8.SR3_F8_XH).astype(np.float32)).reshape(-1, 3, 32), b[..., 96:])
    # and they are the e4m3 roundings: half a last place of 4 significant bits, or half the subnormal spacing 2^-9
    assert np.all(np.abs(xh8 - g) <= np.maximum(2.0 ** -4 * np.abs(g), 2.0 ** -10))
    assert np.all(np.abs(xl8 - lof) <= np.maximum(2.0 ** -4 * np.abs(lof), 2.0 ** -10 * 2.0 ** -f8.SR3_F8_XL))


def test_activation_decoder_on_crafted_values():
    eps = np.float32(1 + 2.0 ** -10)
    # value -> (xh8, xl8 * 2^11)
    table = [(448.0, 448.0, 0.0), (-448.0, -448.0, 0.0), (0.0, 0.0, 0.0), (-0.0, -0.0, 0.0),
             (17.0, 16.0, 0.0), (19.0, 20.0, 0.0), (-17.0, -16.0, 0.0),                # e4m3 ties: to the even neighbour
             (2.0 ** -10, 0.0, 0.0), (2.0 ** -10 * eps, 2.0 ** -9, None),              # below the smallest subnormal 2^-9
             (1.5 * 2.0 ** -9, 2.0 ** -8, None),                                       # a subnormal tie
             (300.125, 288.0, 256.0), (-300.125, -288.0, -256.0),                      # |lo * 2^11| at its 256 bound
             (447.875, 448.0, -256.0)]
    g = np.zeros((1, 1, 1, 32), np.float32)
    g[0, 0, 0, :len(table)] = [t[0] for t in table]
    xh, xl8, xh8 = f8.unpack_f8c_act(gn.pack_format(g, 2))
    for i, (v, h8, l8) in enumerate(table):
        assert xh8[0, 0, 0, i] == h8 and np.signbit(xh8[0, 0, 0, i]) == np.signbit(np.float32(v)), (v, xh8[0, 0, 0, i], h8)
        if l8 is not None:
            assert xl8[0, 0, 0, i] * 2.0 ** f8.SR3_F8_XL == l8, (v, xl8[0, 0, 0, i] * 2048, l8)
    assert np.abs(xl8 * 2.0 ** f8.SR3_F8_XL).max() == 256.0


def test_weight_split_and_decoder():
    rs = np.random.RandomState(1)
    for mx, k in ((0.25, 12), (np.nextafter(np.float32(0.25), np.float32(0)), 13), (1.0, 10), (3e-3, 19)):
        w = rs.standard_normal((64, 96, 3, 3)).astype(np.float32)
        w = (w / np.abs(w).max() * np.float32(mx)).astype(np.float32)
        assert f8.split_scale_exponent(w) == k
        packed = f8.pack_weight(w)
        assert packed.shape == (9 * 64, 96) and packed[5 * 64 + 3, 17] == w[3, 17, 1, 2]
        k2, hi, lo, sb = f8.weight_split(packed)
        assert k2 == k and 1024 <= np.abs(hi.astype(np.float64)).max() <= 2048
        assert np.abs(hi.astype(np.float64) + lo.astype(np.float64) - packed.astype(np.float64) * 2.0 ** k).max() <= 2.0 ** -11
        h = sb.view(np.float16).reshape(-1, 64)
        assert np.array_equal(h[:, :32].reshape(hi.shape), hi) and np.array_equal(h[:, 32:].reshape(lo.shape), lo)
        fb = f8.weight_f8c_bytes(sb)
        assert fb.size == sb.size and np.array_equal(fb.reshape(-1, 128)[:, :64], sb.reshape(-1, 128)[:, :64])
        wh, wh8, wl8 = f8.unpack_f8c_weight(fb, packed.shape)
        assert np.array_equal(wh, hi.astype(np.float64))
        assert np.array_equal(gn.e4m3_bytes((wh8 * 2.0 ** f8.SR3_F8_WH).astype(np.float32)).reshape(-1, 32), fb.reshape(-1, 128)[:, 64:96])
        assert np.array_equal(gn.e4m3_bytes((wl8 * 2.0 ** f8.SR3_F8_WL).astype(np.float32)).reshape(-1, 32), fb.reshape(-1, 128)[:, 96:])
        assert np.abs(wh8 * 2.0 ** f8.SR3_F8_WH).max() <= 256 and np.abs(wl8 * 2.0 ** f8.SR3_F8_WL).max() <= 256
    assert f8.weight_split(np.zeros((9, 32), np.float32))[0] == 0
    # crafted scaled values (k given): hi * 2^-3 = 256 at the top, e4m3 ties, -0, a value whose lo is an fp16 subnormal
    v = np.zeros((1, 32), np.float32)
    v[0, :8] = [2048.0, -2048.0, 8 * 17.0, 8 * 19.0, -0.0, 1.0 + 2.0 ** -20, 8 * 2.0 ** -10, 1544.5]
    k, hi, lo, sb = f8.weight_split(v, 0)
    wh, wh8, wl8 = f8.unpack_f8c_weight(f8.weight_f8c_bytes(sb), v.shape)
    assert list(wh8[0, :5]) == [2048.0, -2048.0, 8 * 16.0, 8 * 20.0, 0.0] and np.signbit(wh8[0, 4])
    assert lo[0, 5] == np.float16(2.0 ** -20) and wl8[0, 5] == 0.0            # 2^-20 * 2^9 = 2^-11: under half of 2^-9
    assert wh8[0, 6] == 0.0                                                   # the tie between 0 and 2^-9: to even
    assert wh[0, 7] == 1544.0 and wl8[0, 7] == 0.5 and wh8[0, 7] == 8 * 192.0


# ---- the model's figures ----------------------------------------------------------------------------------------------------------
SANITY = [f8.CASES[1], f8.CASES[7]]


@pytest.mark.parametrize("case", SANITY, ids=f8.case_id)
def test_model_sits_where_the_formats_put_it(case):
    """2e-5 .. 1e-4 from the exact conv (the corrections are in fp8: the CPU figures are 4.5e-5 .. 5.8e-5), and the same
    model with three f16 products within 1e-6 (the corrections are present: without one it is ~1e-3)."""
    d = f8.case_data(case)
    model, exact = f8.case_refs(case)
    e8 = np.abs(model - exact).max()
    e3 = np.abs(f8.conv_f8c_model(d["x"], d["w"], d["b"], f16x3=True) - exact).max()
    print(f"{f8.case_id(case)}: model vs exact {e8:.2e}; with three f16 products {e3:.2e}")
    assert 2e-5 <= e8 <= 1e-4
    assert e3 <= 1e-6


@pytest.mark.parametrize("case", f8.CASES, ids=f8.case_id)
def test_bar_condition(case):
    b = f8.bar(case)
    print(f"BAR{case} = {b:.2e}")
    assert 0 < b <= f8.BAR_LIMIT, "smaller data, not a larger bar"


# ---- discrimination -----------------------------------------------------------------------------------------------------------------
_POS = np.sort(f8.E4M3[:0x7F])


def _e4m3_truncate(v):
    """e4m3 of v rounded towards zero (float64 in, float64 out)"""
    return np.sign(v) * _POS[np.searchsorted(_POS, np.abs(v), side="right") - 1]


def _taps(o, name):
    return o[name].reshape(9, -1, o[name].shape[-1])        # a view: [tap][Cout][C]


def d_wlo8_4_channels_of_one_tap(o):
    _taps(o, "wl8")[4, :, 8:12] = 0


def d_whi8_truncated(o):
    o["wh8"] = _e4m3_truncate(o["wh"] * 2.0 ** f8.SR3_F8_WH) * 2.0 ** -f8.SR3_F8_WH


def d_xhi8_from_fp16(o):
    o["xh8"] = f8.e4m3_decode(gn.e4m3_bytes(o["xh"].astype(np.float32)))


def d_wlo8_xhi8_lost_one_tap_one_chunk(o):
    _taps(o, "wl8")[7, :, 32:64] = 0


def d_xlo8_one_lane_every_tap(o):
    o["xl8"][..., 40:48] = 0


def d_row0_fp8_bytes_from_previous_image(o):
    for n in ("xl8", "xh8"):
        o[n][1:, 0] = o[n][:-1, 0].copy()


def d_block_scale_2x_one_chunk(o):
    o["xl8"][..., 32:64] *= 2


def d_wlo8_lost_one_output_column(o):
    _taps(o, "wl8")[:, 77, :] = 0


DEFECTS = [
    (d_wlo8_4_channels_of_one_tap, f8.CASES[2]),
    (d_whi8_truncated, f8.CASES[1]),
    (d_xhi8_from_fp16, f8.CASES[4]),
    (d_wlo8_xhi8_lost_one_tap_one_chunk, f8.CASES[2]),
    (d_xlo8_one_lane_every_tap, f8.CASES[5]),
    (d_row0_fp8_bytes_from_previous_image, f8.CASES[5]),
    (d_block_scale_2x_one_chunk, f8.CASES[6]),
    (d_wlo8_lost_one_output_column, f8.CASES[1]),
    (d_wlo8_4_channels_of_one_tap, f8.CASES[7]),           # ... and under the largest BAR, the deepest K
    (d_wlo8_lost_one_output_column, f8.CASES[7]),
]


@pytest.mark.parametrize("defect,case", DEFECTS, ids=lambda v: v.__name__[2:] if callable(v) else f8.case_id(v))
def test_defect_moves_the_model_by_more_than_bar(defect, case):
    d = f8.case_data(case)
    model, exact = f8.case_refs(case)
    o = f8.operands(d["x"], d["w"])
    o = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in o.items()}
    defect(o)
    bad = f8.conv_operands(o) + d["b"].astype(np.float64)
    moved, from_exact = np.abs(bad - model).max(), np.abs(bad - exact).max()
    print(f"{defect.__name__[2:]:40s} {f8.case_id(case):24s} BAR {f8.bar(case):.1e}  vs model {moved:.1e}  vs exact {from_exact:.1e}  "
          f"{'fails' if from_exact >= 2e-4 else 'passes'} 2e-4")
    assert moved > f8.bar(case)


# ---- the case list ------------------------------------------------------------------------------------------------------------------
def test_case_list_plans_as_f8c():
    """Every shape of test_gpu_f8c_model.py (b) and (c2) plans as halo_f8c, unsplit, on the fp8 path — with and without fused
    statistics (host only: no GPU, no context)."""
    shapes = [(B, H, W, C0 + C1, Cout) for B, H, W, C0, C1, Cout in f8.CASES] + \
        [(64, 32, 32, 32, 128), (128, 16, 16, 64, 256), (64, 32, 32, 128, 128), (64, 16, 16, 128, 512)]
    for shape in shapes:
        for stats in (False, True):
            p = engine.conv_plan(*shape, precision="f16f8", stats=stats)
            assert (p["kernel"], p["split"], p["splits"], p["f8"]) == ("halo_f8c", "none", 1, True), (shape, stats, p)
    for B, H, W, C0, C1, Cout in f8.CASES:
        assert C0 % 32 == 0 and C1 % 32 == 0 and cref.images(B).max() == 2
