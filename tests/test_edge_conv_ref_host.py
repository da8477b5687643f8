"""CPU side of test_gpu_edge_convs.py: the references of edge_conv_ref.py against the oracle's conv, and the error bars of
every GPU case on that case's own data — the bar (8 x restatement error) stays at most 1/20 of what a dropped correction
product costs, so a kernel inside the bar has all three products."""
import numpy as np
import pytest

import edge_conv_ref as ref
import sr3_oracle as oracle


def test_float64_convs_match_the_oracle():
    """conv_in64 and final_conv64 against oracle.conv2d / oracle.swish (fp32): 54 resp. 576 fp32 terms of size <= ~1."""
    rs = np.random.RandomState(3)
    x = rs.standard_normal((2, 6, 10, 6)).astype(np.float32)
    w = (rs.standard_normal((32, 6, 3, 3)) / np.sqrt(54)).astype(np.float32)
    b = rs.standard_normal(32).astype(np.float32)
    assert np.abs(ref.conv_in64(x, w, b) - oracle.conv2d(x, w, b)).max() < 2e-6
    x = rs.standard_normal((2, 5, 9, 64)).astype(np.float32)
    w = (rs.standard_normal((3, 64, 3, 3)) / 24).astype(np.float32)
    b = rs.standard_normal(3).astype(np.float32)
    gamma, beta = (1 + 0.1 * rs.standard_normal(64)).astype(np.float32), (2 + 0.1 * rs.standard_normal(64)).astype(np.float32)
    sc, sh = ref.gn_affine64(x, gamma, beta, 32)
    act = oracle.swish(oracle.group_norm(x, gamma, beta, 32))
    want = oracle.conv2d(act, w, b)
    assert np.abs(ref.final_conv64(x, sc, sh, w, b) - want).max() < 5e-6
    assert np.abs(ref.final_conv_f32(x, sc, sh, w, b) - want).max() < 5e-6
    # padding AFTER the activation: padding the raw tensor first puts swish(shift) ~ 1.8 into the border instead of 0,
    # which this data shows at the border pixels and nowhere else
    act_pad = ref.activate(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), sc, sh, np.float64)
    padded_first = ref.conv3x3(act_pad, w, np.float64)[:, 1:-1, 1:-1] + b
    d = np.abs(padded_first - ref.final_conv64(x, sc, sh, w, b))
    assert d[:, 1:-1, 1:-1].max() < 1e-12 and min(d[:, 0].max(), d[:, -1].max(), d[:, :, 0].max(), d[:, :, -1].max()) > 0.1


def test_pack16_and_scale_exponent():
    v = np.array([0.0, 1.0, 1.0 + 2.0 ** -12, -3.14159274, 65504.0, 7e4, np.inf, 1e-9], dtype=np.float32)
    hi, lo = ref.pack16(v)
    assert hi.dtype == lo.dtype == np.float16
    fin = np.isfinite(hi)
    assert list(fin) == [True] * 5 + [False, False, True]
    rec = hi[fin].astype(np.float64) + lo[fin].astype(np.float64)
    assert np.all(np.abs(rec - v[fin]) <= np.abs(v[fin]) * 2.0 ** -21 + 2.0 ** -25)     # 11 + 11 bits, subnormal lo below
    assert lo[1] == 0 and lo[2] == np.float16(2.0 ** -12) and np.isnan(lo[6])
    for mx in (1e-3, 0.4999, 0.5, 1.0, 1023.9, 1024.0, 3000.0):
        k = ref.split_scale_exponent(np.array([mx, -mx / 3], dtype=np.float32))
        assert 1024 <= np.float32(mx) * 2.0 ** k < 2048, (mx, k)
    assert ref.split_scale_exponent(np.zeros(4, np.float32)) == 0


def test_emulation_is_the_three_product_split():
    """Against an independent statement: (xh + xl)(wh + wl) - xl wl in float64 differs from emulate_split only by the fp32
    accumulation."""
    c = ref.conv_in_case((3, 16, 16, 6, 64))
    k = ref.split_scale_exponent(c["w"])
    xh, xl = (a.astype(np.float64) for a in ref.pack16(c["state"]))
    wh, wl = (a.astype(np.float64) for a in ref.pack16(c["w"] * np.float32(2.0 ** k)))
    exact = (ref.conv3x3(xh + xl, wh + wl, np.float64) - ref.conv3x3(xl, wl, np.float64)) * 2.0 ** -k + c["bias"]
    assert np.abs(ref.emulate_split(c["state"], c["w"], c["bias"]) - exact).max() < 2e-6
    assert np.abs(exact - c["want"]).max() < 1e-6         # the xl wl term and the operands' 2^-22: far below fp32 accumulation
    for drop in ("x_lo", "w_lo"):
        assert np.abs(ref.emulate_split(c["state"], c["w"], c["bias"], drop=drop) - exact).max() > 1e-4


def test_image_index():
    for B in (1, 2, 3, 4, 520):
        idx = ref.image_index(B)
        assert idx.shape == (B,) and idx[0] == 0 and idx[B - 1] == 0 and idx.max() == max(0, min(B - 1, 3) - 1)


@pytest.mark.parametrize("shape", ref.CONV_IN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_in_bars(shape):
    c = ref.conv_in_case(shape)
    print(f"conv_in {shape}: emulation {c['emu_err']:.2e}  bar {c['bar']:.2e}  dropped product {c['dropped_err']:.2e}")
    assert c["emu_err"] > 0 and ref.bar_condition(c["bar"], c["dropped_err"])
    # (the range cases of the GPU test scale these weights by 1/4: one 65504 state value then stays inside the twin's range)
    assert 65504 * 0.25 * np.abs(c["w"]).max() + np.abs(c["want"]).max() < 65504


def test_mfma_cases_are_among_the_valu_cases():
    """The two forms are compared on the same data, and test_final_conv_bars below reaches the MFMA cases through the list
    of VALU cases."""
    assert set(ref.FINAL_MFMA) <= set(ref.FINAL_VALU) and len(ref.FINAL_MFMA) == 10 and len(ref.FINAL_VALU) == 60
    assert all(Cout == 3 and C <= 128 for _, C, Cout in ref.FINAL_MFMA)


@pytest.mark.parametrize("case", ref.FINAL_VALU, ids=lambda c: "x".join(map(str, c[0])) + f"-C{c[1]}-Cout{c[2]}")
def test_final_conv_bars(case):
    shape, C, Cout = case
    c = ref.final_case(shape, C, Cout)
    sc, sh = ref.gn_affine64(c["x"], c["gamma"], c["beta"], 32)
    assert np.abs(sh).min() > 1.0                          # swish(shift) far from 0 in every channel
    v = ref.final_refs(c, sc, sh, "valu")
    print(f"final_conv {shape} C={C} Cout={Cout}: fp32 restatement {v['emu_err']:.2e}  bar {v['bar']:.2e}", end="")
    assert v["emu_err"] > 0
    if Cout == 3 and C <= 128:
        m = ref.final_refs(c, sc, sh, "mfma")
        print(f"  | split emulation {m['emu_err']:.2e}  bar {m['bar']:.2e}  dropped product {m['dropped_err']:.2e}", end="")
        assert m["emu_err"] > 0 and ref.bar_condition(m["bar"], m["dropped_err"])
        # the VALU bar of the same data separates as well (the two forms are compared within the sum of their bars)
        assert ref.bar_condition(v["bar"] + m["bar"], m["dropped_err"])
    print()
