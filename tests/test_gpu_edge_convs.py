"""The kernels of csrc/kernels_edge.hip one at a time, through the forward's own launchers, weight packers and gates
(sr3_op_conv_in, sr3_op_final_conv), against the float64 references of edge_conv_ref.py:

  conv_in_kernel + pack_state_kernel   downs.0 (Cin <= 8 -> 32 | 64) on the packed split-f16 state, f16x3 and f16f8
  final_conv_kernel                    GroupNorm + Swish + 3x3 (C -> 1..4) on fp32 VALU, f32
  final_conv_mfma_kernel               the same layer (C 64 | 128 -> 3) in split-f16, hi / lo split on the fly

Error bars: per case 8 x the error of the CPU restatement of the kernel's arithmetic against float64 on the case's own data
(edge_conv_ref.py: the three-product split-f16 emulation, plain fp32 for the VALU form), computed here from the inputs, never
from the kernels' results; asserted to stay at most 1/20 of what a dropped correction product costs on the same data
(4.5e-6 .. 1.2e-5 against 7.8e-4 .. 1.3e-3; test_edge_conv_ref_host.py prints every case's figures).

Statistics: "1e-12 relative" is relative to sum|v| resp. sum v^2 of the slice, as in test_gpu_conv_stats.py (the kernel adds
the same 256 fp32 values in fp64 in another order: <= 256 * 2^-53 of sum|v|).

Defect found by this file and fixed with it: the range check of both MFMA kernels read `__builtin_bit_cast(unsigned short,
vec[e])` of a half-vector element, which compiled to a read of element 0 for every e — 7 of the 8 channels a lane converts
were never checked (final_conv_mfma_kernel: activations; conv_in_kernel: the twin). test_conv_in_range and
test_final_conv_mfma_range fail on those kernels (no error for one out-of-range channel) and pass on the corrected ones.

Observed on an MI355X, max |gpu - float64| over the case (bar in brackets); the worst case is at 0.34 of its bar.
  conv_in (statistics: S1 exact in every case — 256 fp32 values add exactly in fp64 —, S2 1.8e-15 .. 2.7e-15 relative)
    f16x3 1x16x16x6x32    6.68e-07 (4.97e-06)        f16x3 2x16x16x3x64    7.04e-07 (4.45e-06)
    f16x3 3x16x16x6x64    6.57e-07 (6.06e-06)        f16x3 2x16x16x8x32    7.38e-07 (5.62e-06)
    f16x3 2x8x32x6x64     6.08e-07 (4.58e-06)        f16x3 520x16x16x6x64  9.54e-07 (6.19e-06)
    f16x3 1x16x48x6x64    1.03e-06 (6.22e-06)        f16f8 3x16x16x6x64    6.57e-07 (6.06e-06)  (the bits of f16x3)
  final_conv, MFMA form, Cout 3 (f16x3; f16f8 returns the same bits)  |  |mfma - valu| (sum of the two bars)
    2x6x20-C64     9.64e-07 (5.80e-06)  |  9.54e-07 (1.09e-05)        2x6x20-C128    9.75e-07 (7.40e-06)  |  1.43e-06 (1.35e-05)
    1x9x33-C64     9.54e-07 (5.82e-06)  |  9.54e-07 (1.09e-05)        1x9x33-C128    9.65e-07 (6.69e-06)  |  1.43e-06 (1.32e-05)
    3x4x32-C64     1.37e-06 (8.08e-06)  |  1.91e-06 (1.60e-05)        3x4x32-C128    1.14e-06 (7.59e-06)  |  1.43e-06 (1.24e-05)
    1x16x16-C64    8.74e-07 (7.12e-06)  |  9.54e-07 (1.37e-05)        1x16x16-C128   9.62e-07 (1.02e-05)  |  1.43e-06 (2.00e-05)
    2x8x64-C64     1.58e-06 (1.18e-05)  |  1.43e-06 (2.05e-05)        2x8x64-C128    1.28e-06 (8.89e-06)  |  1.43e-06 (1.64e-05)
  final_conv, VALU form (f32), Cout 1 | 2 | 3 | 4
    2x6x20-C64     8.99e-07 (3.63e-06)  6.81e-07 (6.50e-06)  7.62e-07 (5.12e-06)  9.89e-07 (4.42e-06)
    2x6x20-C128    9.65e-07 (5.49e-06)  1.18e-06 (7.17e-06)  1.42e-06 (6.08e-06)  1.20e-06 (7.57e-06)
    2x6x20-C256    1.61e-06 (5.54e-06)  1.89e-06 (6.61e-06)  1.48e-06 (9.46e-06)  2.15e-06 (7.08e-06)
    1x9x33-C64     9.13e-07 (4.43e-06)  8.52e-07 (5.66e-06)  8.34e-07 (5.10e-06)  1.27e-06 (8.68e-06)
    1x9x33-C128    1.25e-06 (6.46e-06)  9.03e-07 (5.24e-06)  1.24e-06 (6.53e-06)  1.09e-06 (7.57e-06)
    1x9x33-C256    1.66e-06 (5.91e-06)  1.55e-06 (6.10e-06)  1.43e-06 (7.81e-06)  2.07e-06 (1.24e-05)
    3x4x32-C64     7.00e-07 (6.55e-06)  7.30e-07 (5.17e-06)  1.02e-06 (7.91e-06)  8.35e-07 (1.04e-05)
    3x4x32-C128    9.63e-07 (5.43e-06)  1.31e-06 (5.16e-06)  1.16e-06 (4.77e-06)  1.37e-06 (7.27e-06)
    3x4x32-C256    1.25e-06 (1.02e-05)  1.41e-06 (6.82e-06)  1.62e-06 (6.79e-06)  1.36e-06 (6.43e-06)
    1x16x16-C64    8.11e-07 (5.66e-06)  8.77e-07 (4.57e-06)  9.03e-07 (6.55e-06)  1.05e-06 (7.45e-06)
    1x16x16-C128   1.04e-06 (6.95e-06)  1.07e-06 (5.55e-06)  1.40e-06 (9.84e-06)  1.50e-06 (6.63e-06)
    1x16x16-C256   1.14e-06 (6.45e-06)  1.83e-06 (5.36e-06)  1.49e-06 (6.77e-06)  1.76e-06 (8.83e-06)
    2x8x64-C64     9.40e-07 (5.37e-06)  1.20e-06 (7.24e-06)  1.27e-06 (8.78e-06)  1.13e-06 (6.80e-06)
    2x8x64-C128    1.16e-06 (5.35e-06)  1.10e-06 (7.08e-06)  1.22e-06 (7.52e-06)  1.44e-06 (6.61e-06)
    2x8x64-C256    1.35e-06 (6.40e-06)  1.51e-06 (9.37e-06)  1.86e-06 (9.62e-06)  1.89e-06 (7.12e-06)
"""
import numpy as np
import pytest

import edge_conv_ref as ref
from conftest import pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
engine = pkg("engine")
Sr3Error = pkg("_lib").Sr3Error


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(synth.tiny_unet_config(), 0)
    yield e
    e.close()


def _sid(s):
    return "x".join(map(str, s))


def _bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _per_image_err(out, want, idx):
    return np.array([np.abs(out[b] - want[idx[b]]).max() for b in range(out.shape[0])])


def _replicas_equal(out, idx):
    """every batch row that holds the same image (row B-1 is a copy of row 0) has the same bits"""
    for k in range(int(idx.max()) + 1):
        rows = np.flatnonzero(idx == k)
        if not all(_same(out[rows[0]], out[r]) for r in rows[1:]):
            return False
    return True


# ---- conv_in ---------------------------------------------------------------------------------------------------------------
CONV_IN = [("f16x3", s) for s in ref.CONV_IN_SHAPES] + [("f16f8", (3, 16, 16, 6, 64))]


def _conv_in_id(case):
    return case[0] + "-" + _sid(case[1])


@pytest.mark.parametrize("case", CONV_IN, ids=_conv_in_id)
def test_conv_in(eng, case):
    prec, shape = case
    B, H, W, Cin, Cout = shape
    c = ref.conv_in_case(shape)
    idx, state = c["idx"], c["state"][c["idx"]]
    assert ref.bar_condition(c["bar"], c["dropped_err"]), (c["bar"], c["dropped_err"])
    eng.set_precision(prec)
    try:
        r1 = eng.op_conv_in(state, c["w"], c["bias"])
        r2 = eng.op_conv_in(state, c["w"], c["bias"])
        r3 = eng.op_conv_in(state, c["w"], c["bias"], want_out=False)
    finally:
        eng.set_precision("f32")
    out, twin, st = r1["out"], r1["twin"], r1["stats"]

    # the output against float64, image by image
    err = _per_image_err(out, c["want"], idx)
    print(f"conv_in {_conv_in_id(case)}: err {err.max():.2e} (bar {c['bar']:.2e}; emulation {c['emu_err']:.2e}, dropped product "
          f"{c['dropped_err']:.2e})", end="")
    assert out.shape == (B, H, W, Cout) and np.all(err < c["bar"]), err.max()
    assert _replicas_equal(out, idx) and _same(out[B - 1], out[0])
    for k in ("out", "twin", "stats", "packed"):
        assert _same(r1[k], r2[k]), k

    # the twin: 32 hi | 32 lo halfs per 32-channel chunk, of the stored fp32 value
    hi, lo = ref.pack16(out.reshape(B, H, W, Cout // 32, 32))
    assert twin.shape == (B, H, W, Cout // 32, 2, 32)
    assert _same(twin[..., 0, :], hi) and _same(twin[..., 1, :], lo)

    # the statistics: one slice per 256-pixel block, of the kernel's own fp32 output
    slices = H * W // 256
    assert st.shape == (B, slices, Cout, 2)
    assert not np.isnan(st).any(), f"{int(np.isnan(st).any(axis=(2, 3)).sum())} of {B * slices} (image, slice) rows hold a NaN sentinel"
    v = out.reshape(B, slices, 256, Cout).astype(np.float64)
    e1 = np.abs(st[..., 0] - v.sum(2)) / np.abs(v).sum(2)
    e2 = np.abs(st[..., 1] - (v * v).sum(2)) / (v * v).sum(2)
    print(f"  stats S1 {e1.max():.1e} S2 {e2.max():.1e} (rel, bar 1e-12)")
    assert e1.max() <= 1e-12 and e2.max() <= 1e-12

    # fp32 output switched off (the split-only forward): the same twin and statistics
    assert r3["out"] is None and _same(r3["twin"], twin) and _same(r3["stats"], st)

    # the packed state the conv read: pack16 of the zero-bordered, zero-padded fp32 state
    full = np.zeros((B, H + 2, W + 2, 8), dtype=np.float32)
    full[:, 1:-1, 1:-1, :Cin] = state
    ph, pl = ref.pack16(full)
    assert r1["packed"].shape == (B, H + 2, W + 2, 2, 8)
    assert _same(r1["packed"][..., 0, :], ph) and _same(r1["packed"][..., 1, :], pl)
    assert not r1["packed"][:, 0].any() and not r1["packed"][:, -1].any() and not r1["packed"][:, :, 0].any() \
        and not r1["packed"][:, :, -1].any() and not r1["packed"][..., Cin:].any()


@pytest.mark.parametrize("case", CONV_IN, ids=_conv_in_id)
def test_conv_in_range(eng, case):
    """The range flag of pack_state_kernel (state) and of the twin store (output): the largest fp16 passes, anything beyond
    or not finite is an error naming the range. The odd value sits in the last live channel of the last pixel of the last
    image; weights at 1/4 keep the outputs around a 65504 state value inside the twin's range (checked on the CPU)."""
    prec, shape = case
    B, H, W, Cin, Cout = shape
    c = ref.conv_in_case(shape)
    w, bias = c["w"] * np.float32(0.25), c["bias"]

    def run(v, **kw):
        state = c["state"][c["idx"]].copy()
        state[B - 1, H - 1, W - 1, Cin - 1] = v
        return eng.op_conv_in(state, kw.pop("w", w), bias, **kw)

    eng.set_precision(prec)
    try:
        r = run(65504.0)
        assert np.isfinite(r["out"]).all() and np.abs(r["out"]).max() < 65504
        assert r["packed"][B - 1, H, W, 0, Cin - 1] == 0x7BFF and r["packed"][B - 1, H, W, 1, Cin - 1] == 0
        for bad in (7e4, -7e4, np.inf):
            with pytest.raises(Sr3Error, match="range"):
                run(bad)
            with pytest.raises(Sr3Error, match="range"):
                run(bad, want_twin=False, want_stats=False)          # pack_state_kernel's own flag
        # an output beyond the twin's range: an error with the twin, none without it
        with pytest.raises(Sr3Error, match="range"):
            run(0.5, w=c["w"] * np.float32(1e5))
        big = run(0.5, w=c["w"] * np.float32(1e5), want_twin=False)["out"]
        assert np.isfinite(big).all() and np.abs(big).max() > 65504
        # ... and so is ONE output channel beyond it, whichever of the 8 channels a lane converts it is (the twin store
        # once checked the first of each lane's 8 only)
        for co in (Cout - 3, 9, 0):
            w1 = w.copy()
            w1[co] *= np.float32(4e5 / np.abs(c["want"][..., co]).max())
            with pytest.raises(Sr3Error, match="range"):
                run(0.5, w=w1)
        # a NaN never ends in a clean finite result
        for kw in ({}, {"want_twin": False}):
            try:
                r = run(np.nan, **kw)
            except Sr3Error as e:
                assert "range" in str(e)
            else:
                assert not np.isfinite(r["out"]).all()
        # and the context goes on working
        assert _same(run(0.5)["out"], run(0.5)["out"])
    finally:
        eng.set_precision("f32")


def test_conv_in_refuses_what_the_forward_refuses(eng):
    rs = np.random.RandomState(5)
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    eng.set_precision("f16x3")
    try:
        for B, H, W, Cin, Cout in [(1, 16, 40, 6, 64), (1, 16, 16, 6, 96), (1, 16, 16, 6, 16), (1, 16, 16, 6, 48),
                                   (1, 8, 16, 6, 64), (1, 16, 16, 9, 64)]:
            assert not (Cin <= 8 and Cout in (32, 64) and W % 16 == 0 and (H * W) % 256 == 0)
            with pytest.raises(Sr3Error, match="no shape of the packed-state conv"):
                eng.op_conv_in(f32(B, H, W, Cin), f32(Cout, Cin, 3, 3), f32(Cout))
        eng.set_precision("f32")          # the exact-f32 forward runs downs.0 on the generic conv
        with pytest.raises(Sr3Error, match="split-f16 arithmetics only"):
            eng.op_conv_in(f32(1, 16, 16, 6), f32(64, 6, 3, 3), f32(64))
    finally:
        eng.set_precision("f32")


# ---- final_conv ------------------------------------------------------------------------------------------------------------
def _final_id(case):
    return _sid(case[0]) + f"-C{case[1]}-Cout{case[2]}"


def _final_inputs(eng, case):
    """the case's data with the GroupNorm affine of its distinct images from op_groupnorm_affine (exact f32)"""
    c = ref.final_case(*case)
    eng.set_precision("f32")
    sc, sh = eng.op_groupnorm_affine(c["x"], c["gamma"], c["beta"], 32)
    assert np.abs(sh).min() > 1.0
    return c, sc, sh


def _final_run(eng, c, sc, sh, prec):
    idx = c["idx"]
    eng.set_precision(prec)
    try:
        a = eng.op_final_conv(c["x"][idx], sc[idx], sh[idx], c["w"], c["bias"], return_form=True)
        b = eng.op_final_conv(c["x"][idx], sc[idx], sh[idx], c["w"], c["bias"], return_form=True)
    finally:
        eng.set_precision("f32")
    assert a[1] == b[1] and _same(a[0], b[0])                  # a second call returns the same bits
    assert _replicas_equal(a[0], idx) and _same(a[0][len(idx) - 1], a[0][0])
    return a


@pytest.mark.parametrize("case", ref.FINAL_VALU, ids=_final_id)
def test_final_conv_valu(eng, case):
    (B, H, W), C, Cout = case
    c, sc, sh = _final_inputs(eng, case)
    refs = ref.final_refs(c, sc, sh, "valu")
    out, form = _final_run(eng, c, sc, sh, "f32")
    err = _per_image_err(out, refs["want"], c["idx"])
    print(f"final_conv valu {_final_id(case)}: err {err.max():.2e} (bar {refs['bar']:.2e}; fp32 restatement {refs['emu_err']:.2e})")
    assert form == "valu" and out.shape == (B, H, W, Cout)
    assert np.all(err < refs["bar"]), err.max()


@pytest.mark.parametrize("prec", ["f16x3", "f16f8"])
@pytest.mark.parametrize("case", ref.FINAL_MFMA, ids=_final_id)
def test_final_conv_mfma(eng, case, prec):
    (B, H, W), C, Cout = case
    c, sc, sh = _final_inputs(eng, case)
    rv, rm = ref.final_refs(c, sc, sh, "valu"), ref.final_refs(c, sc, sh, "mfma")
    assert ref.bar_condition(rm["bar"], rm["dropped_err"]), (rm["bar"], rm["dropped_err"])
    valu, fv = _final_run(eng, c, sc, sh, "f32")
    out, fm = _final_run(eng, c, sc, sh, prec)
    err = _per_image_err(out, rm["want"], c["idx"])
    both = float(np.abs(out - valu).max())
    print(f"final_conv mfma {prec} {_final_id(case)}: err {err.max():.2e} (bar {rm['bar']:.2e}; emulation {rm['emu_err']:.2e}, dropped "
          f"product {rm['dropped_err']:.2e})  |mfma - valu| {both:.2e} (bar {rv['bar'] + rm['bar']:.2e})")
    assert (fv, fm) == ("valu", "mfma") and out.shape == (B, H, W, 3)
    assert np.all(err < rm["bar"]), err.max()
    assert both <= rv["bar"] + rm["bar"]


@pytest.mark.parametrize("prec", ["f16x3", "f16f8"])
def test_final_conv_mfma_range(eng, prec):
    """The activations are split on the fly: one beyond the fp16 range raises the flag, the largest fp16 does not."""
    c = ref.final_case((1, 9, 33), 64, 3)
    x = c["x"].copy()
    one, zero = np.ones((1, 64), np.float32), np.zeros((1, 64), np.float32)
    eng.set_precision(prec)
    try:
        x[0, 8, 32, 63] = 65504.0                                 # swish(65504) = 65504 in fp32
        assert np.isfinite(eng.op_final_conv(x, one, zero, c["w"], c["bias"])).all()
        for bad in (7e4, np.inf, np.nan):
            x[0, 8, 32, 63] = bad
            with pytest.raises(Sr3Error, match="range"):
                eng.op_final_conv(x, one, zero, c["w"], c["bias"])
        x[0, 8, 32, 63] = 1.0
        # every one of the 8 channels a lane splits, in both K-steps, at corners and inside
        for y, xx, ch in [(0, 0, 0), (4, 17, 9), (8, 0, 18), (0, 32, 27), (3, 31, 36), (5, 5, 45), (2, 20, 54), (7, 1, 63)]:
            keep, x[0, y, xx, ch] = x[0, y, xx, ch], 7e4
            with pytest.raises(Sr3Error, match="range"):
                eng.op_final_conv(x, one, zero, c["w"], c["bias"])
            x[0, y, xx, ch] = keep
        assert np.isfinite(eng.op_final_conv(x, one, zero, c["w"], c["bias"])).all()
    finally:
        eng.set_precision("f32")


def test_final_conv_gates(eng):
    """What the forward's gates refuse is an error; C = 256 in split-f16 runs the VALU kernel, as in the forward."""
    rs = np.random.RandomState(9)
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    for prec in ("f32", "f16x3"):
        eng.set_precision(prec)
        try:
            for C, Cout in [(32, 3), (96, 3), (64, 5)]:
                with pytest.raises(Sr3Error, match="no shape of the fused final conv"):
                    eng.op_final_conv(f32(1, 4, 8, C), f32(1, C), f32(1, C), f32(Cout, C, 3, 3), f32(Cout))
        finally:
            eng.set_precision("f32")
    for C, Cout, form in [(256, 3, "valu"), (64, 2, "valu"), (128, 3, "mfma")]:
        x, sc, sh, w, b = f32(2, 5, 12, C), 1 + 0.1 * f32(2, C), 2 + 0.1 * f32(2, C), f32(Cout, C, 3, 3) / 48, f32(Cout)
        exact = eng.op_final_conv(x, sc, sh, w, b)
        eng.set_precision("f16x3")
        try:
            got, took = eng.op_final_conv(x, sc, sh, w, b, return_form=True)
        finally:
            eng.set_precision("f32")
        assert took == form
        assert _same(got, exact) == (form == "valu")
