"""The second launch of a ResnetBlock (run_res: conv2 + a skip form + the write of the block output) through
sr3_op_conv2d_fused, one case per (precision, kernel, split form, skip form) class, each against a float64 reference of
that one launch (tests/conv_fused_ref.py):

    conv3x3_f64(act(x), w) + [in2 ‖ in2b] @ w2^T + b + b2 + chan_bias + resid

The entry point hands the kernels what run_res / prepare_fused hand them (pre-added biases, the common 2^k of w and w2,
in2 / in2b in the plain split format, the identity matrix with its k <= 15 cap), and runs the plan conv_plan(...,
stats=True) names for the 3x3 shape (it fails if the launch would take another).

Per case:
  0. (CPU side) the plan of the shape is in the class the case is meant for; a dispatch change fails here. The Winograd
     rows also assert the form by the engine's launch counters.
  1. out against float64 at the bars the suite holds single convs to, absolute on these data: 2e-5 in f32 and f16x3,
     3e-5 behind a GroupNorm + Swish prologue (test_gpu_ops.py; every third case has one), 2e-4 on F8C (test_gpu_f16f8.py).
  2. no NaN sentinel left in the fused GroupNorm statistics, and per (image, channel) the slices add up to the fp64 sums
     of that call's own stored `out`, to 1e-9 (test_gpu_conv_stats.py items 2 and 3): they feed the next block's GroupNorm
     and must include the term.
  3. split modes: the twin is, bit for bit, hi = fp16(out), lo = fp16(out - hi) of that call's own stored fp32 `out`; a
     second call with the fp32 output switched off returns the identical twin and statistics and leaves a sentinel-filled
     `out` untouched.
  4. image B-1 is a copy of image 0 in every input: the two output rows (and twin rows) are bit-identical.

Separate tests: a residual given as split-format words (rows without a term), the identity K-steps (with the k <= 15 cap
taken), the range flag of the twin store, and the entry point's refusals.
"""
import numpy as np
import pytest

import conv_fused_ref as ref
import gn_stats_ref as gn
from conftest import pkg

synth = pkg("synth")
engine = pkg("engine")
Sr3Error = pkg("_lib").Sr3Error


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(synth.tiny_unet_config(), 0)
    e.load_state_dict(synth.synth_state_dict(e.cfg, 11))
    yield e
    e.set_precision("f32")
    e.close()


G64, G12864, G128128 = "generic_64x64", "generic_128x64", "generic_128x128"
# ((B, H, W, Cin, Cout), kernel, split, splits, [(C2a, C2b), ...]): the generic_64x64 rows run in f32 and f16x3
GENERIC64 = [
    ((2, 16, 8, 32, 64), G64, "none", 1, [(32, 0), (32, 32)]),
    ((2, 16, 8, 128, 64), G64, "inplace", 2, [(96, 32)]),            # four 1x1 chunks: the second split reads in2 and in2b
    ((1, 8, 8, 512, 512), G64, "inplace", 8, [(64, 0), (512, 512)]),   # two chunks over eight splits: splits with no 1x1 K-step
    ((2, 4, 6, 128, 256), G64, "reduce", 2, [(64, 64)]),
    ((2, 2, 2, 512, 512), G64, "reduce", 8, [(256, 256)]),           # ragged M tile (8 pixels)
]
# Winograd rows: (wino_gemm_out, wino_fused_rows) counter deltas of the call
WINO = {(16, 16, 16, 128, 64): (0, 0), (64, 32, 32, 128, 128): (1, 0), (64, 32, 32, 128, 256): (0, 1), (32, 64, 64, 64, 64): (0, 0)}
ROWS = [("f32",) + r for r in GENERIC64] + [
    ("f32", (64, 32, 32, 32, 64), G12864, "none", 1, [(32, 32)]),
    ("f32", (64, 32, 32, 32, 128), G128128, "none", 1, [(64, 0)]),
    ("f32", (16, 16, 16, 128, 64), "wino_three_pass", "none", 1, [(64, 64)]),     # position GEMMs + output kernel
    ("f32", (64, 32, 32, 128, 128), "wino_three_pass", "none", 1, [(64, 64)]),    # wino_gemm_out
    ("f32", (64, 32, 32, 128, 256), "wino_three_pass", "none", 1, [(128, 0)]),    # wino_fused_rows
    ("f32", (32, 64, 64, 64, 64), "wino_one_pass", "none", 1, [(32, 32)]),
] + [("f16x3",) + r for r in GENERIC64] + [
    ("f16x3", (64, 32, 32, 32, 64), "halo_128x64", "none", 1, [(32, 32)]),
    ("f16x3", (64, 32, 32, 32, 128), "halo_128x128_seg32", "none", 1, [(64, 0)]),
    ("f16x3", (128, 16, 16, 64, 256), "halo_128x128_seg8", "none", 1, [(96, 32)]),
    ("f16x3", (32, 8, 8, 256, 512), "halo_128x128_seg8", "inplace_halo", 2, [(96, 32), (512, 512)]),
    ("f16x3", (64, 16, 16, 128, 256), G12864, "none", 1, [(128, 0)]),             # generic kernel on split operands
    ("f16f8", (64, 32, 32, 32, 128), "halo_f8c", "none", 1, [(64, 0)]),
    ("f16f8", (128, 16, 16, 64, 256), "halo_f8c", "none", 1, [(96, 32)]),
]
# (precision, shape, kernel, split, splits, term, GroupNorm + Swish prologue): every third case has the prologue
CASES = [(prec, shape, kernel, split, splits, term) for prec, shape, kernel, split, splits, terms in ROWS for term in terms]
CASES = [c + (i % 3 == 2,) for i, c in enumerate(CASES)]

# the identity K-steps (split modes; Cout <= 128): (shape, {precision: (kernel, split, splits)})
IDENT = [
    ((2, 16, 8, 64, 64), {"f16x3": (G64, "none", 1), "f16f8": (G64, "none", 1)}),
    ((64, 8, 8, 128, 128), {"f16x3": (G64, "inplace", 2), "f16f8": (G64, "inplace", 2)}),
    ((64, 32, 32, 64, 64), {"f16x3": ("halo_128x64", "none", 1), "f16f8": ("halo_128x64", "none", 1)}),
    ((64, 32, 32, 128, 128), {"f16x3": ("halo_128x128_seg32", "none", 1), "f16f8": ("halo_f8c", "none", 1)}),
]
IDENT_CASES = [(prec, shape) + IDENT[i][1][prec] + (cap,) for prec in ("f16x3", "f16f8") for i, (shape, _) in enumerate(IDENT)
               for cap in ((False, True) if i == 0 else (False,))]

# a residual that exists only as its split twin: rows without a term (the first generic_64x64 row and the halo rows)
RESID_SPLIT = [r[:5] for r in ROWS if r[0] == "f16x3" and (r[1] == (2, 16, 8, 32, 64) or r[2].startswith("halo"))]

RANGE = [((2, 16, 8, 32, 64), G64), ((64, 32, 32, 32, 64), "halo_128x64")]


def _id(case):
    prec, shape, kernel, split, splits, term, gnorm = case
    t = "ident" if term == "ident" else "none" if term is None else f"{term[0]}+{term[1]}"
    return f"{prec}-{kernel}-{split}{splits}-" + "x".join(map(str, shape)) + f"-{t}" + ("-gn" if gnorm else "")


def _plan(prec, shape):
    d = engine.conv_plan(*shape, precision=prec, stats=True)
    return d["kernel"], d["split"], d["splits"]


def test_case_list_reaches_every_class():
    """CPU side of the lists: every case is in its class (also asserted per case), and together the 1x1-term cases reach
    every kernel that can run a ResnetBlock's conv2 and every split form."""
    kernels, splits = set(), set()
    for prec, shape, kernel, split, nsp, terms in ROWS:
        assert _plan(prec, shape) == (kernel, split, nsp), (prec, shape, _plan(prec, shape))
        assert engine.conv_plan(*shape, precision=prec, stats=True)["stats_slices"] > 0
        kernels.add(kernel)
        splits.add(split)
        for C2a, C2b in terms:
            assert C2a % 32 == 0 and C2b % 32 == 0
    assert kernels == {"wino_one_pass", "wino_three_pass", "halo_f8c", "halo_128x128_seg32", "halo_128x128_seg8", "halo_128x64",
                       G12864, G64, G128128}
    assert splits == {"none", "reduce", "inplace", "inplace_halo"}
    assert sum(c[-1] for c in CASES) == len(CASES) // 3
    for prec, shape, kernel, split, nsp, cap in IDENT_CASES:
        assert _plan(prec, shape) == (kernel, split, nsp), (prec, shape, _plan(prec, shape))
        assert shape[3] == shape[4] <= 128
    assert len(RESID_SPLIT) == 5 and {r[2] for r in RESID_SPLIT} == {G64, "halo_128x64", "halo_128x128_seg32", "halo_128x128_seg8"}
    for shape, kernel in RANGE:
        assert _plan("f16x3", shape)[0] == kernel


def _call(eng, prec, d, gnorm=False, **kw):
    """One sr3_op_conv2d_fused call on the batch behind d (the distinct images indexed out)."""
    idx = d["idx"]
    pick = lambda a: None if a is None else a[idx]
    if gnorm:
        eng.set_precision("f32")
        sc, sh = eng.op_groupnorm_affine(d["x"], d["gamma"], d["beta"], 32)
        kw.update(gn_scale=sc[idx], gn_shift=sh[idx], swish=True)
    kw.setdefault("resid", pick(d["resid"]))
    eng.set_precision(prec)
    try:
        return eng.op_conv2d_fused(d["x"][idx], d["w"], d["b"], chan_bias=d["cb"][idx], in2=pick(d["in2"]), in2b=pick(d["in2b"]),
                                   w2=d["w2"], b2=d["b2"], **kw)
    finally:
        eng.set_precision("f32")


def _err(out, d, want=None):
    want = d["want"] if want is None else want
    return max(np.abs(out[d["idx"] == k] - want[k]).max() for k in range(d["nd"]))


def _check_stats(st, out):
    B, H, W, Cout = out.shape
    assert st is not None and st.shape[0] == B and st.shape[2:] == (Cout, 2)
    assert not np.isnan(st).any(), f"{int(np.isnan(st).any(axis=(2, 3)).sum())} of {st.shape[0] * st.shape[1]} (image, slice) rows hold a NaN sentinel"
    v = out.reshape(B, H * W, Cout).astype(np.float64)
    a1, a2 = np.abs(v).sum(1), (v * v).sum(1)
    d1, d2 = np.abs(st[..., 0].sum(1) - v.sum(1)), np.abs(st[..., 1].sum(1) - a2)
    print(f"  totals: S1 {np.max(d1 / a1):.1e} S2 {np.max(d2 / a2):.1e} (rel, bar 1e-9)", end="")
    assert np.all(d1 <= 1e-9 * a1) and np.all(d2 <= 1e-9 * a2)


def _check_twin(eng, prec, d, r, gnorm=False, **kw):
    """item 3: the twin of call r (made with twin=True) and the twin-only repeat of it"""
    B = r["out"].shape[0]
    assert np.array_equal(r["twin"], gn.pack_format(r["out"], 1)), "the twin is not hi = fp16(out), lo = fp16(out - hi)"
    assert np.array_equal(r["twin"][0], r["twin"][B - 1])
    t = _call(eng, prec, d, gnorm, twin=True, f32_out=False, **kw)
    assert np.array_equal(t["twin"], r["twin"]), "the twin-only call wrote another twin"
    assert np.array_equal(t["stats"].view(np.uint64), r["stats"].view(np.uint64)), "the twin-only call left other statistics"
    assert np.all(t["out"].view(np.uint32) == engine.Engine.FUSED_SENTINEL), "the twin-only call wrote to the fp32 output"
    print("  twin ok, twin-only ok", end="")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fused_1x1_term(eng, case):
    prec, shape, kernel, split, nsp, term, gnorm = case
    assert _plan(prec, shape) == (kernel, split, nsp)
    B = shape[0]
    d = ref.case_data(shape, term, gnorm)
    split_mode = prec != "f32"
    c0 = (eng.wino_gemm_out_launches(), eng.wino_fused_rows_launches(), eng.up2_wino_launches())
    r = _call(eng, prec, d, gnorm, twin=split_mode)
    dc = (eng.wino_gemm_out_launches() - c0[0], eng.wino_fused_rows_launches() - c0[1], eng.up2_wino_launches() - c0[2])
    out = r["out"]

    bar = 2e-4 if kernel == "halo_f8c" else 3e-5 if gnorm else 2e-5
    err = _err(out, d)
    print(f"{_id(case)}: plan {kernel}/{split} x{nsp}, counters (gemm_out, fused_rows, up2) +{dc}: err {err:.2e} (bar {bar:.0e})", end="")
    assert dc == WINO.get(shape if prec == "f32" else None, (0, 0)) + (0,)
    assert out.shape == (B,) + d["want"].shape[1:]
    assert err < bar
    _check_stats(r["stats"], out)
    assert np.array_equal(out[0].view(np.uint32), out[B - 1].view(np.uint32)), "image B-1 (a copy of image 0) came out differently"
    if split_mode:
        _check_twin(eng, prec, d, r, gnorm)
    print()


@pytest.mark.gpu
@pytest.mark.parametrize("case", IDENT_CASES, ids=lambda c: f"{c[0]}-{c[2]}-{c[3]}{c[4]}-" + "x".join(map(str, c[1])) + ("-cap" if c[5] else ""))
def test_identity_k_steps(eng, case):
    """The identity skip of a narrow block as extra K-steps against the engine's identity matrix: conv + in2 (in2 the block
    input; an independent tensor here, as in run_res, where the conv reads the activated h1). cap: w scaled to max|w| <
    2^-5, so that its exponent is capped at 15 and w is re-split."""
    prec, shape, kernel, split, nsp, cap = case
    assert _plan(prec, shape) == (kernel, split, nsp)
    B = shape[0]
    d = ref.case_data(shape, "ident", resid=False)
    if cap:
        d["w"] = d["w"] * np.float32(2.0 ** -6 / np.abs(d["w"]).max())
        assert np.abs(d["w"]).max() < 2.0 ** -5
        d["want"] = ref.reference(d)
    r = _call(eng, prec, d, ident=True, twin=True)
    bar = 2e-4 if kernel == "halo_f8c" else 2e-5
    err = _err(r["out"], d)
    print(f"{prec} ident {shape}{' cap' if cap else ''}: plan {kernel}/{split} x{nsp}: err {err:.2e} (bar {bar:.0e})", end="")
    assert err < bar
    _check_stats(r["stats"], r["out"])
    assert np.array_equal(r["out"][0].view(np.uint32), r["out"][B - 1].view(np.uint32))
    _check_twin(eng, prec, d, r, ident=True)
    print()


@pytest.mark.gpu
@pytest.mark.parametrize("row", RESID_SPLIT, ids=lambda r: f"{r[2]}-{r[3]}{r[4]}-" + "x".join(map(str, r[1])))
def test_split_residual(eng, row):
    """A residual that exists only as its split twin (resid_split): the words of values that are exactly hi + lo."""
    prec, shape, kernel, split, nsp = row
    assert _plan(prec, shape) == (kernel, split, nsp)
    B = shape[0]
    d = ref.case_data(shape, None, seed=1)
    words, r64 = ref.exact_split(d["resid"])
    want = ref.reference(d, resid64=r64)
    r = _call(eng, prec, d, resid=words[d["idx"]], resid_split=True, twin=True)
    err = _err(r["out"], d, want)
    print(f"{prec} split residual {shape}: plan {kernel}/{split} x{nsp}: err {err:.2e} (bar 2e-05)", end="")
    assert err < 2e-5
    _check_stats(r["stats"], r["out"])
    assert np.array_equal(r["out"][0].view(np.uint32), r["out"][B - 1].view(np.uint32))
    _check_twin(eng, prec, d, r, resid=words[d["idx"]], resid_split=True)
    print()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kernel", RANGE, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_twin_range(eng, shape, kernel):
    """The range flag of the twin store: w and w2 of ONE output channel scaled so that it alone exceeds 65504 (magnitudes
    checked on the CPU): the "range" error with the twin requested, nothing without it."""
    assert _plan("f16x3", shape)[0] == kernel
    Cout = shape[4]
    d = ref.case_data(shape, (32, 32))
    for co in (Cout - 3, 0):
        e = dict(d)
        w, w2 = d["w"].copy(), d["w2"].copy()
        s = np.float32(4e5 / np.abs(d["want"][..., co]).max())
        w[co] *= s
        w2[co] *= s
        e["w"], e["w2"] = w, w2
        want = ref.reference(e)
        peak = np.abs(want).max(axis=(0, 1, 2))
        assert peak[co] > 1e5 and np.isfinite(want).all()
        assert np.all(np.delete(peak, co) < 100), "one channel only"
        with pytest.raises(Sr3Error, match="range"):
            _call(eng, "f16x3", e, twin=True)
        with pytest.raises(Sr3Error, match="range"):
            _call(eng, "f16x3", e, twin=True, f32_out=False)
        out = _call(eng, "f16x3", e)["out"]
        got = np.abs(out).max(axis=(0, 1, 2))
        assert np.isfinite(out).all() and got[co] > 1e5 and np.all(np.delete(got, co) < 100)
    assert _err(_call(eng, "f16x3", d, twin=True)["out"], d) < 2e-5          # (the flag does not outlive the failed calls)


@pytest.mark.gpu
def test_refusals(eng):
    """What run_res never builds is an error and launches nothing."""
    d = ref.case_data((2, 16, 8, 64, 64), (32, 32))
    x, idx = d["x"][d["idx"]], d["idx"]
    f = lambda a: a[idx]
    with pytest.raises(Sr3Error, match="split-f16"):
        eng.op_conv2d_fused(x, d["w"], d["b"], twin=True)                                   # f32: no twin
    with pytest.raises(Sr3Error, match="split-f16"):
        eng.op_conv2d_fused(x, d["w"], d["b"], in2=f(d["resid"]), ident=True)               # f32: no identity K-steps
    with pytest.raises(Sr3Error, match="multiples of 32"):                                  # the engine's fused_ok
        eng.op_conv2d_fused(x, d["w"], d["b"], in2=f(d["in2"])[..., :16], w2=d["w2"][:, :16], b2=d["b2"])
    with pytest.raises(Sr3Error, match="go together"):
        eng.op_conv2d_fused(x, d["w"], d["b"], in2=f(d["in2"]))
    eng.set_precision("f16x3")
    try:
        with pytest.raises(Sr3Error, match="nothing to write"):
            eng.op_conv2d_fused(x, d["w"], d["b"], f32_out=False)
        with pytest.raises(Sr3Error, match="identity"):
            eng.op_conv2d_fused(x, d["w"], d["b"], in2=f(d["in2"]), ident=True)             # C2a != Cout
        with pytest.raises(Sr3Error, match="identity"):
            eng.op_conv2d_fused(x, d["w"], d["b"], in2=f(d["resid"]), w2=d["w2"], ident=True)
        with pytest.raises(Sr3Error, match="there is none"):
            eng.op_conv2d_fused(x, d["w"], d["b"], resid_split=True)
    finally:
        eng.set_precision("f32")
