"""The fp8-correction convs (halo_f8c: conv3x3_halo_h3<..., F8C = true>, the default 'f16f8' arithmetic) against a float64
model of their OWN operand formats (tests/f8c_ref.py) instead of a plain float64 conv: the formats alone put a correct
kernel ~5e-5 from the exact conv, which is why the other files hold it to 2e-4 (test_gpu_f16f8.py, test_gpu_conv_fused.py);
from the model it is fp32 accumulation order away, and the bar here is BAR(case) = 3 x the round-off of one sequential fp32
chain, measured on the CPU alone (f8c_ref.chain_roundoff; test_f8c_ref_host.py holds BAR <= 1.5e-5 and shows which operand
defects it sees that 2e-4 does not).

  a. the weights' `split` and `f8` layouts, bit for bit, against restatements of split_conv_weight_k / make_f8_weights_kernel;
  b. op_conv2d on eight shapes x three kinds of data: |gpu - model| <= BAR, |gpu - exact| >= 4 |gpu - model| (the model has
     to explain the kernel's error: a wrong model fails instead of passing by accident), repeats and replicas bit-identical;
  c. the epilogue (bias + chan_bias + resid + fused statistics) and the fused 1x1 / identity K-steps with the twin store;
  d. behind the GroupNorm + Swish prologue;
  e. one UNet forward against an oracle whose F8C convs use the model's operand formats, at the 1e-4 of the f32 / f16x3
     forwards (test_gpu_unet.py) in place of f16f8's 5e-4.

Every batch repeats three distinct images (conv_fused_ref.images: first = last, the middle one differs), so the CPU side runs
on three images.

BAR per case and what the GPU gave (max abs over the three images, standard-normal data; MI355X):

  (B, H, W, C0, C1, Cout)         BAR      |gpu - model|  |gpu - exact|
  (16, 32, 32, 32, 0, 512)        3.00e-6    1.71e-6        5.77e-5
  (64, 32, 32, 96, 0, 128)        4.46e-6    3.00e-6        5.17e-5
  (128, 8, 16, 64, 0, 512)        3.89e-6    2.11e-6        4.65e-5
  (128, 16, 8, 32, 32, 512)       3.85e-6    1.87e-6        4.87e-5
  (128, 4, 32, 32, 0, 512)        2.19e-6    1.46e-6        5.26e-5
  (48, 12, 32, 64, 0, 512)        4.09e-6    2.40e-6        5.58e-5
  (24, 24, 32, 32, 64, 512)       5.32e-6    3.24e-6        5.30e-5
  (64, 16, 16, 512, 512, 512)     1.37e-5    8.61e-6        4.98e-5

  wide-range data (bar = BAR x max|model|, 124 .. 174): |gpu - model| 0.11 .. 0.15 of the bar, |gpu - exact| 5 .. 60 x |gpu - model|
  neighbours data: the x100 image 0.45 .. 0.75 of BAR x 100 (the accumulation order weighs as on standard-normal data), the
  two plain images exactly their standard-normal figures: no row of the large neighbour is read
  c1 2.0e-6 / 3.1e-6; c2 2.2e-6 (bar 3.8e-6), 3.6e-6 (5.5e-6), 3.3e-6 (5.3e-6); d 7.0e-6 (bar 3.3e-6 + the 7.4e-6 by which the
  model moves when every g moves by +-1 ulp); e 1.39e-5 against the f8c oracle, 3.46e-5 against the plain one
"""
import numpy as np
import pytest
import torch

import conv_fused_ref as cref
import f8c_ref as f8
import gn_stats_ref as gn
from conftest import pkg
from test_gpu_conv_fused import _check_stats

pytestmark = pytest.mark.gpu
synth = pkg("synth")
engine = pkg("engine")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(synth.tiny_unet_config(), 0)
    e.load_state_dict(synth.synth_state_dict(e.cfg, 11))
    yield e
    e.set_precision("f32")
    e.close()


def _f8(eng, fn, *a, **kw):
    eng.set_precision("f16f8")
    try:
        return fn(*a, **kw)
    finally:
        eng.set_precision("f32")


def _per_image(out, idx, want):
    """max |out - want| per distinct image, after checking that the replicas of each are bit-identical."""
    errs = []
    for k in range(int(idx.max()) + 1):
        rows = np.flatnonzero(idx == k)
        first = out[rows[0]]
        for r in rows[1:]:
            assert np.array_equal(first.view(np.uint32), out[r].view(np.uint32)), f"image {r} is no copy of image {rows[0]}"
        errs.append(float(np.abs(first - want[k]).max()))
    return np.array(errs)


def _scales(kind, model):
    """what BAR is multiplied by, per distinct image: 1 on standard-normal data; max(1, max|model|) on the wide-range data;
    on the neighbours data the middle image is 100 x a standard-normal one (its errors scale with it), the others are not."""
    if kind == "wide":
        return np.full(3, max(1.0, float(np.abs(model).max())))
    if kind == "neighbours":
        return np.array([1.0, f8.NEIGHBOUR_SCALE, 1.0])
    return np.ones(3)


# ---- a. the weights' bytes ---------------------------------------------------------------------------------------------------
def _tiny_forward(e, cfg, seed):
    x, nl = synth.synth_unet_input(cfg, 1, 16, 16, seed)
    e.set_precision("f16f8")
    return e.unet_forward_np(x, nl.reshape(-1))


def _packed(w):
    """OIHW parameter -> packed rows with the input channels padded to a multiple of 32"""
    pad = (-w.shape[1]) % 32
    return f8.pack_weight(np.pad(w, ((0, 0), (0, pad), (0, 0), (0, 0))))


def _check_weight_bytes(e, name, w, own_k=None):
    packed = _packed(w)
    k = -int(np.round(np.log2(e.weight_unscale(name))))
    assert 2.0 ** -k == e.weight_unscale(name)
    if own_k is not None:
        assert k == own_k == f8.split_scale_exponent(packed), (name, k, own_k, f8.split_scale_exponent(packed))
    else:
        assert k <= f8.split_scale_exponent(packed)
    split = e.read_weight_layout(name, "split")
    want = f8.weight_split(packed, k)[3]
    assert split.size == want.size, (name, split.size, want.size)
    bad = np.flatnonzero(split != want)
    assert bad.size == 0, f"{name} [split]: {bad.size} of {want.size} bytes differ, first at {bad[0]}"
    got8, want8 = e.read_weight_layout(name, "f8"), f8.weight_f8c_bytes(split)
    bad = np.flatnonzero(got8 != want8)
    assert bad.size == 0, f"{name} [f8]: {bad.size} of {want8.size} bytes differ, first at {bad[0]} (byte {bad[0] % 128} of its chunk)"


def _crafted(shape, rs):
    """name -> (tensor, its own k): the value classes of the issue"""
    n = int(np.prod(shape))
    base = rs.standard_normal(shape).astype(np.float32)
    unit = base / np.abs(base).max()                                     # max|.| == 1 exactly
    out = {}
    out["max a power of two"] = (unit * np.float32(0.25), 12)            # 0.25 = 0.5 * 2^-1 -> k = 12, max * 2^k = 1024
    w = unit * np.float32(0.25)
    w[np.abs(w) == 0.25] = np.nextafter(np.float32(0.25), np.float32(0))
    out["max one ulp below a power of two"] = (w, 13)                    # hi = fp16(2047.9998) = 2048, hi / 8 = 256
    out["all zero"] = (np.zeros(shape, np.float32), 0)
    # hi * 2^-3 on e4m3 ties: (8 + m + 1/2) 2^E in the normal binades (both rounding directions), (m + 1/2) 2^-9 below them
    m = np.arange(8)
    ties = np.concatenate([(8 + m + 0.5) * 2.0 ** E for E in range(-9, 5)] + [(m + 0.5) * 2.0 ** -9])
    v = np.resize(ties * 8.0, n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)       # scaled units: max 1984 -> k = 11
    assert np.array_equal(v.astype(np.float16).astype(np.float64), v)
    out["e4m3 ties"] = ((v * 2.0 ** -11).astype(np.float32).reshape(shape), 11)
    w = (base * 10.0 ** rs.uniform(-12, -5, shape)).astype(np.float32)
    w.reshape(-1)[7] = 1.0                                               # k = 10; the rest: lo an fp16 subnormal or zero
    lo = f8.weight_split(_packed(w))[2]
    tiny = np.abs(lo.astype(np.float64)) < 2.0 ** -14
    assert tiny.mean() > 0.9 and (lo == 0).any() and ((lo != 0) & tiny).any()
    out["lo subnormal or zero"] = (w, 10)
    w = -np.abs(base) - np.float32(1e-3)
    out["negative throughout"] = (w, f8.split_scale_exponent(w))
    return out


@pytest.fixture(scope="module")
def config_d():
    """config D of the sweep after one f16f8 forward at B = 64, 32x32 (three distinct images): the engine (its F8C weight
    copies built), the inputs and the forward's output — shared by (a) and (e)."""
    cfg = synth.sweep_unet_config("D")
    sd = synth.synth_state_dict(cfg, 44)
    e = engine.Engine(cfg, 0)
    e.load_state_dict(sd)
    B = 64
    idx = cref.images(B)
    x, nl = synth.synth_unet_input(cfg, 3, 32, 32, 107)
    e.set_precision("f16f8")
    eps = e.unet_forward_np(x[idx], nl.reshape(-1)[idx])
    assert e.fallback_calls() == 0
    yield {"cfg": cfg, "sd": sd, "eng": e, "B": B, "idx": idx, "x": x, "nl": nl.reshape(-1), "eps": eps}
    e.close()


def test_weight_bytes(config_d):
    e, sd, cfg = config_d["eng"], config_d["sd"], config_d["cfg"]
    names = [n for n, _ in e.param_list() if e.read_weight_layout(n, "f8") is not None]
    paired = [n for n in names if n.endswith("block2.block.3.weight")]
    assert len(names) >= 10 and paired, names
    resplit = 0
    for n in names:
        own = n.endswith("block1.block.3.weight")                     # (conv2 / res_conv share the smaller k of the two)
        _check_weight_bytes(e, n, sd[n], f8.split_scale_exponent(sd[n]) if own else None)
        resplit += -np.log2(e.weight_unscale(n)) < f8.split_scale_exponent(sd[n])
    print(f"config D: {len(names)} F8C weight tensors bit for bit ({resplit} of them re-split to a common k)")
    name = next(n for n in names if n.endswith("block1.block.3.weight"))
    for what, (w, k) in _crafted(sd[name].shape, np.random.RandomState(107)).items():
        e.load_weight(name, w)
        _tiny_forward(e, cfg, 1)                                      # (rebuilds the F8C copies)
        try:
            _check_weight_bytes(e, name, w, k)
        except AssertionError as err:
            raise AssertionError(f"crafted tensor '{what}': {err}") from None
        print(f"  crafted '{what}': k = {k}, bit for bit")
    e.load_weight(name, sd[name])


# ---- b. the conv against the model ----------------------------------------------------------------------------------------------
def test_case_list_plans_f8c(eng):
    for B, H, W, C0, C1, Cout in f8.CASES:
        assert eng.conv_f8_supported(B, H, W, Cout, C0 + C1), (B, H, W, C0, C1, Cout)


@pytest.mark.parametrize("kind", f8.KINDS)
@pytest.mark.parametrize("case", f8.CASES, ids=f8.case_id)
def test_conv_against_model(eng, case, kind):
    B, H, W, C0, C1, Cout = case
    d = f8.case_data(case, kind)
    idx = d["idx"]
    model, exact = f8.case_refs(case, kind)
    x1 = None if d["x1"] is None else d["x1"][idx]
    got = _f8(eng, eng.op_conv2d, d["x0"][idx], d["w"], d["b"], x1=x1)          # (a range error would raise here)
    again = _f8(eng, eng.op_conv2d, d["x0"][idx], d["w"], d["b"], x1=x1)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "a second call gave other bytes"
    em, ee = _per_image(got, idx, model), _per_image(got, idx, exact)
    bar, sc = f8.bar(case), _scales(kind, model)
    print(f"{f8.case_id(case)} [{kind}]: BAR {bar:.2e} x {sc}  |gpu - model| {em}  |gpu - exact| {ee}  max|model| {np.abs(model).max():.3g}")
    assert bar <= f8.BAR_LIMIT
    assert np.all(em <= bar * sc), f"|gpu - model| = {em} over BAR = {bar:.2e} x {sc}"
    assert ee.max() >= 4 * em.max(), f"the model does not explain the kernel's error: |gpu - exact| {ee.max():.2e}, |gpu - model| {em.max():.2e}"


# ---- c. epilogue and fused launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [f8.CASES[1], f8.CASES[3]], ids=f8.case_id)
def test_epilogue_and_statistics(eng, case):
    d = f8.case_data(case)
    idx = d["idx"]
    model, exact = f8.case_refs(case)
    add = d["cb"].astype(np.float64)[:, None, None, :] + d["resid"].astype(np.float64)
    x1 = None if d["x1"] is None else d["x1"][idx]
    out, st = _f8(eng, eng.op_conv2d, d["x0"][idx], d["w"], d["b"], x1=x1, chan_bias=d["cb"][idx], resid=d["resid"][idx],
                  return_stats=True)
    em, ee = _per_image(out, idx, model + add), _per_image(out, idx, exact + add)
    print(f"{f8.case_id(case)} bias + chan_bias + resid: BAR {f8.bar(case):.2e}  |gpu - model| {em}  |gpu - exact| {ee}")
    assert em.max() <= f8.bar(case)
    assert ee.max() >= 4 * em.max()
    _check_stats(st, out)
    print()


FUSED = [((64, 32, 32, 32, 128), (64, 0)), ((128, 16, 16, 64, 256), (96, 32)), ((64, 32, 32, 128, 128), "ident")]


@pytest.mark.parametrize("shape,term", FUSED, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_fused_launch(eng, shape, term):
    assert engine.conv_plan(*shape, precision="f16f8", stats=True)["kernel"] == "halo_f8c"
    d = cref.case_data(shape, term, resid=term != "ident")
    idx = d["idx"]
    pick = lambda a: None if a is None else a[idx]
    t = {"in2": d["in2"], "in2b": d["in2b"], "w2": d["w2"], "b2": d["b2"]}
    model = f8.conv_f8c_model(d["x"], d["w"], d["b"], chan_bias=d["cb"], resid=d["resid"], term=t)
    bar = f8.BAR_FACTOR * f8.chain_roundoff(d["x"], d["w"], term=t)
    r = _f8(eng, eng.op_conv2d_fused, d["x"][idx], d["w"], d["b"], chan_bias=d["cb"][idx], resid=pick(d["resid"]),
            in2=pick(d["in2"]), in2b=pick(d["in2b"]), w2=d["w2"], b2=d["b2"], ident=term == "ident", twin=True)
    em, ee = _per_image(r["out"], idx, model), _per_image(r["out"], idx, d["want"])
    print(f"fused {shape} {term}: BAR {bar:.2e}  |gpu - model| {em}  |gpu - exact| {ee}")
    assert bar <= f8.BAR_LIMIT
    assert em.max() <= bar
    assert ee.max() >= 4 * em.max()
    assert np.array_equal(r["twin"], gn.pack_format(r["out"], 1)), "the twin is not hi = fp16(out), lo = fp16(out - hi)"
    _check_stats(r["stats"], r["out"])
    print()


# ---- d. behind GroupNorm + Swish ------------------------------------------------------------------------------------------------
def test_behind_groupnorm_swish(eng):
    """test_conv2d_f16f8_fused_prologue_epilogue's shape. op_conv2d's pass applies the (scale, shift) it is handed; no entry
    point returns that pass's fp32 g (op_groupnorm_apply derives scale and shift itself, from gamma and beta), so g is
    swish(x * scale + shift) in float64 from the device's own scale and shift, rounded to fp32, and this one case's bar is
    widened by the CPU-measured shift of the model when every g moves by +-1 fp32 ulp with random signs (printed)."""
    rs = np.random.RandomState(5)
    B, H, W, C, Cout = 64, 16, 16, 128, 512
    idx = cref.images(B)
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    x = f32(3, H, W, C) * 2 + 0.5
    gamma, beta = 1 + 0.1 * f32(C), 0.1 * f32(C)
    w, b = f32(Cout, C, 3, 3) / np.float32(np.sqrt(9 * C)), f32(Cout)
    cb, resid = f32(3, Cout), f32(3, H, W, Cout)
    sc, sh = eng.op_groupnorm_affine(x, gamma, beta, 32)
    y = x.astype(np.float64) * sc.astype(np.float64)[:, None, None, :] + sh.astype(np.float64)[:, None, None, :]
    g64 = y / (1.0 + np.exp(-y))
    g = g64.astype(np.float32)
    ulp = np.spacing(np.abs(g)) * np.where(rs.randint(0, 2, g.shape), 1, -1).astype(np.float32)
    model = f8.conv_f8c_model(g, w, b, chan_bias=cb, resid=resid)
    shift = float(np.abs(f8.conv_f8c_model(g + ulp, w, b, chan_bias=cb, resid=resid) - model).max())
    bar = f8.BAR_FACTOR * f8.chain_roundoff(g, w)
    exact = cref.conv3x3_f64(g64, w) + b.astype(np.float64) + cb.astype(np.float64)[:, None, None, :] + resid.astype(np.float64)
    got = _f8(eng, eng.op_conv2d, x[idx], w, b, gn_scale=sc[idx], gn_shift=sh[idx], swish=True, chan_bias=cb[idx], resid=resid[idx])
    em, ee = _per_image(got, idx, model), _per_image(got, idx, exact)
    print(f"behind GroupNorm + Swish: BAR {bar:.2e} + the +-1 ulp shift of g {shift:.2e}  |gpu - model| {em}  |gpu - exact| {ee}")
    assert bar <= f8.BAR_LIMIT
    assert em.max() <= bar + shift
    assert ee.max() >= 4 * em.max()


# ---- e. one forward -----------------------------------------------------------------------------------------------------------
def test_forward_against_the_f8c_oracle(config_d):
    """config D at B = 64, 32x32: the oracle with F.conv2d replaced, for exactly the convs conv_plan(...)["f8"] names, by
    the model's operand formats (emulate_operand_formats.ConvProxy("f8c")). Bar: the 1e-4 of the f32 and f16x3 forwards."""
    import emulate_operand_formats as emu
    import torch.nn.functional as F
    aten = emu.aten
    cfg, B = config_d["cfg"], config_d["B"]
    taken = []

    def f8c_convs(H, W, Cin, Cout, ks, stride, up2):
        if up2:
            took = engine.conv_plan(B, H // 2, W // 2, Cin, Cout, ks, stride, 1, precision="f16f8", stats=True)["f8"]
        else:
            took = engine.conv_plan(B, H, W, Cin, Cout, ks, stride, 0, precision="f16f8", stats=True)["f8"]
        taken.append(((H, W, Cin, Cout), took))
        return took

    tsd = aten.to_torch_state(config_d["sd"])
    tx, tnl = torch.from_numpy(config_d["x"]), torch.from_numpy(config_d["nl"])
    with torch.no_grad():
        plain = aten.unet_forward(tsd, cfg, tx, tnl).numpy()
        aten.F = emu.ConvProxy("f8c", f8c_convs)
        try:
            want = aten.unet_forward(tsd, cfg, tx, tnl).numpy()
        finally:
            aten.F = F
    n8 = sum(t for _, t in taken)
    assert n8 >= 8, taken
    e8, ep = _per_image(config_d["eps"], config_d["idx"], want), _per_image(config_d["eps"], config_d["idx"], plain)
    print(f"config D forward, B = {B}, 32x32, {n8} of {len(taken)} 3x3 convs on the fp8 path: vs the f8c oracle {e8.max():.2e} "
          f"(bar 1e-4), vs the plain oracle {ep.max():.2e}")
    assert e8.max() < 1e-4
