"""The fused GroupNorm statistics of the conv epilogues (ConvParams::stats), one case per (precision, kernel, split form,
phases, ks / stride) class that can emit them, through sr3_op_conv2d_stats: the conv runs as the engine runs it, with the
statistics offered, so the dispatch plan is conv_plan(..., stats=True).

Per case:
  0. (CPU side) the plan of the shape is in the class the case is meant for; a dispatch change fails here.
  1. out against a float64 conv (+ bias + FeatureWiseAffine bias + residual) at the bars the suite holds these ops to:
     2e-5 plain, 3e-5 behind a GroupNorm + Swish prologue (test_gpu_ops.py), 2e-4 on the F8C kernel (test_gpu_f16f8.py).
  2. no NaN sentinel left anywhere in [B][slices][Cout][2] (the entry point fills the buffer with 0xFF bytes first).
  3. per (image, channel): the slices add up to the fp64 sum / sum of squares of THAT CALL'S OWN stored f32 `out`, to
     1e-9 of sum|v| resp. sum v^2 (the kernels add the stored f32 value in fp64: only the order differs, N * 2^-53 <=
     1.5e-11 for N <= 2^17 terms). Not circular: 1. pins `out` itself.
  4. where sr3_internal.h documents the layout, the same per slice: slice = tile_m consecutive pixels (unsplit and
     in-place split kernels), HWo / slices consecutive pixels (conv + reduce). Not for the Winograd forms and the
     4-phase launches.
  5. chain: the partials go to sr3_op_groupnorm_apply (route 0, mode 2, format 0) with `out`; against float64
     swish(group_norm(float64 conv)) at 3e-5. (Not for Cout = 3: the apply pass takes channels in multiples of 8, and no
     GroupNorm follows the UNet's final conv.)

bias, chan_bias and resid are present in every case (a statistic taken before one of them is off by O(1) per pixel).
Large batches repeat three distinct images (first, middle and last image differ), so the float64 conv runs on three.
"""
import numpy as np
import pytest

import gn_stats_ref as ref
from conftest import pkg

synth = pkg("synth")
engine = pkg("engine")


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(synth.tiny_unet_config(), 0)
    e.load_state_dict(synth.synth_state_dict(e.cfg, 11))
    yield e
    e.set_precision("f32")
    e.close()


# (precision, (B, H, W, Cin, Cout[, ks, stride, up2]), kernel, split, phases, GroupNorm + Swish prologue)
# Shapes: the smallest conv_plan confirms for the class, B >= 2 throughout, more than one slice per image where the
# class allows it (HWo = 128 on 64-row tiles, 1024 / 256 on 128-row tiles).
G64, G12832, G12864, G128128 = "generic_64x64", "generic_128x32", "generic_128x64", "generic_128x128"
GENERIC = [
    # unsplit 64x64 tile: 3x3 | 1x1 | stride 2 | upsample (4 phases in one launch)
    ((2, 16, 8, 32, 64), G64, "none", 1),
    ((2, 16, 8, 64, 64, 1), G64, "none", 1),
    ((2, 32, 16, 32, 64, 3, 2), G64, "none", 1),
    ((2, 16, 8, 32, 64, 3, 1, 1), G64, "none", 4),
    ((2, 16, 16, 32, 3), G12832, "none", 1),                 # Cout = 3: masked columns
    # in-place split-K (the last block of a tile adds the partials and runs the epilogue)
    ((2, 16, 8, 128, 64), G64, "inplace", 1),
    ((2, 16, 8, 128, 64, 1), G64, "inplace", 1),
    ((2, 16, 8, 128, 64, 3, 1, 1), G64, "inplace", 4),
    ((2, 32, 16, 128, 64, 3, 2), G64, "inplace", 1),
    # conv + reduce kernel (HWo = 24: no whole 64-row tile per image; one pixel per slice) and HWo = 160 (two per slice)
    ((2, 4, 6, 128, 256), G64, "reduce", 1),
    ((2, 10, 16, 128, 64), G64, "reduce", 1),
    ((2, 4, 6, 256, 256, 1), G64, "reduce", 1),
    ((2, 4, 6, 128, 64, 3, 1, 1), G64, "reduce", 4),
    ((2, 8, 12, 128, 128, 3, 2), G64, "reduce", 1),
    # 128-row tiles need 512 blocks: M = 65536 pixels
    ((64, 32, 32, 32, 64, 1), G12864, "none", 1),
    ((64, 32, 32, 32, 128, 1), G128128, "none", 1),
]
CASES = [("f32", s, k, sp, ph, False) for s, k, sp, ph in GENERIC] + [
    ("f32", (64, 32, 32, 32, 64), G12864, "none", 1, False),
    ("f32", (64, 32, 32, 32, 128), G128128, "none", 1, False),
    ("f32", (16, 16, 16, 128, 64), "wino_three_pass", "none", 1, False),
    ("f32", (16, 16, 16, 128, 128), "wino_three_pass", "none", 1, True),      # U written by the GroupNorm pass (u_ready)
    ("f32", (32, 64, 64, 64, 64), "wino_one_pass", "none", 1, False),
] + [("f16x3", s, k, sp, ph, False) for s, k, sp, ph in GENERIC] + [
    ("f16x3", (64, 32, 32, 32, 64), "halo_128x64", "none", 1, False),
    ("f16x3", (64, 32, 32, 32, 128), "halo_128x128_seg32", "none", 1, False),
    ("f16x3", (32, 32, 32, 32, 256, 3, 1, 1), "halo_128x128_seg32", "none", 4, False),
    ("f16x3", (512, 16, 16, 32, 128), "halo_128x128_seg8", "none", 1, False),
    ("f16x3", (128, 16, 16, 32, 256, 3, 1, 1), "halo_128x128_seg8", "none", 4, False),
    ("f16x3", (32, 8, 8, 256, 512), "halo_128x128_seg8", "inplace_halo", 1, True),
    ("f16f8", (128, 16, 16, 32, 256), "halo_f8c", "none", 1, False),
    ("f16f8", (128, 16, 16, 64, 256), "halo_f8c", "none", 1, True),
]


def _full(shape):
    return tuple(shape) + (3, 1, 0)[len(shape) - 5:]


def _id(case):
    prec, shape, kernel, split, phases, gn = case
    return f"{prec}-{kernel}-{split}-ph{phases}-" + "x".join(map(str, shape)) + ("-gn" if gn else "")


def conv64(x, w, stride):
    """float64 nn.Conv2d(k, padding=k//2, stride) on NHWC x, w OIHW."""
    x, w = x.astype(np.float64), w.astype(np.float64)
    B, H, W, C = x.shape
    O, _, k, _ = w.shape
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    out = np.zeros((B * Ho * Wo, O))
    for dy in range(k):
        for dx in range(k):
            patch = xp[:, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride, :]
            out += np.ascontiguousarray(patch).reshape(-1, C) @ w[:, :, dy, dx].T
    return out.reshape(B, Ho, Wo, O)


def _images(B):
    """index of the distinct image behind each batch entry: all distinct up to 3, else 3 repeated with first, middle and
    last different"""
    if B <= 3:
        return np.arange(B)
    idx = np.arange(B) % 3
    idx[0], idx[B // 2], idx[-1] = 0, 1, 2
    return idx


def test_case_list_reaches_every_emitting_class():
    """CPU side of the list: every case is in its class (also asserted per case), and together they reach every kernel
    and split form of the plan."""
    kernels, splits = set(), set()
    for prec, shape, kernel, split, phases, gn in CASES:
        d = engine.conv_plan(*_full(shape), precision=prec, stats=True)
        assert (d["kernel"], d["split"], d["phases"]) == (kernel, split, phases) and d["stats_slices"] > 0, (_id((prec, shape, kernel, split, phases, gn)), d)
        kernels.add(kernel)
        splits.add(split)
    assert kernels == {"wino_one_pass", "wino_three_pass", "halo_f8c", "halo_128x128_seg32", "halo_128x128_seg8", "halo_128x64",
                       G12832, G12864, G64, G128128}
    assert splits == {"none", "reduce", "inplace", "inplace_halo"}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_conv_statistics(eng, case):
    prec, shape, kernel, split, phases, gn = case
    B, H, W, Cin, Cout, ks, stride, up2 = _full(shape)
    plan = engine.conv_plan(B, H, W, Cin, Cout, ks, stride, up2, precision=prec, stats=True)
    assert (plan["kernel"], plan["split"], plan["phases"]) == (kernel, split, phases) and plan["stats_slices"] > 0, plan
    slices, tile_m = plan["stats_slices"], plan["tile"][0]

    rs = np.random.RandomState(sum(shape) + len(prec))
    idx = _images(B)
    nd = int(idx.max()) + 1
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    xd = f32(nd, H, W, Cin)
    if gn:
        xd = xd * 2 + 0.5
    w = f32(Cout, Cin, ks, ks) / np.float32(np.sqrt(Cin * ks * ks))
    b, cbd = f32(Cout), f32(nd, Cout)
    Hv, Wv = (2 * H, 2 * W) if up2 else (H, W)
    Ho, Wo = (Hv + 2 * (ks // 2) - ks) // stride + 1, (Wv + 2 * (ks // 2) - ks) // stride + 1
    rd = f32(nd, Ho, Wo, Cout)
    gamma, beta = 1 + 0.1 * f32(Cin), 0.1 * f32(Cin)

    kw = {}
    eng.set_precision("f32")
    if gn:
        sc, sh = eng.op_groupnorm_affine(xd, gamma, beta, 32)
        kw = dict(gn_scale=sc[idx], gn_shift=sh[idx], swish=True)
    eng.set_precision(prec)
    try:
        out, st = eng.op_conv2d(xd[idx], w, b, stride=stride, up2=bool(up2), chan_bias=cbd[idx], resid=rd[idx], return_stats=True, **kw)
    finally:
        eng.set_precision("f32")

    # 1. the output itself
    xin = ref.group_norm64(xd, gamma, beta, 32, swish=True) if gn else xd.astype(np.float64)
    if up2:
        xin = xin.repeat(2, axis=1).repeat(2, axis=2)
    want = conv64(xin, w, stride) + b.astype(np.float64) + cbd[:, None, None, :].astype(np.float64) + rd
    bar = 2e-4 if kernel == "halo_f8c" else 3e-5 if gn else 2e-5
    err = max(np.abs(out[idx == k] - want[k]).max() for k in range(nd))
    print(f"{_id(case)}: conv err {err:.2e} (bar {bar:.0e})", end="")
    assert out.shape == (B, Ho, Wo, Cout)
    assert err < bar

    # 2. every slice written
    assert st is not None and st.shape == (B, slices, Cout, 2)
    assert not np.isnan(st).any(), f"{int(np.isnan(st).any(axis=(2, 3)).sum())} of {B * slices} (image, slice) rows hold a NaN sentinel"

    # 3. totals per (image, channel) against the call's own stored output
    HWo = Ho * Wo
    v = out.reshape(B, HWo, Cout).astype(np.float64)
    tol1, tol2 = 1e-9 * np.abs(v).sum(1), 1e-9 * (v * v).sum(1)
    d1, d2 = np.abs(st[..., 0].sum(1) - v.sum(1)), np.abs(st[..., 1].sum(1) - (v * v).sum(1))
    print(f"  totals: S1 {np.max(d1 / np.abs(v).sum(1)):.1e} S2 {np.max(d2 / (v * v).sum(1)):.1e} (rel, bar 1e-9)", end="")
    assert np.all(d1 <= tol1) and np.all(d2 <= tol2)

    # 4. per slice, where the layout is documented
    if phases == 1 and not kernel.startswith("wino"):
        per = HWo // slices
        assert per * slices == HWo and (split == "reduce" or per == tile_m or (split == "inplace_halo" and slices == 1))
        vs = v.reshape(B, slices, per, Cout)
        e1 = np.abs(st[..., 0] - vs.sum(2)) / np.abs(vs).sum(2)
        e2 = np.abs(st[..., 1] - (vs * vs).sum(2)) / (vs * vs).sum(2)
        print(f"  slices of {per} px: S1 {e1.max():.1e} S2 {e2.max():.1e}", end="")
        assert e1.max() <= 1e-9 and e2.max() <= 1e-9

    # 5. the consumer behind it
    if Cout % 8 == 0:
        g2, b2 = 1 + 0.1 * f32(Cout), 0.1 * f32(Cout)
        groups = 32 if Cout % 32 == 0 else 8
        r = eng.op_groupnorm_apply(out, g2, b2, groups, stats0=st, mode=2, fmt=0, route=0)
        act = ref.group_norm64(want, g2, b2, groups, swish=True)
        cerr = max(np.abs(r["out"][idx == k] - act[k]).max() for k in range(nd))
        print(f"  chain (route {r['route']}) err {cerr:.2e} (bar 3e-5)", end="")
        assert not r["range_flag"]
        assert cerr < 3e-5
    print()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_ragged_shape_reports_no_slices_and_the_same_output(eng, prec):
    """HWo = 240 is no multiple of the 64-row tile: the plan has no fused statistics, the conv runs without them."""
    B, H, W, Cin, Cout = 3, 12, 20, 64, 96
    assert engine.conv_plan(B, H, W, Cin, Cout, precision=prec, stats=True)["stats_slices"] == 0
    rs = np.random.RandomState(7)
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    x, w, b, cb, resid = f32(B, H, W, Cin), f32(Cout, Cin, 3, 3) / 24, f32(Cout), f32(B, Cout), f32(B, H, W, Cout)
    eng.set_precision(prec)
    try:
        out, st = eng.op_conv2d(x, w, b, chan_bias=cb, resid=resid, return_stats=True)
        plain = eng.op_conv2d(x, w, b, chan_bias=cb, resid=resid)
    finally:
        eng.set_precision("f32")
    assert st is None
    assert np.array_equal(out.view(np.uint32), plain.view(np.uint32))
    want = conv64(x, w, 1) + b.astype(np.float64) + cb[:, None, None, :].astype(np.float64) + resid
    assert np.abs(out - want).max() < 2e-5
