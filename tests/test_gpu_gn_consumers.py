"""The consumers of the fused GroupNorm statistics, independent of any conv, through sr3_op_groupnorm_apply: the fold in
the apply pass's prologue (gn_scale_shift_to_lds), gn_finalize_kernel / gn_finalize_group_kernel + the streaming
gn_apply_rows_kernel, the statistics-kernel fallback, the three output formats, the raw side output, split-f16 inputs and
the range flag.

The partials are built in numpy, in fp64, from x itself: the pixels of an image split into `slices` contiguous chunks of
unequal length, a different number for each half of a concatenation. Reference: float64 GroupNorm (+ Swish) of x. Data as
in test_gpu_ops.py::test_groupnorm_affine (x0 = 3 N(0,1) + 10, x1 = N(0,1) - 4: E[x^2] - mean^2 cancels 3-4 digits), bars
as there and in test_conv2d_fused_prologue_epilogue: 2e-5 affine, 3e-5 affine + Swish.

Branches (GA_T = 512 threads per block of the folded pass, 256 of the others; see the table at CASES):
  fold prologue       L = 512 / min(C, 512) slice lanes per channel; 8-deep body needs slices > 7 L
  gn_finalize_group   B * 4 < 128, max slices >= 16, Cg <= 64; 256 / Cg lanes; 8-deep body needs slices > 7 lanes
  gn_finalize         otherwise; grid y = 4, or 1 where groups % 4; 4-deep body needs slices > 3 lanes
  route 0             finalize + rows iff B * 4 < 128 and max slices >= 64 (or a pass over 200 MB: not reached here)
"""
import numpy as np
import pytest

import gn_stats_ref as ref
from conftest import pkg

synth = pkg("synth")
engine = pkg("engine")

FOLDED, ROWS = 1, 2


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(synth.tiny_unet_config(), 0)
    e.load_state_dict(synth.synth_state_dict(e.cfg, 11))
    yield e
    e.close()


# name: (B, H, W, C0, C1, groups, slices0, slices1, route 0 takes)
CASES = {
    # Cg = 3 (real in the UNet: 96 channels in 32 groups), group 10 = channels 30..32 straddles x || skip. Route 2: group
    # finalize with 85 lanes (tail only); rows NR = 2, W * C / 8 = 120 items: one ragged block. Fold: L = 5, slices 100 =
    # body + tail, 7 = tail only; 2 blocks of 50 pixels on 42 pixel lanes: 2 (loop only) or 1 (tail only) per lane.
    "cg3_straddle": (2, 10, 10, 32, 64, 32, 100, 7, ROWS),
    # Cg = 64 (the group kernel's limit), group 1 = channels 64..127 straddles. Group finalize with 4 lanes: slices 100 =
    # 8-deep body + tail, 7 = tail only. H odd: rows NR = 1; 13 * 24 = 312 items: two blocks, the last ragged.
    "cg64_straddle_h_odd": (2, 9, 13, 96, 96, 3, 7, 100, ROWS),
    # B = 32: route 0 folds (B * 4 = 128); route 2 runs gn_finalize_kernel on grid y = 4 with 32 lanes: slices 256 / 100 =
    # 4-deep body + tail. Fold: L = 5, 256 = body + tail. 3 blocks of 86, 86, 84 pixels (HW no multiple of the block), 42
    # pixel lanes: 3 (loop + tail) or 2 per lane.
    "b32_finalize_y4": (32, 16, 16, 32, 64, 32, 256, 100, FOLDED),
    # groups % 4 != 0 and fewer than 16 slices: gn_finalize_kernel on its single-y grid (85 lanes: tail only)
    "groups3_single_y": (2, 8, 8, 96, 96, 3, 7, 1, FOLDED),
    # Cg = 1, C0 = 8 (one channel octet before the boundary), HW = 35 odd: one pixel per lane
    "cg1": (3, 5, 7, 8, 24, 32, 7, 1, FOLDED),
    # C = 2048 at 4x4: the fold's dynamic LDS is 57 KB (> 48 KB: the attribute branch), 4 channel passes of 512 in the
    # prologue with L = 1: slices 7 = tail only; rows: 1024 items = 4 whole blocks
    "wide_lds": (2, 4, 4, 1024, 1024, 32, 7, 1, FOLDED),
    # C = 2048, L = 1, 100 slices: 8-deep body (12 rounds) + tail of 4; group finalize (Cg = 64); H odd
    "wide_many_slices": (1, 5, 20, 1024, 1024, 32, 100, 7, ROWS),
    # one source, 64 channels
    "single_source": (2, 12, 12, 64, 0, 32, 100, 0, ROWS),
}


def fold_geometry(B, HW, C):
    """(pixels per block, blocks, pixel lanes, set of pixels-per-lane counts) of the folded apply (launch_gn_apply_impl)."""
    C8 = C // 8
    P = max(1, min(-(-1024 // B), -(-HW * C8 // 1024)))
    ppb = -(-HW // P)
    rows = 512 // min(C8, 512)
    blocks = -(-HW // ppb)
    counts = set()
    for n in {ppb, HW - (blocks - 1) * ppb}:
        counts |= {-(-(n - pl) // rows) for pl in range(min(rows, n))}
    return ppb, blocks, rows, counts


def test_cases_reach_the_branches():
    """CPU side: the geometry the comments at CASES claim (a change of the launch heuristics that moves a case off its
    branch fails here)."""
    geo = {k: fold_geometry(v[0], v[1] * v[2], v[3] + v[4]) for k, v in CASES.items()}
    assert any(v[1] * v[2] % geo[k][0] for k, v in CASES.items())                        # HW no multiple of pixels per block
    counts = set().union(*(g[3] for g in geo.values()))
    assert 1 in counts and 2 in counts and 3 in counts                                   # tail only | loop only | loop + tail
    for k, (B, H, W, C0, C1, groups, s0, s1, r0) in CASES.items():
        many = B * 4 < 128 and max(s0, s1) >= 64
        assert r0 == (ROWS if many else FOLDED), k
        assert 8.0 * B * H * W * (C0 + C1) < 200e6
    lds = lambda C, groups: 2 * C * 4 + (C + 512) * 16 + 2 * groups * 4
    assert lds(2048, 32) > 48 * 1024 > lds(192, 3)
    assert {v[1] % 2 for v in CASES.values()} == {0, 1}                                  # rows NR = 2 and NR = 1
    assert any((v[2] * (v[3] + v[4]) // 8) % 256 for v in CASES.values())                # ragged last block of the rows kernel


def _data(name, split0=False, split1=False):
    """x0, x1 (float32, or their split-f16 words), float64 values of both, partials, gamma, beta."""
    B, H, W, C0, C1, groups, s0, s1, _ = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    f32 = lambda *s: rs.standard_normal(s).astype(np.float32)
    x0 = f32(B, H, W, C0) * 3 + 10
    x1 = f32(B, H, W, C1) - 4 if C1 else None
    gamma, beta = 1 + 0.1 * f32(C0 + C1), 0.1 * f32(C0 + C1)
    v0, v1 = x0.astype(np.float64), None if x1 is None else x1.astype(np.float64)
    if split0:
        x0 = ref.pack_format(x0, 1)
        v0 = np.add(*ref.split_halves(x0))
    if split1:
        x1 = ref.pack_format(x1, 1)
        v1 = np.add(*ref.split_halves(x1))
    p0 = ref.partials(v0, ref.chunk_bounds(rs, H * W, s0))
    p1 = ref.partials(v1, ref.chunk_bounds(rs, H * W, s1)) if C1 else None
    v = v0 if v1 is None else np.concatenate([v0, v1], -1)
    return x0, x1, v, p0, p1, gamma, beta, groups


BARS = {1: 2e-5, 2: 3e-5}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_partials_to_activation(eng, name):
    """Routes 1 and 2 in both modes, and route 0 taking the form run_gn_act takes."""
    x0, x1, v, p0, p1, gamma, beta, groups = _data(name)
    want = {m: ref.group_norm64(v, gamma, beta, groups, swish=(m == 2)) for m in (1, 2)}
    for route in (FOLDED, ROWS, 0):
        for mode in (1, 2):
            r = eng.op_groupnorm_apply(x0, gamma, beta, groups, x1=x1, stats0=p0, stats1=p1, mode=mode, fmt=0, route=route)
            err = np.abs(r["out"] - want[mode]).max()
            print(f"{name}: route {route} -> {r['route']} mode {mode}: {err:.2e} (bar {BARS[mode]:.0e})")
            assert r["route"] == (route or CASES[name][8])
            assert not r["range_flag"]
            assert err < BARS[mode]
    r = eng.op_groupnorm_apply(x0, gamma, beta, groups, x1=x1, stats0=p0, stats1=p1, mode=0, fmt=0, route=FOLDED)
    assert np.array_equal(r["out"], v.astype(np.float32))               # mode 0: the concatenation itself


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cg3_straddle", "cg64_straddle_h_odd", "single_source", "wide_lds"])
def test_statistics_kernel_fallback(eng, name):
    """No partials: gn_partial_kernel's (the concatenation as ONE source) feed either form; route 0 folds."""
    x0, x1, v, _, _, gamma, beta, groups = _data(name)
    want = ref.group_norm64(v, gamma, beta, groups, swish=True)
    for route in (0, FOLDED, ROWS):
        r = eng.op_groupnorm_apply(x0, gamma, beta, groups, x1=x1, mode=2, fmt=0, route=route)
        err = np.abs(r["out"] - want).max()
        print(f"{name}: fallback route {route} -> {r['route']}: {err:.2e} (bar 3e-5)")
        assert r["route"] == (route or FOLDED) and not r["range_flag"]
        assert err < 3e-5


# C0 = 32, C1 = 64 (whole 32-channel chunks on both sides), 10x10 and 9x13: rows NR = 2 and NR = 1
FORMAT_CASES = ["cg3_straddle", "cg64_straddle_h_odd"]


@pytest.mark.gpu
@pytest.mark.parametrize("route", [FOLDED, ROWS])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", FORMAT_CASES)
def test_output_formats_bitwise(eng, name, mode, route):
    """Formats 1 and 2 hold, bit for bit, what the numpy restatement of store8 makes of the SAME route's and mode's
    format-0 output; `raw` holds the packed input (format 1 for both, fp32 bits in format 0)."""
    x0, x1, v, p0, p1, gamma, beta, groups = _data(name)
    call = lambda fmt: eng.op_groupnorm_apply(x0, gamma, beta, groups, x1=x1, stats0=p0, stats1=p1, mode=mode, fmt=fmt, route=route,
                                              want_raw=True)
    base = call(0)
    x = np.concatenate([x0, x1], -1)
    assert np.abs(base["out"]).max() < 448 and np.abs(x).max() < 448
    assert np.array_equal(base["raw"].view(np.uint32), x.view(np.uint32))
    for fmt in (1, 2):
        r = call(fmt)
        assert r["route"] == route and not r["range_flag"]
        want = ref.pack_format(base["out"], fmt)
        diff = np.argwhere(r["out"] != want)
        for i in map(tuple, diff[:4]):       # (word c of a pixel: chunk c // 32; halfs 2c, 2c + 1 of the chunk's 64 in format 1)
            print(f"{name} mode {mode} route {route} format {fmt}: word {i} got {r['out'][i]:#010x} want {want[i]:#010x}")
        assert len(diff) == 0, f"format {fmt}: {len(diff)} of {want.size} words differ from the packed format-0 output"
        assert np.array_equal(r["raw"], ref.pack_format(x, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("route", [FOLDED, ROWS])
@pytest.mark.parametrize("in_split", [1, 2, 3])
def test_split_inputs(eng, in_split, route):
    """An input stored as hi | lo halfs is read as hi + lo: against the float64 reference of exactly those values."""
    name = "cg64_straddle_h_odd" if in_split == 3 else "cg3_straddle"
    x0, x1, v, p0, p1, gamma, beta, groups = _data(name, split0=bool(in_split & 1), split1=bool(in_split & 2))
    want = ref.group_norm64(v, gamma, beta, groups, swish=True)
    r = eng.op_groupnorm_apply(x0, gamma, beta, groups, x1=x1, stats0=p0, stats1=p1, mode=2, fmt=0, in_split=in_split, route=route,
                               want_raw=True)
    err = np.abs(r["out"] - want).max()
    print(f"in_split {in_split} route {route}: {err:.2e} (bar 3e-5)")
    assert not r["range_flag"]
    assert err < 3e-5
    assert np.array_equal(r["raw"], v.astype(np.float32))        # hi + lo is exact in fp32 (it was split from one)


@pytest.mark.gpu
@pytest.mark.parametrize("route", [FOLDED, ROWS])
def test_range_flag(eng, route):
    """One value beyond the fp16 range raises the flag in format 1 (and 2), one beyond e4m3's 448 only in format 2, none
    in format 0; mode 0, so the value reaches the store as it is."""
    x0, x1, v, p0, p1, gamma, beta, groups = _data("cg3_straddle")
    flag = lambda x, fmt: eng.op_groupnorm_apply(x, gamma, beta, groups, x1=x1, stats0=p0, stats1=p1, mode=0, fmt=fmt,
                                                 route=route)["range_flag"]
    big, mid = x0.copy(), x0.copy()
    big[1, 7, 3, 21] = 7e4
    mid[1, 7, 3, 21] = -500.0
    assert [flag(big, f) for f in (0, 1, 2)] == [False, True, True]
    assert [flag(mid, f) for f in (0, 1, 2)] == [False, False, True]
    assert [flag(x0, f) for f in (0, 1, 2)] == [False, False, False]
    x1b = x1.copy()
    x1b[0, 0, 9, 63] = 500.0                                       # ... and in the second source's last channel
    r = eng.op_groupnorm_apply(x0, gamma, beta, groups, x1=x1b, stats0=p0, stats1=p1, mode=0, fmt=2, route=route)
    assert r["range_flag"]


@pytest.mark.gpu
def test_argument_errors(eng):
    x0, x1, v, p0, p1, gamma, beta, groups = _data("cg3_straddle")
    Sr3Error = pkg("_lib").Sr3Error
    with pytest.raises(Sr3Error):
        eng.op_groupnorm_apply(x0, gamma, beta, groups, x1=x1, stats0=p0)            # partials of one half only
    with pytest.raises(Sr3Error):
        eng.op_groupnorm_apply(x0, gamma, beta, 7, x1=x1, stats0=p0, stats1=p1)      # groups do not divide C
