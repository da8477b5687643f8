"""The gate that decides whether block1's GroupNorm + Swish pass also multiplies the block's 1x1 res_conv
(csrc/conv_plan.hip: gn_res1x1_gate), asked through the host-only export sr3_gn_res1x1_gate — no GPU.

valid  exact f32; a res_conv whose operands are x / skip themselves, unsplit, no raw copy wanted; mode 2; conv1 reads the
       plain activated tensor (its GroupNorm pass does not write the Winograd U); conv2's plan is a Winograd plan;
       C0 % 32 == 0, C1 % 32 == 0, C0 + C1 <= 1024, Cout % 64 == 0, H * W % 128 == 0.
tuned  the 32x32 level and above, from 1024 blocks of 128 pixels x 64 | 128 output channels on.
Both are restated here from the exported conv plans (the unexported tile-row form of the three-pass plan from
tests/test_gpu_wino_fused_rows.py's restatement) and compared over every ResnetBlock of the UNets the suite and the
benchmark run."""
import os

import pytest

from conftest import pkg

import test_gpu_config_sweep as sweep
import test_gpu_wino_fused_rows as rows

engine = pkg("engine")
synth = pkg("synth")

SWITCHES = ("SR3_NO_GN_RES1X1", "SR3_GN_RES1X1_FORCE", "SR3_NO_GN_WINO", "SR3_NO_WINOGRAD", "SR3_NO_WINO_FUSED_ROWS",
            "SR3_WINO_FUSED_ROWS_FORCE")
MAX_CIN, MIN_HW, MIN_BLOCKS = 1024, 32 * 32, 1024         # csrc/sr3_internal.h, csrc/conv_plan.hip


@pytest.fixture(autouse=True)
def no_switches():
    set_ = [s for s in SWITCHES if s in os.environ]
    assert not set_, f"the gate is restated with every switch unset; set: {set_}"


def res_blocks(cfg, h):
    """(H = W, C0, C1, Cout) of every ResnetBlock of one forward at h x h pixels (unet.py:161-265)"""
    inner, n = cfg.inner_channel, len(cfg.channel_mults)
    out, pre = [], inner
    feat = [pre]
    for ind, mult in enumerate(cfg.channel_mults):
        for _ in range(cfg.res_blocks):
            out.append((h, pre, 0, inner * mult))
            pre = inner * mult
            feat.append(pre)
        if ind != n - 1:
            h = (h - 1) // 2 + 1
            feat.append(pre)
    out += [(h, pre, 0, pre), (h, pre, 0, pre)]
    for ind in reversed(range(n)):
        for _ in range(cfg.res_blocks + 1):
            out.append((h, pre, feat.pop(), inner * cfg.channel_mults[ind]))
            pre = inner * cfg.channel_mults[ind]
        if ind >= 1:
            h *= 2
    return out


def restated(B, H, W, C0, C1, Cout, precision="f32", has_res=True, direct=True, raw_wanted=False, in_split=False, mode=2):
    C = C0 + C1
    shapes_ok = C0 > 0 and C0 % 32 == 0 and C1 % 32 == 0 and C <= MAX_CIN and Cout % 64 == 0 and (H * W) % 128 == 0
    valid = precision == "f32" and has_res and direct and not raw_wanted and not in_split and mode == 2 and shapes_ok
    if valid:
        p1 = engine.conv_plan(B, H, W, C, Cout, precision="f32", stats=True)
        p2 = engine.conv_plan(B, H, W, Cout, Cout, precision="f32", stats=True)
        reads_u = p1["kernel"] == "wino_three_pass" and rows.gate((B, H, W, C, Cout), True, False) == 0
        valid = p2["kernel"].startswith("wino") and not reads_u
    tuned = False
    if valid:
        tiles_m = B * H * W // 128
        bn = 128 if Cout % 128 == 0 and tiles_m * (Cout // 128) >= 512 else 64
        tuned = H * W >= MIN_HW and tiles_m * (Cout // bn) >= MIN_BLOCKS
    return {"valid": valid, "tuned": tuned}


def ask(*a, **kw):
    g = engine.gn_res1x1_gate(*a, **kw)
    assert g["takes"] == (g["valid"] and g["tuned"])          # no switch is set
    return {"valid": g["valid"], "tuned": g["tuned"]}


def test_the_benchmark_step_takes_its_eleven_blocks():
    cfg = synth.yml_unet_config(128)
    blocks = res_blocks(cfg, 128)
    taken = [(h, c0, c1, co) for h, c0, c1, co in blocks if c0 % 32 == 0 and ask(64, h, h, c0, c1, co, has_res=c0 + c1 != co)["tuned"]]
    assert sorted(taken) == sorted([(128, 128, 64, 64), (128, 64, 64, 64), (128, 64, 64, 64),
                                    (64, 64, 0, 128), (64, 256, 128, 128), (64, 128, 128, 128), (64, 128, 64, 128),
                                    (32, 128, 0, 256), (32, 512, 256, 256), (32, 256, 256, 256), (32, 256, 128, 256)])
    # the seven res_conv blocks of the 16x16 and 8x8 levels stay on their two launches: conv1's pass writes U there
    rest = [b for b in blocks if b[1] + b[2] != b[3] and b not in taken]
    assert len(rest) == 7 and all(h <= 16 for h, *_ in rest)
    assert not any(ask(64, h, h, c0, c1, co)["valid"] for h, c0, c1, co in rest)


def test_gate_equals_its_restatement_over_the_suites_unets():
    seen = {"valid": 0, "tuned": 0, "refused": 0}
    configs = [(synth.yml_unet_config(s), B, 128) for s in (224, 128) for B in (1, 4, 32, 64)]
    configs += [(synth.tiny_unet_config(), B, 16) for B in (1, 2)]
    configs += [(sweep._cfg(name), B, H) for name, (B, H, W), _, _ in sweep.ROWS if H == W]
    for cfg, B, hw in configs:
        for h, c0, c1, co in res_blocks(cfg, hw):
            if c0 % 32:
                continue
            kw = dict(has_res=c0 + c1 != co)
            got, want = ask(B, h, h, c0, c1, co, **kw), restated(B, h, h, c0, c1, co, **kw)
            assert got == want, (B, h, c0, c1, co, got, want)
            seen["valid"] += got["valid"]
            seen["tuned"] += got["tuned"]
            seen["refused"] += not got["valid"]
    assert all(seen.values()), seen


def test_each_validity_rule_alone_refuses():
    ok = (64, 64, 64, 128, 64, 128)          # a block of the benchmark step
    assert ask(*ok) == {"valid": True, "tuned": True}
    for kw in (dict(precision="f16x3"), dict(precision="f16f8"), dict(has_res=False), dict(direct=False), dict(raw_wanted=True),
               dict(in_split=True), dict(mode=1), dict(mode=0)):
        assert ask(*ok, **kw) == {"valid": False, "tuned": False}, kw
        assert restated(*ok, **kw) == {"valid": False, "tuned": False}, kw
    B, H, W, C0, C1, Cout = ok
    for bad in ((B, H, W, 48, 16, Cout),           # C0 not a multiple of 32 (the sum is)
                (B, H, W, 144, 48, Cout),          # neither part
                (B, H, W, 1024, 32, Cout),         # more than 1024 input channels: the block's scale / shift table
                (B, H, W, C0, C1, 96),             # Cout not a multiple of 64
                (B, 8, 8, 512, 512, 512),          # 64 pixels per image: no whole tile
                (B, 16, 16, 256, 0, 512),          # conv1's pass writes the Winograd U
                (2, H, W, C0, C1, Cout)):          # conv2 on the direct kernel (too few tiles for a Winograd plan)
        assert not ask(*bad)["valid"], bad
        if bad[3] % 32 == 0 and bad[4] % 32 == 0 and bad[5] % 32 == 0:
            assert not restated(*bad)["valid"], bad


def test_tuning_is_a_level_and_a_block_count():
    # valid at every batch size that leaves conv2 a Winograd plan; adopted from 1024 blocks on
    for B, tuned in ((64, True), (32, True), (16, False)):
        g = ask(B, 64, 64, 128, 64, 128)
        assert g["valid"] and g["tuned"] == tuned, (B, g)
        assert g == restated(B, 64, 64, 128, 64, 128)
