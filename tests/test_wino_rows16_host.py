"""The default gate of the one-pass Winograd kernel's tile-row forms (csrc/conv_plan.hip: wino_fused_rows) with the 16x16
level adopted where it measured at or under 0.9 of the three-pass form (profiles/README.md, finding 102) - no GPU.

The form is an unexported field of the three-pass plan, so the gate is restated here from the exported plan with its three
constants (csrc/sr3_internal.h) and asked over every conv of the UNets the suite and the benchmark run:
  width 32   R = 2 from WINO_FUSED_ROWS_MIN_BLOCKS = 2048 blocks on (unchanged)
  width 16   R = 4 from WINO_FUSED_ROWS_MIN_BLOCKS_16 = 1024 blocks on, up to WINO_FUSED_ROWS_MAX_CIN_16 = 512 input channels
  width 8    never (the kernel has no instantiation for it)
tests/test_gpu_wino_stage_rows.py's default-gate cases tie the restatement to what the library launches at the block floor,
one block count below it and one Cin above the range. What must not move with the constants: the exported plans
(tests/conv_plans.json) and the validity of gn_res1x1_gate for the 16x16 ResnetBlocks of the benchmark step (conv1 of a
block on wino_fused_kernel<4> refuses it, as conv1 reading U did)."""
import os

import pytest

from conftest import pkg

import test_conv_plan_host as plans
import test_gn_res1x1_host as gnres
import test_gpu_config_sweep as sweep

engine = pkg("engine")
synth = pkg("synth")

MIN_BLOCKS = {2: 2048, 4: 1024}          # WINO_FUSED_ROWS_MIN_BLOCKS, _16 (csrc/sr3_internal.h)
MAX_CIN_16 = 512                         # WINO_FUSED_ROWS_MAX_CIN_16
SWITCHES = ("SR3_NO_WINOGRAD", "SR3_NO_WINO_FUSED_ROWS", "SR3_WINO_FUSED_ROWS_FORCE", "SR3_NO_GN_WINO", "SR3_NO_GN_RES1X1",
            "SR3_GN_RES1X1_FORCE")


@pytest.fixture(autouse=True)
def no_switches():
    set_ = [s for s in SWITCHES if s in os.environ]
    assert not set_, f"the gate is restated with every switch unset; set: {set_}"


def gate(shape, stats=True):
    """wino_fused_rows under the default gate, restated from the exported plan: tile rows per block, 0 = a three-pass form"""
    B, H, W, Cin, Cout = shape
    plan = engine.conv_plan(B, H, W, Cin, Cout, precision="f32", stats=stats)
    R = {32: 2, 16: 4}.get(W, 0)
    if plan["kernel"] != "wino_three_pass" or R == 0 or H % (2 * R) or Cin % 32 or Cout % 64:
        return 0
    bpi = (H // 2) * (W // 2) // 32
    if stats and (plan["stats_slices"] <= 0 or plan["stats_slices"] % bpi or plan["stats_slices"] // bpi not in (1, 2, 4)):
        return 0
    if R == 4 and Cin > MAX_CIN_16:
        return 0
    return R if B * bpi * (Cout // 64) >= MIN_BLOCKS[R] else 0


def convs3x3(cfg, B, hw):
    """(B, H, W, Cin, Cout) of the 3x3 / stride 1 convs of one forward, in launch order"""
    return [c[:5] for c in plans.unet_convs(cfg, B, hw, hw) if c[5:] == (3, 1, 0)]


def test_the_benchmark_step_takes_seven_convs_at_16():
    took = {B: [(s, gate(s)) for s in convs3x3(synth.yml_unet_config(128), B, 128)] for B in (64, 32, 16)}
    at16 = [(s[3], s[4]) for s, r in took[64] if s[2] == 16]
    assert sorted(at16) == sorted([(256, 512)] + 6 * [(512, 512)] + [(768, 512)] + 2 * [(1024, 512)]), at16
    assert sorted((s[3], s[4]) for s, r in took[64] if r == 4) == sorted([(256, 512)] + 6 * [(512, 512)])
    # every conv taken at R = 4 is at 16x16 with 1024 blocks; the 8x8 level and the deeper K stay on the three-pass forms
    for s, r in took[64]:
        kernel = engine.conv_plan(*s, precision="f32", stats=True)["kernel"]
        if s[2] == 8:
            assert r == 0 and kernel == "wino_three_pass", s
        if s[2] == 16:
            assert kernel == "wino_three_pass" and r == (4 if s[3] <= MAX_CIN_16 else 0), s
        if s[2] == 32:
            assert r == 2, s             # (unchanged: 2048 blocks)
        if s[2] >= 64:
            assert r == 0, s
    # B = 32 and 16: 512 and 256 blocks at 16x16 (and 1024 and 512 at 32x32), below both floors
    for B in (32, 16):
        assert not any(r for _, r in took[B]), (B, [x for x in took[B] if x[1]])


def test_the_224_unet_and_the_sweep_configs():
    took = [(s, gate(s)) for B in (64, 32, 16, 4, 1) for s in convs3x3(synth.yml_unet_config(224), B, 128)]
    for name, (B, H, W), _, _ in sweep.ROWS:
        if H == W:
            took += [(s, gate(s)) for s in convs3x3(sweep._cfg(name), B, H)]
    for (B, H, W, Cin, Cout), r in took:
        blocks = B * (H * W // 128) * (Cout // 64)
        if r == 4:
            assert W == 16 and blocks >= MIN_BLOCKS[4] and Cin <= MAX_CIN_16, (B, H, W, Cin, Cout)
        if r == 2:
            assert W == 32 and blocks >= MIN_BLOCKS[2], (B, H, W, Cin, Cout)
        if W == 8 or (W == 16 and (blocks < MIN_BLOCKS[4] or Cin > MAX_CIN_16)) or (W == 32 and blocks < MIN_BLOCKS[2]):
            assert r == 0, (B, H, W, Cin, Cout)
    # the sweep configurations run at B <= 40: none of their 16x16 convs reaches the floor
    assert not any(r == 4 for (B, *_), r in took if B < 64)


def test_the_floor_and_the_range_are_sharp():
    assert gate((64, 16, 16, 512, 512)) == 4 and gate((64, 16, 16, 512, 512), stats=False) == 4     # exactly 1024 blocks
    assert gate((63, 16, 16, 512, 512)) == 0 and gate((32, 16, 16, 512, 512)) == 0
    assert gate((64, 16, 16, 544, 512)) == 0 and gate((64, 16, 16, 768, 512)) == 0
    assert gate((64, 16, 16, 256, 512)) == 4 and gate((64, 16, 16, 128, 512)) == 4
    assert gate((128, 16, 16, 512, 256)) == 4 and gate((128, 16, 16, 512, 192)) == 0                 # 1024 and 768 blocks
    assert gate((256, 8, 8, 512, 512)) == 0


def test_exported_plans_do_not_move():
    with open(plans.TABLE) as f:
        assert plans.table_text() == f.read()


def test_gn_res1x1_stays_refused_at_16():
    blocks = [b for b in gnres.res_blocks(synth.yml_unet_config(128), 128) if b[0] == 16]
    assert len(blocks) == 5 and sum(c0 + c1 != co for _, c0, c1, co in blocks) == 4
    for h, c0, c1, co in blocks:
        for has_res in (True, c0 + c1 != co):
            g = engine.gn_res1x1_gate(64, h, h, c0, c1, co, has_res=has_res)
            assert not g["valid"] and not g["takes"], (h, c0, c1, co, g)
    # the block whose conv1 left U for wino_fused_kernel<4>: neither reading U nor any other rule refuses it now
    assert gate((64, 16, 16, 256, 512)) == 4
    assert engine.gn_res1x1_gate(64, 32, 32, 128, 0, 256)["valid"]        # (conv1 on wino_fused_kernel<2>: valid as before)
