"""The dispatch plans of the batch-invariant mode, asked through the host-only export
sr3_conv_plan_invariant — no GPU.

With a planning batch P every field of a conv's plan that names an arithmetic — kernel, tile, split kind, split count,
phases, statistics slices, Winograd workspace per image, fragment-major flag, fp8 operands — must be the same for every
real batch B up to the mode's maximum batch; only the two buffer sizes scale with B. The default plans, on the other hand,
do depend on B (the teeth check): that is what the mode is for.

Two things this file does not show. (1) The exported plan has twelve fields; the three sub-forms of a plan — the
tile-row form of the three-pass Winograd plan (wino_fused_rows), its one-kernel form (wino_gemm_out) and the sub-pixel
Winograd form of the Upsample convs (up2_wino) — are not among them. Their gates count the planning batch like the rest;
tests/test_gpu_batch_invariant.py compares the engines' launch counters of those forms between B = 1 and the batched
call. (2) A batch above the mode's maximum is an error, not a plan, so the batch sizes compared end at that maximum. It
is at least 64 everywhere but in one row: the yml UNet at 128x128 planned for ONE image (P = 1) takes at most 16 images
per call — a 64-slot rolling session is refused there; plan for the batch you serve.
"""
import functools

import pytest

from conftest import pkg

import test_conv_plan_host as plans
import test_gpu_config_sweep as sweep

engine = pkg("engine")
synth = pkg("synth")

PRECISIONS = ("f32", "f16x3", "f16f8")
PLAN_BATCHES = (1, 8, 64)
BATCHES = (1, 2, 3, 5, 8, 16, 64)
# name, input size (square)
UNETS = [("tiny", 16), ("tiny", 32), ("A", 48), ("B", 32), ("C", 64), ("D", 32), ("yml128", 64), ("yml128", 128)]


def _cfg(name):
    return synth.tiny_unet_config() if name == "tiny" else sweep._cfg(name)


@functools.lru_cache(maxsize=None)
def _convs(name, size):
    """(H, W, Cin, Cout, ks, stride, up2) of every conv of the UNet at size x size, duplicates dropped."""
    return tuple(dict.fromkeys(c[1:] for c in plans.unet_convs(_cfg(name), 1, size, size)))


def arithmetic(plan, B):
    """the fields of a plan that pick an arithmetic (the buffer sizes part_floats / wino_ws_floats scale with B)"""
    assert plan["wino_ws_floats"] % B == 0
    return (plan["kernel"], tuple(plan["tile"]), plan["split"], plan["splits"], plan["phases"], plan["stats_slices"],
            plan["wino_ws_floats"] // B, plan["needs_wino_frag"], plan["f8"])


def mode_max_batch(name, size, prec, P):
    return min(engine.conv_plan_invariant_max_batch(P, *conv, precision=prec, stats=True) for conv in _convs(name, size))


@pytest.mark.parametrize("P", PLAN_BATCHES)
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name,size", UNETS)
def test_plans_do_not_depend_on_the_batch(name, size, prec, P):
    bmax = mode_max_batch(name, size, prec, P)
    # (the maximum is below 64 for one row: the yml UNet at 128x128 planned for ONE image splits the K loop of convs
    # with 512 tiles per image in place, and the arrival counters of those tiles end at 16 images)
    assert bmax >= (64 if P >= 8 else 16), "the mode's maximum batch is below the planning batch"
    for conv in _convs(name, size):
        want = arithmetic(engine.conv_plan(1, *conv, precision=prec, stats=True, plan_batch=P), 1)
        for B in tuple(b for b in BATCHES if b <= bmax) + (bmax,):
            # (a plan error — a batch past the plan's limit, an fp8 request no kernel honours — raises here)
            got = arithmetic(engine.conv_plan(B, *conv, precision=prec, stats=True, plan_batch=P), B)
            assert got == want, f"P={P} B={B} conv {conv}: {got} != {want} (B = 1)"


@pytest.mark.parametrize("prec", PRECISIONS)
def test_a_batch_past_the_maximum_is_refused_not_replanned(prec):
    """the yml UNet at 128x128 planned for ONE image: an in-place split-K has one arrival counter per tile, so the mode's
    maximum batch is far below the 4 GiB bound; one image more is an error of the plan, never another arithmetic"""
    convs = _convs("yml128", 128)
    limits = {conv: engine.conv_plan_invariant_max_batch(1, *conv, precision=prec, stats=True) for conv in convs}
    conv, bmax = min(limits.items(), key=lambda kv: kv[1])
    assert bmax < 64, "no in-place split-K bounds the batch of this configuration any more: pick another row"
    assert engine.conv_plan(bmax, *conv, precision=prec, stats=True, plan_batch=1)["needs_counters"]
    with pytest.raises(RuntimeError):
        engine.conv_plan(bmax + 1, *conv, precision=prec, stats=True, plan_batch=1)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_default_plans_depend_on_the_batch(prec):
    """teeth: without the mode, config D at 32x32 plans other arithmetic at B = 5 than at B = 1 (46 / 39 / 39 of its 52
    conv launches when this test was written)"""
    convs = [c[1:] for c in plans.unet_convs(_cfg("D"), 1, 32, 32)]
    assert len(convs) == 52
    differ = sum(arithmetic(engine.conv_plan(1, *c, precision=prec, stats=True), 1) !=
                 arithmetic(engine.conv_plan(5, *c, precision=prec, stats=True), 5) for c in convs)
    print(f"{prec}: {differ} of {len(convs)} convs change their plan between B = 1 and B = 5")
    assert differ >= 1


def test_the_mode_off_is_the_default_plan():
    for conv in _convs("D", 32):
        for B in (1, 5, 64):
            assert engine.conv_plan(B, *conv, precision="f16f8", stats=True, plan_batch=None) == \
                   engine.conv_plan(B, *conv, precision="f16f8", stats=True)
