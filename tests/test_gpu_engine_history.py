"""What a context carries from one call to the next: one engine, the veteran, is taken through a history of
calls — changing batch sizes and shapes, settings switched on and off, side buffers grown from outside, row sessions,
abandoned calls — and every sampler call of it, made twice, is held to the bytes of the same call on an engine created for
that call alone (engine_history_ref.py). A second veteran created under SR3_NO_GRAPH=1 walks the same history.

Byte equality: the plan of every launch is a function of the call's shape, arithmetic and settings, never of the engine's
past, so veteran and fresh engine run the same kernels with the same arguments, and no kernel on this path adds
floating-point values atomically (tests/test_gpu_step_graphs.py relies on the same). Engine.step_graph_captures() is
checked where the count is known: the repeat of a call captures nothing, and the first call on a new workspace captures
once per step form it runs. In every scenario one fresh call is held to the numpy restatement of the sampler
(dyn_threshold_ref.sample_loop) at the sampler tests' BAR of 1e-3, and the fresh images show that threshold and projection
are live on these inputs.

Shapes: tiny UNet, 16x16 from 8x8 unless a scenario varies the shape, dpmpp_2m with S = 4 unless it varies the sampler
(the smallest count that warms, captures and replays a form within one call), injected noise, batches of at most 9.

The module has teeth: a build of the library whose launch_abs_quantile zeroes the select's counts with hipMemsetAsync (a
memset node in the captured step; the form before thr_zero_kernel) fails every thresholded history here from the repeat of
the first call on a replaced workspace on, with the threshold-off image, and passes the controls (DESIGN.md §8,
profiles/README.md finding 104).

Wall time of the module on the MI355X, measured once: 7.4 s for its 25 GPU tests, 0.1 - 0.8 s each."""
from dataclasses import replace

import numpy as np
import pytest

import engine_history_ref as H
import test_conv_plan_host as plans
from conftest import pkg
from engine_history_ref import CAP, RATIO, Call, Setup

gpu = pytest.mark.gpu
synth = pkg("synth")
engine = pkg("engine")
F32 = np.float32

# ---- the scenario lists (checked on the CPU by test_scenario_lists_hold_what_they_are_meant_to) ----------------------------
KINDS = [("dpmpp_2m", 4), ("ddim", 4), ("ddpm", None)]
KIND_IDS = ["dpmpp_2m_S4", "ddim_S4", "ddpm_T8"]
PRECISIONS_A = ["f32", "f16x3"]
BATCHES_A = [6, 4, 4, 4, 2, 2, 6, 6]                    # (a) the recorded sequence: B = 6, then B = 4 three times, and on
BATCHES_B = [6, 4, 4]
NEIGHBOURS_B = {                                        # (b) per batch of BATCHES_B, the calls in their order
    "projection": [dict(dyn=(RATIO,), lr=True)],
    "cap_then_none": [dict(dyn=(RATIO, CAP)), dict(dyn=(RATIO,))],
    "feature_cache": [dict(dyn=(RATIO,), cache=(2, 1))],
}
SHAPES_C = [(16, 16), (32, 32), (16, 16), (16, 32), (16, 16)]       # (c), B = 2
FORMS_C = {(16, 16): "lds", (32, 32): "lds", (16, 32): "lds"}       # the projection's form per shape: no call here takes the scratch
B_C = 2
ROWS_D, PLANE_D, B_FORWARD_D = 9, 128, 5                # (d) rows of the threshold ops, the scratch form's plane, the forward's batch
SLOTS_E = [6, 4, 4]                                     # (e) the sessions; uniform calls at B = 4 between the first two
TOGGLES_G = ["batch_invariant", "dropout", "f16f8", "other_weights", "device_weights"]
THR, PLAIN = Call(dyn=(RATIO,)), Call()


def _plans_agree(prec, b0, b1, size=H.R):
    """do the convs of the UNet take the same plan at both batches (but for the two buffer sizes, which count the images)?"""
    def plan(b, c):
        p = engine.conv_plan(b, *c[1:], precision=prec, stats=True)
        return {k: v for k, v in p.items() if k not in ("part_floats", "wino_ws_floats")}
    return all(plan(b0, c) == plan(b1, c) for c in plans.unet_convs(H.config(), 1, size, size))


def test_scenario_lists_hold_what_they_are_meant_to():
    """CPU side of the lists."""
    # (a): larger -> smaller -> its repeat -> larger, for every sampler kind and arithmetic, with the threshold on
    b = BATCHES_A
    assert any(b[i] > b[i + 1] == b[i + 2] and any(x > b[i + 1] for x in b[i + 3:]) for i in range(len(b) - 3))
    assert b[:4] == [6, 4, 4, 4]                        # the sequence DESIGN.md §8 records
    assert {k for k, _ in KINDS} == {"dpmpp_2m", "ddim", "ddpm"} and set(PRECISIONS_A) == {"f32", "f16x3"}
    ids = {(k, p, on) for k, _, p, on in _cases_a()}
    assert ids == {(k, p, on) for k, _ in KINDS for p in PRECISIONS_A for on in (True, False)}
    # every batch within the inputs and at most 9, every shape a multiple of the configuration's divisor
    cfg = H.config()
    div = 2 ** (len(cfg.channel_mults) - 1)
    assert max(BATCHES_A + BATCHES_B + SLOTS_E + [B_C, B_FORWARD_D]) <= H.N_IN <= 9 and ROWS_D <= 9
    for h, w in SHAPES_C + [(H.R, H.R)]:
        assert h % div == 0 and w % div == 0 and h % 2 == 0 and w % 2 == 0
    # (c): the shape changes at every call, comes back to 16x16 from a larger and from a non-square one, and the form of
    # the projection per shape is the one written down
    assert all(s != t for s, t in zip(SHAPES_C, SHAPES_C[1:])) and SHAPES_C.count((16, 16)) == 3
    assert any(h != w for h, w in SHAPES_C) and max(h * w for h, w in SHAPES_C) > 16 * 16
    assert {s: H.lr_form(*s) for s in set(SHAPES_C)} == FORMS_C
    # the B = 4 inputs are the first four of the B = 6 inputs
    for s in (Setup(), Setup("ddpm", None)):
        big, small = H.inputs(s, Call(batch=6, lr=True)), H.inputs(s, Call(batch=4, lr=True))
        for x, y in zip(big, small):
            assert np.array_equal(x[:, :4] if x.ndim == 5 else x[:4], y)
    # where the plans of two batches agree (the B = 4 call is then rows 0..3 of the B = 6 call): reported, asserted on the GPU
    for prec in PRECISIONS_A:
        print(f"{prec}: conv plans of B = 4 and 6 agree: {_plans_agree(prec, 4, 6)}, of B = 2 and 6: {_plans_agree(prec, 2, 6)}")


# ---- (a) the recorded sequence ------------------------------------------------------------------------------------------
def _cases_a():
    return [(k, s, p, on) for k, s in KINDS for p in PRECISIONS_A for on in (True, False)]


@gpu
@pytest.mark.parametrize("kind,steps,prec,on", _cases_a(),
                         ids=[f"{i}-{p}-{'threshold' if on else 'control'}" for i, (k, s) in zip(KIND_IDS, KINDS)
                              for p in PRECISIONS_A for on in (True, False)])
def test_the_recorded_sequence(monkeypatch, kind, steps, prec, on):
    """B = 6, 4, 4, 4, 2, 2, 6, 6 on one veteran, every call twice; with the threshold off the same order is the control."""
    setup = Setup(kind, steps)
    call = Call(dyn=(RATIO,) if on else None, prec=prec)
    H.assert_live(setup, replace(call, batch=4))
    H.assert_anchored(setup, replace(call, batch=4))
    v = H.Veterans(setup, monkeypatch)
    got = {}
    for i, b in enumerate(BATCHES_A):
        got.setdefault(b, v.sample(f"(a) call {i}", replace(call, batch=b)))
    # the rows of the smaller calls are the rows of the veteran's own B = 6 call where the plans of the two batches agree
    for b in (4, 2):
        if _plans_agree(prec, b, 6):
            assert got[b].tobytes() == got[6][:b].tobytes(), f"B = {b} against rows 0..{b - 1} of B = 6"
    v.close()


# ---- (b) the threshold with its neighbours, across batch changes -----------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", list(NEIGHBOURS_B))
def test_threshold_with_its_neighbours_across_batch_changes(monkeypatch, which):
    setup = Setup()
    calls = [Call(**kw) for kw in NEIGHBOURS_B[which]]
    for c in calls:
        H.assert_live(setup, c)
    H.assert_anchored(setup, calls[0])
    if which == "cap_then_none":        # (the cap is live: the two thresholds give other images)
        assert H.fresh(setup, calls[0]).tobytes() != H.fresh(setup, calls[1]).tobytes()
    v = H.Veterans(setup, monkeypatch)
    for i, b in enumerate(BATCHES_B):
        for c in calls:
            v.sample(f"(b) {which} {i}", replace(c, batch=b))
    if which == "feature_cache":
        assert v.g.feature_cache_steps() == (2, 2)
    v.close()


# ---- (c) resolution instead of batch ------------------------------------------------------------------------------------
@gpu
def test_resolution_changes(monkeypatch):
    """x0hat keeps the 32x32 size; the LR operators, dyn_n and the threshold's rank change with the shape"""
    setup = Setup()
    call = Call(batch=B_C, dyn=(RATIO,), lr=True)
    for h, w in set(SHAPES_C):
        H.assert_live(setup, replace(call, H=h, W=w))
    H.assert_anchored(setup, replace(call, H=16, W=32))
    v = H.Veterans(setup, monkeypatch)
    for i, (h, w) in enumerate(SHAPES_C):
        v.sample(f"(c) call {i}", replace(call, H=h, W=w))
    v.close()


# ---- (d) side buffers grown from outside between sampler calls ----------------------------------------------------------
@gpu
def test_side_buffers_grown_from_outside(monkeypatch):
    setup = Setup()
    both = Call(dyn=(RATIO,), lr=True)
    H.assert_live(setup, THR)
    H.assert_live(setup, both)
    H.assert_anchored(setup, both)
    rs = np.random.RandomState(H.SEED)
    rows = (rs.standard_normal((ROWS_D, 3 * H.R * H.R)) * 1.5).astype(F32)
    big, y = np.zeros((1, 3, PLANE_D, PLANE_D), F32), np.zeros((1, 3, 16, 16), F32)
    x5, nl5 = synth.synth_unet_input(H.config(), B_FORWARD_D, H.R, H.R, H.SEED)
    v = H.Veterans(setup, monkeypatch)

    def after(what):
        v.sample(f"(d) after {what}", THR)
        v.sample(f"(d) after {what}", both)

    after("nothing")
    for e in v.both:            # thr_op_bins for 9 rows
        e.op_abs_quantile(rows, RATIO, CAP)
        e.op_dynamic_threshold(rows, RATIO)
    after("the threshold ops over 9 rows")
    for e in v.both:            # lr_scratch (as step 7 of test_gpu_step_graphs.py)
        e.lr_project_np(big, y, form="scratch")
    after("the scratch form on a 128x128 plane")
    for e in v.both:            # a larger workspace
        e.unet_forward_np(x5, nl5.reshape(-1))
    v.touched((B_FORWARD_D, H.R, H.R, 0))
    after("a forward at B = 5")
    for e in v.both:            # the feature cache's validity, on the sampler's own workspace
        e.unet_forward_np(x5[:4], nl5.reshape(-1)[:4])
        e.unet_forward_cached_np(x5[:4], nl5.reshape(-1)[:4], 1)
    after("a whole and a shallow forward at B = 4")
    v.close()


# ---- (e) row sessions and uniform calls on one engine ---------------------------------------------------------------------
@gpu
def test_row_sessions_and_uniform_calls(monkeypatch):
    setup = Setup()
    dyn = (RATIO, CAP)          # (as test_gpu_rows.py::test_staggered_rows_with_the_dynamic_threshold)
    call = Call(dyn=dyn)
    H.assert_live(setup, call)
    H.assert_anchored(setup, call)
    assert H.fresh_session(setup, dyn, 4, False).tobytes() != H.fresh_session(setup, None, 4, False).tobytes()
    assert H.fresh_session(setup, dyn, 4, True).tobytes() != H.fresh_session(setup, dyn, 4, False).tobytes()
    v = H.Veterans(setup, monkeypatch)
    v.session("(e) 1", dyn, SLOTS_E[0])
    v.sample("(e) 2", call)
    v.session("(e) 3", dyn, SLOTS_E[1])
    v.session("(e) 4", dyn, SLOTS_E[2], armed=True)
    v.sample("(e) 5", call)
    v.close()


# ---- (f) abandoned calls ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["step_session", "row_session"])
def test_abandoned_calls(monkeypatch, which):
    setup = Setup()
    H.assert_live(setup, THR)
    H.assert_anchored(setup, THR)
    v = H.Veterans(setup, monkeypatch)
    keep = []
    if which == "step_session":     # sr3_sample_begin and two steps at B = 6, never ended
        six = replace(THR, batch=6)
        cond, noise, _ = H.inputs(setup, six)
        slab = noise[0].nbytes
        for e in v.both:
            H.settings(e, setup, six)
            dc, dn = e.to_device(cond), e.to_device(noise)
            keep += [dc, dn]
            e.sample_begin(dc.ptr, 6, H.R, H.R, dn.ptr)
            for t in (setup.S - 1, setup.S - 2):
                e.sample_step(t, dn.ptr + (setup.S - t) * slab)
        v.touched((6, H.R, H.R, 0))
    else:                           # a row session at the calls' own batch, ended with two rows mid-trajectory
        v.sample("(f) before", THR)
        cond, _, _ = H.inputs(setup, THR)
        for e in v.both:
            H.settings(e, setup, THR)
            dc = [e.to_device(c) for c in cond[:2]]
            keep += dc
            e.rows_begin(4, H.R, H.R, H.SEED)
            e.rows_admit(0, dc[0].ptr, 100)
            assert e.rows_step() == 1
            e.rows_admit(2, dc[1].ptr, 101)
            assert e.rows_step() == 2 and e.rows_position(0) == setup.S - 2
            e.rows_end()
    for e in v.both:
        e.synchronize()
    v.sample("(f) after", THR)
    v.sample("(f) after", PLAIN)
    v.close()


# ---- (g) setting toggles that must leave no trace ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("toggle", TOGGLES_G)
def test_toggles_leave_no_trace(monkeypatch, toggle):
    """plain and thresholded call, the setting on for a call and off again, plain and thresholded call: against fresh
    engines that never saw the setting"""
    setup = Setup(dropout=0.2) if toggle == "dropout" else Setup()
    H.assert_live(setup, THR)
    H.assert_anchored(setup, THR)
    v = H.Veterans(setup, monkeypatch)
    v.sample("(g) before", PLAIN)
    v.sample("(g) before", THR)
    for e in v.both:
        if toggle == "batch_invariant":
            on = H.run(e, setup, replace(THR, plan_batch=8))
            assert e.batch_invariant() == 8
            e.set_batch_invariant(0)
        elif toggle == "dropout":
            e.set_dropout(True, 5)
            on = H.run(e, setup, THR)
            e.set_dropout(False)
            assert on.tobytes() != H.fresh(setup, THR).tobytes()            # (the masks were live)
        elif toggle == "f16f8":
            on = H.run(e, setup, replace(THR, prec="f16f8"))
            assert on.tobytes() != H.fresh(setup, THR).tobytes()
        elif toggle == "other_weights":
            e.load_state_dict(H.weights(H.SEED + 1))
            on = H.run(e, setup, THR)
            e.load_state_dict(H.weights(H.SEED))
            assert on.tobytes() != H.fresh(setup, THR).tobytes()
        else:
            import torch
            sd = H.weights(H.SEED)
            tensors = [(n, torch.from_numpy(sd[n]).cuda()) for n, _ in e.param_list()]
            assert e.load_weights_device(tensors) == len(tensors)
            e.synchronize()
    if toggle == "batch_invariant":
        v.touched(None)
    v.sample("(g) after", PLAIN)
    v.sample("(g) after", THR)
    v.close()
