"""Elastic row sessions on the GPU (sr3_rows_step_batch, sr3_rows_move; DESIGN.md §3.5g "live rows only"): in the
batch-invariant mode a step runs over slots [0, batch) of the session's workspace alone, rows are compacted by one-launch
moves, and every request is still the bytes of its B = 1 uniform call. Every comparison is np.array_equal; P = 64; T = 6,
S = 4 as in tests/test_gpu_batch_invariant.py, whose configurations, weights and helpers this module uses.

The byte comparisons alone would pass on a library that accepts `batch` and runs all slots (an idle row is never written
anyway): the rows_rows_run assertions are the ones that hold the steps to their batch.

Configurations: tiny at 16x16; "Dc" at 32x32, sweep configuration D (128 / 256 / 512 channels, attention at 8x8, two blocks
per level) with a 3-channel conditioning input — D itself is unconditional, and a row session admits requests by their
conditioning image (sr3_rows_begin refuses the unconditional model); F8, the two-level 128 / 256-channel configuration
whose fp8 layer set the planning batch switches on."""
import functools

import numpy as np
import pytest

from conftest import pkg

import test_gpu_batch_invariant as bi

pytestmark = pytest.mark.gpu
synth = pkg("synth")
rolling = pkg("rolling")
engine_mod = pkg("engine")
UNetConfig = pkg("graph").UNetConfig
Sr3Error = pkg("_lib").Sr3Error
F32 = np.float32

P, SEED = bi.P, bi.SEED
PRECISIONS = bi.PRECISIONS
KINDS, KIND_IDS = bi.KINDS, bi.KIND_IDS
_same, _set_sampler = bi._same, bi._set_sampler


def _cfg(name):
    if name == "Dc":
        return UNetConfig(in_channel=6, out_channel=3, inner_channel=128, norm_groups=32, channel_mults=(1, 2, 4),
                          attn_res=(8,), res_blocks=2, dropout=0.0, image_size=32)
    return bi._cfg(name)


def _size(name):
    return 16 if name == "tiny" else 32


@functools.lru_cache(maxsize=None)
def _weights(name):
    return synth.synth_state_dict(_cfg(name), 600 + sum(map(ord, name)))


def _new_engine(name, plan_batch=P):
    e = engine_mod.Engine(_cfg(name), 0)
    e.load_state_dict(_weights(name))
    assert e.weights_missing() == 0
    e.set_batch_invariant(plan_batch)
    return e


@functools.lru_cache(maxsize=None)
def _engine(name, role):
    """one engine per (configuration, role) for the module: "rows" runs the sessions, "one" the B = 1 calls"""
    return _new_engine(name)


def _arm(e, prec, kind, steps):
    e.set_precision(prec)
    e.set_lr_consistency(None)
    e.set_dynamic_threshold(None)
    return _set_sampler(e, kind, steps)


@functools.lru_cache(maxsize=None)
def _cond(name, n):
    s = _size(name)
    return synth.synth_cond(n, s, s // 2, SEED)


@functools.lru_cache(maxsize=None)
def _init(name, n):
    s = _size(name)
    return np.random.RandomState(SEED + 5).uniform(-1, 1, (n, 3, s, s)).astype(F32)


def _alone(e1, name, i, image_id, start_step=None, **kw):
    """request i as its B = 1 uniform call"""
    if start_step is not None:
        kw.update(init=_init(name, 8)[i:i + 1], start_step=start_step)
    return e1.sample_np(_cond(name, 8)[i:i + 1], seed=SEED, image_offset=image_id, **kw)


def _live(trace):
    return [sum(h is not None for h in t) for t in trace]


# ---- batch == slots -------------------------------------------------------------------------------------------------------
def test_batch_equal_to_the_slots_is_rows_step():
    """sr3_rows_step_batch(slots) launches what sr3_rows_step launches: the same bytes from the same graph"""
    e = _new_engine("tiny")
    try:
        _arm(e, "f16f8", "dpmpp_2m", 4)
        cond = _cond("tiny", 8)
        reqs = [{"cond": cond[i], "image_id": 50 + i, "at": at} for i, at in enumerate([0, 0, 2, 3, 4])]
        want, trace = e.rows_np(reqs, 3, seed=SEED)
        n = e.step_graph_captures()
        run = e.rows_rows_run()
        assert run == 3 * sum(1 for v in _live(trace) if v)
        got, trace2, batches = e.rows_np(reqs, 3, seed=SEED, elastic=True, ladder=(3,))
        assert trace2 == trace and set(batches) <= {0, 3}
        assert e.step_graph_captures() == n, "a step at batch == slots captured a graph of its own"
        assert e.rows_rows_run() - run == sum(batches)
        _same(np.stack(got), np.stack(want), "rows_step_batch(slots) against rows_step")
    finally:
        e.close()


# ---- requests are their single-image calls --------------------------------------------------------------------------------
def _staggered(S):
    """six slots; (request, at, slot, start_step): 0 alone at the top slot, 1 joins, then 2, 3 (one step each) and 4; the
    live count runs 1, 2, 5, 3, ..., 2, 1 and the rows that are left move down as the slots below them come free"""
    return [(0, 0, 5, None), (1, 1, None, None), (2, 2, None, 1), (3, 2, None, 1), (4, 2, None, None)]


def _check_requests(name, kind, steps, prec):
    e6, e1 = _engine(name, "rows"), _engine(name, "one")
    for e in (e6, e1):
        S = _arm(e, prec, kind, steps)
    cond, init = _cond(name, 8), _init(name, 8)
    reqs = []
    for i, at, slot, s0 in _staggered(S):
        rq = {"cond": cond[i], "image_id": 200 + i, "at": at}
        if slot is not None:
            rq["slot"] = slot
        if s0 is not None:
            rq.update(init=init[i], start_step=s0)
        reqs.append(rq)
    run0 = e6.rows_rows_run()
    got, trace, batches = e6.rows_np(reqs, 6, seed=SEED, elastic=True)
    live = _live(trace)
    assert live[:4] == [1, 2, 5, 3] and live[-1] == 1, live
    # the batch of every step covers its rows and is the ladder's smallest that holds them after the moves
    ladder = rolling.default_ladder(6)
    for t, b, n in zip(trace, batches, live):
        assert b == next(x for x in ladder if x >= n) and all(h is None for h in t[b:]), (t, b)
    # moves: request 0 leaves slot 5 before its first step, request 4 moves down twice mid-trajectory
    assert trace[0][0] == 0 and trace[2][4] == 4 and trace[3][2] == 4 and trace[-1][0] == 4
    assert e6.rows_rows_run() - run0 == sum(batches) < 6 * len(batches)
    for k, (i, _, _, s0) in enumerate(_staggered(S)):
        want = _alone(e1, name, i, 200 + i, s0)
        _same(np.asarray(got[k])[None], want, f"{name} {kind} {prec}: request {i} against its B = 1 call")
    assert e6.fallback_calls() == 0 and e1.fallback_calls() == 0


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("kind,steps", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", ["tiny", "Dc"])
def test_requests_are_their_single_image_calls(name, kind, steps, prec):
    _check_requests(name, kind, steps, prec)


def test_requests_where_the_planning_batch_switches_fp8_on():
    assert bi._f8_convs("F8", 32, 1, P) and not bi._f8_convs("F8", 32, 1, None)
    _check_requests("F8", "dpmpp_2m", 4, "f16f8")


# ---- the move itself ------------------------------------------------------------------------------------------------------
def _snapshot(e, B, size):
    state, packed = e.read_packed_state()
    return state.copy(), packed.copy(), e.read_history(B, size, size).copy()


def test_move_carries_every_slab_and_the_position():
    name, S = "tiny", 4
    e = _engine(name, "rows")
    _arm(e, "f16f8", "dpmpp_2m", S)
    cond = _cond(name, 8)
    ref, _ = e.rows_np([{"cond": cond[1], "image_id": 301, "slot": 1}, {"cond": cond[3], "image_id": 303, "slot": 3}], 4,
                       seed=SEED)
    dc = [e.to_device(cond[i]) for i in (1, 3)]
    out = e.buffer(3 * 16 * 16)
    e.rows_begin(4, 16, 16, SEED)
    try:
        e.rows_admit(1, dc[0].ptr, 301)
        e.rows_admit(3, dc[1].ptr, 303)
        assert e.rows_step() == 2 and e.rows_step() == 2      # (the third step reads the history: c3 != 0 from here on)
        s0, p0, h0 = _snapshot(e, 4, 16)
        assert np.any(s0[3]) and np.any(p0[3]) and np.any(h0[3]) and not np.any(s0[0]) and not np.any(p0[0])
        e.rows_move(3, 0)
        s1, p1, h1 = _snapshot(e, 4, 16)
        for a0, a1, what in ((s0, s1, "state"), (p0, p1, "packed state"), (h0, h1, "x0 history")):
            assert np.array_equal(a1[0], a0[3]), f"{what}: slot 0 does not hold slot 3's bytes"
            assert np.array_equal(a1[1], a0[1]) and np.array_equal(a1[2], a0[2]), f"{what}: a bystander changed"
        assert not np.any(s1[3]) and not np.any(p1[3]), "the source slot was not left zero"
        assert [e.rows_position(r) for r in range(4)] == [2, 2, -1, -1]
        run = e.rows_rows_run()
        assert e.rows_step(None, 2) == 2 and e.rows_step(None, 2) == 2
        assert e.rows_rows_run() - run == 4
        got = []
        for slot in (1, 0):
            e.rows_retire(slot, out.ptr)
            got.append(out.download((3, 16, 16)).copy())
    finally:
        e.rows_end()
        for b in dc + [out]:
            b.free()
    _same(np.stack(got), np.stack(ref), "the session with the move against the session without")


def test_rows_outside_the_batch_are_not_touched():
    """slots 2 and 3 hold the finished images of retired occupants: three steps at batch 2 leave every byte of their
    state, packed copy and history"""
    name, S = "tiny", 4
    e = _engine(name, "rows")
    _arm(e, "f16f8", "dpmpp_2m", S)
    cond, init = _cond(name, 8), _init(name, 8)
    bufs = [e.to_device(cond[i]) for i in range(4)] + [e.to_device(init[i]) for i in (2, 3)]
    out = e.buffer(3 * 16 * 16)
    e.rows_begin(4, 16, 16, SEED)
    try:
        e.rows_admit(0, bufs[0].ptr, 400)
        e.rows_admit(1, bufs[1].ptr, 401)
        e.rows_admit(2, bufs[2].ptr, 402, bufs[4].ptr, 1)
        e.rows_admit(3, bufs[3].ptr, 403, bufs[5].ptr, 1)
        assert e.rows_step() == 4
        for slot in (2, 3):
            e.rows_retire(slot, out.ptr)
        s0, p0, h0 = _snapshot(e, 4, 16)
        assert np.any(s0[2]) and np.any(s0[3]) and np.any(h0[3])
        run = e.rows_rows_run()
        for _ in range(3):
            assert e.rows_step(None, 2) == 2
        assert e.rows_rows_run() - run == 6
        s1, p1, h1 = _snapshot(e, 4, 16)
        for a0, a1, what in ((s0, s1, "state"), (p0, p1, "packed state"), (h0, h1, "x0 history")):
            assert np.array_equal(a1[2:], a0[2:]), f"{what} of a slot outside the batch changed"
            assert not np.array_equal(a1[:2], a0[:2]), f"{what} of the live rows did not move"
        assert [e.rows_position(r) for r in range(4)] == [0, 0, -1, -1]
    finally:
        e.rows_end()
        for b in bufs + [out]:
            b.free()


# ---- armed session --------------------------------------------------------------------------------------------------------
def test_armed_session_moves_a_held_row_with_its_lr_image_and_frames():
    """LR consistency per row 8 -> 16, the dynamic threshold and frames: request 0 (held, frames) sits at slot 2 and
    moves to slot 0 after two steps, when the short request there has retired; request 1 next to it is not held"""
    name, S = "tiny", 4
    e, e1 = _engine(name, "rows"), _engine(name, "one")
    for x in (e, e1):
        _arm(x, "f16x3", "ddim", S)
        x.set_dynamic_threshold(0.995, 1.25)
    cond, init = _cond(name, 8), _init(name, 8)
    lr = np.random.RandomState(SEED + 9).uniform(-1, 1, (1, 3, 8, 8)).astype(F32)
    reqs = [{"cond": cond[0], "image_id": 500, "slot": 2, "lr": lr[0], "lr_strength": 0.75, "frames": True},
            {"cond": cond[1], "image_id": 501, "slot": 1},
            {"cond": cond[2], "image_id": 502, "slot": 0, "init": init[2], "start_step": 2}]
    keep = None
    try:
        fixed, _ = e.rows_np(reqs, 4, seed=SEED)
        got, trace, batches = e.rows_np(reqs, 4, seed=SEED, elastic=True)
        assert [t.index(0) for t in trace] == [2, 2, 0, 0] and batches == [3, 3, 2, 2], (trace, batches)
        for k in (1, 2):
            _same(np.asarray(got[k]), np.asarray(fixed[k]), f"request {k} against the fixed session")
        _same(got[0][0], fixed[0][0], "the held request against the fixed session")
        _same(got[0][1], fixed[0][1], "the held request's frames against the fixed session")
        _same(np.asarray(got[1])[None], _alone(e1, name, 1, 501), "the unheld request against its B = 1 call")
        _same(np.asarray(got[2])[None], _alone(e1, name, 2, 502, 2), "the short request against its B = 1 call")
        keep = e1.to_device(lr)
        e1.set_lr_consistency(keep.ptr, 1, 8, 8, row_offset=0, strength=0.75)
        want, frames = _alone(e1, name, 0, 500, frames=True)
        _same(got[0][0][None], want, "the held request against its B = 1 call with set_lr_consistency")
        _same(got[0][1], frames[:, 0], "the held request's frames against those of its B = 1 call")
        # (and the LR image is live: without it the image differs)
        e1.set_lr_consistency(None)
        assert not np.array_equal(_alone(e1, name, 0, 500), want)
    finally:
        for x in (e, e1):
            x.set_lr_consistency(None)
            x.set_dynamic_threshold(None)
        if keep is not None:
            keep.free()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _refused(e, call, match):
    before = (_snapshot(e, 4, 16), [e.rows_position(r) for r in range(4)], e.rows_rows_run(), e.step_graph_captures())
    with pytest.raises(Sr3Error, match=match):
        call()
    s, pos, run, cap = _snapshot(e, 4, 16), [e.rows_position(r) for r in range(4)], e.rows_rows_run(), e.step_graph_captures()
    assert all(np.array_equal(a, b) for a, b in zip(s, before[0])), f"{match}: a refused call changed the state"
    assert (pos, run, cap) == before[1:], f"{match}: a refused call moved the host's record"


def test_refusals_leave_state_and_positions():
    cond = _cond("tiny", 8)
    e = _engine("tiny", "rows")
    _arm(e, "f16f8", "dpmpp_2m", 4)
    dc = [e.to_device(cond[i]) for i in range(2)]
    e.rows_begin(4, 16, 16, SEED)
    try:
        e.rows_admit(0, dc[0].ptr, 600)
        e.rows_admit(2, dc[1].ptr, 601)
        assert e.rows_step() == 2
        _refused(e, lambda: e.rows_step(None, 2), "slot 2")
        _refused(e, lambda: e.rows_step(None, 0), r"batch 0 outside \[1, 4\]")
        _refused(e, lambda: e.rows_step(None, 5), r"batch 5 outside \[1, 4\]")
        _refused(e, lambda: e.rows_move(0, 2), "destination slot 2 is live")
        _refused(e, lambda: e.rows_move(1, 3), "source slot 1 is idle")
        _refused(e, lambda: e.rows_move(0, 0), "slot 0")
        _refused(e, lambda: e.rows_move(0, 4), "row 4 outside")
        assert e.rows_step(None, 3) == 2            # (and the session goes on)
    finally:
        e.rows_end()
    # the mode off: only the whole session steps
    e0 = _new_engine("tiny", 0)
    try:
        _arm(e0, "f16f8", "dpmpp_2m", 4)
        d0 = e0.to_device(cond[0])
        e0.rows_begin(4, 16, 16, SEED)
        e0.rows_admit(0, d0.ptr, 600)
        assert e0.rows_step() == 1
        _refused(e0, lambda: e0.rows_step(None, 2), "sr3_set_batch_invariant")
        assert e0.rows_step(None, 4) == 1
        e0.rows_end()
        with pytest.raises(ValueError, match="set_batch_invariant"):
            e0.rows_np([{"cond": cond[0], "image_id": 1}], 4, elastic=True)
        d0.free()
    finally:
        e0.close()
    for b in dc:
        b.free()


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def _graph_session(e):
    """four slots over ladder (1, 2, 4), every batch value for two steps or more: three live (batch 4), then request 0 alone
    (batch 1), then two short ones (batch 2)"""
    cond, init = _cond("tiny", 8), _init("tiny", 8)
    reqs = [{"cond": cond[0], "image_id": 700, "at": 0},
            {"cond": cond[1], "image_id": 701, "at": 0, "init": init[1], "start_step": 2},
            {"cond": cond[2], "image_id": 702, "at": 0, "init": init[2], "start_step": 2},
            {"cond": cond[3], "image_id": 703, "at": 4, "init": init[3], "start_step": 2},
            {"cond": cond[4], "image_id": 704, "at": 4, "init": init[4], "start_step": 2}]
    got, trace, batches = e.rows_np(reqs, 4, seed=SEED, elastic=True, ladder=(1, 2, 4))
    assert batches == [4, 4, 1, 1, 2, 2], batches
    return np.stack(got)


def test_one_graph_per_batch_value(monkeypatch):
    e = _new_engine("tiny")
    with monkeypatch.context() as m:
        m.setenv("SR3_NO_GRAPH", "1")       # read in sr3_create
        ref = _new_engine("tiny")
    try:
        for x in (e, ref):
            _arm(x, "f16f8", "dpmpp_2m", 4)
        n0 = e.step_graph_captures()
        first = _graph_session(e)
        n1 = e.step_graph_captures()
        second = _graph_session(e)
        n2 = e.step_graph_captures()
        assert (n1 - n0, n2 - n1) == (3, 0)
        want = _graph_session(ref)
        assert ref.step_graph_captures() == 0
        _same(first, want, "first session against the engine without graphs")
        _same(second, want, "second session against the engine without graphs")
    finally:
        e.close()
        ref.close()


# ---- facade -----------------------------------------------------------------------------------------------------------------
def test_facade_stream_of_mixed_strengths():
    import torch
    strengths = [None, 0.5, 0.25, None, 0.25, 0.5, None]
    n = len(strengths)
    x = torch.from_numpy(synth.synth_cond(n, 16, 8, SEED)).cuda()
    img = torch.from_numpy(np.random.RandomState(SEED).uniform(-1, 1, (n, 3, 16, 16)).astype(F32)).cuda()
    one, roll = bi._model("tiny"), bi._model("tiny")
    for m in (one, roll):
        m.set_sampler("dpmpp_2m", steps=4)
    want = []
    for i, s in enumerate(strengths):
        if s is None:
            want.append(one.super_resolution_batch(x[i:i + 1], seed=SEED, image_offset=i)[0].cpu().numpy())
        else:
            want.append(one.refine(x[i:i + 1], img[i:i + 1], s, seed=SEED, image_offset=i)[0].cpu().numpy())

    def source():
        for i, s in enumerate(strengths):
            yield {"x_in_row": x[i], "init": None if s is None else img[i], "strength": s}

    with roll.rolling(slots=4, seed=SEED, elastic=True) as rs:
        assert rs.elastic and rs.ladder == (1, 2, 3, 4)
        run0 = roll._engine().rows_rows_run()
        got = dict(rs.stream(source()))
        torch.cuda.synchronize()
        assert rs.moves > 0 and min(rs.batch_trace) < 4 and len(rs.batch_trace) == len(rs.trace) == rs.steps_run
        assert roll._engine().rows_rows_run() - run0 == sum(rs.batch_trace) < 4 * rs.steps_run
        assert rs.restarts == 0
    assert sorted(got) == list(range(n))
    for t in range(n):
        _same(got[t].cpu().numpy(), want[t], f"request {t} (strength {strengths[t]}) against its B = 1 call")
    plain = bi._model("tiny", on=False)
    with pytest.raises(ValueError, match="set_batch_invariant"):
        plain.rolling(slots=4, elastic=True)
