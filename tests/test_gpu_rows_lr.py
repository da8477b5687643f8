"""Low-resolution consistency and frames per ROW of a row session (sr3_rows_lr_consistency, sr3_rows_admit_lr,
sr3_rows_frames). The oracle is the uniform sampler at B = SLOTS, with sr3_set_lr_consistency for a held
row and without it for a row that is not held: short batches padded, the LR rows gathered per chunk, row_offset 0. A held
plane runs the stages of the uniform projection on its own LR image and an unheld plane is skipped, so every comparison is
tobytes() equality; the only bar is BAR_OP of test_gpu_lr_consistency.py, for the residual itself. Tiny UNet, 4 slots."""
import numpy as np
import pytest

import test_gpu_rows as tr
from conftest import pkg
from test_gpu_lr_consistency import BAR_OP

pytestmark = pytest.mark.gpu
synth = pkg("synth")
schedule = pkg("schedule")
samplers = pkg("samplers")
Sr3Error = pkg("_lib").Sr3Error
F32 = np.float32

SLOTS, R, L, SEED, OFFSET = tr.SLOTS, tr.R, tr.L, tr.SEED, tr.OFFSET
RATIO, CAP = tr.RATIO, tr.CAP
_same, _engine, _staggered = tr._same, tr._engine, tr._staggered
T20 = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}


def _cond(n, H=R, W=R):
    if (H, W) == (R, R):
        return tr._cond(n)
    return np.random.RandomState(SEED + H * W).uniform(-1, 1, (n, 3, H, W)).astype(F32)


def _lr(n, lh=L, lw=L):
    return np.random.RandomState(SEED ^ 0x10C0).uniform(-1, 1, (n, 3, lh, lw)).astype(F32)


def _uniform(e, cond, ids0, lr=None, strength=1.0, frames=False, **kw):
    """rows of uniform calls at B = SLOTS (tr._uniform's chunks and padding), held to lr [n,3,lh,lw] when given; with
    frames, (images [n,...], frames [nf,n,...])"""
    n, out, frs = cond.shape[0], [], []
    for a in range(0, n, SLOTS):
        idx = [min(a + j, n - 1) for j in range(SLOTS)]
        k = dict(kw)
        if k.get("init") is not None:
            k["init"] = k["init"][idx]
        dl = None
        if lr is not None:
            dl = e.to_device(np.ascontiguousarray(lr[idx]))
            e.set_lr_consistency(dl.ptr, SLOTS, lr.shape[2], lr.shape[3], 0, strength)
        got = e.sample_np(cond[idx], seed=SEED, image_offset=ids0 + a, frames=frames, **k)
        e.synchronize()
        e.set_lr_consistency(None)
        if dl is not None:
            dl.free()
        got, fr = got if frames else (got, None)
        out.append(got[:min(SLOTS, n - a)])
        if frames:
            frs.append(fr[:, :min(SLOTS, n - a)])
    out = np.concatenate(out)
    return (out, np.concatenate(frs, axis=1)) if frames else out


def _plain_session_ok(e, cond, want, what):
    got, _ = e.rows_np([{"cond": cond[i], "image_id": OFFSET + i} for i in range(SLOTS)], SLOTS, seed=SEED)
    _same(np.stack(got), want, what)


# ---- 1. all rows admitted at the top, every row held ----------------------------------------------------------------------
@pytest.mark.parametrize("prec", tr.PRECISIONS)
@pytest.mark.parametrize("kind,steps", tr.KINDS, ids=tr.KIND_IDS)
def test_held_rows_admitted_at_the_top_are_the_uniform_lr_call(kind, steps, prec):
    cond, lr = _cond(SLOTS), _lr(SLOTS)
    e = _engine(kind, steps, prec)
    want = _uniform(e, cond, OFFSET, lr)
    assert np.abs(want - _uniform(e, cond, OFFSET)).max() > 1e-3        # (the projection is live on these inputs)
    reqs = [{"cond": cond[i], "image_id": OFFSET + i, "lr": lr[i]} for i in range(SLOTS)]
    got, trace = e.rows_np(reqs, SLOTS, seed=SEED)
    assert len(trace) == tr._steps(kind, steps) and all(t == [0, 1, 2, 3] for t in trace)
    _same(np.stack(got), want, f"{kind} {prec}")
    assert e.fallback_calls() == 0
    e.close()


# ---- 2. staggered, held and unheld rows side by side ----------------------------------------------------------------------
STAGGERED = [("dpmpp_2m", 4, 8, 8, 16, 16), ("ddpm", None, 8, 8, 16, 16), ("dpmpp_2m", 4, 8, 12, 16, 24), ("dpmpp_2m", 4, 10, 10, 24, 24)]


@pytest.mark.parametrize("kind,steps,lh,lw,H,W", STAGGERED, ids=[f"{c[0]}_{c[2]}x{c[3]}to{c[4]}x{c[5]}" for c in STAGGERED])
def test_staggered_held_and_unheld_rows(kind, steps, lh, lw, H, W):
    """images 0, 2, 4 are held and 1, 3, 5 are not; an idle slot (not yet used, or retired) keeps its bytes"""
    S = tr._steps(kind, steps)
    cond, lr = _cond(6, H, W), _lr(6, lh, lw)
    e = _engine(kind, steps)
    held, free = _uniform(e, cond, OFFSET, lr), _uniform(e, cond, OFFSET)
    assert all(np.abs(held[i] - free[i]).max() > 1e-3 for i in range(6))
    reqs = [dict({"cond": cond[i], "image_id": OFFSET + i, "at": at}, **({"lr": lr[i]} if i % 2 == 0 else {}))
            for i, at in enumerate(_staggered(S))]
    snaps = []

    def read_back(k):
        got = e.read_packed_state()
        snaps.append(None if got is None else (got[0].copy(), got[1].copy()))

    got, trace = e.rows_np(reqs, SLOTS, seed=SEED, on_step=read_back)
    assert trace[0] == [0, 1, None, None] and trace[3] == [0, 1, 2, 3] and trace[S] == [4, 5, 2, 3] and len(trace) == 2 * S
    for i in range(6):
        _same(got[i], (held if i % 2 == 0 else free)[i], f"image {i} ({'held' if i % 2 == 0 else 'not held'})")
    if (H, W) == (R, R):
        assert snaps[0] is not None, "the 16x16 tiny UNet keeps a packed state"
    if snaps[0] is not None:
        idle = 0
        for k in range(len(trace)):
            for s in range(SLOTS):
                if trace[k][s] is not None:
                    continue
                idle += 1
                for part in (0, 1):
                    if all(trace[j][s] is None for j in range(k + 1)):
                        assert not snaps[k][part][s].any(), (k, s)       # never used: the zeros of sr3_rows_begin
                    else:
                        assert snaps[k][part][s].tobytes() == snaps[k - 1][part][s].tobytes(), (k, s)
        assert idle >= 5
    e.close()


def test_a_session_that_takes_the_scratch_form():
    """96 -> 128: (H + lh) * lw floats are 84 KB, above the LDS form's 64 KB, so the session's steps run the four-launch
    projection over the scratch of B * C planes (the uniform oracle picks the same form). Rows 0 and 2 held, row 1 not,
    slot 3 idle; a second session replays the captured step."""
    kind, S, l, r = "dpmpp_2m", 4, 96, 128
    cond, lr = _cond(3, r, r), _lr(3, l, l)
    e = _engine(kind, S)
    with pytest.raises(Sr3Error, match="LDS form needs"):
        e.lr_project_np(cond[:1], lr[:1], form="lds")
    held, free = _uniform(e, cond, OFFSET, lr), _uniform(e, cond, OFFSET)
    reqs = [dict({"cond": cond[i], "image_id": OFFSET + i}, **({"lr": lr[i]} if i != 1 else {})) for i in range(3)]
    n0 = e.step_graph_captures()
    for session in ("first", "second"):
        got, trace = e.rows_np(reqs, SLOTS, seed=SEED)
        assert trace == [[0, 1, 2, None]] * S
        for i in range(3):
            assert np.abs(held[i] - free[i]).max() > 1e-3
            _same(got[i], (free if i == 1 else held)[i], f"{session} session, image {i}")
    assert e.step_graph_captures() - n0 == 1
    e.close()


# ---- 3. a reused slot -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_held", [True, False], ids=["held_then_unheld", "unheld_then_held"])
def test_a_reused_slot_does_not_read_the_lr_image_of_its_last_occupant(first_held):
    kind, S = "dpmpp_2m", 4
    cond, lr = _cond(2), _lr(2)
    e = _engine(kind, S)
    want_held, want_free = _uniform(e, cond[1:2], 9, lr[1:2])[0], _uniform(e, cond[1:2], 9)[0]
    assert np.abs(want_held - want_free).max() > 1e-3
    first = {"cond": cond[0], "image_id": 5, "slot": 0}
    second = {"cond": cond[1], "image_id": 9, "slot": 0, "at": S}
    (first if first_held else second)["lr"] = lr[0] if first_held else lr[1]
    # (the session must be armed either way: the numpy session arms itself when any request carries an lr)
    out, trace = e.rows_np([first, second], SLOTS, seed=SEED)
    assert trace[0] == [0, None, None, None] and trace[S] == [1, None, None, None]
    _same(out[1], want_free if first_held else want_held, "the second occupant of slot 0")
    e.close()


# ---- 4. strength per row --------------------------------------------------------------------------------------------------
def test_strength_is_per_row():
    kind, S = "ddim", 4
    cond, lr = _cond(SLOTS), _lr(SLOTS)
    strengths = [1.0, 0.5, 0.5, 1.0]
    e = _engine(kind, S)
    want = {s: _uniform(e, cond, OFFSET, lr, strength=s) for s in (1.0, 0.5)}
    assert np.abs(want[1.0] - want[0.5]).max() > 1e-3
    reqs = [{"cond": cond[i], "image_id": OFFSET + i, "lr": lr[i], "lr_strength": strengths[i]} for i in range(SLOTS)]
    got, _ = e.rows_np(reqs, SLOTS, seed=SEED)
    for i, s in enumerate(strengths):
        _same(got[i], want[s][i], f"row {i} at strength {s}")
    e.close()


# ---- 5. with the dynamic threshold ----------------------------------------------------------------------------------------
def test_staggered_held_rows_with_the_dynamic_threshold():
    """one engine runs both chunks of the oracle, a thresholded call of 6 (a larger workspace), the session and the first
    chunk again, as test_gpu_rows.py::test_staggered_rows_with_the_dynamic_threshold does (the replay
    difference that kept these apart went with the memset node of the select)"""
    kind, S = "dpmpp_2m", 4
    cond, lr = _cond(6), _lr(6)
    e = _engine(kind, S)
    only_lr = _uniform(e, cond[:SLOTS], OFFSET, lr[:SLOTS])
    e.set_dynamic_threshold(RATIO, CAP)
    want = [_uniform(e, cond[:SLOTS], OFFSET, lr[:SLOTS])]
    assert np.abs(want[0] - only_lr).max() > 1e-3           # (the threshold is live on these inputs)
    want.append(_uniform(e, cond[SLOTS:], OFFSET + SLOTS, lr[SLOTS:]))
    want = np.concatenate(want)
    e.sample_np(cond, seed=SEED, image_offset=OFFSET)       # (B = 6: the session's workspace replaces a larger one)
    reqs = [{"cond": cond[i], "image_id": OFFSET + i, "at": at, "lr": lr[i]} for i, at in enumerate(_staggered(S))]
    n0 = e.dynamic_threshold_launches()
    got, trace = e.rows_np(reqs, SLOTS, seed=SEED)
    assert trace[S] == [4, 5, 2, 3] and e.dynamic_threshold_launches() - n0 == 2 * S
    _same(np.stack(got), want, "thresholded and held")
    _same(_uniform(e, cond[:SLOTS], OFFSET, lr[:SLOTS]), want[:SLOTS], "the first chunk again, after the session")
    e.close()


# ---- 6. consistency itself ------------------------------------------------------------------------------------------------
def test_held_rows_downsample_to_their_lr_image_and_unheld_rows_do_not():
    kind, S = "dpmpp_2m", 4
    cond, lr = _cond(SLOTS), _lr(SLOTS)
    e = _engine(kind, S)
    # the uniform oracle alone shows the gap on these inputs (test_reference_chain_shows_the_gap's bars)
    res_free = e.lr_residual_np(_uniform(e, cond, OFFSET), lr)["max_abs"]
    res_held = e.lr_residual_np(_uniform(e, cond, OFFSET, lr), lr)["max_abs"]
    print(f"uniform oracle, max |A img - y| per image: free {res_free}, held {res_held}")
    assert res_free.min() > 1e-2 and res_held.max() <= BAR_OP
    reqs = [dict({"cond": cond[i], "image_id": OFFSET + i}, **({"lr": lr[i]} if i % 2 == 0 else {})) for i in range(SLOTS)]
    got, _ = e.rows_np(reqs, SLOTS, seed=SEED)
    res = e.lr_residual_np(np.stack(got), lr)["max_abs"]
    print(f"row session, max |A img - y| per row: {res}")
    assert res[[0, 2]].max() <= BAR_OP
    assert res[[1, 3]].min() > BAR_OP
    e.close()


# ---- 7. both forms of the rows projection, alone --------------------------------------------------------------------------
OP_SHAPES = [(8, 8, 16, 16), (8, 12, 16, 24), (10, 10, 24, 24), (16, 16, 64, 64)]


@pytest.fixture(scope="module")
def op_engine():
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    yield e
    e.close()


@pytest.mark.parametrize("lh,lw,H,W", OP_SHAPES, ids=[f"{a}x{b}to{c}x{d}" for a, b, c, d in OP_SHAPES])
def test_both_forms_of_the_rows_projection(op_engine, lh, lw, H, W):
    """B = 4: row 0 held at 1.0, row 1 idle (its strength must not matter), row 2 live and not held, row 3 held at 0.5"""
    rs = np.random.RandomState(lh * 1000 + W)
    x = np.clip(rs.standard_normal((4, 3, H, W)), -1, 1).astype(F32)
    y = rs.uniform(-1, 1, (4, 3, lh, lw)).astype(F32)
    live, strengths = [1, 0, 1, 1], [1.0, 1.0, 0.0, 0.5]
    got = {form: op_engine.lr_project_rows_np(x, y, strengths, live, form=form) for form in ("lds", "scratch", "auto")}
    for form in ("lds", "scratch"):
        for b in (0, 3):
            want = op_engine.lr_project_np(x[b:b + 1], y[b:b + 1], strength=strengths[b], form=form)
            assert np.abs(want - x[b:b + 1]).max() > 1e-3
            _same(got[form][b:b + 1], want, f"{form}: held row {b}")
        for b in (1, 2):
            _same(got[form][b], x[b], f"{form}: row {b}, which is not held")
    _same(got["lds"], got["scratch"], "LDS form against scratch form")
    _same(got["auto"], got["lds"], "auto")
    with pytest.raises(Sr3Error, match="strength"):
        op_engine.lr_project_rows_np(x, y, [1.0, 1.0, 0.0, 1.5], live)


# ---- 8. frames ------------------------------------------------------------------------------------------------------------
def _engine_T20():
    cfg, sd = tr._weights()
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    with np.errstate(divide="ignore", invalid="ignore"):
        e.set_schedule(schedule.schedule_buffers(T20))
    return e


@pytest.mark.parametrize("kind", ["ddpm_T20", "dpmpp_2m_S4"])
def test_frames_per_row(kind):
    """rows 0 and 1 from the top with frames, row 2 a warm start below the top with frames, row 3 without frames; T = 20
    writes a frame every third step (1 | T // 10), so which steps carry a frame pointer matters"""
    e, S, k = (_engine_T20(), 20, 7) if kind == "ddpm_T20" else (_engine("dpmpp_2m", 4), 4, 2)
    cond = _cond(SLOTS)
    init = np.random.RandomState(SEED + 1).uniform(-1, 1, (SLOTS, 3, R, R)).astype(F32)
    top, top_fr = _uniform(e, cond, OFFSET, frames=True)
    warm, warm_fr = _uniform(e, cond, OFFSET, frames=True, init=init, start_step=k)
    assert top_fr.shape[0] == e.num_frames() and warm_fr.shape[0] == e.num_frames(k) < top_fr.shape[0]
    if S == 20:
        assert (top_fr.shape[0], warm_fr.shape[0]) == (7, 3)
    reqs = [{"cond": cond[0], "image_id": OFFSET, "frames": True},
            {"cond": cond[1], "image_id": OFFSET + 1, "frames": True},
            {"cond": cond[2], "image_id": OFFSET + 2, "frames": True, "init": init[2], "start_step": k},
            {"cond": cond[3], "image_id": OFFSET + 3}]
    got, _ = e.rows_np(reqs, SLOTS, seed=SEED)
    for b in (0, 1):
        _same(got[b][0], top[b], f"row {b}")
        _same(got[b][1], top_fr[:, b], f"frames of row {b}")
        _same(got[b][1][-1], top[b], f"last frame of row {b}")
    _same(got[2][0], warm[2], "warm row")
    _same(got[2][1], warm_fr[:, 2], "frames of the warm row")
    _same(got[3], top[3], "the row without frames")
    # a capacity below the count fails and changes nothing: the row then takes a buffer of the right size
    dc, out = e.to_device(cond[0]), e.buffer(3 * R * R)
    nf = e.num_frames()
    fr = e.buffer(nf * 3 * R * R)
    e.rows_begin(SLOTS, R, R, SEED)
    e.rows_admit(0, dc.ptr, OFFSET)
    with pytest.raises(Sr3Error, match="capacity"):
        e.rows_frames(0, fr.ptr, nf - 1)
    with pytest.raises(Sr3Error, match="idle"):
        e.rows_frames(1, fr.ptr, nf)
    e.rows_frames(0, fr.ptr, nf)
    assert e.rows_step() == 1
    with pytest.raises(Sr3Error, match="first step"):
        e.rows_frames(0, fr.ptr, nf)
    while e.rows_position(0) > 0:
        e.rows_step()
    e.rows_retire(0, out.ptr)
    _same(out.download((3, R, R)), top[0], "after the refused calls")
    _same(fr.download((nf, 3, R, R)), top_fr[:, 0], "frames after the refused calls")
    e.rows_end()
    e.close()


# ---- 9. graphs ------------------------------------------------------------------------------------------------------------
def test_an_armed_session_adds_one_graph_and_leaves_the_unarmed_one_alone():
    kind, S = "dpmpp_2m", 4
    cond, lr = _cond(6), _lr(6)
    e = _engine(kind, S)
    held, free = _uniform(e, cond, OFFSET, lr), _uniform(e, cond, OFFSET)
    armed = [{"cond": cond[i], "image_id": OFFSET + i, "at": at, "lr": lr[i]} for i, at in enumerate(_staggered(S))]
    n0 = e.step_graph_captures()
    unarmed = tr._run_staggered(e, cond, S)
    n1 = e.step_graph_captures()
    first, _ = e.rows_np(armed, SLOTS, seed=SEED)
    n2 = e.step_graph_captures()
    second, _ = e.rows_np(armed, SLOTS, seed=SEED)
    n3 = e.step_graph_captures()
    again = tr._run_staggered(e, cond, S)
    n4 = e.step_graph_captures()
    assert (n1 - n0, n2 - n1, n3 - n2, n4 - n3) == (1, 1, 0, 0)
    _same(np.stack(first), held, "first armed session")
    _same(np.stack(second), held, "second armed session")
    _same(unarmed, free, "unarmed session")
    _same(again, free, "unarmed session after the armed ones")
    e.close()


# ---- 10. errors -----------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    kind, S = "dpmpp_2m", 4
    cond, lr = _cond(SLOTS), _lr(SLOTS)
    e = _engine(kind, S)
    want = _uniform(e, cond, OFFSET)
    dc, dl = e.to_device(cond[0]), e.to_device(lr[0])
    # arming after an admit
    e.rows_begin(SLOTS, R, R, SEED)
    e.rows_admit(0, dc.ptr, OFFSET)
    with pytest.raises(Sr3Error, match="admitted already"):
        e.rows_lr_consistency(L, L)
    # an LR image for a session that is not armed
    with pytest.raises(Sr3Error, match="not armed"):
        e.rows_admit(1, dc.ptr, OFFSET + 1, lr=dl.ptr)
    assert e.rows_position(1) == -1
    e.rows_end()
    _plain_session_ok(e, cond, want, "after arming too late and an LR image for an unarmed session")
    # a strength outside [0, 1]
    e.rows_begin(SLOTS, R, R, SEED)
    e.rows_lr_consistency(L, L)
    for bad in (1.5, -0.25, float("nan")):
        with pytest.raises(Sr3Error, match="strength"):
            e.rows_admit(0, dc.ptr, OFFSET, lr=dl.ptr, lr_strength=bad)
        assert e.rows_position(0) == -1
    e.rows_end()
    _plain_session_ok(e, cond, want, "after a strength outside [0, 1]")
    # an LR size that cannot constrain H x W: the message of the uniform path
    e.rows_begin(SLOTS, R, R, SEED)
    for lh, lw in ((R, R), (L, R), (0, L)):
        with pytest.raises(Sr3Error, match="an LR size below the image size"):
            e.rows_lr_consistency(lh, lw)
    e.rows_end()
    with pytest.raises(Sr3Error, match="outside a row session"):
        e.rows_lr_consistency(L, L)
    _plain_session_ok(e, cond, want, "after an LR size that cannot constrain the image")
    e.close()
