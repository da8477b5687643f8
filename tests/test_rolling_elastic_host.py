"""The host side of elastic rolling sessions (rolling.RollingSampler(elastic=True), DESIGN.md §3.5g "live rows only"):
the ladder, the compaction policy, the slot bookkeeping through moves and restarts — against the recording fake of
tests/test_rolling_host.py, extended here by the three calls an elastic session adds — and the property of the
batch-invariant dispatch plans that lets a step run over a prefix of the workspace at all. No GPU, no torch."""
import functools
import itertools
import warnings

import pytest

from conftest import pkg

import test_batch_invariant_host as inv
import test_rolling_host as host

rolling = pkg("rolling")
engine = pkg("engine")
Sr3Error = pkg("_lib").Sr3Error
Buf = host.Buf


class ElasticFake(host.FakeEngine):
    """FakeEngine with the library's rules for sr3_rows_step_batch and sr3_rows_move; mode: what batch_invariant() says"""

    def __init__(self, S=4, mode=64, **kw):
        super().__init__(S=S, **kw)
        self.mode, self.batches, self.moved = mode, [], []

    def batch_invariant(self):
        return self.mode

    def rows_step(self, noise_ptrs=None, batch=None):
        slots = len(self.pos)
        b = slots if batch is None else batch
        if not 1 <= b <= slots:
            raise Sr3Error(f"sr3_rows_step_batch: batch {b} outside [1, {slots}]")
        if b < slots and not self.mode:
            raise Sr3Error("sr3_rows_step_batch: needs sr3_set_batch_invariant")
        for r, p in enumerate(self.pos):
            if p > 0 and r >= b:
                raise Sr3Error(f"sr3_rows_step_batch: slot {r} is live and lies outside batch {b}")
        n = super().rows_step(noise_ptrs)
        if n:
            self.batches.append(b)
        return n

    def rows_move(self, src, dst):
        if self.pos[src] < 0:
            raise Sr3Error(f"sr3_rows_move: source slot {src} is idle")
        if self.pos[dst] >= 0:
            raise Sr3Error(f"sr3_rows_move: destination slot {dst} is live")
        self.calls.append(("move", src, dst, self.ids[src]))
        self.moved.append((src, dst))
        for a in (self.pos, self.ids, self.ran):
            a[dst] = a[src]
        self.pos[src], self.ids[src], self.ran[src] = -1, None, 0


def _sampler(eng, slots=4, **kw):
    return rolling.RollingSampler(eng, slots, eng.T, seed=5, alloc=lambda r: Buf((3, 16, 16)), elastic=True, **kw)


def _books_agree(rs, eng):
    """the scheduler's slots hold the requests the library's slots hold, with the same steps left"""
    if eng.pos is None:             # (no session yet)
        assert all(r is None for r in rs._rows)
        return
    for s, r in enumerate(rs._rows):
        if r is None:
            assert eng.pos[s] <= 0, f"slot {s}: the scheduler thinks it free, the engine has {eng.pos[s]} steps left there"
        else:
            assert (eng.ids[s], eng.pos[s]) == (r.image_id, rs._left[s]), f"slot {s}"


# ---- ladder ---------------------------------------------------------------------------------------------------------
def test_default_ladder():
    assert rolling.default_ladder(64) == (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)
    assert rolling.default_ladder(6) == (1, 2, 3, 4, 6)
    assert rolling.default_ladder(5) == (1, 2, 3, 4, 5)
    assert rolling.default_ladder(1) == (1,)
    assert rolling.default_ladder(100) == (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 100)
    for slots in range(1, 130):
        lad = rolling.default_ladder(slots)
        assert lad[-1] == slots and len(lad) <= rolling.MAX_LADDER and rolling.check_ladder(lad, slots) == lad
    assert rolling.check_ladder(None, 6) == (1, 2, 3, 4, 6)
    assert rolling.check_ladder([2, 4], 4) == (2, 4)


@pytest.mark.parametrize("ladder,slots,what", [
    ([], 4, "increasing"), ([0, 4], 4, "positive"), ([1, 3, 2, 4], 4, "increasing"), ([1, 2, 2, 4], 4, "increasing"),
    ([1, 2], 4, "end at"), ([1, 2, 4, 8], 4, "end at"), (list(range(1, 18)), 17, "at most 16"),
])
def test_a_bad_ladder_is_refused(ladder, slots, what):
    with pytest.raises(ValueError, match=what):
        rolling.check_ladder(ladder, slots)
    with pytest.raises(ValueError, match=what):
        _sampler(ElasticFake(), slots=slots, ladder=ladder)


def test_a_ladder_without_elastic_is_refused():
    with pytest.raises(ValueError, match="elastic"):
        rolling.RollingSampler(ElasticFake(), 4, 4, ladder=[1, 4])


def test_ladder_choice_second_move():
    # three live rows at 2, 3, 5 of six: b = 3; the row at 5 goes to 0, then the row at 3 to 1; batch 3
    assert rolling.elastic_plan([False, False, True, True, False, True], (1, 2, 3, 4, 6)) == ([(5, 0), (3, 1)], 3)


@pytest.mark.parametrize("slots,ladder", [(4, (1, 2, 4)), (6, None), (7, (1, 3, 7)), (5, (5,))])
def test_moves_only_where_they_lower_the_batch(slots, ladder):
    """every occupancy pattern: the plan's moves take rows from at or above b to below it, the batch is the smallest
    entry that holds the live rows whenever anything moved, it always covers the highest live slot, and nothing moves
    when the rows already sit below b"""
    lad = rolling.check_ladder(ladder, slots)
    for occ in itertools.product([False, True], repeat=slots):
        live = sum(occ)
        if not live:
            assert rolling.elastic_plan(occ, lad) == ([], lad[0])
            continue
        b = next(x for x in lad if x >= live)
        before = next(x for x in lad if x >= max(s for s, o in enumerate(occ) if o) + 1)
        moves, batch = rolling.elastic_plan(occ, lad)
        now = list(occ)
        for src, dst in moves:
            assert now[src] and not now[dst] and src >= b > dst
            assert dst == now.index(False) and src == max(s for s, o in enumerate(now) if o)
            now[src], now[dst] = False, True
        top = max(s for s, o in enumerate(now) if o)
        assert batch in lad and top < batch and batch == next(x for x in lad if x >= top + 1)
        assert sum(now) == live
        if moves:
            assert batch == b < before
        else:
            assert batch == before
        if live == slots:
            assert (moves, batch) == ([], slots)


def test_ladder_choice_cases():
    plan = rolling.elastic_plan
    F, T = False, True
    assert plan([F, F, F, T], (1, 2, 4)) == ([(3, 0)], 1)
    assert plan([T, F, T, T], (1, 2, 4)) == ([], 4)               # three rows take batch 4 wherever they sit: no move
    assert plan([T, F, T, F], (1, 2, 4)) == ([(2, 1)], 2)
    assert plan([F, T, F, F], (1, 2, 4)) == ([(1, 0)], 1)
    assert plan([T, T, T, T], (1, 2, 4)) == ([], 4)
    assert plan([F, T, T, F], (1, 2, 4)) == ([(2, 0)], 2)
    assert plan([F, F, F, F], (1, 2, 4)) == ([], 1)


# ---- sessions against the fake ----------------------------------------------------------------------------------------
def test_mode_off_is_refused():
    with pytest.raises(ValueError, match="set_batch_invariant"):
        _sampler(ElasticFake(mode=0))
    with pytest.raises(ValueError, match="set_batch_invariant"):
        _sampler(host.FakeEngine())                 # (an engine that knows no mode has none)
    # and without elastic the same engines serve as before
    rs = rolling.RollingSampler(ElasticFake(mode=0), 2, 4)
    assert rs.ladder == (2,) and not rs.elastic


def test_a_full_session_never_moves():
    eng = ElasticFake(S=4)
    rs = _sampler(eng, slots=4)
    for _ in range(12):
        rs.submit(Buf())
    out = rs.drain()
    assert sorted(t for t, _ in out) == list(range(12))
    assert rs.moves == 0 and eng.moved == [] and rs.batch_trace == [4] * 12 == eng.batches
    rs.close()


def test_a_lone_request_runs_at_batch_one():
    eng = ElasticFake(S=4)
    rs = _sampler(eng, slots=64)
    rs.submit(Buf())
    rs.drain()
    assert rs.batch_trace == [1] * 4 and rs.moves == 0
    rs.close()


def test_every_step_covers_the_live_rows_and_moves_lower_the_batch():
    """strengths chosen so that low slots free up under a long row at a high slot"""
    eng = ElasticFake(S=8)
    rs = _sampler(eng, slots=6)
    assert rs.ladder == (1, 2, 3, 4, 6)
    for strength in (0.25, 0.25, 0.5, 0.25, None, 0.75):
        rs.submit(Buf(), strength=strength)
    n_moves = 0
    while rs.pending:
        at = len(eng.calls)
        rs.step()                   # (ElasticFake.rows_step raises if a live row sits outside the batch)
        _books_agree(rs, eng)
        new = eng.calls[at:]
        moves = [c for c in new if c[0] == "move"]
        step = next(c for c in new if c[0] == "step")
        live, batch = len(step[1]), rs.batch_trace[-1]
        assert batch == next(x for x in rs.ladder if x >= max(step[1]) + 1)
        if moves:
            # they happened before the step and the step runs at the smallest batch that holds its rows
            assert new.index(moves[-1]) < new.index(step) and batch == next(x for x in rs.ladder if x >= live)
        n_moves += len(moves)
        rs.poll()
    assert rs.batch_trace == eng.batches
    # 6 live for two steps, then 0, 1, 3 retire: rows at 2, 4, 5 -> b = 3: two moves; later the long rows compact further
    assert rs.batch_trace[:3] == [6, 6, 3] and rs.moves == n_moves == len(eng.moved) >= 3
    assert rs.batch_trace[-1] == 1 and sum(rs.batch_trace) < 6 * len(rs.batch_trace)
    assert len(rs.trace) == len(rs.batch_trace) and all(len(t) == 3 for t in rs.trace)
    rs.close()


def test_stream_of_ten_through_four_slots():
    eng = ElasticFake(S=4)
    rs = _sampler(eng, slots=4, ladder=(1, 2, 4))
    strengths = [None, 0.5, 0.25, None, 0.5, None, 0.25, 0.25, None, 0.5]
    seen = []

    def source():
        for s in strengths:
            _books_agree(rs, eng)
            yield {"x_in_row": Buf(), "strength": s}

    for t, _ in rs.stream(source()):
        seen.append(t)
        _books_agree(rs, eng)
    assert sorted(seen) == list(range(10)) and len(set(seen)) == 10
    done = {}
    for img_id, _, ran in eng.finished:
        assert img_id not in done
        done[img_id] = ran
    assert [done[i] for i in range(10)] == [4 if s is None else max(1, round(s * 4)) for s in strengths]
    assert rs.moves == len(eng.moved) > 0 and min(rs.batch_trace) < 4 and set(rs.batch_trace) <= {1, 2, 4}
    # the slots stayed full while the source had something to give, elastic or not
    assert all(live == 4 or (queued == 0 and exhausted) for live, queued, exhausted in rs.trace)
    rs.close()


def test_bookkeeping_after_a_restart():
    """a range trip mid-flight after rows have moved: the dropped slots are the ones the rows sit in NOW, every request
    is re-admitted and finishes once more, one arithmetic down"""
    eng = ElasticFake(S=8, trip_at=3)
    eng.precision = "f16f8"
    rs = _sampler(eng, slots=4, ladder=(1, 2, 4), precision="f16f8")
    for strength in (0.125, 0.125, None, None):     # rows 0 and 1 retire after one step: rows 2, 3 move to 0, 1
        rs.submit(Buf(), strength=strength)
    rs.step()
    assert [t for t, _ in rs.poll()] == [0, 1]
    rs.step()
    assert eng.moved == [(3, 0), (2, 1)] and rs.batch_trace == [4, 2]
    _books_agree(rs, eng)
    rs.step()                                       # (the flag goes up here)
    rs.submit(Buf(), strength=0.125)                # finishes at the next step, which makes poll check the range
    rs.step()
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        assert rs.poll() == []
    assert rs.restarts == 1 and rs.precision == "f16x3"
    drops = [c for c in eng.calls if c[0] == "drop"]
    assert sorted((c[1], c[2]) for c in drops) == [(0, 3), (1, 2)]      # (slot, image id): where the rows had moved to
    _books_agree(rs, eng)
    out = rs.drain()
    assert sorted(t for t, _ in out) == [2, 3, 4]
    _books_agree(rs, eng)
    fin = {}
    for img_id, prec, ran in eng.finished:
        fin.setdefault(img_id, []).append((prec, ran))
    assert fin[2] == [("f16x3", 8)] and fin[3] == [("f16x3", 8)] and fin[4] == [("f16f8", 1), ("f16x3", 1)]
    rs.close()


# ---- plans: why a step may run over a prefix of the workspace -------------------------------------------------------------
PLAN_UNETS = [("A", 48), ("B", 32), ("C", 64), ("D", 32), ("yml128", 128)]


@functools.lru_cache(maxsize=None)
def _plan(P, B, conv, prec):
    return engine.conv_plan(B, *conv, precision=prec, stats=True, plan_batch=P)


@pytest.mark.parametrize("P", [1, 64])
@pytest.mark.parametrize("prec", inv.PRECISIONS)
@pytest.mark.parametrize("name,size", PLAN_UNETS)
def test_a_smaller_batch_asks_no_more_of_the_workspace(name, size, prec, P):
    """for every conv and every pair B' < B of the default ladder up to the mode's maximum batch: the same kernel, tile and
    split count, the same statistics slices per image, and split-K partials and Winograd workspace at B' within those at
    B — what sr3_rows_step_batch relies on when it launches a step for rows [0, B') of a workspace carved at B"""
    bmax = min(inv.mode_max_batch(name, size, prec, P), 64)
    ladder = rolling.default_ladder(bmax)
    for conv in inv._convs(name, size):
        got = [_plan(P, B, conv, prec) for B in ladder]
        for i, small in enumerate(got):
            for big in got[i + 1:]:
                for k in ("kernel", "tile", "split", "splits", "phases", "stats_slices", "needs_wino_frag", "f8"):
                    assert small[k] == big[k], f"{name} P={P} {prec} conv {conv}: {k} moves along the ladder"
                assert small["part_floats"] <= big["part_floats"], f"{name} P={P} {prec} conv {conv}: split-K partials"
                assert small["wino_ws_floats"] <= big["wino_ws_floats"], f"{name} P={P} {prec} conv {conv}: Winograd workspace"
