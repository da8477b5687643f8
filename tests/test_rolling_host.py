"""The host side of the rolling-batch sampler (rolling.RollingSampler) against a fake engine that
records calls: the slot scheduler, ticket order, queueing beyond the slots, the occupancy trace of stream() and the
bookkeeping of a range-trip restart. No GPU, no torch."""
import warnings

import pytest

from conftest import pkg

rolling = pkg("rolling")
Sr3Error = pkg("_lib").Sr3Error
Sr3RangeWarning = pkg("_lib").Sr3RangeWarning


class Buf:
    """stands in for a device tensor: an address and a shape"""
    _next = 0x1000

    def __init__(self, shape=(6, 16, 16)):
        self.shape = shape
        Buf._next += 0x100
        self.addr = Buf._next

    def data_ptr(self):
        return self.addr


class FakeEngine:
    """Engine's rows_* surface with the library's own bookkeeping and error rules; trip_at: the range check fails once
    when it is made after that many steps (or more) in a split arithmetic."""

    def __init__(self, S=4, trip_at=None, replay=False):
        self.replay = replay        # the trip is the library's "a bounded wait gave up" report, not an overflow
        self.T, self.calls, self.pos, self.open = S, [], None, False
        self.precision, self.trip_at, self.steps, self.flag = "f32", trip_at, 0, False
        self.finished = []          # (image_id, precision, steps it ran) per retired row

    def rows_begin(self, B, H, W, seed=0):
        self.calls.append(("begin", B, H, W, seed))
        self.pos, self.ids, self.ran, self.open = [-1] * B, [None] * B, [0] * B, True

    def rows_admit(self, row, cond_ptr, image_id, init_ptr=None, start_step=None, noised=True, noise0_ptr=None):
        if self.pos[row] >= 0:
            raise Sr3Error(f"sr3_rows_admit: slot {row} is live")
        s0 = self.T if start_step is None else start_step
        assert 1 <= s0 <= self.T and (init_ptr is not None or s0 == self.T)
        self.calls.append(("admit", row, image_id, init_ptr, s0))
        self.pos[row], self.ids[row], self.ran[row] = s0, image_id, 0

    def rows_step(self, noise_ptrs=None):
        live = [r for r, p in enumerate(self.pos) if p > 0]
        if not live:
            return 0
        self.steps += 1
        if self.trip_at is not None and self.steps >= self.trip_at and self.precision != "f32":
            self.flag, self.trip_at = True, None
        for r in live:
            self.pos[r] -= 1
            self.ran[r] += 1
        self.calls.append(("step", tuple(live)))
        return len(live)

    def rows_position(self, row):
        return self.pos[row]

    def rows_retire(self, row, out_ptr):
        if self.pos[row] != 0:
            raise Sr3Error(f"sr3_rows_retire: slot {row} has {self.pos[row]} steps left")
        self.calls.append(("retire", row, self.ids[row]))
        self.finished.append((self.ids[row], self.precision, self.ran[row]))
        self.pos[row] = -1

    def rows_drop(self, row):
        self.calls.append(("drop", row, self.ids[row]))
        self.pos[row] = -1

    def rows_end(self):
        self.calls.append(("end",))
        self.open = False

    def range_check(self):
        self.calls.append(("range_check",))
        if self.flag:
            self.flag = False
            if self.replay:
                raise Sr3Error("sr3_range_check: its bounded wait gave up: this result is invalid; the context now uses the "
                               "conv path without inter-block waits — repeat the call")
            raise Sr3Error("sr3_range_check: an activation exceeded the fp16 range")

    def set_precision(self, name):
        self.calls.append(("precision", name))
        self.precision = name


def _sampler(eng, slots=4, **kw):
    return rolling.RollingSampler(eng, slots, eng.T, seed=5, alloc=lambda r: Buf((3, 16, 16)), **kw)


def test_requests_take_the_lowest_free_slot_and_queue_beyond_the_slots():
    eng = FakeEngine(S=4)
    rs = _sampler(eng, slots=2)
    tickets = [rs.submit(Buf()) for _ in range(5)]
    assert tickets == [0, 1, 2, 3, 4]
    assert eng.calls[0] == ("begin", 2, 16, 16, 5)
    assert [c[1:3] for c in eng.calls if c[0] == "admit"] == [(0, 0), (1, 1)]      # (slot, image id = ticket)
    assert rs.in_flight == 2 and rs.pending == 5
    out = rs.drain()
    assert [t for t, _ in out] == tickets
    # the third and fourth request entered the slots the first two left, in the step that freed them; the fifth waited
    admits = [(i, c[1], c[2]) for i, c in enumerate(eng.calls) if c[0] == "admit"]
    assert [(s, t) for _, s, t in admits] == [(0, 0), (1, 1), (0, 2), (1, 3), (0, 4)]
    steps = [i for i, c in enumerate(eng.calls) if c[0] == "step"]
    assert len(steps) == 12 and admits[2][0] < steps[4] and admits[4][0] < steps[8]
    assert all(n == 4 for _, _, n in eng.finished)
    assert rs.pending == 0 and rs.restarts == 0
    rs.close()
    assert eng.calls[-1] == ("end",) and ("precision", "f32") not in eng.calls


def test_tickets_come_back_in_completion_order():
    """a short warm start admitted later finishes before a full run admitted first"""
    eng = FakeEngine(S=8)
    rs = _sampler(eng, slots=4)
    a = rs.submit(Buf())                            # 8 steps
    b = rs.submit(Buf(), strength=0.25)             # 2 steps, from its own conditioning image
    c = rs.submit(Buf(), init=Buf(), strength=0.5)  # 4 steps from an explicit image
    d = rs.submit(Buf(), init=Buf())                # all 8 steps, from an image noised to the top level
    adm = {c_[2]: c_ for c_ in eng.calls if c_[0] == "admit"}
    assert adm[a][3] is None and adm[a][4] == 8
    assert adm[b][3] is not None and adm[b][4] == 2
    assert adm[c][4] == 4 and adm[d][4] == 8 and adm[d][3] is not None
    got = []
    while rs.pending:
        rs.step()
        got += [(rs.steps_run, t) for t, _ in rs.poll()]
    assert got == [(2, b), (4, c), (8, a), (8, d)]
    assert rs.poll() == []
    rs.close()


def test_explicit_image_ids_and_one_image_size():
    eng = FakeEngine(S=2)
    rs = _sampler(eng)
    rs.submit(Buf(), image_id=40)
    rs.submit(Buf(), image_id=7)
    assert [c[2] for c in eng.calls if c[0] == "admit"] == [40, 7]
    with pytest.raises(ValueError, match="one image size"):
        rs.submit(Buf((6, 16, 24)))
    with pytest.raises(ValueError):
        rolling.RollingSampler(eng, 0, 2)
    rs.close()


def test_stream_keeps_the_slots_full():
    eng = FakeEngine(S=4)
    rs = _sampler(eng, slots=4)
    strengths = [None, 0.5, 0.25, None, 0.5, None, 0.25, 0.25, None, 0.5]
    pulled = []

    def source():
        for i, s in enumerate(strengths):
            pulled.append((i, rs.steps_run))
            yield {"x_in_row": Buf(), "strength": s}

    out = list(rs.stream(source()))
    assert sorted(t for t, _ in out) == list(range(10))
    # never an idle slot while the source still had a request
    assert rs.trace and all(live == 4 or (queued == 0 and exhausted) for live, queued, exhausted in rs.trace)
    # the source is read lazily: the fifth request is pulled only after a slot came free
    assert pulled[4][1] >= 1
    done_at = {}
    for img_id, _, ran in eng.finished:
        done_at[img_id] = ran
    assert [done_at[i] for i in range(10)] == [4 if s is None else max(1, round(s * 4)) for s in strengths]
    rs.close()


def test_range_trip_restarts_what_it_can_have_touched():
    """S = 4, 2 slots, split arithmetic. Requests 0 and 1 finish after 4 steps and are delivered by a clean check. The
    flag is raised during step 6: requests 2 and 3 are in flight (2 steps done). They finish after step 8, the check
    trips: both go back to their start one arithmetic down; the delivered results stay delivered."""
    eng = FakeEngine(S=4, trip_at=6)
    eng.precision = "f16f8"
    rs = _sampler(eng, slots=2, precision="f16f8")
    for _ in range(5):
        rs.submit(Buf())
    first = []
    while len(first) < 2:
        rs.step()
        first += rs.poll()
    assert [t for t, _ in first] == [0, 1] and rs.restarts == 0
    kept = [(t, o.data_ptr()) for t, o in first]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        rest = rs.drain()
    assert any(issubclass(w.category, Sr3RangeWarning) for w in rec)
    assert rs.restarts == 1 and rs.precision == "f16x3"
    assert [t for t, _ in rest] == [2, 3, 4]
    # requests 2 and 3 were retired once in f16f8 (never delivered), then again in f16x3 after all 4 steps
    fin = {}
    for img_id, prec, ran in eng.finished:
        fin.setdefault(img_id, []).append((prec, ran))
    assert fin[0] == [("f16f8", 4)] and fin[1] == [("f16f8", 4)]
    assert fin[2] == [("f16f8", 4), ("f16x3", 4)] and fin[3] == [("f16f8", 4), ("f16x3", 4)]
    assert fin[4] == [("f16x3", 4)]
    # re-admitted oldest first, in front of the request that was still queued
    i = eng.calls.index(("precision", "f16x3"))
    assert [c[2] for c in eng.calls[i:] if c[0] == "admit"] == [2, 3, 4]
    assert [(t, o.data_ptr()) for t, o in first] == kept
    rs.close()
    assert eng.calls[-2:] == [("end",), ("precision", "f16f8")]        # the arithmetic is put back


def test_range_trip_mid_flight_drops_live_rows():
    """the check trips while rows are mid-trajectory: they are dropped, not retired"""
    eng = FakeEngine(S=4, trip_at=1)
    eng.precision = "f16x3"
    rs = _sampler(eng, slots=2, precision="f16x3")
    rs.submit(Buf(), strength=0.25)     # 1 step
    rs.submit(Buf())                    # 4 steps
    rs.step()
    with pytest.warns(Sr3RangeWarning):
        assert rs.poll() == []
    assert ("drop", 1, 1) in eng.calls and rs.restarts == 1 and rs.precision == "f32"
    out = rs.drain()
    assert [t for t, _ in out] == [0, 1]
    assert ("range_check",) not in eng.calls[eng.calls.index(("precision", "f32")):]     # nothing to check in f32
    rs.close()


def test_a_wait_that_gave_up_restarts_in_the_same_arithmetic():
    """sr3_range_check's other report: an in-place split-K wait gave up and everything since the last check is invalid
    ("repeat the call"). The same requests restart, but the arithmetic stays, `restarts` does not move and `replays`
    counts it — also under the strict policy, which is about the range only."""
    for strict in (False, True):
        eng = FakeEngine(S=4, trip_at=3, replay=True)
        eng.precision = "f16f8"
        rs = _sampler(eng, slots=2, precision="f16f8", strict=strict)
        for _ in range(3):
            rs.submit(Buf())
        with pytest.warns(pkg("_lib").Sr3ReplayWarning, match="repeat the call"):
            out = rs.drain()
        assert [t for t, _ in out] == [0, 1, 2]
        assert (rs.restarts, rs.replays, rs.precision) == (0, 1, "f16f8")
        assert not any(c[0] == "precision" for c in eng.calls)
        fin = {}
        for img_id, prec, ran in eng.finished:
            fin.setdefault(img_id, []).append((prec, ran))
        # 0 and 1 were retired once on the invalid steps (never delivered) and once more after the restart
        assert fin[0] == [("f16f8", 4)] * 2 and fin[1] == [("f16f8", 4)] * 2 and fin[2] == [("f16f8", 4)]
        rs.close()


def test_strict_policy_raises():
    eng = FakeEngine(S=2, trip_at=1)
    eng.precision = "f16x3"
    rs = _sampler(eng, slots=2, precision="f16x3", strict=True)
    rs.submit(Buf())
    rs.step(); rs.step()
    with pytest.raises(Sr3Error, match="range"):
        rs.poll()
    assert rs.restarts == 0
    rs.close()
