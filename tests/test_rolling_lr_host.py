"""LR consistency and frames per request on the host side of the rolling-batch sampler (rolling.RollingSampler, DESIGN.md
§3.5g), against the recording fake of test_rolling_host.py: when the session arms itself, lr_size, the two errors, and
the LR image and the frames of a request surviving a restart. No GPU, no torch."""
import pytest

from conftest import pkg
from test_rolling_host import Buf, FakeEngine

rolling = pkg("rolling")
Sr3Error = pkg("_lib").Sr3Error
Sr3RangeWarning = pkg("_lib").Sr3RangeWarning


class FakeLrEngine(FakeEngine):
    """FakeEngine with the per-row surface: arming, the LR image of an admit, frames; the library's rules for each"""

    def rows_begin(self, B, H, W, seed=0):
        super().rows_begin(B, H, W, seed)
        self.armed, self.admitted = None, False
        self.held, self.frames = [None] * B, [None] * B

    def rows_lr_consistency(self, lh, lw):
        if self.admitted:
            raise Sr3Error("sr3_rows_lr_consistency: a row was admitted already")
        self.calls.append(("arm", lh, lw))
        self.armed = (lh, lw)

    def rows_admit(self, row, cond_ptr, image_id, init_ptr=None, start_step=None, noised=True, noise0_ptr=None, lr=None,
                   lr_strength=1.0):
        if lr is not None and self.armed is None:
            raise Sr3Error("sr3_rows_admit_lr: an LR image for a session that is not armed")
        super().rows_admit(row, cond_ptr, image_id, init_ptr, start_step, noised, noise0_ptr)
        self.admitted = True
        self.held[row], self.frames[row] = (lr, lr_strength) if lr is not None else None, None
        self.calls.append(("held", row, image_id, lr, lr_strength if lr is not None else None))

    def num_frames(self, start_step=None):
        s0 = self.T if start_step is None else start_step
        return sum(1 for i in range(s0) if i % (1 | self.T // 10) == 0)

    def rows_frames(self, row, frames_ptr, capacity):
        if self.pos[row] < 0 or self.ran[row] != 0:
            raise Sr3Error("sr3_rows_frames: the slot is idle or past its first step")
        if capacity < self.num_frames(self.pos[row]):
            raise Sr3Error("sr3_rows_frames: capacity")
        self.calls.append(("frames", row, self.ids[row], frames_ptr, capacity))
        self.frames[row] = frames_ptr


def _sampler(eng, slots=4, **kw):
    return rolling.RollingSampler(eng, slots, eng.T, seed=5, alloc=lambda r: Buf((3, 16, 16)),
                                  alloc_frames=lambda r, n: Buf((n, 3, 16, 16)), **kw)


def _lr(l=8):
    return Buf((3, l, l))


def test_the_first_queued_lr_arms_the_session():
    eng = FakeLrEngine(S=4)
    rs = _sampler(eng, slots=2)
    a, b = _lr(), _lr()
    rs.submit(Buf(), lr=a)
    rs.submit(Buf())                        # not held, in the same session
    rs.submit(Buf(), lr=b, lr_strength=0.5)
    assert eng.calls[:2] == [("begin", 2, 16, 16, 5), ("arm", 8, 8)]
    held = [c for c in eng.calls if c[0] == "held"]
    assert held == [("held", 0, 0, a.data_ptr(), 1.0), ("held", 1, 1, None, None)]
    out = rs.drain()
    assert [t for t, _ in out] == [0, 1, 2]
    held = [c for c in eng.calls if c[0] == "held"]
    assert held[2] == ("held", 0, 2, b.data_ptr(), 0.5)
    assert sum(1 for c in eng.calls if c[0] == "arm") == 1
    # another LR size in the same session
    with pytest.raises(ValueError, match="one LR size"):
        rs.submit(Buf(), lr=_lr(4))
    with pytest.raises(ValueError, match="lr_strength"):
        rs.submit(Buf(), lr=_lr(), lr_strength=1.5)
    assert rs.pending == 0
    rs.close()
    # lr_strength 0 is "not held": nothing is passed, and the session is not armed by it
    eng = FakeLrEngine(S=2)
    rs = _sampler(eng, slots=2)
    rs.submit(Buf(), lr=_lr(), lr_strength=0.0)
    assert not any(c[0] == "arm" for c in eng.calls) and [c for c in eng.calls if c[0] == "held"][0][3] is None
    rs.close()


def test_lr_size_arms_a_session_whose_first_request_has_no_lr():
    eng = FakeLrEngine(S=2)
    rs = _sampler(eng, slots=2, lr_size=(8, 12))
    rs.submit(Buf())
    assert eng.calls[1] == ("arm", 8, 12)
    y = Buf((3, 8, 12))
    rs.submit(Buf(), lr=y)
    assert [c for c in eng.calls if c[0] == "held"][1] == ("held", 1, 1, y.data_ptr(), 1.0)
    with pytest.raises(ValueError, match="one LR size"):
        rs.submit(Buf(), lr=_lr(8))
    assert [t for t, _ in rs.drain()] == [0, 1]
    rs.close()


def test_an_lr_for_a_session_begun_unarmed_is_refused_naming_lr_size():
    eng = FakeLrEngine(S=2)
    rs = _sampler(eng, slots=2)
    rs.submit(Buf())
    assert not any(c[0] == "arm" for c in eng.calls)
    with pytest.raises(ValueError, match="lr_size"):
        rs.submit(Buf(), lr=_lr())
    assert rs.pending == 1 and [t for t, _ in rs.drain()] == [0]
    rs.close()
    # the next session of the same sampler begins afresh
    rs.submit(Buf(), lr=_lr())
    assert eng.calls[-4][0] == "begin" and eng.calls[-3] == ("arm", 8, 8)
    rs.drain()
    rs.close()


def test_continous_requests_get_their_frames():
    eng = FakeLrEngine(S=20)                # a frame every third step
    rs = _sampler(eng, slots=2)
    a = rs.submit(Buf(), continous=True)
    b = rs.submit(Buf(), init=Buf(), strength=0.35, continous=True)      # 7 steps: 3 frames
    c = rs.submit(Buf())
    fr = {c_[2]: c_ for c_ in eng.calls if c_[0] == "frames"}
    assert fr[a][4] == 7 and fr[b][4] == 3
    # frames are set right after the admit of their row, before any step
    i = eng.calls.index(fr[a])
    assert eng.calls[i - 2][0] == "admit" and eng.calls[i - 2][1] == fr[a][1]
    out = dict(rs.drain())
    assert out[a][1].shape == (7, 3, 16, 16) and out[a][1].data_ptr() == fr[a][3] and out[a][0].shape == (3, 16, 16)
    assert out[b][1].shape == (3, 3, 16, 16)
    assert isinstance(out[c], Buf)
    assert c not in {c_[2] for c_ in eng.calls if c_[0] == "frames"}
    rs.close()


def test_lr_and_frames_survive_a_restart():
    """S = 4, 2 slots, f16f8; the flag is raised during step 2, requests 0 (held, frames) and 1 (not held) finish after
    step 4 and the check trips: both are re-admitted one arithmetic down, request 0 with its LR image and a fresh frame
    buffer that is set again before its first step"""
    eng = FakeLrEngine(S=4, trip_at=2)
    eng.precision = "f16f8"
    rs = _sampler(eng, slots=2, precision="f16f8")
    y = _lr()
    rs.submit(Buf(), lr=y, lr_strength=0.75, continous=True)
    rs.submit(Buf())
    with pytest.warns(Sr3RangeWarning):
        out = dict(rs.drain())
    assert rs.restarts == 1 and rs.precision == "f16x3"
    i = eng.calls.index(("precision", "f16x3"))
    before, after = eng.calls[:i], eng.calls[i:]
    for part in (before, after):
        assert [c for c in part if c[0] == "held"] == [("held", 0, 0, y.data_ptr(), 0.75), ("held", 1, 1, None, None)]
        assert [c[1:3] + (c[4],) for c in part if c[0] == "frames"] == [(0, 0, 4)]
    f0, f1 = [c[3] for c in eng.calls if c[0] == "frames"]
    assert f0 != f1 and out[0][1].data_ptr() == f1           # (the delivered frames are those of the run that counted)
    assert sum(1 for c in eng.calls if c[0] == "arm") == 1   # the session stays armed through the restart
    fin = {}
    for img_id, prec, ran in eng.finished:
        fin.setdefault(img_id, []).append((prec, ran))
    assert fin[0] == [("f16f8", 4), ("f16x3", 4)] and fin[1] == [("f16f8", 4), ("f16x3", 4)]
    rs.close()


def test_a_refused_request_leaves_the_sampler_as_it_was():
    """a request refused for its image size (after its lr was looked at) must not fix the LR size or arm the next
    session; continous without a frame allocator is refused at submit, before any slot is touched"""
    eng = FakeLrEngine(S=2)
    rs = _sampler(eng, slots=2)
    rs.submit(Buf(), lr=_lr(8))
    rs.drain()
    rs.close()
    with pytest.raises(ValueError, match="one image size"):
        rs.submit(Buf((6, 16, 24)), lr=_lr(4))
    n = len(eng.calls)
    rs.submit(Buf())                        # the next session: begun unarmed, nothing of the refused request is left
    assert [c[0] for c in eng.calls[n:]] == ["begin", "admit", "held"]
    rs.drain()
    rs.close()
    bare = rolling.RollingSampler(eng, 2, eng.T, seed=5, alloc=lambda r: Buf((3, 16, 16)))
    n = len(eng.calls)
    with pytest.raises(ValueError, match="alloc_frames"):
        bare.submit(Buf(), continous=True)
    assert len(eng.calls) == n and bare.pending == 0
