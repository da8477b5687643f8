"""`RollingSampler`: requests that arrive one at a time, served through a batch that stays full.

The library's row session (sr3_rows_*) lets every batch row sit at its own position of the schedule. This module is the
host side: a slot scheduler that admits a queued request as soon as a slot is free, steps all live rows together,
retires the rows that finish, and hands results back in completion order. A request is a pure function of (seed, image
id, conditioning, start image, start step) and of the session's slot count: its result is the bytes of its row in a
uniform call of `slots` images with the same image id and seed, whatever else shared the batch and wherever it sat. The
slot count matters because every step runs at batch `slots`, and the library's conv dispatch depends on the batch
(against a call at another batch size an image moves by fp32 round-off in f32 / f16x3 and at the 1e-5
level in f16f8, whose fp8 path runs only from 32 or 64 images on). In the batch-invariant mode that dependence is gone,
and a session may be elastic (elastic=True): each step then runs over the slots of its live rows alone, compacted by
one-launch moves, and an idle slot costs nothing (elastic_plan; DESIGN.md §3.5g, "live rows only").

The scheduler itself touches no torch and no GPU: it drives an engine object (`Engine`'s rows_* methods, or a recording
fake in the host tests) with device addresses it gets from `data_ptr()` of whatever the caller submits.
"""
from __future__ import annotations

import warnings
from collections import deque
from typing import Callable, Deque, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

from ._lib import Sr3Error, Sr3RangeWarning, Sr3ReplayWarning

LADDER = {"f16f8": "f16x3", "f16x3": "f32"}       # one arithmetic down (the library's range policy, f32 at the bottom)

# Elastic sessions (batch-invariant mode; DESIGN.md §3.5g "live rows only"): a step runs at the smallest batch of a ladder
# that covers the live rows. The library keeps one captured graph per batch value and at most MAX_LADDER of them per form.
BATCH_LADDER = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)
MAX_LADDER = 16


def default_ladder(slots: int) -> Tuple[int, ...]:
    """BATCH_LADDER within [1, slots], and slots itself"""
    return tuple(sorted({b for b in BATCH_LADDER if b <= int(slots)} | {int(slots)}))


def check_ladder(ladder, slots: int) -> Tuple[int, ...]:
    """The ladder of an elastic session as a tuple (None: default_ladder): positive, increasing, ending at `slots`, at
    most MAX_LADDER entries — anything else is a ValueError."""
    if ladder is None:
        return default_ladder(slots)
    lad = tuple(int(b) for b in ladder)
    if not lad or lad[0] < 1 or any(b <= a for a, b in zip(lad, lad[1:])):
        raise ValueError(f"ladder must be a non-empty increasing sequence of positive batch sizes, got {list(ladder)}")
    if lad[-1] != int(slots):
        raise ValueError(f"ladder must end at the session's slot count {slots}, got {list(ladder)}")
    if len(lad) > MAX_LADDER:
        raise ValueError(f"ladder may hold at most {MAX_LADDER} batch sizes (one captured graph each), got {len(lad)}")
    return lad


def elastic_plan(occupied: Sequence[bool], ladder: Sequence[int]) -> Tuple[List[Tuple[int, int]], int]:
    """The policy of an elastic step. occupied[s]: slot s holds a live row. With L live rows and b the smallest ladder
    entry >= L: while a live row sits at a slot >= b, the highest live row moves to the lowest free slot. Returns
    (moves as (src, dst) in order, the batch of the step: the smallest ladder entry >= highest live slot + 1 after the
    moves). Moves happen only where they lower the batch: every one takes a row from at or above b to below it, and a
    session whose rows already sit below b — a full one among them — records none."""
    occ = [bool(o) for o in occupied]
    live = sum(occ)
    if not live:
        return [], ladder[0]
    b = next(x for x in ladder if x >= live)
    moves = []
    while True:
        hi = max(s for s, o in enumerate(occ) if o)
        if hi < b:
            break
        lo = occ.index(False)       # (below b: fewer than b rows are live below it while one sits at or above it)
        moves.append((hi, lo))
        occ[hi], occ[lo] = False, True
    return moves, next(x for x in ladder if x >= hi + 1)


class _Request:
    __slots__ = ("ticket", "cond", "init", "start_step", "noised", "image_id", "out", "lr", "lr_strength", "continous",
                 "frames")

    def __init__(self, ticket, cond, init, start_step, noised, image_id, lr=None, lr_strength=1.0, continous=False):
        self.ticket, self.cond, self.init = ticket, cond, init
        self.start_step, self.noised, self.image_id = start_step, noised, image_id
        self.lr, self.lr_strength, self.continous = lr, lr_strength, continous
        self.out = self.frames = None


class RollingSampler:
    """Serves single-image requests through `slots` batch rows.

      submit(x_in_row, init=None, strength=None, image_id=None, lr=None, lr_strength=1.0, continous=False) -> ticket
      step()              one step of every live row; finished rows retire, queued requests take the free slots
      poll()              [(ticket, image)] of the rows finished since the last poll, in completion order
      drain()             steps until nothing is queued or in flight; returns what poll would
      stream(iterable)    generator over requests, yielding (ticket, image) as rows finish, the slots kept full

    Range policy (split-f16 arithmetic). poll makes one range check for all the steps since the last one. A clean check
    certifies every step before it, so a trip can only have touched the requests in flight and those that finished since
    the last clean check: under the default policy the sampler goes one arithmetic down (f16f8 -> f16x3 -> f32), drops
    those rows and re-admits their requests from their start — the result is what the lower arithmetic would have given —
    and counts the event in `restarts`; it stays in the lower arithmetic until close(). Under the strict policy the
    check raises. The check's other report, an in-place split-K wait that gave up ("repeat the call": the library has
    switched conv paths, everything since the last check is invalid), restarts the same requests in the same arithmetic
    under either policy and is counted in `replays`, as p_sample repeats its step.

    LR consistency is per request: a request submitted with an `lr` image is held to it, one without is
    not, in the same session. The session must be armed for the LR size when it begins — it begins with the first
    submit — either by `lr_size` or by that first request carrying an `lr`. A restart re-admits a request with its LR
    image and writes its frames again from the first.

    `trace` records one entry per step: (live rows, requests still queued, whether the stream's source is exhausted).

    elastic=True (a model in batch-invariant mode only: ValueError otherwise): a step runs over the live rows' slots
    alone. After retiring and filling, before each step, elastic_plan compacts the live rows below the smallest entry of
    `ladder` (default default_ladder(slots)) that holds them — Engine.rows_move, one launch each, only where it lowers
    the batch — and the step runs at the smallest entry that covers the highest live slot. In that mode a row's bytes do
    not depend on the batch of the launch, so every request is still its B = 1 call. `batch_trace` records the batch
    of every step, `moves` counts the moves. elastic=False: every step runs all slots, as it always did.
    """

    def __init__(self, engine, slots: int, steps: int, seed: int = 0, precision: str = "f32", strict: bool = False,
                 start_steps: Optional[Callable] = None, alloc: Optional[Callable] = None,
                 ready: Optional[Callable] = None, finish: Optional[Callable] = None,
                 lr_size: Optional[Tuple[int, int]] = None, to_lr: Optional[Callable] = None,
                 alloc_frames: Optional[Callable] = None, deliver: Optional[Callable] = None,
                 elastic: bool = False, ladder: Optional[Sequence[int]] = None):
        if int(slots) < 1:
            raise ValueError(f"slots must be >= 1, got {slots}")
        self.elastic = bool(elastic)
        if self.elastic:
            mode = getattr(engine, "batch_invariant", None)
            if not (mode() if callable(mode) else mode):
                raise ValueError("elastic=True needs the batch-invariant mode: a step over fewer rows than the session has "
                                 "slots keeps a row's bytes only there — call set_batch_invariant() on the model first")
            self.ladder = check_ladder(ladder, slots)
        elif ladder is not None:
            raise ValueError("a ladder belongs to an elastic session: pass elastic=True")
        else:
            self.ladder = (int(slots),)
        self.eng, self.slots, self.S, self.seed = engine, int(slots), int(steps), int(seed)
        self.precision, self._precision0, self.strict = precision, precision, bool(strict)
        self._start_steps = start_steps or (lambda S, strength: max(1, min(S, int(round(float(strength) * S)))))
        self._alloc = alloc
        self._ready, self._finish = ready or (lambda: None), finish or (lambda: None)
        # to_lr(lr) -> the LR image as the engine takes it (fp32 [C,lh,lw] with a data_ptr); alloc_frames(request, n) ->
        # the buffer of its n frames; deliver(request) -> what poll hands back for it (default: its image, or
        # (image, frames) for a request with continous)
        self._to_lr = to_lr or self._row
        self._alloc_frames = alloc_frames
        self._deliver = deliver or (lambda r: (r.out, r.frames) if r.continous else r.out)
        self._lr_size0 = self._lr_size = None if lr_size is None else (int(lr_size[0]), int(lr_size[1]))
        self._armed = False
        self._queue: Deque[_Request] = deque()
        self._rows: List[Optional[_Request]] = [None] * self.slots
        self._left: List[int] = [0] * self.slots         # steps left per slot (the library keeps the same count)
        self._done: List[_Request] = []                  # finished since the last clean range check, completion order
        self._open = False
        self._shape = None
        self._next_ticket = 0
        self._source_done = True
        self.restarts = 0
        self.replays = 0
        self.steps_run = 0
        self.trace: List[Tuple[int, int, bool]] = []
        self.batch_trace: List[int] = []
        self.moves = 0

    # ---- requests ---------------------------------------------------------------------------------------
    def submit(self, x_in_row, init=None, strength=None, image_id: Optional[int] = None, lr=None, lr_strength: float = 1.0,
               continous: bool = False) -> int:
        """Queues one request and returns its ticket. x_in_row: the conditioning image [Cc,H,W] (or [1,Cc,H,W]).
        strength in (0, 1]: a warm start over the last max(1, round(strength * S)) steps from `init` [C,H,W], or from the
        conditioning image itself without one; init without a strength starts at the top level. image_id keys the
        request's Philox streams (default: the ticket). lr: the request's LR image ([C,l,l] fp32 in [-1,1], or what the
        sampler's to_lr converts), to which every step holds the row at lr_strength in [0, 1] (0, or no lr: not held).
        continous: poll hands back the frames of the request as well."""
        cond = self._row(x_in_row)
        # every check first: a refused request leaves the sampler as it was (image size, LR size, arming)
        if not 0.0 <= float(lr_strength) <= 1.0:
            raise ValueError(f"lr_strength must lie in [0, 1], got {lr_strength}")
        if continous and self._alloc_frames is None:
            raise ValueError("continous=True needs a sampler built with alloc_frames: the buffer the row writes its frames to")
        shape = tuple(cond.shape[-2:])
        if self._shape is not None and shape != self._shape:
            raise ValueError(f"a rolling session serves one image size: got {shape}, the session runs {self._shape}")
        lr_size = self._lr_size
        if lr is not None and float(lr_strength) != 0.0:
            lr = self._to_lr(lr)
            size = tuple(int(v) for v in lr.shape[-2:])
            if self._open and not self._armed:
                raise ValueError("this session was begun without LR consistency: a request with an lr needs a session armed "
                                 "from its start — pass lr_size=(lh, lw) to rolling(), or submit an lr with the first request")
            if lr_size is None:
                lr_size = size
            elif size != lr_size:
                raise ValueError(f"a rolling session holds rows to one LR size: got {size}, the session runs {lr_size}")
        else:
            lr = None
        if init is not None:
            init = self._row(init)
        elif strength is not None:
            init = cond
        start = self.S if strength is None else int(self._start_steps(self.S, strength))
        self._shape, self._lr_size = shape, lr_size
        ticket = self._next_ticket
        self._next_ticket += 1
        self._queue.append(_Request(ticket, cond, init, start, True, ticket if image_id is None else int(image_id), lr,
                                    float(lr_strength), bool(continous)))
        self._fill()
        return ticket

    @staticmethod
    def _row(t):
        if hasattr(t, "dim") and t.dim() == 4:
            if t.shape[0] != 1:
                raise ValueError(f"one image per request: got a batch of {t.shape[0]}")
            t = t[0]
        if hasattr(t, "contiguous"):
            t = t.contiguous()
        return t

    # ---- the session ------------------------------------------------------------------------------------
    def _begin(self):
        if not self._open:
            H, W = self._shape
            self.eng.rows_begin(self.slots, H, W, self.seed)
            self._open = True
            # armed by lr_size, or by the LR image of the request whose submit begins the session: the session begins
            # with the first submit, so no later request can arm it (submit refuses their lr, naming lr_size)
            if self._lr_size is not None:
                self.eng.rows_lr_consistency(*self._lr_size)
                self._armed = True

    def _fill(self):
        """queued requests into free slots, lowest slot first"""
        if not self._queue:
            return
        for s in range(self.slots):
            if not self._queue:
                break
            if self._rows[s] is not None:
                continue
            self._begin()
            r = self._queue.popleft()
            n_frames = self.eng.num_frames(r.start_step) if r.continous else 0
            if r.continous:
                r.frames = self._alloc_frames(r, n_frames)
            self._ready()
            held = {} if r.lr is None else {"lr": r.lr.data_ptr(), "lr_strength": r.lr_strength}
            self.eng.rows_admit(s, r.cond.data_ptr(), r.image_id, r.init.data_ptr() if r.init is not None else None,
                                r.start_step if r.init is not None else None, r.noised, **held)
            if r.continous:
                self.eng.rows_frames(s, r.frames.data_ptr(), n_frames)
            self._rows[s], self._left[s] = r, r.start_step

    @property
    def in_flight(self) -> int:
        return sum(1 for r in self._rows if r is not None)

    @property
    def pending(self) -> int:
        """requests queued or in flight"""
        return len(self._queue) + self.in_flight

    def step(self) -> int:
        """One step of every live row. Returns the number of rows stepped."""
        self._fill()
        if not self.in_flight:
            return 0
        self.trace.append((self.in_flight, len(self._queue), self._source_done))
        if self.elastic:
            moves, batch = elastic_plan([r is not None for r in self._rows], self.ladder)
            for a, b in moves:
                self.eng.rows_move(a, b)
                self._rows[b], self._left[b] = self._rows[a], self._left[a]
                self._rows[a], self._left[a] = None, 0
            self.moves += len(moves)
            n = self.eng.rows_step(None, batch)
        else:
            batch = self.slots
            n = self.eng.rows_step()
        self.batch_trace.append(batch)
        self.steps_run += 1
        for s, r in enumerate(self._rows):
            if r is None:
                continue
            self._left[s] -= 1
            if self._left[s] == 0:
                r.out = self._alloc(r) if self._alloc else None
                self._ready()           # (the library's stream writes a buffer the caller's stream has just handed out)
                self.eng.rows_retire(s, r.out.data_ptr() if r.out is not None else 0)
                self._done.append(r)
                self._rows[s] = None
        self._fill()
        return n

    def poll(self) -> list:
        """[(ticket, image)] finished since the last poll, in completion order; one range check for all of them."""
        if not self._done:
            return []
        if self.precision != "f32":
            try:
                self.eng.range_check()
            except Sr3Error as e:
                # an in-place split-K wait that gave up (the library has switched conv paths): the same arithmetic again
                replay = "repeat the call" in str(e)
                if not replay and (self.strict or "range" not in str(e) or self.precision not in LADDER):
                    raise
                self._restart(e, lower=not replay)
                return []
        self._finish()
        out = [(r.ticket, self._deliver(r)) for r in self._done]
        self._done = []
        return out

    def _restart(self, err, lower=True):
        """everything a trip can have touched goes back to the head of the queue, oldest first — one arithmetic down, or
        (lower False: a wait that gave up, sr3_range_check's "repeat the call") in the same one, counted in `replays`"""
        nxt = LADDER[self.precision] if lower else self.precision
        hit = list(self._done) + [r for r in self._rows if r is not None]
        for s, r in enumerate(self._rows):
            if r is not None:
                self.eng.rows_drop(s)
                self._rows[s] = None
        self._done = []
        for r in sorted(hit, key=lambda r: r.ticket, reverse=True):
            r.out = r.frames = None     # (the LR image stays with the request: it is re-admitted held, its frames restart)
            self._queue.appendleft(r)
        if lower:
            self.set_precision(nxt)
            self.restarts += 1
        else:
            self.replays += 1
        kind = Sr3RangeWarning if lower else Sr3ReplayWarning
        warnings.warn(kind(f"rolling sampler: {len(hit)} requests restarted in {nxt}: {err}"), stacklevel=3)
        self._fill()

    def set_precision(self, name: str) -> None:
        """The arithmetic of the steps from here on (allowed between steps: sr3_set_precision)."""
        self.eng.set_precision(name)
        self.precision = name

    def drain(self) -> list:
        """Steps until nothing is queued or in flight; returns everything poll would have."""
        out = self.poll()
        while self.pending or self._done:       # (a trip at the very end restarts: step on)
            if self.pending:
                self.step()
            out += self.poll()
        return out

    def stream(self, requests: Iterable) -> Iterator:
        """requests: conditioning rows, or dicts / tuples of submit's arguments. Yields (ticket, image) as rows finish;
        the source is read only as slots come free, so the slots stay full while it has something to give."""
        it = iter(requests)
        self._source_done = False
        try:
            while True:
                while not self._source_done and self.pending < self.slots:
                    try:
                        rq = next(it)
                    except StopIteration:
                        self._source_done = True
                        break
                    if isinstance(rq, dict):
                        self.submit(**rq)
                    elif isinstance(rq, (tuple, list)):
                        self.submit(*rq)
                    else:
                        self.submit(rq)
                if not self.pending and not self._done:
                    break
                if self.pending:
                    self.step()
                for item in self.poll():
                    yield item
        finally:
            self._source_done = True

    def close(self) -> None:
        """Ends the session (rows in flight are abandoned) and restores the arithmetic a restart lowered."""
        if self._open:
            self.eng.rows_end()
            self._open = False
        self._armed, self._lr_size = False, self._lr_size0
        self._rows = [None] * self.slots
        if self.precision != self._precision0:
            self.set_precision(self._precision0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
