"""The history runner of tests/test_gpu_engine_history.py: one engine (the veteran) is taken through a list of calls, and
every call is held to the bytes of the same call on an engine that has run nothing else.

  Setup      what an engine is created with and keeps: the sampler, the weights, the configuration.
  Call       what one sampler call is made with: batch, shape, arithmetic, projection, threshold, feature cache.
  fresh      the bytes of a call on an engine created for that call only, run once, closed (memoised: the same call on
             the same setup is the same fresh engine's call).
  Veterans   the veteran that replays graphs and a second one created under SR3_NO_GRAPH=1, walked through the same
             history. Every sampler call is made twice on both; all four results must be fresh()'s bytes. A mismatch of
             the graph veteran alone is the replay's, a mismatch of both is carried state. Mismatches are collected and
             asserted at the end of the history (Veterans.close), so one run names every call that is off.
  restated   the CPU restatement of a call (dyn_threshold_ref.sample_loop: the update in numpy fp32, statement for
             statement, eps from an engine of its own through unet_forward_np), the anchor the fresh engines are held to.

The inputs of a call of B images are rows 0..B-1 of the inputs of N_IN images of its shape. Not a test module (no test_
prefix)."""
import functools
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

import dyn_threshold_ref
import fast_sampler_ref
import lr_consistency_ref
from conftest import pkg
from test_gpu_lr_consistency import SCHED, _bufs, _lr_images
from test_gpu_step_graphs import CAP, LR_LDS_MAX_BYTES, RATIO

synth = pkg("synth")
samplers = pkg("samplers")
F32 = np.float32

SEED = 31
R, L = 16, 8
N_IN = 6                        # rows of every input: the largest sampler batch of the histories
BAR = 1e-3                      # test_gpu_fast_samplers.py / test_gpu_dyn_threshold.py: restated chains
SCHED_DDPM = dict(SCHED["ddpm"], n_timestep=8)


@dataclass(frozen=True)
class Setup:
    kind: str = "dpmpp_2m"
    steps: Optional[int] = 4    # None: ddpm over the T = 8 of SCHED_DDPM
    wseed: int = SEED
    dropout: float = 0.0        # the configuration's p (0.2: sr3_set_dropout has something to switch)

    @property
    def S(self):
        return self.steps if self.steps else SCHED_DDPM["n_timestep"]

    @property
    def eta(self):              # (ddim with eta > 0: its steps read the injected draws)
        return 0.5 if self.kind == "ddim" else 0.0

    @property
    def sched(self):
        return SCHED_DDPM if self.kind == "ddpm" else SCHED["fast"]


@dataclass(frozen=True)
class Call:
    batch: int = 4
    H: int = R
    W: int = R
    lr: bool = False                        # the projection, onto LR images of H/2 x W/2
    dyn: Optional[Tuple[float, ...]] = None  # (ratio,) | (ratio, max_value)
    cache: Optional[Tuple[int, int]] = None  # (interval, depth)
    prec: str = "f32"
    plan_batch: int = 0                     # batch-invariant mode

    @property
    def forms(self):
        """step forms a call runs: the whole step, and the shallow one with the feature cache"""
        return 2 if self.cache else 1

    def __str__(self):
        on = [f"B={self.batch}", f"{self.H}x{self.W}", self.prec]
        on += ["lr"] if self.lr else []
        on += [f"dyn{self.dyn}"] if self.dyn else []
        on += [f"cache{self.cache}"] if self.cache else []
        on += [f"P={self.plan_batch}"] if self.plan_batch else []
        return " ".join(on)


def lr_form(H, W):
    """the form of the projection a sampler call at H x W takes (lr_lds_bytes in csrc/kernels_consist.hip)"""
    lh, lw = H // 2, W // 2
    return "lds" if (H * lw + lh * lw) * 4 <= LR_LDS_MAX_BYTES else "scratch"


@functools.lru_cache(maxsize=None)
def config(dropout=0.0):
    cfg = synth.tiny_unet_config()
    return cfg if dropout == 0.0 else type(cfg)(**{**cfg.__dict__, "dropout": dropout})


@functools.lru_cache(maxsize=None)
def weights(wseed):
    return synth.synth_state_dict(config(), wseed)


@functools.lru_cache(maxsize=None)
def _inputs(S, H, W):
    """(cond, noise, lr) of N_IN images, never modified"""
    if H == W:
        cond, lr = synth.synth_cond(N_IN, H, H // 2, SEED), _lr_images(N_IN, H // 2, SEED)
    else:
        cond = np.random.RandomState(SEED).uniform(-1, 1, (N_IN, 3, H, W)).astype(F32)
        lr = np.random.RandomState(SEED ^ 0x10C0).uniform(-1, 1, (N_IN, 3, H // 2, W // 2)).astype(F32)
    noise = synth.synth_noise(S, N_IN, 3, H, W, SEED)
    for a in (cond, noise, lr):
        a.setflags(write=False)
    return cond, noise, lr


def inputs(setup, call):
    """the first call.batch rows of the N_IN inputs of the call's shape"""
    cond, noise, lr = _inputs(setup.S, call.H, call.W)
    b = call.batch
    assert b <= N_IN
    return cond[:b], np.ascontiguousarray(noise[:, :b]), lr[:b]


def make_engine(setup):
    e = pkg("engine").Engine(config(setup.dropout), 0)
    e.load_state_dict(weights(setup.wseed))
    if setup.kind == "ddpm":
        e.set_schedule(_bufs(setup.sched))
    else:
        e.set_sampler_schedule(samplers.sampler_tables(_bufs(setup.sched), setup.kind, setup.steps, setup.eta))
    e._history_keep = {}        # device copies of the LR images the engine is set to (the steps read them)
    return e


def settings(e, setup, call):
    e.set_batch_invariant(call.plan_batch)
    e.set_precision(call.prec)
    if call.lr:
        lr = inputs(setup, call)[2]
        key = (call.batch, call.H, call.W)
        if key not in e._history_keep:
            e._history_keep[key] = e.to_device(lr)
        e.set_lr_consistency(e._history_keep[key].ptr, lr.shape[0], lr.shape[2], lr.shape[3], 0, 1.0)
    else:
        e.set_lr_consistency(None)
    e.set_dynamic_threshold(*(call.dyn or (None,)))
    e.set_feature_cache(*(call.cache or (None,)))


def run(e, setup, call):
    settings(e, setup, call)
    cond, noise, _ = inputs(setup, call)
    return e.sample_np(cond, noise=noise)


_FRESH = {}


def fresh(setup, call):
    """the call on an engine of its own: created, given the settings, run once, closed"""
    if (setup, call) not in _FRESH:
        e = make_engine(setup)
        try:
            got = run(e, setup, call)
            assert e.fallback_calls() == 0
        finally:
            e.close()
        got.setflags(write=False)
        _FRESH[setup, call] = got
    return _FRESH[setup, call]


def assert_live(setup, call):
    """the conditions under which a history proves something, on the fresh engines' images: the threshold and the
    projection each move the call's image"""
    want = fresh(setup, call)
    if call.dyn:
        assert fresh(setup, replace(call, dyn=None)).tobytes() != want.tobytes(), f"{call}: the threshold changes nothing"
    if call.lr:
        assert fresh(setup, replace(call, lr=False)).tobytes() != want.tobytes(), f"{call}: the projection changes nothing"


# ---- row sessions -----------------------------------------------------------------------------------------------------
def staggered_requests(setup, armed=False):
    """the request list of test_gpu_rows.py::test_staggered_rows_with_the_dynamic_threshold (Philox noise); armed: every
    row held to its LR image, at strengths 1, 0.5, 1, ..."""
    from test_gpu_rows import OFFSET, _staggered
    cond, _, lr = _inputs(setup.S, R, R)
    reqs = []
    for i, at in enumerate(_staggered(setup.S)):
        rq = {"cond": cond[i], "image_id": OFFSET + i, "at": at}
        if armed:
            rq.update(lr=lr[i], lr_strength=0.5 if i % 2 else 1.0)
        reqs.append(rq)
    return reqs


def run_session(e, setup, dyn, slots, armed):
    settings(e, setup, Call(dyn=dyn))
    out, trace = e.rows_np(staggered_requests(setup, armed), slots, seed=SEED)
    assert any(sum(h is not None for h in t) == min(slots, 4) for t in trace)   # (rows at different positions side by side)
    return np.stack(out)


_FRESH_SESSIONS = {}


def fresh_session(setup, dyn, slots, armed):
    key = (setup, dyn, slots, armed)
    if key not in _FRESH_SESSIONS:
        e = make_engine(setup)
        try:
            _FRESH_SESSIONS[key] = run_session(e, setup, dyn, slots, armed)
        finally:
            e.close()
    return _FRESH_SESSIONS[key]


# ---- the veterans -----------------------------------------------------------------------------------------------------
def _off(got, want):
    return "equal" if got.tobytes() == want.tobytes() else f"{float(np.abs(got.astype(np.float64) - want).max()):.3e} off"


class Veterans:
    def __init__(self, setup, monkeypatch):
        self.setup = setup
        self.g = make_engine(setup)
        with monkeypatch.context() as m:
            m.setenv("SR3_NO_GRAPH", "1")       # read in sr3_create
            self.ng = make_engine(setup)
        self.both = (self.g, self.ng)
        self.ws = None          # (B, H, W, plan_batch) of the workspace the graph veteran holds; None: none
        self.failures = []
        self.calls = 0

    def touched(self, ws):
        """something outside sample() built another workspace (or freed it: None)"""
        self.ws = ws

    def sample(self, what, call):
        """the call twice on both veterans against the fresh engine. Returns the graph veteran's first result."""
        s = self.setup
        want = fresh(s, call)
        n0 = self.g.step_graph_captures()
        g1 = run(self.g, s, call)
        n1 = self.g.step_graph_captures()
        g2 = run(self.g, s, call)
        n2 = self.g.step_graph_captures()
        r1, r2 = run(self.ng, s, call), run(self.ng, s, call)
        ws = (call.batch, call.H, call.W, call.plan_batch)
        new_ws, self.ws = ws != self.ws, ws
        self.calls += 1
        line = (f"[{self.calls}] {what}: {call}: graphs: first {_off(g1, want)}, repeat {_off(g2, want)}; no graphs: first "
                f"{_off(r1, want)}, repeat {_off(r2, want)}; captures {n1 - n0} then {n2 - n1}"
                + (f" (a new workspace: expected {call.forms} then 0)" if new_ws else " (expected 0 in the repeat)"))
        print(line)
        ok = all(x.tobytes() == want.tobytes() for x in (g1, g2, r1, r2)) and n2 - n1 == 0
        if new_ws:
            ok = ok and n1 - n0 == call.forms
        if not ok:
            self.failures.append(line)
        return g1

    def session(self, what, dyn, slots, armed=False):
        s = self.setup
        want = fresh_session(s, dyn, slots, armed)
        got = [run_session(e, s, dyn, slots, armed) for e in self.both]
        self.ws = (slots, R, R, 0)
        self.calls += 1
        line = (f"[{self.calls}] {what}: session of {slots} slots{' armed' if armed else ''}, dyn{dyn}: graphs "
                f"{_off(got[0], want)}; no graphs {_off(got[1], want)}")
        print(line)
        if any(x.tobytes() != want.tobytes() for x in got):
            self.failures.append(line)

    def close(self):
        assert self.ng.step_graph_captures() == 0
        assert self.g.fallback_calls() == 0 and self.ng.fallback_calls() == 0
        for e in self.both:
            e.close()
        assert not self.failures, "calls that are not the fresh engine's:\n" + "\n".join(self.failures)


# ---- the anchor -------------------------------------------------------------------------------------------------------
def restated(setup, call):
    """the final images of the call by dyn_threshold_ref.sample_loop, eps from an engine of its own in exact f32 (whole
    and shallow forwards in the call's order with the feature cache)"""
    cond, noise, lr = inputs(setup, call)
    e = pkg("engine").Engine(config(setup.dropout), 0)
    e.load_state_dict(weights(setup.wseed))
    k = [0]

    def eps_fn(x, nl):
        inp, level = np.concatenate([cond, x], axis=1), np.full((call.batch,), nl, F32)
        shallow = call.cache is not None and k[0] % call.cache[0] != 0
        k[0] += 1
        return e.unet_forward_cached_np(inp, level, call.cache[1]) if shallow else e.unet_forward_np(inp, level)

    if setup.kind == "ddpm":
        co = lr_consistency_ref.ddpm_coefficients(setup.sched)
    else:
        co = fast_sampler_ref.coefficients(setup.sched, setup.kind, setup.steps, setup.eta)
    try:
        out = dyn_threshold_ref.sample_loop(
            eps_fn, co, noise, call.dyn[0] if call.dyn else None, call.dyn[1] if call.dyn and len(call.dyn) > 1 else None,
            project=(lambda x0: lr_consistency_ref.project(x0, lr).astype(F32)) if call.lr else None)
    finally:
        e.close()
    return out["final"]


def assert_anchored(setup, call):
    """the fresh engine's call within the sampler tests' bar of its restatement"""
    err = float(np.abs(fresh(setup, call) - restated(setup, call)).max())
    print(f"anchor: {setup.kind} {call}: fresh engine against the restatement {err:.2e} (bar {BAR})")
    assert err <= BAR
