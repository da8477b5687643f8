"""The cache of captured sampler steps (StepKey in csrc/sr3_api.hip): an engine that replays graphs is
walked through every setting that a captured step bakes in, next to an engine created under SR3_NO_GRAPH=1 that launches
every kernel itself. The two run the same kernels with the same arguments, so their images are compared with tobytes()
equality, and Engine.step_graph_captures() says what each call cost:

  (a) the second of two identical calls captures nothing,
  (b) the first call after a change captures once per distinct step form it runs (1; 2 with whole and shallow steps when
      neither is cached),
  (c) returning to a form whose baked-in values were never touched captures nothing.

dpmpp_2m with 4 steps: the smallest count at which a form is warmed (step 1, eager), captured (step 2) and replayed
(steps 3 and 4) within one call; with the feature cache at interval 2 the whole steps are 1 and 3, the shallow ones 2
and 4, so each form is warmed and captured once and never replayed in its first call, and only replayed in the second."""
import numpy as np
import pytest

from conftest import pkg
from test_gpu_lr_consistency import SCHED, _bufs, _lr_images

pytestmark = pytest.mark.gpu
synth = pkg("synth")
samplers = pkg("samplers")

KIND, STEPS = "dpmpp_2m", 4
SEED = 31
B, R, L = 2, 16, 8
RATIO, CAP = 0.995, 1.25        # test_gpu_dyn_threshold.py: RATIO, and the finite max_value of its selection tests
LR_LDS_MAX_BYTES = 64 * 1024    # csrc/sr3_internal.h


def _engine(cfg, sd):
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_sampler_schedule(samplers.sampler_tables(_bufs(SCHED["fast"]), KIND, STEPS, 0.0))
    return e


class Pair:
    """The engine with graphs, the engine without, and the device copies of the LR images they are set to."""

    def __init__(self, cfg, monkeypatch):
        sd = synth.synth_state_dict(cfg, SEED)
        self.e = _engine(cfg, sd)
        with monkeypatch.context() as m:
            m.setenv("SR3_NO_GRAPH", "1")       # read in sr3_create
            self.ref = _engine(cfg, sd)
        self.lr_dev = {}

    def close(self):
        self.e.close()
        self.ref.close()

    def settings(self, lr=None, dyn=None, cache=None, prec="f32"):
        for i, eng in enumerate((self.e, self.ref)):
            eng.set_precision(prec)
            if lr is None:
                eng.set_lr_consistency(None)
            else:
                if (i, id(lr)) not in self.lr_dev:
                    self.lr_dev[i, id(lr)] = (eng.to_device(lr), lr)       # (kept alive: the steps read it)
                eng.set_lr_consistency(self.lr_dev[i, id(lr)][0].ptr, lr.shape[0], lr.shape[2], lr.shape[3], 0, 1.0)
            eng.set_dynamic_threshold(*(dyn or (None,)))
            eng.set_feature_cache(*(cache or (None,)))

    def sample(self, what, first, batch=B, **settings):
        """Both engines get the settings; the graph engine samples twice. Its first call must add `first` captures, its
        second none (a), and both must be the bytes of the engine without graphs. Returns those bytes."""
        self.settings(**settings)
        cond, noise = synth.synth_cond(batch, R, L, SEED), synth.synth_noise(STEPS, batch, 3, R, R, SEED)
        want = self.ref.sample_np(cond, noise=noise).tobytes()
        n0 = self.e.step_graph_captures()
        got1 = self.e.sample_np(cond, noise=noise).tobytes()
        n1 = self.e.step_graph_captures()
        got2 = self.e.sample_np(cond, noise=noise).tobytes()
        n2 = self.e.step_graph_captures()
        print(f"{what}: captures {n1 - n0} then {n2 - n1} (expected {first} then 0)")
        assert got1 == want and got2 == want, what
        assert (n1 - n0, n2 - n1) == (first, 0), what
        assert self.ref.step_graph_captures() == 0
        return want


def test_captured_steps_follow_what_they_bake_in(monkeypatch):
    cfg = synth.tiny_unet_config()
    p = Pair(cfg, monkeypatch)
    lr8, lr4 = _lr_images(B, L, SEED), _lr_images(B, 4, SEED)
    out = {}
    out[1] = p.sample("1 everything off", 1)
    out[2] = p.sample("2 projection on", 1, lr=lr8)
    out[3] = p.sample("3 threshold on as well", 1, lr=lr8, dyn=(RATIO,))
    out[4] = p.sample("4 another max_value", 1, lr=lr8, dyn=(RATIO, CAP))
    out[5] = p.sample("5 the first max_value again", 1, lr=lr8, dyn=(RATIO,))       # (the slot holds one graph)
    out[6] = p.sample("6 LR images of 4x4", 1, lr=lr4, dyn=(RATIO,))
    # the conditions under which the steps above prove something: every setting changed the images
    assert len({out[i] for i in (1, 2, 3, 4, 6)}) == 5 and out[5] == out[3]

    # 7. the projection alone again: nothing it bakes in was touched by 3..6 (c). Then the scratch of the multi-launch form
    # grows (128x128 planes). A captured step holds that pointer only in the scratch form, which a plane of R x R needs
    # when its intermediates do not fit the LDS
    p.sample("7 projection alone again", 0, lr=lr8)
    sampler_takes_scratch = (R * L + L * L) * 4 > LR_LDS_MAX_BYTES
    big, y = np.zeros((1, 3, 128, 128), np.float32), np.zeros((1, 3, 16, 16), np.float32)
    for eng in (p.e, p.ref):
        eng.lr_project_np(big, y, form="scratch")
    assert p.sample("7 after the scratch grew", 1 if sampler_takes_scratch else 0, lr=lr8) == out[2]

    # 8. feature cache: the whole step is the graph of setting 1 (c), the shallow step is new
    assert len(cfg.channel_mults) == 2      # (depth 2 needs three levels: the test below)
    p.sample("8 feature cache, interval 2 depth 1", 1, cache=(2, 1))
    assert p.e.feature_cache_steps() == (2, 2)

    # 9. another arithmetic, and back (c)
    p.sample("9 f16x3", 1, prec="f16x3")
    assert p.e.fallback_calls() == 0
    p.sample("9 f32 again", 0)

    # 10. a new workspace drops every graph: each form is captured again when it next runs, two in a call with both
    p.sample("10 B = 3", 1, batch=3)
    p.sample("10 B = 3, feature cache", 1, batch=3, cache=(2, 1))
    p.sample("10 B = 2 again, feature cache", 2, cache=(2, 1))

    # 11. and after all of it the plain sampler is the plain sampler
    assert p.sample("11 everything off", 0) == out[1]
    assert p.ref.step_graph_captures() == 0
    p.close()


def test_the_depth_of_the_shallow_step_is_part_of_the_key(monkeypatch):
    """Setting 8 at both depths, on the smallest configuration with three levels (sweep configuration A)."""
    cfg = synth.sweep_unet_config("A")
    p = Pair(cfg, monkeypatch)
    whole = p.sample("everything off", 1)
    d1 = p.sample("interval 2 depth 1", 1, cache=(2, 1))         # the whole step is cached (c)
    d2 = p.sample("interval 2 depth 2", 1, cache=(2, 2))         # only the shallow form is recaptured
    assert p.sample("interval 2 depth 1 again", 1, cache=(2, 1)) == d1
    assert len({whole, d1, d2}) == 3
    assert p.sample("everything off again", 0) == whole
    p.close()
