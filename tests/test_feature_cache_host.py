"""The numpy restatement of the feature cache (feature_cache_ref.py) against the CPU oracle: the module
split of every legal depth, the shallow forward on the cache of its own call (the whole forward bit for bit), the
interval-1 loop (oracle.p_sample_loop bit for bit), how far interval 2 and 3 move a sample (so a device test cannot pass
by ignoring the setting), a stale cache, and the facade's argument checks. No GPU."""
import functools

import numpy as np
import pytest

import feature_cache_ref as ref
import sr3_oracle as oracle
from conftest import pkg

synth = pkg("synth")
F32 = np.float32
TINY = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
SEEDS = {"A": 31, "C": 33, "D": 34, "tiny": 17}


def _cfg(name):
    if name == "tiny":
        return synth.tiny_unet_config()
    if name.startswith("yml"):
        return synth.yml_unet_config(int(name[3:]))
    return synth.sweep_unet_config(name)


@pytest.mark.parametrize("name", ["tiny", "A", "C", "D", "yml224", "yml128"])
def test_module_split(name):
    cfg = _cfg(name)
    rb, n = cfg.res_blocks, len(cfg.channel_mults)
    downs, mid, ups = oracle.unet_plan(cfg)
    assert ref.max_depth(cfg) == n - 1
    for d in range(1, n):
        fd, skipped, fu = ref.split(cfg, d)
        assert len(fd) == 1 + d * rb + (d - 1) and len(fu) == d * (rb + 1) + (d - 1)
        assert fd + skipped + fu == downs + mid + ups
        assert fd[0][0] == "conv" and skipped[0][0] == "down" and skipped[-1][0] == "up"
        # the fresh up blocks pop exactly the fresh down outputs
        assert sum(k == "res" for k, _, _ in fu) == len(fd)
        # levels: the fresh part never leaves the top d levels
        assert sum(k == "down" for k, _, _ in fd) == d - 1 == sum(k == "up" for k, _, _ in fu)
    for bad in (0, n, -1):
        with pytest.raises(ValueError):
            ref.split(cfg, bad)
    if name == "yml224":
        fd, skipped, fu = ref.split(cfg, 1)
        assert [p for _, p, _ in fd] == ["downs.0", "downs.1", "downs.2"]
        assert skipped[-1][1] == "ups.15" and [p for _, p, _ in fu] == ["ups.16", "ups.17", "ups.18"]


IDENTITY = [("tiny", (2, 16, 16), 1), ("A", (2, 16, 24), 1), ("A", (2, 16, 24), 2), ("D", (2, 8, 8), 1), ("D", (2, 8, 8), 2)]


@functools.lru_cache(maxsize=None)
def _whole(name, shape):
    cfg = _cfg(name)
    sd = synth.synth_state_dict(cfg, SEEDS[name])
    B, H, W = shape
    x, nl = synth.synth_unet_input(cfg, B, H, W, SEEDS[name])
    want = oracle.unet_forward(sd, cfg, x, nl)
    got, cache = ref.forward(sd, cfg, x, nl)
    return cfg, sd, x, nl, want, got, cache


@pytest.mark.parametrize("name,shape,d", IDENTITY, ids=[f"{n}-{s[1]}x{s[2]}-d{d}" for n, s, d in IDENTITY])
def test_shallow_forward_on_its_own_cache_is_the_whole_forward(name, shape, d):
    cfg, sd, x, nl, want, got, cache = _whole(name, shape)
    np.testing.assert_array_equal(got, want)                 # the whole forward of the restatement is the oracle's
    n_up = len(cfg.channel_mults) - 1
    assert len(cache) == n_up
    eps, again = ref.forward(sd, cfg, x, nl, d, cache)
    assert again is cache
    np.testing.assert_array_equal(eps, want)


@pytest.mark.parametrize("name,shape,d", IDENTITY, ids=[f"{n}-{s[1]}x{s[2]}-d{d}" for n, s, d in IDENTITY])
def test_stale_cache_is_far_from_the_exact_forward(name, shape, d):
    """A shallow forward of an unrelated input on a stale cache: O(1) from that input's exact forward (the deep part
    matters), so comparing a device result with the restatement on the same stale cache is a real check."""
    cfg, sd, x, nl, _, _, cache = _whole(name, shape)
    B, H, W = shape
    xb, nlb = synth.synth_unet_input(cfg, B, H, W, SEEDS[name] + 100)
    exact = oracle.unet_forward(sd, cfg, xb, nlb)
    stale, _ = ref.forward(sd, cfg, xb, nlb, d, cache)
    dist = float(np.abs(stale - exact).max())
    print(f"{name} {shape} d={d}: shallow forward on a stale cache vs exact forward: max abs {dist:.3f}")
    assert dist >= 0.1 and np.isfinite(stale).all()


@functools.lru_cache(maxsize=None)
def _loop_setup(name):
    cfg = _cfg(name)
    sd = synth.synth_state_dict(cfg, 17)
    B, r, T = 2, 16, TINY["n_timestep"]
    cond = synth.synth_cond(B, r, 8, 17)
    noise = synth.synth_noise(T, B, 3, r, r, 17)
    sched = oracle.noise_schedule(TINY)
    exact, exact_fr = oracle.p_sample_loop(sd, cfg, sched, cond, noise)
    return cfg, sd, sched, cond, noise, exact, exact_fr


@pytest.mark.parametrize("name", ["tiny", "A"])
def test_interval_1_is_the_reference_loop(name):
    cfg, sd, sched, cond, noise, exact, exact_fr = _loop_setup(name)
    for interval in (None, 1):
        got, got_fr = ref.sample_loop(sd, cfg, sched, cond, noise, interval, 1)
        np.testing.assert_array_equal(got, exact)
        np.testing.assert_array_equal(got_fr, exact_fr)


def test_few_step_loop_with_interval_1_is_the_few_step_restatement():
    import fast_sampler_ref as fast
    cfg, sd, _, cond, noise, _, _ = _loop_setup("tiny")
    for kind, S, eta in (("ddim", 10, 0.5), ("dpmpp_2m", 10, 0.0)):
        want, want_fr = fast.sample_loop(sd, cfg, TINY, cond, noise[:S], kind, S, eta)
        got, got_fr = ref.fast_sample_loop(sd, cfg, TINY, cond, noise[:S], kind, S, eta, 1, 1)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_fr, want_fr)


def test_the_setting_moves_the_sample():
    """Interval 2 and 3 move the result by at least 1e-2 max-abs, ten times the device tests' bar: a sampler that ignored
    the setting would miss the restatement. Depths 1 and 2 differ from each other as well."""
    res = {}
    for name, d in (("tiny", 1), ("A", 1), ("A", 2)):
        cfg, sd, sched, cond, noise, exact, _ = _loop_setup(name)
        for interval in (2, 3):
            got, _ = ref.sample_loop(sd, cfg, sched, cond, noise, interval, d)
            res[name, d, interval] = got
            dist = float(np.abs(got - exact).max())
            print(f"{name} d={d} interval={interval}: max abs from the exact loop {dist:.4f}")
            assert dist >= 1e-2, (name, d, interval, dist)
    for interval in (2, 3):
        assert float(np.abs(res["A", 1, interval] - res["A", 2, interval]).max()) >= 1e-3


def test_step_counts():
    cfg, sd, _, _, _, _, _ = _loop_setup("tiny")
    f = ref.CachedEps(sd, cfg, 7, 1)
    x, nl = synth.synth_unet_input(cfg, 1, 16, 16, 5)
    for _ in range(20):
        f(x, nl)
    assert (f.whole, f.shallow) == (3, 17)                   # ceil(20 / 7), the rest


def _facade():
    opt = synth.yml_opt(8, 16, 20)
    opt["sr"]["model"]["unet"].update(inner_channel=32, channel_multiplier=[1, 2, 4], res_blocks=1, attn_res=[8])
    opt["sr"]["model"]["diffusion"].update(image_size=16, conditional=True)
    netG = pkg().define_G(opt)
    netG.set_new_noise_schedule(opt["sr"]["model"]["beta_schedule"]["val"], ["cpu"])
    return netG


def test_facade_argument_checks():
    netG = _facade()
    keys = list(netG.state_dict())
    assert netG._fc is None
    for bad in (0, -1, 2.5, "3", True, float("nan")):
        with pytest.raises(ValueError):
            netG.set_feature_cache(bad)
    for bad in (0, 3, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            netG.set_feature_cache(3, depth=bad)
    with pytest.raises(ValueError):
        netG.set_feature_cache(None, depth=3)                       # the depth is checked even when turning off
    assert netG._fc is None                                         # a refused setting leaves the old one
    netG.set_feature_cache(3)
    assert netG._fc == (3, 1)
    netG.set_feature_cache(np.int64(5), depth=2)
    assert netG._fc == (5, 2)
    # survives the sampler and the schedule, adds nothing to state_dict()
    netG.set_sampler("dpmpp_2m", steps=10)
    netG.set_new_noise_schedule({"schedule": "linear", "n_timestep": 30, "linear_start": 1e-4, "linear_end": 2e-2}, ["cpu"])
    assert netG._fc == (5, 2) and list(netG.state_dict()) == keys
    netG.set_feature_cache(1)                                       # interval 1 is off
    assert netG._fc is None
    netG.set_feature_cache(4)
    netG.set_feature_cache(None)
    assert netG._fc is None
