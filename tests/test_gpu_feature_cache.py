"""The feature cache on the GPU (sr3_set_feature_cache / sr3_unet_forward_cached): the shallow forward
against the numpy restatement (feature_cache_ref.py) on a cache made from another input, the shallow forward on the cache
of its own input against the whole forward bit for bit (with Dropout as well: the layer numbering across the jump), the
entry points' errors, the samplers against the restatement's loops, off-is-off, the step API and the warm start, the
range guard's replay, and the torch facade.

Bars are the project's: forward 1e-4 max-abs in f32 and f16x3, 5e-4 in f16f8 (tests/test_gpu_config_sweep.py); sampler
1e-3 (tests/test_gpu_sampler.py). tests/test_feature_cache_host.py shows the setting moves these results by 1e-2 or more
and a stale cache moves a forward by O(1)."""
import dataclasses
import functools
import warnings

import numpy as np
import pytest

import feature_cache_ref as ref
import sr3_oracle as oracle
from conftest import cfg_from_meta, load_golden, pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
schedule = pkg("schedule")
samplers = pkg("samplers")
Sr3Error = pkg("_lib").Sr3Error

TOL = {"f32": 1e-4, "f16x3": 1e-4, "f16f8": 5e-4}
BAR = 1e-3
ALL3 = ("f32", "f16x3", "f16f8")
TINY = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
SEEDS = {"tiny": 17, "A": 31, "D": 34}


def _cfg(name):
    return synth.tiny_unet_config() if name == "tiny" else synth.sweep_unet_config(name)


@functools.lru_cache(maxsize=None)
def _weights(name):
    return synth.synth_state_dict(_cfg(name), SEEDS[name])


def _bufs(sched_opt):
    with np.errstate(divide="ignore", invalid="ignore"):
        return schedule.schedule_buffers(sched_opt)


def _engine(cfg, sd, prec="f32", sched_opt=None, kind=None, steps=None, eta=0.0):
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_precision(prec)
    if sched_opt is not None and kind is None:
        e.set_schedule(_bufs(sched_opt))
    elif sched_opt is not None:
        e.set_sampler_schedule(samplers.sampler_tables(_bufs(sched_opt), kind, steps, eta))
    return e


def _ceil(a, b):
    return -(-a // b)


# ---- 1. the shallow forward against the restatement ------------------------------------------------------------------
FORWARD = [("tiny", (2, 16, 16), 1), ("A", (3, 16, 24), 1), ("A", (3, 16, 24), 2), ("D", (2, 16, 16), 1), ("D", (2, 16, 16), 2)]
FORWARD_CASES = [(n, s, d, m) for n, s, d in FORWARD for m in ALL3]


@functools.lru_cache(maxsize=None)
def _forward_inputs(name, shape):
    """Two unrelated inputs of one shape and the restatement's cache of the first."""
    cfg = _cfg(name)
    B, H, W = shape
    xa, nla = synth.synth_unet_input(cfg, B, H, W, SEEDS[name])
    xb, nlb = synth.synth_unet_input(cfg, B, H, W, SEEDS[name] + 100)
    _, cache = ref.forward(_weights(name), cfg, xa, nla)
    return xa, nla.reshape(-1), xb, nlb.reshape(-1), cache


@functools.lru_cache(maxsize=None)
def _forward_want(name, shape, d):
    _, _, xb, nlb, cache = _forward_inputs(name, shape)
    return ref.forward(_weights(name), _cfg(name), xb, nlb, d, cache)[0]


@pytest.mark.parametrize("name,shape,d,prec", FORWARD_CASES,
                         ids=[f"{n}-{s[0]}x{s[1]}x{s[2]}-d{d}-{m}" for n, s, d, m in FORWARD_CASES])
def test_cached_forward_against_the_restatement(name, shape, d, prec):
    """A whole forward of xa, then the shallow forward of an unrelated xb at other noise levels: the restatement's shallow
    forward of xb on the oracle's cache of xa. (A d = 2: attention inside the fresh part, 20-channel groups straddling the
    concatenation; D: unconditional.) A second identical shallow call reproduces the first bit for bit: the fresh part
    leaves the cached output, its twin and its statistics alone."""
    xa, nla, xb, nlb, _ = _forward_inputs(name, shape)
    want = _forward_want(name, shape, d)
    e = _engine(_cfg(name), _weights(name), prec)
    e.unet_forward_np(xa, nla)
    got = e.unet_forward_cached_np(xb, nlb, d)
    again = e.unet_forward_cached_np(xb, nlb, d)
    assert e.fallback_calls() == 0
    e.close()
    err = float(np.abs(got - want).max())
    print(f"cached forward {name} {shape} d={d} [{prec}]: max abs err vs restatement {err:.3e}")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err <= TOL[prec]
    np.testing.assert_array_equal(again, got)


# ---- 2. identity on the device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ALL3)
@pytest.mark.parametrize("B", [2, 64])
def test_cached_forward_of_the_same_input_is_the_whole_forward(B, prec):
    """(At B = 64 the conv plans differ: Winograd in f32, F8C operands in f16f8.)"""
    cfg = _cfg("tiny")
    x, nl = synth.synth_unet_input(cfg, B, 16, 16, 5)
    e = _engine(cfg, _weights("tiny"), prec)
    whole = e.unet_forward_np(x, nl)
    got = e.unet_forward_cached_np(x, nl, 1)
    e.close()
    np.testing.assert_array_equal(got, whole)


@pytest.mark.parametrize("prec", ALL3)
@pytest.mark.parametrize("name,shape,d", [("tiny", (2, 16, 16), 1), ("A", (3, 16, 24), 1), ("A", (3, 16, 24), 2)])
def test_identity_under_dropout(name, shape, d, prec):
    """Train-mode Dropout with one seed: the fresh blocks behind the jump draw the masks of their own layer numbers and
    offsets, so the shallow forward is the whole forward bit for bit; with Dropout off it is not that forward."""
    cfg = dataclasses.replace(_cfg(name), dropout=0.2)
    B, H, W = shape
    x, nl = synth.synth_unet_input(cfg, B, H, W, 6)
    e = _engine(cfg, _weights(name), prec)
    plain = e.unet_forward_np(x, nl)
    e.set_dropout(True, 99, 3)
    whole = e.unet_forward_np(x, nl)
    got = e.unet_forward_cached_np(x, nl, d)
    e.close()
    assert np.abs(whole - plain).max() > 1e-2                        # the masks are live
    np.testing.assert_array_equal(got, whole)


# ---- 3. errors -------------------------------------------------------------------------------------------------------
def test_errors():
    cfg = _cfg("tiny")
    sd = _weights("tiny")
    x, nl = synth.synth_unet_input(cfg, 2, 16, 16, 5)
    e = _engine(cfg, sd, "f32")
    with pytest.raises(Sr3Error, match="no whole forward"):          # nothing ran yet
        e.unet_forward_cached_np(x, nl, 1)
    e.unet_forward_np(x, nl)
    e.unet_forward_cached_np(x, nl, 1)
    for bad in (0, 2, -1):                                           # n_mults = 2: depth 1 only
        with pytest.raises(Sr3Error, match="depth"):
            e.unet_forward_cached_np(x, nl, bad)
        with pytest.raises(Sr3Error, match="depth"):
            e.set_feature_cache(3, bad)
    e.unet_forward_cached_np(x, nl, 1)                               # (a refused call leaves the cache)
    e.set_precision("f16x3")
    with pytest.raises(Sr3Error, match="no whole forward"):
        e.unet_forward_cached_np(x, nl, 1)
    e.set_precision("f32")
    with pytest.raises(Sr3Error, match="no whole forward"):          # back in the cache's own arithmetic: still gone
        e.unet_forward_cached_np(x, nl, 1)
    e.unet_forward_np(x, nl)
    name = "downs.1.res_block.block1.block.3.weight"
    e.load_weight(name, sd[name])
    with pytest.raises(Sr3Error, match="no whole forward"):
        e.unet_forward_cached_np(x, nl, 1)
    e.unet_forward_np(x, nl)
    with pytest.raises(Sr3Error, match="no whole forward"):          # another shape
        e.unet_forward_cached_np(x[:1], nl[:1], 1)
    x2, nl2 = synth.synth_unet_input(cfg, 2, 16, 32, 5)
    with pytest.raises(Sr3Error, match="no whole forward"):
        e.unet_forward_cached_np(x2, nl2, 1)
    e.unet_forward_cached_np(x, nl, 1)
    e.close()


# ---- 4. the samplers against the restatement -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loop_inputs(name, B):
    cfg = _cfg(name)
    sd = synth.synth_state_dict(cfg, 17)
    r, T = 16, TINY["n_timestep"]
    return cfg, sd, synth.synth_cond(B, r, 8, 17), synth.synth_noise(T, B, 3, r, r, 17)


@functools.lru_cache(maxsize=None)
def _ddpm_want(name, B, interval, d):
    cfg, sd, cond, noise = _loop_inputs(name, B)
    return ref.sample_loop(sd, cfg, oracle.noise_schedule(TINY), cond, noise, interval, d)


DDPM = [("tiny", 2, 2, 1), ("tiny", 2, 3, 1), ("tiny", 2, 7, 1), ("A", 2, 3, 2), ("A", 2, 2, 1)]
DDPM_CASES = [(n, B, i, d, m) for n, B, i, d in DDPM for m in ("f32", "f16x3")] + [("tiny", 64, 3, 1, "f16f8")]


@pytest.mark.parametrize("name,B,interval,d,prec", DDPM_CASES,
                         ids=[f"{n}-B{B}-N{i}-d{d}-{m}" for n, B, i, d, m in DDPM_CASES])
def test_ddpm_against_the_restatement(name, B, interval, d, prec):
    cfg, sd, cond, noise = _loop_inputs(name, B)
    want, want_fr = _ddpm_want(name, B, interval, d)
    T = TINY["n_timestep"]
    e = _engine(cfg, sd, prec, TINY)
    e.set_feature_cache(interval, d)
    got, got_fr = e.sample_np(cond, noise=noise, frames=True)
    counts = e.feature_cache_steps()
    assert e.fallback_calls() == 0
    e.close()
    err = np.abs(got_fr - want_fr).reshape(want_fr.shape[0], -1).max(1)
    e_fin = float(np.abs(got - want).max())
    print(f"ddpm {name} B={B} interval={interval} d={d} [{prec}]: per-frame max abs err {np.array2string(err, precision=2)}, "
          f"final {e_fin:.2e}; steps {counts}")
    assert counts == (_ceil(T, interval), T - _ceil(T, interval))
    assert err.max() <= BAR and e_fin <= BAR


@pytest.mark.parametrize("prec", ("f32", "f16x3"))
@pytest.mark.parametrize("kind,S,eta,interval", [("ddim", 10, 0.5, 2), ("dpmpp_2m", 10, 0.0, 3)])
def test_few_step_samplers_against_the_restatement(kind, S, eta, interval, prec):
    cfg, sd, cond, noise = _loop_inputs("tiny", 2)
    want, want_fr = ref.fast_sample_loop(sd, cfg, TINY, cond, noise[:S], kind, S, eta, interval, 1)
    e = _engine(cfg, sd, prec, TINY, kind, S, eta)
    e.set_feature_cache(interval, 1)
    got, got_fr = e.sample_np(cond, noise=noise[:S], frames=True)
    counts = e.feature_cache_steps()
    e.close()
    err = np.abs(got_fr - want_fr).reshape(want_fr.shape[0], -1).max(1)
    print(f"{kind} S={S} eta={eta} interval={interval} [{prec}]: per-frame max abs err {np.array2string(err, precision=2)}; "
          f"steps {counts}")
    assert counts == (_ceil(S, interval), S - _ceil(S, interval))
    assert err.max() <= BAR and float(np.abs(got - want).max()) <= BAR


# ---- 5. off is off ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ("f32", "f16x3"))
def test_off_is_off(prec):
    g = load_golden("sampler_tiny.npz")
    m = g["meta"]
    cfg = cfg_from_meta(m)
    B, r, T = m["B"], m["r"], m["schedule"]["n_timestep"]
    noise = synth.synth_noise(T, B, 3, r, r, m["seed"])
    e = _engine(cfg, synth.synth_state_dict(cfg, m["seed"]), prec, m["schedule"])
    first = e.sample_np(g["cond"], noise=noise)
    assert e.feature_cache_steps() == (T, 0)
    e.set_feature_cache(3, 1)
    on = e.sample_np(g["cond"], noise=noise)
    assert e.feature_cache_steps() == (_ceil(T, 3), T - _ceil(T, 3))
    e.set_feature_cache(None)
    third = e.sample_np(g["cond"], noise=noise)
    assert e.feature_cache_steps() == (T, 0)
    e.set_feature_cache(1)
    one = e.sample_np(g["cond"], noise=noise)
    assert e.feature_cache_steps() == (T, 0)
    e.close()
    np.testing.assert_array_equal(third, first)
    np.testing.assert_array_equal(one, first)
    err = float(np.abs(first[-1] - g["last"]).max())
    print(f"off is off [{prec}]: max abs err vs the reference's run {err:.2e}; interval 3 moved it by {np.abs(on - first).max():.3f}")
    assert err <= BAR
    assert not np.array_equal(on, first)


# ---- 6. the step API and the warm start ------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ("f32", "f16x3"))
def test_step_api_equals_sample(prec):
    cfg, sd, cond, noise = _loop_inputs("tiny", 2)
    B, r, T = 2, 16, TINY["n_timestep"]
    e = _engine(cfg, sd, prec, TINY)
    e.set_feature_cache(3, 1)
    want = e.sample_np(cond, noise=noise)
    dc, dn, out = e.to_device(cond), e.to_device(noise), e.buffer(B * 3 * r * r)
    slab = B * 3 * r * r * 4
    e.sample_begin(dc.ptr, B, r, r, dn.ptr)
    for t in reversed(range(T)):
        e.sample_step(t, dn.ptr + (T - t) * slab if t > 0 else None)
    e.sample_end(out.ptr)
    got = out.download((B, 3, r, r))
    counts = e.feature_cache_steps()
    e.close()
    np.testing.assert_array_equal(got, want)
    assert counts == (_ceil(T, 3), T - _ceil(T, 3))


def test_warm_start_step_api_equals_sample_from():
    """A call begun at step 11 of 20: the counter starts at the begin, so its first step is whole, and the step API is
    sr3_sample_from bit for bit."""
    cfg, sd, cond, noise = _loop_inputs("tiny", 2)
    B, r, s0 = 2, 16, 11
    init = synth.synth_cond(B, r, 8, 23)
    e = _engine(cfg, sd, "f32", TINY)
    e.set_feature_cache(3, 1)
    dc, di, dn, out = e.to_device(cond), e.to_device(init), e.to_device(noise[:s0]), e.buffer(B * 3 * r * r)
    e.sample(dc.ptr, B, r, r, out.ptr, dn.ptr, 0, 0, None, init_ptr=di.ptr, start_step=s0)
    want = out.download((B, 3, r, r))
    assert e.feature_cache_steps() == (_ceil(s0, 3), s0 - _ceil(s0, 3))
    slab = B * 3 * r * r * 4
    e.sample_begin_from(dc.ptr, B, r, r, di.ptr, s0, True, dn.ptr)
    assert e.feature_cache_steps() == (0, 0)
    for n, t in enumerate(reversed(range(s0))):
        e.sample_step(t, dn.ptr + (s0 - t) * slab if t > 0 else None)
        if n == 0:
            assert e.feature_cache_steps() == (1, 0)
        if n == 1:
            assert e.feature_cache_steps() == (1, 1)
    e.sample_end(out.ptr)
    got = out.download((B, 3, r, r))
    assert e.feature_cache_steps() == (_ceil(s0, 3), s0 - _ceil(s0, 3))
    e.close()
    np.testing.assert_array_equal(got, want)


def test_a_forward_between_steps_discards_the_cache():
    """sr3_unet_forward overwrites the sampler state and has always ended the live sampling call: the next step is an
    error, not a shallow step on that forward's features. The call begun afterwards starts with a whole step, and the
    shallow forward entry point still finds the forward's features (they are the workspace's)."""
    cfg, sd, cond, noise = _loop_inputs("tiny", 2)
    B, r, T = 2, 16, TINY["n_timestep"]
    e = _engine(cfg, sd, "f32", TINY)
    e.set_feature_cache(3, 1)
    dc, dn = e.to_device(cond), e.to_device(noise)
    slab = B * 3 * r * r * 4
    e.sample_begin(dc.ptr, B, r, r, dn.ptr)
    e.sample_step(T - 1, dn.ptr + slab)
    e.sample_step(T - 2, dn.ptr + 2 * slab)
    assert e.feature_cache_steps() == (1, 1)
    x, nl = synth.synth_unet_input(cfg, B, r, r, 5)
    whole = e.unet_forward_np(x, nl)
    with pytest.raises(Sr3Error, match="before sr3_sample_begin"):
        e.sample_step(T - 3, dn.ptr + 3 * slab)
    assert e.feature_cache_steps() == (1, 1)
    np.testing.assert_array_equal(e.unet_forward_cached_np(x, nl, 1), whole)
    e.sample_begin(dc.ptr, B, r, r, dn.ptr)
    e.sample_step(T - 1, dn.ptr + slab)
    assert e.feature_cache_steps() == (1, 0)
    e.synchronize()
    e.close()


# ---- 7. the range guard ----------------------------------------------------------------------------------------------
def test_mid_call_fallback_replays_whole_intervals():
    """The construction of test_gpu_fast_samplers.py::test_mid_call_fallback_restores_the_x0_history (dpmpp_2m, S = 20,
    step i = 8 leaves the fp16 range) with interval 3: the guard's segments are 3 steps, not 2, so the flag is seen after
    step 8 (12 steps run), the checkpoint is the one in front of step 10 (9 steps run, a multiple of 3) and steps 10, 9, 8
    are replayed in f32 as whole, shallow, shallow — the pattern of the step index. 23 steps in all, 8 of them whole."""
    Sr3RangeWarning = pkg("_lib").Sr3RangeWarning
    import fast_sampler_ref as fast
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 12)
    sched = {"schedule": "linear", "n_timestep": 40, "linear_start": 1e-4, "linear_end": 2e-2}
    B, r, S, i_hot = 2, 16, 20, 8
    tables = samplers.sampler_tables(_bufs(sched), "dpmpp_2m", S)
    tables["sigma"][i_hot] = 1.0
    co = fast.coefficients(sched, "dpmpp_2m", S)
    co[i_hot]["sigma"] = 1.0
    cond = synth.synth_cond(B, r, 8, 12)
    noise = synth.synth_noise(S, B, 3, r, r, 12)
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_sampler_schedule(tables)
    e.set_precision("f16x3")
    e.set_feature_cache(3, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # ordinary noise: no fallback
        e.sample_np(cond, noise=noise)
    assert e.feature_cache_steps() == (7, 13)
    noise[S - i_hot] *= np.float32(1e5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        fin, frames = e.sample_np(cond, noise=noise, frames=True)
    n_fb, counts = e.fallback_calls(), e.feature_cache_steps()
    e.set_range_policy(True)
    with pytest.raises(Sr3Error, match="fp16 range"):
        e.sample_np(cond, noise=noise)
    e.close()
    assert any(issubclass(w.category, Sr3RangeWarning) for w in rec) and n_fb == 1
    assert counts == (8, 15)
    want_fin, want = ref.fast_sample_loop(sd, cfg, sched, cond, noise, "dpmpp_2m", S, 0.0, 3, 1, coefs=co)
    steps = schedule.frame_steps(S)
    assert steps[:4] == [18, 15, 12, 9]
    dref = np.abs(frames[:4] - want[:4]).reshape(4, -1).max(1)
    e_fin = float(np.abs(fin - want_fin).max())
    print(f"mid-call fallback with interval 3, frames i = 18, 15, 12, 9: max |f16x3 + f32 replay - restatement| "
          f"{np.array2string(dref, precision=2)}, final {e_fin:.2e}")
    assert np.isfinite(fin).all() and dref.max() <= BAR and e_fin <= BAR


# ---- 8. the torch facade ---------------------------------------------------------------------------------------------
def _netG(seed):
    import torch
    cfg = synth.tiny_unet_config()
    opt = {"phase": "val", "sr": {"model": {
        "which_model_G": "sr3",
        "unet": {"in_channel": 6, "out_channel": 3, "inner_channel": cfg.inner_channel,
                 "channel_multiplier": list(cfg.channel_mults), "attn_res": list(cfg.attn_res),
                 "res_blocks": cfg.res_blocks, "dropout": 0.0},
        "beta_schedule": {"train": TINY, "val": TINY},
        "diffusion": {"image_size": cfg.image_size, "channels": 3, "conditional": True}}}}
    netG = pkg().define_G(opt).to("cuda:0")
    netG.load_state_dict({"denoise_fn." + k: torch.from_numpy(v) for k, v in synth.synth_state_dict(cfg, seed).items()},
                         strict=False)
    netG.set_new_noise_schedule(TINY, [0])
    return netG


def test_facade():
    import torch
    netG = _netG(61)
    cfg = synth.tiny_unet_config()
    B, r, L = 5, 16, 8
    cond = synth.synth_cond(B, r, L, 61)
    x = torch.from_numpy(cond).cuda()
    plain = netG.super_resolution_batch(x, seed=1234)
    netG.set_feature_cache(3, 1)
    got = netG.super_resolution_batch(x, seed=1234)
    eng = netG.denoise_fn.engine()
    assert eng.feature_cache_steps() == (7, 13)
    e = _engine(cfg, synth.synth_state_dict(cfg, 61), getattr(eng, "precision", "f32"), TINY)
    e.set_feature_cache(3, 1)
    want = e.sample_np(cond, seed=1234)
    e.close()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert not torch.equal(got, plain)
    # every chunk is a call of its own and starts with a whole step
    chunked = netG.sample_batch(x, seed=1234, max_chunk=2)
    assert float((chunked - got).abs().max()) <= 2e-6
    # with the projection and the dynamic threshold on as well
    lr = torch.from_numpy(np.random.RandomState(61 ^ 0x10C0).uniform(-1, 1, (B, 3, L, L)).astype(np.float32))
    netG.set_lr_consistency(lr)
    netG.set_dynamic_threshold(0.995)
    both = netG.sample_batch(x, seed=1234)
    assert eng.feature_cache_steps() == (7, 13) and torch.isfinite(both).all()
    res = pkg("validation").lr_consistency(netG, both, lr)["max_abs"]
    print(f"facade, interval 3 with projection and threshold: max |A img - y| {res.max():.2e}")
    assert res.max() <= 5e-7                                         # the bound README.md states for the projection
    # off again: the plain sampler
    netG.set_lr_consistency(None)
    netG.set_dynamic_threshold(None)
    netG.set_feature_cache(None)
    assert torch.equal(netG.super_resolution_batch(x, seed=1234), plain)
    assert eng.feature_cache_steps() == (20, 0)
    torch.cuda.synchronize()
