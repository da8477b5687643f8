"""Few-step samplers on the GPU (sr3_set_sampler_schedule): DDIM with eta = 1 over every step against
the reference-made golden runs, DDIM / DPM-Solver++(2M) over a few steps against the numpy restatement
(fast_sampler_ref.py), the x0 history across the step API, checkpoint replays and calls, and the torch facade.
Bar 1e-3 max-abs as in test_gpu_sampler.py."""
import warnings

import numpy as np
import pytest

import fast_sampler_ref as ref
from conftest import cfg_from_meta, load_golden, pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
schedule = pkg("schedule")
samplers = pkg("samplers")
BAR = 1e-3
PRECISIONS = ["f32", "f16x3"]
TINY = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}


def _bufs(sched_opt):
    with np.errstate(divide="ignore", invalid="ignore"):
        return schedule.schedule_buffers(sched_opt)


def _engine(cfg, sd, sched_opt, prec="f32", kind=None, steps=None, eta=0.0):
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_precision(prec)
    if kind is None:
        e.set_schedule(_bufs(sched_opt))
    else:
        e.set_sampler_schedule(samplers.sampler_tables(_bufs(sched_opt), kind, steps, eta))
    return e


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ["sampler_tiny.npz", "sampler_uncond_tiny.npz", "sampler_cfg1_8_16.npz"])
def test_ddim_eta1_full_schedule_matches_reference(name, prec):
    g = load_golden(name)
    m = g["meta"]
    cfg = cfg_from_meta(m)
    B, r, T = m["B"], m["r"], m["schedule"]["n_timestep"]
    e = _engine(cfg, synth.synth_state_dict(cfg, m["seed"]), m["schedule"], prec, "ddim", None, 1.0)
    noise = synth.synth_noise(T, B, 3, r, r, m["seed"])
    cond = g["cond"] if m["conditional"] else None
    final, frames = e.sample_np(cond, noise=noise, frames=True, shape=(B, 3, r, r))
    nf = frames.shape[0]
    assert nf == len(schedule.frame_steps(T)) == (g["ret_img"].shape[0] // B - 1)
    err = np.abs(frames - g["ret_img"][B:].reshape(nf, B, 3, r, r)).reshape(nf, -1).max(1)
    e_last = np.abs(final[-1] - g["last"]).max()
    print(f"{name} ddim eta=1 S=T [{prec}]: per-frame max abs err {np.array2string(err, precision=2)}, last {e_last:.2e}")
    e.close()
    assert err.max() <= BAR and e_last <= BAR
    np.testing.assert_array_equal(final, frames[-1])


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("kind,S,eta", [("ddim", 5, 0.0), ("ddim", 10, 0.5), ("dpmpp_2m", 3, 0.0),
                                        ("dpmpp_2m", 5, 0.0), ("dpmpp_2m", 10, 0.0)])
def test_few_step_samplers_match_restatement(kind, S, eta, prec):
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 17)
    B, r = 2, 16
    cond = synth.synth_cond(B, r, 8, 17)
    noise = synth.synth_noise(S, B, 3, r, r, 17)
    want_f, want_fr = ref.sample_loop(sd, cfg, TINY, cond, noise, kind, S, eta)
    e = _engine(cfg, sd, TINY, prec, kind, S, eta)
    got_f, got_fr = e.sample_np(cond, noise=noise, frames=True)
    e.close()
    assert got_fr.shape == want_fr.shape and want_fr.shape[0] == len(schedule.frame_steps(S))
    err = np.abs(got_fr - want_fr).reshape(want_fr.shape[0], -1).max(1)
    print(f"{kind} S={S} eta={eta} [{prec}]: per-frame max abs err {np.array2string(err, precision=2)}")
    assert err.max() <= BAR
    np.testing.assert_array_equal(got_f, got_fr[-1])


@pytest.mark.parametrize("kind,eta", [("ddim", 0.0), ("dpmpp_2m", 0.0)])
def test_sigma_zero_samplers_ignore_later_noise_slabs(kind, eta):
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 23)
    B, r, S = 2, 16, 8
    cond = synth.synth_cond(B, r, 8, 23)
    n1 = synth.synth_noise(S, B, 3, r, r, 23)
    n2 = synth.synth_noise(S, B, 3, r, r, 24)
    n2[0] = n1[0]
    e = _engine(cfg, sd, TINY, "f32", kind, S, eta)
    a, b = e.sample_np(cond, noise=n1), e.sample_np(cond, noise=n2)
    e.close()
    np.testing.assert_array_equal(a, b)


def test_step_api_equals_sample_dpmpp_2m():
    """The x0 history lives in the library across external sr3_sample_step calls."""
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 41)
    B, r, S = 2, 16, 7
    e = _engine(cfg, sd, TINY, "f32", "dpmpp_2m", S)
    cond, noise = synth.synth_cond(B, r, 8, 41), synth.synth_noise(S, B, 3, r, r, 41)
    want = e.sample_np(cond, noise=noise)
    dc, dn, out = e.to_device(cond), e.to_device(noise), e.buffer(B * 3 * r * r)
    slab = B * 3 * r * r * 4
    e.sample_begin(dc.ptr, B, r, r, dn.ptr)
    for t in reversed(range(S)):
        e.sample_step(t, dn.ptr + (S - t) * slab if t > 0 else None)
    e.sample_end(out.ptr)
    got = out.download((B, 3, r, r))
    np.testing.assert_array_equal(got, want)
    assert np.abs(got).max() <= 1.0
    # a caller that starts below t = S-1: the first step after sr3_sample_begin reads no history of the earlier call
    fresh = _engine(cfg, sd, TINY, "f32", "dpmpp_2m", S)
    outs = []
    for eng in (e, fresh):
        o, c_d, n_d = eng.buffer(B * 3 * r * r), eng.to_device(cond), eng.to_device(noise)   # (kept alive: async use)
        eng.sample_begin(c_d.ptr, B, r, r, n_d.ptr)
        for t in reversed(range(S - 2)):
            eng.sample_step(t, None)
        eng.sample_end(o.ptr)
        outs.append(o.download((B, 3, r, r)))
        del c_d, n_d
    e.close()
    fresh.close()
    np.testing.assert_array_equal(outs[0], outs[1])


def test_mid_call_fallback_restores_the_x0_history():
    """The range flag trips in the middle of a dpmpp_2m call, where the x0 history is live: the dpmpp_2m tables get a
    noise term on step i = 8 only, and its injected slab is scaled so that the state leaves the fp16 range there (the
    construction of test_gpu_round3.py::test_overflow_late_in_the_loop_replays_from_the_last_checkpoint). The guard
    (segments of 2 steps) sees the flag at the boundary before step 7 and rewinds to the checkpoint before step 9, whose
    history is the x0 of step 10; step 9 is replayed in f32 and reads it. Its frame (i = 9) and every earlier frame meet
    the all-f32 call and the restatement; with the history left out of the checkpoint, frame i = 9 misses the f32 call."""
    Sr3RangeWarning = pkg("_lib").Sr3RangeWarning
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 12)
    sched = {"schedule": "linear", "n_timestep": 40, "linear_start": 1e-4, "linear_end": 2e-2}
    B, r, S, i_hot = 2, 16, 20, 8
    tables = samplers.sampler_tables(_bufs(sched), "dpmpp_2m", S)
    tables["sigma"][i_hot] = 1.0
    co = ref.coefficients(sched, "dpmpp_2m", S)
    co[i_hot]["sigma"] = 1.0
    cond = synth.synth_cond(B, r, 8, 12)
    noise = synth.synth_noise(S, B, 3, r, r, 12)
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_sampler_schedule(tables)
    e.set_precision("f16x3")
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # ordinary noise: no fallback
        e.sample_np(cond, noise=noise)
    noise[S - i_hot] *= np.float32(1e5)                     # the draw of step i = 8: |x| ~ 1e5 after it
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        fin, frames = e.sample_np(cond, noise=noise, frames=True)
    n_fb = e.fallback_calls()
    e.set_precision("f32")
    fin32, frames32 = e.sample_np(cond, noise=noise, frames=True)
    e.close()
    assert any(issubclass(w.category, Sr3RangeWarning) for w in rec) and n_fb == 1
    _, want = ref.sample_loop(sd, cfg, sched, cond, noise, "dpmpp_2m", S, coefs=co)
    steps = schedule.frame_steps(S)
    assert steps[:4] == [18, 15, 12, 9] and frames.shape[0] == len(steps)
    d32 = np.abs(frames[:4] - frames32[:4]).reshape(4, -1).max(1)
    dref = np.abs(frames[:4] - want[:4]).reshape(4, -1).max(1)
    late = np.abs(frames[4:] - frames32[4:]).max() / max(1.0, float(np.abs(frames32[4:]).max()))
    print(f"mid-call fallback, frames i = 18, 15, 12, 9: max |f16x3 + f32 replay - all f32| {np.array2string(d32, precision=2)}, "
          f"- restatement {np.array2string(dref, precision=2)}; later frames relative {late:.1e}")
    # the f16x3 segments before the rewind differ from f32 by ~1e-6: a tighter bar than BAR for the replayed frame
    # (the history left out of the checkpoint puts frame i = 9 ~2e-3 off)
    assert d32.max() <= 2e-5 and dref.max() <= BAR
    assert np.isfinite(fin).all() and late <= 1e-4 and np.abs(fin - fin32).max() <= BAR


def test_fp8_range_fallback_reported_for_dpmpp_2m():
    """The network of test_gpu_f16f8.py::test_fp8_range_falls_back_to_f16x3_first (32x32-level activations beyond the
    fp8 operand range on every forward): a dpmpp_2m call in f16f8 trips in its first segment, finishes one arithmetic
    down, reports the fallback and meets the f32 call. (The history across a restore: the test above.)"""
    Sr3RangeWarning = pkg("_lib").Sr3RangeWarning
    cfg = synth.yml_unet_config(224)
    sd = synth.synth_state_dict(cfg, 3)
    name = next(k for k, v in sd.items() if k.startswith("downs.") and k.endswith("res_block.block2.block.0.weight") and v.shape == (256,))
    sd[name] = sd[name] * np.float32(400.0)
    B, S = 64, 10
    sched = {"schedule": "linear", "n_timestep": 100, "linear_start": 1e-6, "linear_end": 1e-2}
    cond = synth.synth_cond(B, 128, 16, 5)
    e = _engine(cfg, sd, sched, "f32", "dpmpp_2m", S)
    want = e.sample_np(cond, seed=7)
    e.set_precision("f16f8")
    with pytest.warns(Sr3RangeWarning, match="f16x3"):
        got = e.sample_np(cond, seed=7)
    n_fb = e.fallback_calls()
    e.close()
    err = float(np.abs(got - want).max())
    print(f"dpmpp_2m S={S} f16f8 -> f16x3 fallback vs f32: max abs err {err:.2e}")
    assert n_fb == 1 and err <= BAR


def test_ddpm_after_dpmpp_2m_is_unaffected():
    """No table, history or captured graph of a dpmpp_2m call leaks into a later DDPM call on the same engine."""
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 51)
    B, r = 3, 16
    cond = synth.synth_cond(B, r, 8, 51)
    for prec in PRECISIONS:
        fresh = _engine(cfg, sd, TINY, prec)
        want, want_fr = fresh.sample_np(cond, seed=99, frames=True)
        fresh.close()
        e = _engine(cfg, sd, TINY, prec, "dpmpp_2m", 6)
        e.sample_np(cond, seed=99)
        e.set_schedule(_bufs(TINY))
        got, got_fr = e.sample_np(cond, seed=99, frames=True)
        e.close()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_fr, want_fr)


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


def test_facade_sampler_setting():
    import torch
    netG = _netG(61)
    B, r = 5, 16
    x = torch.from_numpy(synth.synth_cond(B, r, 8, 61)).cuda()
    keys = list(netG.state_dict())
    netG.set_sampler("dpmpp_2m", steps=7)
    assert netG.num_sampling_steps == 7 and netG.num_timesteps == 20 and list(netG.state_dict()) == keys
    # continous: cond + one frame per recorded step of the S-step loop
    ret = netG.super_resolution(x[:2], continous=True)
    assert ret.shape[0] == 2 * (1 + len(schedule.frame_steps(7)))
    # injected noise has S slabs and meets the restatement
    noise = synth.synth_noise(7, 2, 3, r, r, 61)
    out = netG.super_resolution_batch(x[:2], noise=torch.from_numpy(noise))
    want, _ = ref.sample_loop(synth.synth_state_dict(synth.tiny_unet_config(), 61), synth.tiny_unet_config(), TINY,
                              x[:2].cpu().numpy(), noise, "dpmpp_2m", 7)
    assert float(np.abs(out.cpu().numpy() - want).max()) <= BAR
    with pytest.raises(RuntimeError):
        netG.super_resolution_batch(x[:2], noise=torch.from_numpy(synth.synth_noise(20, 2, 3, r, r, 61)))
    # chunked == unchunked with device Philox, and a shard reproduces its slice
    netG.set_sampler("ddim", steps=9, eta=0.5)
    full = netG.sample_batch(x, seed=1234)
    chunked = netG.sample_batch(x, seed=1234, max_chunk=2)
    assert float((full - chunked).abs().max()) <= 2e-6
    shard = netG.super_resolution_batch(x[2:], seed=1234, image_offset=2)
    assert float((shard - full[2:]).abs().max()) <= 2e-6
    # the setting persists over a new schedule; "ddpm" is the reference loop again
    netG.set_new_noise_schedule(dict(TINY, n_timestep=30), [0])
    assert netG.num_sampling_steps == 9
    assert netG.sample_batch(x[:1], seed=5).shape == (1, 3, r, r)
    netG.set_sampler("ddpm")
    got = netG.super_resolution_batch(x[:2], seed=77)
    fresh = _netG(61)
    fresh.set_new_noise_schedule(dict(TINY, n_timestep=30), [0])
    torch.testing.assert_close(got, fresh.super_resolution_batch(x[:2], seed=77), rtol=0, atol=0)
    torch.cuda.synchronize()


def test_headline_shape_dpmpp_2m_f16f8_vs_f32():
    """B = 64, 16 -> 128, the yml UNet of bench.py, T = 1000, dpmpp_2m with S = 20: f16f8 meets f32, no fallback."""
    cfg = synth.yml_unet_config(224)
    sd = synth.synth_state_dict(cfg, 0)
    sched = {"schedule": "linear", "n_timestep": 1000, "linear_start": 1e-6, "linear_end": 1e-2}
    B = 64
    cond = synth.synth_cond(B, 128, 16, 0)
    e = _engine(cfg, sd, sched, "f32", "dpmpp_2m", 20)
    want = e.sample_np(cond, seed=11)
    e.set_precision("f16f8")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = e.sample_np(cond, seed=11)
    assert e.fallback_calls() == 0
    e.close()
    err = float(np.abs(got - want).max())
    print(f"dpmpp_2m S=20 B={B} 16->128 f16f8 vs f32: max abs err {err:.2e}")
    assert err <= BAR
