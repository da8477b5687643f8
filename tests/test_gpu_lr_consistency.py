"""Low-resolution consistency on the GPU: the projection op in both forms and the residual score against
the float64 reference (lr_consistency_ref.py), strength 0 = the old sampler bit for bit, strength 1 = a sample that
downsamples to its LR input and follows the float64 projected chain, and the invariances of the rest of the sampler
(offsets, chunks, validation batches, range replays, graph toggling, Dropout) with the feature on.

Bars. Projection and residual after it: 1e-5 absolute, the bar of the fp32 post-processing chain; a numpy fp32 emulation
of the four stages is 8.6e-7 / 4.8e-7 off on these shapes. Chains: 1e-4, the TOL of the fixture tests."""
import functools
import warnings

import numpy as np
import pytest

import lr_consistency_ref as ref
from conftest import pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
schedule = pkg("schedule")
samplers = pkg("samplers")

BAR_OP = 1e-5
BAR_CHAIN = 1e-4
SCHED = {"ddpm": {"schedule": "linear", "n_timestep": 6, "linear_start": 1e-4, "linear_end": 2e-2},
         "fast": {"schedule": "linear", "n_timestep": 12, "linear_start": 1e-4, "linear_end": 2e-2}}
CASES = [("ddpm", None, 0.0), ("ddim", 4, 0.0), ("ddim", 4, 0.5), ("dpmpp_2m", 4, 0.0)]
CASE_IDS = ["ddpm_T6", "ddim_S4", "ddim_S4_eta0.5", "dpmpp_2m_S4"]
SEED = 31
B, R, L, N_LR, ROW0 = 3, 16, 8, 3, 0


def _bufs(sched_opt):
    with np.errstate(divide="ignore", invalid="ignore"):
        return schedule.schedule_buffers(sched_opt)


def _sched(kind):
    return SCHED["ddpm" if kind == "ddpm" else "fast"]


def _engine(cfg, sd, kind, steps, eta, prec="f32"):
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_precision(prec)
    if kind == "ddpm":
        e.set_schedule(_bufs(_sched(kind)))
    else:
        e.set_sampler_schedule(samplers.sampler_tables(_bufs(_sched(kind)), kind, steps, eta))
    return e


def _lr_images(n, l, seed, C=3):
    return np.random.RandomState(seed ^ 0x10C0).uniform(-1, 1, (n, C, l, l)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(kind, steps):
    cfg = synth.tiny_unet_config()
    S = steps if steps else _sched(kind)["n_timestep"]
    return (cfg, synth.synth_state_dict(cfg, SEED), synth.synth_cond(B, R, L, SEED), synth.synth_noise(S, B, 3, R, R, SEED),
            _lr_images(N_LR, L, SEED))


@functools.lru_cache(maxsize=None)
def _chain(kind, steps, eta, projected):
    """float64 chain of the case (computed once, shared, never modified)."""
    cfg, sd, cond, noise, lr = _inputs(kind, steps)
    fin, frames = ref.sample_loop(sd, cfg, _sched(kind), cond, noise, kind, steps, eta, lr=lr if projected else None,
                                  row_offset=ROW0)
    fin.setflags(write=False)
    frames.setflags(write=False)
    return fin, frames


def _run(e, cond, noise, lr=None, strength=1.0, row_offset=ROW0, frames=True):
    dl = e.to_device(lr) if lr is not None else None
    if lr is not None:
        e.set_lr_consistency(dl.ptr, lr.shape[0], lr.shape[2], lr.shape[3], row_offset, strength)
    else:
        e.set_lr_consistency(None)
    out = e.sample_np(cond, noise=noise, frames=frames)
    e.synchronize()
    return out


# ---- the projection op --------------------------------------------------------------------------------------------------
OP_SHAPES = [(8, 8, 16, 16, "auto"), (4, 4, 16, 16, "auto"), (10, 10, 24, 24, "auto"), (8, 12, 16, 24, "auto"),
             (16, 16, 128, 128, "lds"), (16, 16, 128, 128, "scratch"), (32, 32, 256, 256, "auto"), (32, 32, 256, 256, "scratch")]


@pytest.fixture(scope="module")
def op_engine():
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    yield e
    e.close()


def _op_inputs(lh, lw, H, W):
    rs = np.random.RandomState(lh * 1000 + W)
    x = np.clip(rs.standard_normal((3, 3, H, W)), -1, 1).astype(np.float32)
    y = rs.uniform(-1, 1, (2, 3, lh, lw)).astype(np.float32)
    return x, y


@pytest.mark.parametrize("lh,lw,H,W,form", OP_SHAPES, ids=[f"{a}x{b}to{c}x{d}_{f}" for a, b, c, d, f in OP_SHAPES])
def test_projection_matches_float64(op_engine, lh, lw, H, W, form):
    e = op_engine
    x, y = _op_inputs(lh, lw, H, W)
    want = ref.project(x, y, row_offset=1)
    got = e.lr_project_np(x, y, row_offset=1, strength=1.0, form=form)
    half = e.lr_project_np(x, y, row_offset=1, strength=0.5, form=form)
    twice = e.lr_project_np(got, y, row_offset=1, strength=1.0, form=form)
    err = float(np.abs(got - want).max())
    res = float(ref.residual(got.astype(np.float64), y, row_offset=1)["max_abs"].max())
    e_half = float(np.abs(half - 0.5 * (x.astype(np.float64) + want)).max())
    e_twice = float(np.abs(twice - got).max())
    moved = float(np.abs(want - x).max())
    print(f"{lh}x{lw}->{H}x{W} [{form}]: |gpu - f64| {err:.2e}, |A X' - Y| {res:.2e}, strength 0.5 off the midpoint {e_half:.2e}, "
          f"second projection moves {e_twice:.2e} (the first moved {moved:.2f})")
    assert err <= BAR_OP and res <= BAR_OP and e_half <= BAR_OP and e_twice <= BAR_OP
    assert moved > 0.1


@pytest.mark.parametrize("lh,lw,H,W", [(16, 16, 128, 128), (32, 32, 256, 256), (10, 10, 24, 24)])
def test_both_forms_agree(op_engine, lh, lw, H, W):
    x, y = _op_inputs(lh, lw, H, W)
    a = op_engine.lr_project_np(x, y, row_offset=1, form="lds")
    b = op_engine.lr_project_np(x, y, row_offset=1, form="scratch")
    d = float(np.abs(a - b).max())
    print(f"{lh}x{lw}->{H}x{W}: LDS form vs scratch form {d:.2e}")
    assert d <= 1e-6


def test_lds_form_refuses_planes_that_do_not_fit(op_engine):
    x, y = _op_inputs(64, 64, 512, 512)
    with pytest.raises(pkg("_lib").Sr3Error, match="LDS form"):
        op_engine.lr_project_np(x[:1], y, form="lds")
    got = op_engine.lr_project_np(x[:1], y, form="auto")         # (takes the scratch form)
    assert float(np.abs(got - ref.project(x[:1], y)).max()) <= BAR_OP


@pytest.mark.parametrize("lh,lw,H,W", [(8, 8, 16, 16), (10, 10, 24, 24), (8, 12, 16, 24), (16, 16, 128, 128)])
def test_residual_score_matches_float64(op_engine, lh, lw, H, W):
    x, y = _op_inputs(lh, lw, H, W)
    got = op_engine.lr_residual_np(x, y, row_offset=1)
    want = ref.residual(x, y, row_offset=1)
    rel = float(np.abs(got["sumsq"] / want["sumsq"] - 1).max())
    dmax = float(np.abs(got["max_abs"] - want["max_abs"]).max())
    print(f"{lh}x{lw}->{H}x{W}: sumsq relative error {rel:.2e}, max_abs off by {dmax:.2e}")
    assert rel <= 1e-6 and dmax <= 1e-6
    again = op_engine.lr_residual_np(x, y, row_offset=1)
    assert again["sumsq"].tobytes() == got["sumsq"].tobytes() and again["max_abs"].tobytes() == got["max_abs"].tobytes()


# ---- strength 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("kind,steps,eta", CASES, ids=CASE_IDS)
def test_strength_zero_is_the_old_sampler_bit_for_bit(kind, steps, eta, prec):
    cfg, sd, cond, noise, lr = _inputs(kind, steps)
    e = _engine(cfg, sd, kind, steps, eta, prec)
    S = noise.shape[0]
    off, off_fr = _run(e, cond, noise)
    zero, zero_fr = _run(e, cond, noise, lr, strength=0.0)
    assert zero.tobytes() == off.tobytes() and zero_fr.tobytes() == off_fr.tobytes()
    # the step API
    dc, dn, dl, out = e.to_device(cond), e.to_device(noise), e.to_device(lr), e.buffer(B * 3 * R * R)
    slab = B * 3 * R * R * 4
    e.set_lr_consistency(dl.ptr, N_LR, L, L, ROW0, 0.0)
    e.sample_begin(dc.ptr, B, R, R, dn.ptr)
    for t in reversed(range(S)):
        e.sample_step(t, dn.ptr + (S - t) * slab if t > 0 else None)
    e.sample_end(out.ptr)
    stepped = out.download((B, 3, R, R))
    e.close()
    assert stepped.tobytes() == off.tobytes()


# ---- strength 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,steps,eta", CASES, ids=CASE_IDS)
def test_reference_chain_shows_the_gap(kind, steps, eta):
    """Without the projection the float64 chain of this seed does NOT downsample to the LR images (so the test below
    proves something), with it it does."""
    _, _, _, _, lr = _inputs(kind, steps)
    free = ref.residual(_chain(kind, steps, eta, False)[0], lr, ROW0)["max_abs"]
    held = ref.residual(_chain(kind, steps, eta, True)[0], lr, ROW0)["max_abs"]
    print(f"float64 chain, max |A img - y| per image: free {np.array2string(free, precision=3)}, projected {np.array2string(held, precision=2)}")
    assert free.min() > 1e-2 and held.max() <= 1e-12


@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16f8"])
@pytest.mark.parametrize("kind,steps,eta", CASES, ids=CASE_IDS)
def test_strength_one_is_consistent_and_follows_the_float64_chain(kind, steps, eta, prec):
    cfg, sd, cond, noise, lr = _inputs(kind, steps)
    want, want_fr = _chain(kind, steps, eta, True)
    e = _engine(cfg, sd, kind, steps, eta, prec)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got, got_fr = _run(e, cond, noise, lr, 1.0)
        free, _ = _run(e, cond, noise)
    res = e.lr_residual_np(got, lr, ROW0)["max_abs"]
    res_free = e.lr_residual_np(free, lr, ROW0)["max_abs"]
    S = noise.shape[0]
    # the same through the step API
    dc, dn, dl, out = e.to_device(cond), e.to_device(noise), e.to_device(lr), e.buffer(B * 3 * R * R)
    slab = B * 3 * R * R * 4
    e.set_lr_consistency(dl.ptr, N_LR, L, L, ROW0, 1.0)
    e.sample_begin(dc.ptr, B, R, R, dn.ptr)
    for t in reversed(range(S)):
        e.sample_step(t, dn.ptr + (S - t) * slab if t > 0 else None)
    e.sample_end(out.ptr)
    stepped = out.download((B, 3, R, R))
    e.close()
    err = float(np.abs(got - want).max())
    err_fr = np.abs(got_fr - want_fr).reshape(want_fr.shape[0], -1).max(1)
    print(f"{kind} S={S} eta={eta} [{prec}]: max |A img - y| {res.max():.2e} (feature off: {res_free.min():.2e}), final vs float64 chain "
          f"{err:.2e}, frames {np.array2string(err_fr, precision=2)}")
    assert got_fr.shape == want_fr.shape
    assert res.max() <= BAR_OP
    assert res_free.min() > 1e-2
    assert err <= BAR_CHAIN and err_fr.max() <= BAR_CHAIN
    assert stepped.tobytes() == got.tobytes()
    np.testing.assert_array_equal(got, got_fr[-1])


# ---- invariances (f32, bitwise) -----------------------------------------------------------------------------------------
TINY = SCHED["fast"]


def _netG(seed, dropout=0.0):
    import torch
    cfg = synth.tiny_unet_config()
    opt = {"phase": "val", "sr": {"model": {
        "which_model_G": "sr3",
        "unet": {"in_channel": 6, "out_channel": 3, "inner_channel": cfg.inner_channel,
                 "channel_multiplier": list(cfg.channel_mults), "attn_res": list(cfg.attn_res),
                 "res_blocks": cfg.res_blocks, "dropout": dropout},
        "beta_schedule": {"train": TINY, "val": TINY},
        "diffusion": {"image_size": cfg.image_size, "channels": 3, "conditional": True}}}}
    netG = pkg().define_G(opt).to("cuda:0")
    netG.load_state_dict({"denoise_fn." + k: torch.from_numpy(v) for k, v in synth.synth_state_dict(cfg, seed).items()},
                         strict=False)
    netG.set_new_noise_schedule(TINY, [0])
    return netG


def test_offsets_and_chunks_do_not_change_a_row():
    import torch
    netG = _netG(SEED)
    netG.set_sampler("ddim", steps=4, eta=0.5)
    x = torch.from_numpy(synth.synth_cond(5, R, L, SEED)).cuda()
    lr = torch.from_numpy(_lr_images(5, L, SEED))
    netG.set_lr_consistency(lr)
    full = netG.sample_batch(x[:3], seed=77)
    part = netG.super_resolution_batch(x[1:3], seed=77, image_offset=1)
    assert torch.equal(part, full[1:3])
    whole = netG.sample_batch(x, seed=77)
    chunked = netG.sample_batch(x, seed=77, max_chunk=2)
    assert torch.equal(chunked, whole)
    sc = pkg("validation").lr_consistency(netG, whole, lr)
    assert sc["max_abs"].max() <= BAR_OP and sc["mse"].shape == (5,)
    # uint8 crops give the same setting as their tensor
    u8 = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (5, L, L, 3)).astype(np.uint8))
    netG.set_lr_consistency(u8)
    a = netG.sample_batch(x, seed=77)
    netG.set_lr_consistency(pkg("diffusion").lr_to_tensor(u8).cuda())
    assert torch.equal(netG.sample_batch(x, seed=77), a)
    assert pkg("validation").lr_consistency(netG, a, u8)["max_abs"].max() <= BAR_OP
    # off again: the plain sampler
    netG.set_lr_consistency(None)
    plain = netG.sample_batch(x, seed=77)
    assert torch.equal(plain, _fresh_plain(x))
    torch.cuda.synchronize()


def _fresh_plain(x):
    netG = _netG(SEED)
    netG.set_sampler("ddim", steps=4, eta=0.5)
    return netG.sample_batch(x, seed=77)


def test_validate_batch_scores_consistency():
    import torch
    val = pkg("validation")
    netG = _netG(SEED)
    netG.set_sampler("dpmpp_2m", steps=4)
    N = 2
    sr = torch.from_numpy(synth.synth_cond(N, R, L, SEED)).cuda()
    lr = torch.from_numpy(_lr_images(N, L, SEED))
    netG.set_lr_consistency(lr)
    r = val.validate_batch(netG, sr, None, samples=2, seed=9, lr=lr)
    assert r["psnr"] is None and r["consistency"].shape == (2, N) and tuple(r["images"].shape) == (2 * N, 3, R, R)
    for k in range(2):      # sample k of image i is row k*N + i
        alone = netG.super_resolution_batch(sr, seed=9, image_offset=k * N)
        assert torch.equal(alone, r["images"][k * N:(k + 1) * N])
    own = val.lr_consistency(netG, r["images"], lr)
    assert own["mse"].reshape(2, N).tobytes() == r["consistency"].tobytes()
    assert own["max_abs"].max() <= BAR_OP and r["mean_consistency"] == float(r["consistency"].mean())
    # with HR the scores are added to the usual ones; the projection is netG's setting, not validate_batch's
    netG.set_lr_consistency(None)
    r2 = val.validate_batch(netG, sr, sr, samples=1, seed=9, lr=lr)
    assert r2["psnr"].shape == (1, N) and r2["consistency"].min() > 1e-4
    torch.cuda.synchronize()


# ---- the rest of the sampler with the feature on --------------------------------------------------------------------------
def test_late_range_overflow_replays_with_the_projection():
    """The injected noise slab of test_gpu_round3.py::test_packed_state_overflow_from_injected_noise_is_caught, scaled
    until x_t leaves the fp16 range in the middle of the loop: the f16x3 call is finished in f32 from the last clean
    checkpoint and meets the all-f32 call, both with the projection on (that test's bar, 1e-4: the segments before the
    overflow are f16x3)."""
    Sr3RangeWarning = pkg("_lib").Sr3RangeWarning
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 12)
    T = 12
    e = _engine(cfg, sd, "ddim", T, 1.0, "f16x3")           # (12 of the 12 levels, eta 1: every step draws noise)
    cond, noise = synth.synth_cond(2, R, L, 4), synth.synth_noise(T, 2, 3, R, R, 4)
    lr = _lr_images(2, L, 4)
    noise[5] *= np.float32(3e6)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        fin, fr = _run(e, cond, noise, lr, 1.0)
    n_fb = e.fallback_calls()
    e.set_precision("f32")
    fin32, fr32 = _run(e, cond, noise, lr, 1.0)
    res = e.lr_residual_np(fin, lr)["max_abs"]
    e.close()
    assert any(issubclass(w.category, Sr3RangeWarning) for w in rec) and n_fb == 1
    d = float(np.abs(fin - fin32).max())
    print(f"late overflow with the projection: |f16x3 + f32 replay - all f32| {d:.2e}, max |A img - y| {res.max():.2e}")
    assert np.isfinite(fin).all() and d <= 1e-4 and res.max() <= BAR_OP


def test_toggling_keeps_the_captured_graphs_apart():
    kind, steps, eta = "dpmpp_2m", 4, 0.0
    cfg, sd, cond, noise, lr = _inputs(kind, steps)
    fresh = _engine(cfg, sd, kind, steps, eta)
    want_off = _run(fresh, cond, noise)[0]
    fresh.close()
    fresh = _engine(cfg, sd, kind, steps, eta)
    want_on = _run(fresh, cond, noise, lr, 1.0)[0]
    fresh.close()
    e = _engine(cfg, sd, kind, steps, eta)
    _run(e, cond, noise)                                    # (graphs of the plain step are captured and replayed)
    on1 = _run(e, cond, noise, lr, 1.0)[0]
    off = _run(e, cond, noise)[0]
    on2 = _run(e, cond, noise, lr, 1.0)[0]
    # what varies between calls is read from device memory: other images, offset and strength on the same graphs
    lr2 = _lr_images(2, L, SEED + 1)
    moved = _run(e, cond, noise, lr2, 1.0, row_offset=1)[0]
    res = e.lr_residual_np(moved, lr2, 1)["max_abs"]
    half = _run(e, cond, noise, lr, 0.5)[0]
    e.close()
    assert on1.tobytes() == want_on.tobytes() and off.tobytes() == want_off.tobytes() and on2.tobytes() == want_on.tobytes()
    assert res.max() <= BAR_OP
    assert np.abs(half - want_on).max() > 1e-3 and np.abs(half - want_off).max() > 1e-3


def test_dropout_sampling_stays_consistent_and_reproducible():
    import dataclasses
    cfg = dataclasses.replace(synth.tiny_unet_config(), dropout=0.2)
    sd = synth.synth_state_dict(cfg, SEED)
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_schedule(_bufs(SCHED["ddpm"]))
    cond, lr = synth.synth_cond(B, R, L, SEED), _lr_images(N_LR, L, SEED)
    dl = e.to_device(lr)
    e.set_lr_consistency(dl.ptr, N_LR, L, L, 0, 1.0)
    plain = e.sample_np(cond, seed=5)
    e.set_dropout(True, seed=1234)
    a = e.sample_np(cond, seed=5)
    b = e.sample_np(cond, seed=5)
    res = e.lr_residual_np(a, lr)["max_abs"]
    e.close()
    assert a.tobytes() == b.tobytes() and np.abs(a - plain).max() > 1e-3
    print(f"dropout sampling with the projection: max |A img - y| {res.max():.2e}")
    assert res.max() <= BAR_OP
