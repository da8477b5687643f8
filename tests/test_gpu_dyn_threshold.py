"""Dynamic thresholding of the sampler's x0 prediction on the GPU: the exact per-image selection and the
in-place op bit for bit against the numpy restatement (dyn_threshold_ref.py), off = the old sampler, max_value = 1 = the
static clamp, the thresholded chains step by step against the restatement driven with the library's own eps, the
dpmpp_2m history, the composition with the low-resolution projection, batch independence and the range fallback.

Bars. Selection and op: bit equality. Chains: 1e-3 max-abs, the BAR of test_gpu_fast_samplers.py for restated few-step
chains. With the projection: BAR_OP 1e-5 (residual) and BAR_CHAIN 1e-4 of test_gpu_lr_consistency.py."""
import functools
import warnings

import numpy as np
import pytest

import dyn_threshold_ref as ref
import fast_sampler_ref as fast
import lr_consistency_ref as lrr
from conftest import pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
schedule = pkg("schedule")
samplers = pkg("samplers")
F32 = np.float32

BAR = 1e-3              # test_gpu_fast_samplers.py
BAR_OP = 1e-5           # test_gpu_lr_consistency.py
BAR_CHAIN = 1e-4        # test_gpu_lr_consistency.py
TINY = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
SEED = 21
B, R, L = 3, 16, 8
RATIO = 0.995
KINDS = [("ddpm", None), ("ddim", 7), ("dpmpp_2m", 7)]
KIND_IDS = ["ddpm_T20", "ddim_S7", "dpmpp_2m_S7"]


def _bufs(sched_opt):
    with np.errstate(divide="ignore", invalid="ignore"):
        return schedule.schedule_buffers(sched_opt)


def _engine(cfg, sd, kind, steps, prec="f32"):
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_precision(prec)
    if kind == "ddpm":
        e.set_schedule(_bufs(TINY))
    else:
        e.set_sampler_schedule(samplers.sampler_tables(_bufs(TINY), kind, steps, 0.0))
    return e


def _steps(kind, steps):
    return steps if steps else TINY["n_timestep"]


def _co(kind, steps):
    return lrr.ddpm_coefficients(TINY) if kind == "ddpm" else fast.coefficients(TINY, kind, steps, 0.0)


@functools.lru_cache(maxsize=None)
def _inputs(kind, steps):
    cfg = synth.tiny_unet_config()
    return cfg, synth.synth_state_dict(cfg, SEED), synth.synth_cond(B, R, L, SEED), synth.synth_noise(_steps(kind, steps), B, 3, R, R, SEED)


def _lr_images():
    return np.random.RandomState(SEED ^ 0x10C0).uniform(-1, 1, (B, 3, L, L)).astype(F32)


@functools.lru_cache(maxsize=None)
def _chain(kind, steps, mode):
    """The restatement's chain of the case, driven with the library's own exact-f32 eps on the restatement's state
    (computed once, shared, never modified). mode: "off" | "on" | "on_clamped_history" | "on_lr"."""
    cfg, sd, cond, noise = _inputs(kind, steps)
    e = _engine(cfg, sd, kind, steps)

    def eps_fn(x, nl):
        return e.unet_forward_np(np.concatenate([cond, x], axis=1), np.full((B,), nl, F32))

    lr = _lr_images()
    out = ref.sample_loop(eps_fn, _co(kind, steps), noise, None if mode == "off" else RATIO,
                          project=(lambda x0: lrr.project(x0, lr).astype(F32)) if mode == "on_lr" else None,
                          history="clamped" if mode == "on_clamped_history" else "thresholded")
    e.close()
    for v in out.values():
        v.setflags(write=False)
    return out


def _step_states(e, cond, noise):
    """The state after every step through the step API: [S,B,3,R,R]."""
    S = noise.shape[0]
    dc, dn, out = e.to_device(cond), e.to_device(noise), e.buffer(B * 3 * R * R)
    slab = B * 3 * R * R * 4
    states = []
    e.sample_begin(dc.ptr, B, R, R, dn.ptr)
    for t in reversed(range(S)):
        e.sample_step(t, dn.ptr + (S - t) * slab if t > 0 else None)
        e.sample_end(out.ptr)
        states.append(out.download((B, 3, R, R)))
    return np.stack(states)


# ---- the selection and the in-place op: bit equality ------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 2), (3, 192), (3, 1728), (2, 4800), (1, 49152), (1, 65537)]
DATA = ["normal", "levels8", "equal", "mix"]
RATIOS = [1e-6, 0.5, 0.9, 0.995, 1.0]       # 1e-6: k = 0 at every n here


def _data(kind, Bn, n):
    rs = np.random.RandomState(n * 7 + Bn + len(kind))
    if kind == "normal":
        return (rs.standard_normal((Bn, n)) * 1.5).astype(F32)
    if kind == "levels8":       # |x| on 8 levels (0.25 .. 2), random signs: ties across every k / k+1 boundary
        return ((rs.randint(1, 9, (Bn, n)) * 0.25) * rs.choice([-1.0, 1.0], (Bn, n))).astype(F32)
    if kind == "equal":
        return np.full((Bn, n), -1.75, F32)
    pool = np.array([0.0, -0.0, 1e-45, -1e-40, 3e-39, 1e-30, -1e-30, 3e38, -3e38], F32)
    return pool[rs.randint(0, pool.size, (Bn, n))]


@pytest.fixture(scope="module")
def op_engine():
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    yield e
    e.close()


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(got, F32).view(np.uint32), np.ascontiguousarray(want, F32).view(np.uint32)
    assert g.shape == w.shape and (g == w).all(), f"{what}: {got.ravel()[:4]} != {want.ravel()[:4]} ({int((g != w).sum())} differ)"


@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("Bn,n", SHAPES, ids=[f"{b}x{n}" for b, n in SHAPES])
def test_selection_is_bit_equal_to_the_restatement(op_engine, Bn, n, kind):
    x = _data(kind, Bn, n)
    for ratio in RATIOS:
        for cap in (None, 1.25):
            want = ref.select(x, ratio, cap)
            for misalign in (False, True):
                got = op_engine.op_abs_quantile(x, ratio, cap, misalign=misalign)
                again = op_engine.op_abs_quantile(x, ratio, cap, misalign=misalign)
                for key in ("lo", "hi", "s"):
                    _same_bits(got[key], want[key], f"{key} ratio={ratio} cap={cap} misalign={misalign}")
                    _same_bits(again[key], got[key], f"second call, {key}")


@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("Bn,n", SHAPES, ids=[f"{b}x{n}" for b, n in SHAPES])
def test_in_place_op_is_bit_equal_to_the_restatement(op_engine, Bn, n, kind):
    x = _data(kind, Bn, n)
    for ratio in RATIOS:
        for cap in (None, 1.25):
            want, want_s = ref.threshold(x, ratio, cap)
            for misalign in (False, True):
                got, s = op_engine.op_dynamic_threshold(x, ratio, cap, misalign=misalign)
                _same_bits(s, want_s, f"s ratio={ratio} cap={cap}")
                _same_bits(got, want, f"x ratio={ratio} cap={cap} misalign={misalign}")
    got, s = op_engine.op_dynamic_threshold(x, RATIO, 1.0)           # s = 1: the static clamp
    assert (s == 1).all()
    _same_bits(got, np.fmin(np.fmax(x, F32(-1)), F32(1)), "max_value = 1")


def test_selection_larger_shape(op_engine):
    x = _data("normal", 1, 3 * 256 * 256)
    for ratio in (0.5, RATIO):
        want, got = ref.select(x, ratio), op_engine.op_abs_quantile(x, ratio)
        for key in ("lo", "hi", "s"):
            _same_bits(got[key], want[key], f"{key} ratio={ratio}")


def test_op_argument_errors(op_engine):
    Sr3Error = pkg("_lib").Sr3Error
    x = _data("normal", 1, 16)
    for ratio, cap in ((0.0, None), (1.5, None), (float("nan"), None), (0.5, 0.5), (0.5, float("nan"))):
        with pytest.raises(Sr3Error):
            op_engine.op_abs_quantile(x, ratio, cap)
        with pytest.raises(Sr3Error):
            op_engine.op_dynamic_threshold(x, ratio, cap)
    for ratio, cap in ((1.5, 2.0), (float("nan"), 2.0), (0.5, 0.5), (0.5, float("nan"))):
        with pytest.raises(Sr3Error):
            op_engine.set_dynamic_threshold(ratio, cap)
    op_engine.set_dynamic_threshold(-1.0, 0.0)      # ratio <= 0 is "off" whatever max_value says
    op_engine.set_dynamic_threshold(None)


# ---- the sampler --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,steps", KINDS, ids=KIND_IDS)
def test_off_is_off(kind, steps):
    cfg, sd, cond, noise = _inputs(kind, steps)
    fresh = _engine(cfg, sd, kind, steps)
    want, want_fr = fresh.sample_np(cond, noise=noise, frames=True)
    fresh.close()
    e = _engine(cfg, sd, kind, steps)
    e.set_dynamic_threshold(None)
    got, got_fr = e.sample_np(cond, noise=noise, frames=True)
    assert got.tobytes() == want.tobytes() and got_fr.tobytes() == want_fr.tobytes() and e.dynamic_threshold_launches() == 0
    e.set_dynamic_threshold(RATIO)
    on = e.sample_np(cond, noise=noise)
    n_on = e.dynamic_threshold_launches()
    e.set_dynamic_threshold(None)
    got, got_fr = e.sample_np(cond, noise=noise, frames=True)
    stepped = _step_states(e, cond, noise)[-1]
    n_off = e.dynamic_threshold_launches()
    e.close()
    assert n_on == _steps(kind, steps) and n_off == n_on
    assert got.tobytes() == want.tobytes() and got_fr.tobytes() == want_fr.tobytes() and stepped.tobytes() == want.tobytes()
    assert np.abs(on - want).max() > 0.1


@pytest.mark.parametrize("kind,steps", KINDS, ids=KIND_IDS)
def test_max_value_one_is_the_static_clamp(kind, steps):
    cfg, sd, cond, noise = _inputs(kind, steps)
    S = _steps(kind, steps)
    e = _engine(cfg, sd, kind, steps)
    want, want_fr = e.sample_np(cond, noise=noise, frames=True)
    e.set_dynamic_threshold(RATIO, 1.0)
    n0 = e.dynamic_threshold_launches()
    got, got_fr = e.sample_np(cond, noise=noise, frames=True)
    n1 = e.dynamic_threshold_launches()
    stepped = _step_states(e, cond, noise)[-1]
    n2 = e.dynamic_threshold_launches()
    e.close()
    assert (n0, n1, n2) == (0, S, 2 * S)
    assert got.tobytes() == want.tobytes() and got_fr.tobytes() == want_fr.tobytes() and stepped.tobytes() == want.tobytes()


def _assert_threshold_is_live(kind, steps):
    """The condition of the chain tests: the restatement's threshold is above 1 in at least 90 % of the (step, image)
    pairs, and its final images are more than 0.1 away from the feature-off chain somewhere (CPU oracle, ddpm: 59 of 60
    pairs and 0.96)."""
    on, off = _chain(kind, steps, "on"), _chain(kind, steps, "off")
    live = int((on["s"] > 1).sum())
    moved = float(np.abs(on["final"] - off["final"]).max())
    print(f"{kind}: s > 1 in {live} of {on['s'].size} (step, image) pairs, s of the first / last step {on['s'][0]} / {on['s'][-1]}; "
          f"final on vs off {moved:.2f}")
    assert live >= 0.9 * on["s"].size and moved > 0.1


@pytest.mark.parametrize("kind,steps", KINDS, ids=KIND_IDS)
def test_sampler_follows_the_restatement_step_by_step(kind, steps):
    cfg, sd, cond, noise = _inputs(kind, steps)
    want = _chain(kind, steps, "on")
    _assert_threshold_is_live(kind, steps)
    e = _engine(cfg, sd, kind, steps)
    e.set_dynamic_threshold(RATIO)
    states = _step_states(e, cond, noise)
    whole, frames = e.sample_np(cond, noise=noise, frames=True)
    n = e.dynamic_threshold_launches()
    e.close()
    err = np.abs(states - want["states"]).reshape(states.shape[0], -1).max(1)
    print(f"{kind} [f32]: per-step max abs err vs the restatement {np.array2string(err, precision=2)}")
    assert err.max() <= BAR
    assert n == 2 * states.shape[0]
    assert whole.tobytes() == states[-1].tobytes() and frames[-1].tobytes() == whole.tobytes()


@pytest.mark.parametrize("prec", ["f16x3", "f16f8"])
@pytest.mark.parametrize("kind,steps", KINDS, ids=KIND_IDS)
def test_split_f16_sampler_follows_the_restatement(kind, steps, prec):
    cfg, sd, cond, noise = _inputs(kind, steps)
    want = _chain(kind, steps, "on")
    _assert_threshold_is_live(kind, steps)
    e = _engine(cfg, sd, kind, steps, prec)
    e.set_dynamic_threshold(RATIO)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = e.sample_np(cond, noise=noise)
    n = e.dynamic_threshold_launches()
    e.close()
    err = float(np.abs(got - want["final"]).max())
    print(f"{kind} [{prec}]: final max abs err vs the restatement {err:.2e}")
    assert err <= BAR and n == _steps(kind, steps)


def test_dpmpp_2m_history_holds_the_thresholded_x0():
    """The second step of dpmpp_2m reads the first step's x0 from the history: the state after it meets the restatement,
    whose history is the thresholded x0, and not the variant that keeps the statically clamped one."""
    kind, steps = "dpmpp_2m", 7
    cfg, sd, cond, noise = _inputs(kind, steps)
    want, other = _chain(kind, steps, "on"), _chain(kind, steps, "on_clamped_history")
    gap = float(np.abs(want["states"][1] - other["states"][1]).max())
    assert want["states"][0].tobytes() == other["states"][0].tobytes() and gap > 10 * BAR
    e = _engine(cfg, sd, kind, steps)
    e.set_dynamic_threshold(RATIO)
    states = _step_states(e, cond, noise)
    e.close()
    err = float(np.abs(states[1] - want["states"][1]).max())
    print(f"dpmpp_2m second step: vs thresholded history {err:.2e}, the clamped-history variant is {gap:.2e} away")
    assert err <= BAR


@pytest.mark.parametrize("kind,steps", [KINDS[0], KINDS[2]], ids=[KIND_IDS[0], KIND_IDS[2]])
def test_with_the_lr_projection_as_well(kind, steps):
    cfg, sd, cond, noise = _inputs(kind, steps)
    lr = _lr_images()
    want, plain = _chain(kind, steps, "on_lr"), _chain(kind, steps, "on")
    e = _engine(cfg, sd, kind, steps)
    dl = e.to_device(lr)
    e.set_lr_consistency(dl.ptr, B, L, L, 0, 1.0)
    e.set_dynamic_threshold(RATIO)
    got = e.sample_np(cond, noise=noise)
    e.synchronize()
    n = e.dynamic_threshold_launches()
    e.set_lr_consistency(None)
    free = e.sample_np(cond, noise=noise)
    res, res_free = e.lr_residual_np(got, lr, 0)["max_abs"], e.lr_residual_np(free, lr, 0)["max_abs"]
    e.close()
    err = float(np.abs(got - want["final"]).max())
    print(f"{kind} threshold + projection: max |A img - y| {res.max():.2e} (projection off: {res_free.min():.2e}), final vs the "
          f"composed restatement {err:.2e}")
    assert n == _steps(kind, steps)
    assert res.max() <= BAR_OP and res_free.min() > 1e-2
    assert err <= BAR_CHAIN
    assert np.abs(free - plain["final"]).max() <= BAR


def _netG():
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
    netG.load_state_dict({"denoise_fn." + k: torch.from_numpy(v) for k, v in synth.synth_state_dict(cfg, SEED).items()},
                         strict=False)
    netG.set_new_noise_schedule(TINY, [0])
    return netG


def test_rows_do_not_depend_on_the_batch():
    """f32, bitwise: a row of a B = 3 call is the B = 1 call at its image offset, also from a warm start and in chunks;
    the facade's setting reaches the engine and p_sample stays the reference's step."""
    import torch
    netG = _netG()
    netG.set_sampler("dpmpp_2m", steps=7)
    x = torch.from_numpy(synth.synth_cond(B, R, L, SEED)).cuda()
    plain = netG.sample_batch(x, seed=77)
    netG.set_dynamic_threshold(RATIO)
    for start in (None, 0.6):
        netG.set_start(start)
        full = netG.sample_batch(x, seed=77)
        for i in range(B):
            row = netG.super_resolution_batch(x[i:i + 1], seed=77, image_offset=i)
            assert torch.equal(row[0], full[i]), (start, i)
        assert torch.equal(netG.sample_batch(x, seed=77, max_chunk=2), full), start
    netG.set_start(None)
    eng = netG._engine()
    n = eng.dynamic_threshold_launches()
    assert n > 0 and float((netG.sample_batch(x, seed=77) - plain).abs().max()) > 0.1
    # the reference's single step is never thresholded
    xt = torch.from_numpy(synth.synth_noise(1, B, 3, R, R, 3)[0]).cuda() * 3.0
    netG.set_sampler("ddpm")
    n = netG._engine().dynamic_threshold_launches()
    one = netG.p_sample(xt, 19, condition_x=x, noise=torch.zeros_like(xt))
    assert netG._engine().dynamic_threshold_launches() == n
    netG.set_dynamic_threshold(None)
    assert torch.equal(netG.p_sample(xt, 19, condition_x=x, noise=torch.zeros_like(xt)), one)
    netG.set_sampler("dpmpp_2m", steps=7)
    assert torch.equal(netG.sample_batch(x, seed=77), plain)
    torch.cuda.synchronize()


def test_range_fallback_keeps_the_threshold():
    """The scaled-downs.0 net of test_gpu_round3.py (first conv output beyond fp16 on every forward): the f16x3 call is
    finished in f32 by the range policy with the threshold still in every step, and meets the all-f32 call."""
    Sr3RangeWarning = pkg("_lib").Sr3RangeWarning
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 77)
    sd["downs.0.weight"] = sd["downs.0.weight"] * F32(3e5)
    kind, S = "dpmpp_2m", 7
    cond, noise = synth.synth_cond(2, R, L, 1), synth.synth_noise(S, 2, 3, R, R, 1)
    e = _engine(cfg, sd, kind, S, "f16x3")
    e.set_dynamic_threshold(RATIO)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = e.sample_np(cond, noise=noise)
    n_fb, n = e.fallback_calls(), e.dynamic_threshold_launches()
    e.set_precision("f32")
    want = e.sample_np(cond, noise=noise)
    e.set_dynamic_threshold(None)
    off = e.sample_np(cond, noise=noise)
    e.close()
    err, moved = float(np.abs(got - want).max()), float(np.abs(want - off).max())
    print(f"range fallback with the threshold: |f16x3 -> f32 replay - all f32| {err:.2e}; threshold on vs off {moved:.2e}")
    assert any(issubclass(w.category, Sr3RangeWarning) for w in rec) and n_fb == 1 and n >= S
    assert np.isfinite(got).all() and err <= BAR and moved > BAR
