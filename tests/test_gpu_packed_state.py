"""The packed split-f16 copy of the sampler state (x0p, read by conv_in_kernel) against the fp32 state it shadows, after
every kernel that writes it: pack_state_kernel (sample_begin, unet_forward, warm start from a given image),
ddpm_update_kernel (sample_step), update_from_x0_kernel (steps with the low-resolution consistency on) and
q_sample_state_kernel (denoise_loss, noised warm start). Each has its own hi / lo code; the copy is kept current in exact f32
as well, because the arithmetic may change between steps.

After every call, through sr3_read_packed_state: packed == pack16(state) bit for bit (edge_conv_ref.pack16), the one-pixel
border is zero and so are the channels from in_channel on. Tiny config, 16x16, B = 2, 4 steps."""
import numpy as np
import pytest

import edge_conv_ref as ref
from conftest import pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
schedule = pkg("schedule")
samplers = pkg("samplers")

B, R, L, S, SEED = 2, 16, 8, 4, 17
SCHED = {"schedule": "linear", "n_timestep": S, "linear_start": 1e-4, "linear_end": 2e-2}
SCHED_FAST = dict(SCHED, n_timestep=12)


def _bufs(opt):
    with np.errstate(divide="ignore", invalid="ignore"):
        return schedule.schedule_buffers(opt)


@pytest.fixture(scope="module", params=["f32", "f16x3"])
def eng(request):
    cfg = synth.tiny_unet_config()
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(synth.synth_state_dict(cfg, SEED))
    e.set_precision(request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    return {"cond": synth.synth_cond(B, R, L, SEED), "noise": synth.synth_noise(S, B, 3, R, R, SEED),
            "hr": synth.synth_cond(B, R, L, SEED + 1),
            "lr": np.random.RandomState(SEED).uniform(-1, 1, (B, 3, L, L)).astype(np.float32)}


def _check(e, what, fresh=None):
    """packed == pack16(state), zero border, zero pad channels; fresh: the state differs from that earlier one (the call
    under test wrote it). Returns the state."""
    e.synchronize()
    got = e.read_packed_state()
    assert got is not None, what
    state, packed = got
    cin = e.cfg.in_channel
    assert state.shape == (B, R + 2, R + 2, 8) and packed.shape == (B, R + 2, R + 2, 2, 8), what
    assert np.isfinite(state).all() and np.abs(state[:, 1:-1, 1:-1, :cin]).min() > 0, what      # a written, live state
    hi, lo = ref.pack16(state)
    bad = (packed[..., 0, :] != hi.view(np.uint16)) | (packed[..., 1, :] != lo.view(np.uint16))
    assert not bad.any(), f"{what}: {int(bad.sum())} packed values differ from pack16(state), first at {tuple(np.argwhere(bad)[0])}"
    for name, a in (("state", state), ("packed", packed)):
        assert not a[:, 0].any() and not a[:, -1].any() and not a[:, :, 0].any() and not a[:, :, -1].any(), f"{what}: {name} border"
    assert not state[..., cin:].any() and not packed[..., cin:].any(), f"{what}: channels >= in_channel"
    if fresh is not None:
        assert not np.array_equal(state, fresh), f"{what}: the call did not write the state"
    return state


def test_ddpm_steps_injected_noise_and_philox(eng, data):
    e = eng
    e.set_lr_consistency(None)
    e.set_schedule(_bufs(SCHED))
    dc, dn = e.to_device(data["cond"]), e.to_device(data["noise"])
    slab = B * 3 * R * R * 4
    for philox in (False, True):
        e.sample_begin(dc.ptr, B, R, R, None if philox else dn.ptr, seed=SEED)
        prev = _check(e, f"sample_begin philox={philox}")
        if not philox:                         # the state is cond | the injected initial image
            assert np.array_equal(prev[:, 1:-1, 1:-1, :6].transpose(0, 3, 1, 2), np.concatenate([data["cond"], data["noise"][0]], 1))
        for t in range(S - 1, -1, -1):
            e.sample_step(t, None if philox or t == 0 else dn.ptr + (S - t) * slab)
            prev = _check(e, f"sample_step t={t} philox={philox}", fresh=prev)
        e.range_check()


def test_step_with_lr_consistency(eng, data):
    e = eng
    e.set_schedule(_bufs(SCHED))
    dc, dn, dl = e.to_device(data["cond"]), e.to_device(data["noise"]), e.to_device(data["lr"])
    e.set_lr_consistency(dl.ptr, B, L, L, 0, 1.0)
    try:
        e.sample_begin(dc.ptr, B, R, R, dn.ptr)
        prev = _check(e, "sample_begin (lr consistency)")
        for t in (S - 1, S - 2):
            e.sample_step(t, None)
            prev = _check(e, f"sample_step t={t} (lr consistency)", fresh=prev)
        e.range_check()
    finally:
        e.set_lr_consistency(None)


def test_step_of_dpmpp_2m(eng, data):
    e = eng
    e.set_lr_consistency(None)
    e.set_sampler_schedule(samplers.sampler_tables(_bufs(SCHED_FAST), "dpmpp_2m", S))
    dc, dn = e.to_device(data["cond"]), e.to_device(data["noise"])
    e.sample_begin(dc.ptr, B, R, R, dn.ptr)
    prev = _check(e, "sample_begin (dpmpp_2m)")
    for t in (S - 1, S - 2, S - 3):            # first-order step, then two with the x0 history
        e.sample_step(t, None)
        prev = _check(e, f"dpmpp_2m step t={t}", fresh=prev)
    e.range_check()


@pytest.mark.parametrize("noised", [True, False])
def test_sample_begin_from(eng, data, noised):
    e = eng
    e.set_lr_consistency(None)
    e.set_schedule(_bufs(SCHED))
    dc, di, dz = e.to_device(data["cond"]), e.to_device(data["hr"]), e.to_device(data["noise"][0])
    e.sample_begin_from(dc.ptr, B, R, R, di.ptr, 2, noised, dz.ptr if noised else None, SEED)
    prev = _check(e, f"sample_begin_from noised={noised}")
    if not noised:
        assert np.array_equal(prev[:, 1:-1, 1:-1, 3:6].transpose(0, 3, 1, 2), data["hr"])
    e.sample_step(1, None)
    _check(e, f"step after sample_begin_from noised={noised}", fresh=prev)
    e.range_check()


def test_denoise_loss_and_unet_forward(eng, data):
    e = eng
    e.set_lr_consistency(None)
    e.set_schedule(_bufs(SCHED))
    lv = np.array([0.9, 0.3], dtype=np.float32)
    sv = np.sqrt(np.float32(1) - lv * lv)
    dh, dc, dl, ds = e.to_device(data["hr"]), e.to_device(data["cond"]), e.to_device(lv), e.to_device(sv)
    per = e.buffer(2 * B)
    for noise in (None, e.to_device(data["noise"][0])):
        e.denoise_loss(dh.ptr, dc.ptr, B, 0, dl.ptr, ds.ptr, B, R, R, per.ptr, "l1", noise.ptr if noise else None, seed=SEED)
        prev = _check(e, f"denoise_loss philox={noise is None}")
    x, nl = synth.synth_unet_input(e.cfg, B, R, R, SEED)
    out = e.unet_forward_np(x, nl)
    state = _check(e, "unet_forward", fresh=prev)
    assert np.isfinite(out).all() and np.array_equal(state[:, 1:-1, 1:-1, :6].transpose(0, 3, 1, 2), x)


def test_no_packed_state_at_24x40(eng):
    """W = 40 is no multiple of the 16-pixel M-tile: conv_in_supported refuses, the forward runs downs.0 on the generic conv"""
    e = eng
    x, nl = synth.synth_unet_input(e.cfg, B, 24, 40, SEED)
    assert np.isfinite(e.unet_forward_np(x, nl)).all()
    assert e.read_packed_state() is None
    x, nl = synth.synth_unet_input(e.cfg, B, R, R, SEED)          # and back
    e.unet_forward_np(x, nl)
    _check(e, "unet_forward after 24x40")
