"""The sampler's warm start on the host: the reference-made fixture warm_start_tiny.npz against the CPU
oracle's p_sample looped from the reference's q_sample state, the frame bookkeeping, and the facade's set_start setting.
CPU only."""
import numpy as np
import pytest

import sr3_oracle as oracle
import warm_start_ref as ws
from conftest import pkg

schedule = pkg("schedule")
synth = pkg("synth")


def _facade(conditional=True, T=20):
    opt = synth.yml_opt(8, 16, T)
    opt["sr"]["model"]["unet"].update(inner_channel=32, channel_multiplier=[1, 2], res_blocks=1, attn_res=[8])
    if not conditional:
        opt["sr"]["model"]["unet"]["in_channel"] = 3
    opt["sr"]["model"]["diffusion"].update(image_size=16, conditional=conditional)
    netG = pkg().define_G(opt)
    netG.set_new_noise_schedule(opt["sr"]["model"]["beta_schedule"]["val"], ["cpu"])
    return netG


@pytest.mark.parametrize("tag", ["cond", "img"])
@pytest.mark.parametrize("s0", [1, 9, 20])
def test_fixture_matches_the_oracle(s0, tag):
    """The reference's q_sample state is the plain fp32 expression bit for bit (at the stored elements), and the oracle's
    p_sample, looped from it over reversed(range(s0)), gives the reference's frames at test_oracle_golden's bar for
    sampler_tiny (1e-4)."""
    f = ws.fixture()
    m = f["meta"]
    T = m["schedule"]["n_timestep"]
    sch = oracle.noise_schedule(m["schedule"])
    state_sub, frames_sub = f["cases"][(s0, tag)]
    init = f["cond"] if tag == "cond" else f["img"]
    state = ws.q_sample(init, sch["sqrt_alphas_cumprod_prev"][s0], f["noise"][0])
    np.testing.assert_array_equal(state.reshape(-1)[::m["state_stride"]], state_sub)
    # the coefficient is the one the package forms for the loss (diffusion.noise_coefficient)
    a = np.float32(sch["sqrt_alphas_cumprod_prev"][s0])
    assert pkg("diffusion").noise_coefficient([a])[0] == np.sqrt(np.float32(1) - a * a)
    frames = ws.ddpm_tail(f["sd"], f["cfg"], sch, f["cond"], state, f["noise"][:s0], s0, T)
    st = m["frame_stride"]
    assert frames.shape[0] == len(schedule.frame_steps(T, s0)) == frames_sub.shape[0]
    np.testing.assert_allclose(frames[..., ::st, ::st], frames_sub, atol=1e-4, rtol=0)


def test_frame_steps_with_a_start():
    assert schedule.frame_steps(20, 9) == [6, 3, 0]
    assert schedule.frame_steps(20, 1) == [0]
    assert schedule.frame_steps(20, 20) == schedule.frame_steps(20) == schedule.frame_steps(20, None)
    assert schedule.frame_steps(20, 10) == [9, 6, 3, 0]                # (step 9 itself runs when s0 = 10)
    for T in (1, 7, 20, 100, 1000):
        si = 1 | (T // 10)
        for s0 in sorted({1, min(2, T), T // 2 or 1, T}):
            steps = schedule.frame_steps(T, s0)
            assert steps == [i for i in schedule.frame_steps(T) if i < s0]
            assert steps[-1] == 0 and all(i % si == 0 for i in steps)
    for bad in (0, 21, -1):
        with pytest.raises(ValueError):
            schedule.frame_steps(20, bad)


def test_set_start_argument_errors():
    netG = _facade()
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            netG.set_start(bad)
    with pytest.raises(ValueError, match="step"):
        netG.set_start(step=21)
    with pytest.raises(ValueError, match="step"):
        netG.set_start(step=0)
    with pytest.raises(ValueError, match="not both"):
        netG.set_start(0.5, step=4)
    with pytest.raises(ValueError, match="init"):
        netG.set_start(0.5, init="noise")
    assert netG._start is None and netG.num_steps_run == netG.num_sampling_steps == 20
    with pytest.raises(ValueError, match="conditional"):
        _facade(conditional=False).set_start(0.5)
    # a valid setting, then off again
    netG.set_start(1.0)
    assert netG.num_steps_run == 20
    netG.set_start(step=20)
    assert netG.num_steps_run == 20
    netG.set_start(None)
    assert netG._start is None


def test_start_follows_the_sampler_and_the_schedule():
    netG = _facade()
    keys = list(netG.state_dict())
    netG.set_start(strength=0.45)
    assert netG.num_sampling_steps == 20 and netG.num_steps_run == 9       # round(0.45 * 20)
    netG.set_sampler("ddim", steps=8)
    assert netG.num_sampling_steps == 8 and netG.num_steps_run == 4        # round(3.6)
    netG.set_sampler("dpmpp_2m", steps=5)
    assert netG.num_steps_run == 2
    netG.set_sampler("ddpm")
    assert netG.num_steps_run == 9
    netG.set_new_noise_schedule({"schedule": "linear", "n_timestep": 100, "linear_start": 1e-6, "linear_end": 1e-2}, ["cpu"])
    assert netG.num_sampling_steps == 100 and netG.num_steps_run == 45
    netG.set_start(strength=0.01)
    netG.set_sampler("ddim", steps=4)
    assert netG.num_steps_run == 1                                          # max(1, round(0.04))
    assert list(netG.state_dict()) == keys                                  # nothing added to state_dict()
    # an absolute step is kept as given and checked against the S of the moment
    netG.set_sampler("ddpm")
    netG.set_start(step=30)
    assert netG.num_steps_run == 30
    netG.set_sampler("ddim", steps=10)
    with pytest.raises(ValueError, match="step"):
        netG.num_steps_run
    netG.set_start(None)
    assert netG.num_steps_run == 10
