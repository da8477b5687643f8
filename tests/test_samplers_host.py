"""Few-step samplers on the host: the tables of samplers.sampler_tables against the reference's DDPM
buffers and against independent float64 restatements, and the numpy restatement of the loops (fast_sampler_ref.py)
against the reference-made golden run. CPU only."""
import math

import numpy as np
import pytest

import fast_sampler_ref as ref
import sr3_oracle as oracle
from conftest import cfg_from_meta, load_golden, pkg

samplers = pkg("samplers")
schedule = pkg("schedule")
synth = pkg("synth")

SCHEDULES = [{"schedule": "linear", "linear_start": 1e-4, "linear_end": 2e-2},
             {"schedule": "linear", "linear_start": 1e-6, "linear_end": 1e-2},
             {"schedule": "cosine", "linear_start": 1e-4, "linear_end": 2e-2},
             {"schedule": "warmup10", "linear_start": 1e-4, "linear_end": 2e-2}]


def _bufs(opt, T):
    with np.errstate(divide="ignore", invalid="ignore"):
        return schedule.schedule_buffers(dict(opt, n_timestep=T))


def _ulp(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


@pytest.mark.parametrize("T", [6, 100, 1000])
@pytest.mark.parametrize("opt", SCHEDULES, ids=lambda o: f"{o['schedule']}-{o['linear_start']}")
def test_ddim_eta1_full_is_the_ddpm_posterior(opt, T):
    b = _bufs(opt, T)
    tb = samplers.sampler_tables(b, "ddim", None, 1.0)
    assert tb["S"] == T and not tb["uses_history"]
    np.testing.assert_array_equal(tb["noise_level"], b["noise_level"])
    np.testing.assert_array_equal(tb["a"], b["sqrt_recip_alphas_cumprod"])
    np.testing.assert_array_equal(tb["b"], b["sqrt_recipm1_alphas_cumprod"])
    assert _ulp(tb["c1"], b["posterior_mean_coef1"]) <= 4
    assert _ulp(tb["c2"], b["posterior_mean_coef2"]) <= 4
    assert _ulp(tb["sigma"].astype(np.float64) ** 2, b["posterior_variance"]) <= 4
    assert not tb["c3"].any()
    for k in ("noise_level", "a", "b", "c1", "c2", "c3", "sigma"):
        assert tb[k].dtype == np.float32


def test_levels_and_validation():
    for T in (1, 6, 100, 1000):
        for S in sorted({1, 2, 3, 7, T // 3 or 1, T}):
            if S > T:
                continue
            K = samplers.sampler_levels(T, S)
            assert K[0] == 0 and K[-1] == T and len(K) == S + 1 and np.all(np.diff(K) > 0)
        np.testing.assert_array_equal(samplers.sampler_levels(T, T), np.arange(T + 1))
    b = _bufs(SCHEDULES[0], 20)
    for kind, steps, eta in [("ddim", 0, 0.0), ("ddim", 21, 0.0), ("dpmpp_2m", 0, 0.0), ("dpmpp_2m", 21, 0.0),
                             ("plms", 10, 0.0), ("ddim", 10, -0.5), ("dpmpp_2m", 10, 0.5), ("ddpm", 10, 0.0),
                             ("ddim", 2.5, 0.0), ("ddim", 10, float("nan"))]:
        with pytest.raises(ValueError):
            samplers.sampler_tables(b, kind, steps, eta)
    assert samplers.sampler_tables(b, "ddim", 20, 0.5)["S"] == 20
    assert samplers.sampler_tables(b, "ddpm")["S"] == 20


@pytest.mark.parametrize("S", [1, 2, 3, 5, 10, 50])
@pytest.mark.parametrize("opt", SCHEDULES, ids=lambda o: f"{o['schedule']}-{o['linear_start']}")
def test_dpmpp_2m_tables(opt, S):
    T = 1000
    b = _bufs(opt, T)
    tb = samplers.sampler_tables(b, "dpmpp_2m", S)
    assert tb["S"] == S and tb["uses_history"]
    for k in ("c1", "c2", "c3", "sigma", "noise_level", "a", "b"):
        assert np.all(np.isfinite(tb[k])), k
    assert not tb["sigma"].any()
    assert tb["c3"][S - 1] == 0 and tb["c3"][0] == 0          # first and last steps are first order
    assert tb["c1"][0] == 1 and tb["c2"][0] == 0               # the last step returns x0
    # independent float64 restatement: x' = (sigma_t / sigma_s) x + alpha_t (1 - e^-h) D,
    # D = (1 + 1/(2r)) x0 - 1/(2r) x0_prev, r = h_prev / h
    abar = np.concatenate([[1.0], np.cumprod(1.0 - oracle.make_beta_schedule(
        opt["schedule"], T, opt["linear_start"], opt["linear_end"]))])
    K = [j * T // S for j in range(S + 1)]
    lam = lambda k: math.log(math.sqrt(abar[k]) / math.sqrt(1.0 - abar[k]))  # noqa: E731
    for i in range(1, S):
        s, t = K[i + 1], K[i]
        h = lam(t) - lam(s)
        phi = 1.0 - math.exp(-h)
        want_c2 = math.sqrt(1.0 - abar[t]) / math.sqrt(1.0 - abar[s])
        if i == S - 1:
            want_c1, want_c3 = math.sqrt(abar[t]) * phi, 0.0
        else:
            r = (lam(s) - lam(K[i + 2])) / h
            want_c1 = math.sqrt(abar[t]) * phi * (1.0 + 1.0 / (2.0 * r))
            want_c3 = -math.sqrt(abar[t]) * phi / (2.0 * r)
        for k, w in (("c1", want_c1), ("c2", want_c2), ("c3", want_c3)):
            assert abs(float(tb[k][i]) - w) <= 1e-6 * max(1.0, abs(w)), (k, i, float(tb[k][i]), w)
    # the test's restatement and fast_sampler_ref agree as well (they feed the GPU tests)
    co = ref.coefficients(dict(opt, n_timestep=T), "dpmpp_2m", S)
    for i in range(S):
        for k in ("c1", "c2", "c3"):
            assert abs(float(tb[k][i]) - co[i][k]) <= 1e-6 * max(1.0, abs(co[i][k]))
        assert tb["a"][i] == co[i]["a"] and tb["b"][i] == co[i]["b"] and tb["noise_level"][i + 1] == co[i]["nl"]


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_ddim_tables_match_restatement(eta):
    opt = dict(SCHEDULES[1], n_timestep=1000)
    tb = samplers.sampler_tables(_bufs(SCHEDULES[1], 1000), "ddim", 50, eta)
    co = ref.coefficients(opt, "ddim", 50, eta)
    for i in range(50):
        for k in ("c1", "c2", "sigma"):
            assert abs(float(tb[k][i]) - co[i][k]) <= 1e-6 * max(1.0, abs(co[i][k])), (k, i)
    assert tb["sigma"][0] == 0 and tb["c1"][0] == 1 and tb["c2"][0] == 0


def test_restatement_reproduces_reference_golden():
    """DDIM with eta = 1 over every step is the reference's DDPM loop: the restatement, with the fixture's injected
    noise, meets tests/golden/sampler_tiny.npz at the bar the DDPM restatement is held to (test_oracle_golden.py)."""
    g = load_golden("sampler_tiny.npz")
    m = g["meta"]
    cfg = cfg_from_meta(m)
    sd = synth.synth_state_dict(cfg, m["seed"])
    B, r, T = m["B"], m["r"], m["schedule"]["n_timestep"]
    noise = synth.synth_noise(T, B, 3, r, r, m["seed"])
    final, frames = ref.sample_loop(sd, cfg, m["schedule"], g["cond"], noise, "ddim", T, 1.0)
    ret = np.concatenate([g["cond"], frames.reshape(-1, *frames.shape[2:])], axis=0)
    assert ret.shape == g["ret_img"].shape
    np.testing.assert_allclose(ret, g["ret_img"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(final[-1], g["last"], atol=1e-4, rtol=0)


def test_restatement_samplers_are_deterministic_at_sigma_zero():
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 5)
    opt = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
    cond = synth.synth_cond(1, 16, 8, 5)
    n1 = synth.synth_noise(5, 1, 3, 16, 16, 5)
    n2 = n1.copy()
    n2[1:] = synth.synth_noise(5, 1, 3, 16, 16, 6)[1:]
    for kind in ("ddim", "dpmpp_2m"):
        a, _ = ref.sample_loop(sd, cfg, opt, cond, n1, kind, 5)
        b, _ = ref.sample_loop(sd, cfg, opt, cond, n2, kind, 5)
        np.testing.assert_array_equal(a, b)
        assert np.all(np.abs(a) <= 1.0 + 1e-6) and np.isfinite(a).all()


def test_facade_set_sampler_on_cpu():
    """set_sampler validates, persists over set_new_noise_schedule, adds nothing to state_dict(), and the facade still
    refuses to compute without a GPU."""
    import torch
    opt = synth.yml_opt(8, 16, 100)
    opt["sr"]["model"]["unet"].update(inner_channel=32, channel_multiplier=[1, 2], res_blocks=1, attn_res=[8])
    opt["sr"]["model"]["diffusion"]["image_size"] = 16
    netG = pkg().define_G(opt)
    with pytest.raises(ValueError):
        netG.set_sampler("plms")
    with pytest.raises(ValueError):
        netG.set_sampler("ddim", steps=0)
    netG.set_new_noise_schedule(opt["sr"]["model"]["beta_schedule"]["val"], ["cpu"])
    keys = list(netG.state_dict())
    assert netG.num_sampling_steps == netG.num_timesteps == 100
    with pytest.raises(ValueError):
        netG.set_sampler("ddim", steps=101)
    with pytest.raises(ValueError):
        netG.set_sampler("ddim", steps=10, eta=-1.0)
    with pytest.raises(ValueError):
        netG.set_sampler("dpmpp_2m", steps=10, eta=0.5)
    netG.set_sampler("dpmpp_2m", steps=10)
    assert netG.num_sampling_steps == 10 and netG.num_timesteps == 100
    assert list(netG.state_dict()) == keys
    sched = dict(opt["sr"]["model"]["beta_schedule"]["val"], n_timestep=40)
    netG.set_new_noise_schedule(sched, ["cpu"])
    assert netG.num_sampling_steps == 10 and netG.num_timesteps == 40
    assert list(netG.state_dict()) == keys
    with pytest.raises(pkg("_lib").Sr3Error):
        netG.super_resolution(torch.zeros(1, 3, 16, 16))
    netG.set_sampler("ddpm")
    assert netG.num_sampling_steps == 40
