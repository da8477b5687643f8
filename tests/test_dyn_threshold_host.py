"""Dynamic thresholding on the host: the numpy restatement (dyn_threshold_ref.py) against numpy's own
float64 quantile, its edge cases, and the facade's set_dynamic_threshold argument checks. CPU only."""
import numpy as np
import pytest

import dyn_threshold_ref as ref
from conftest import pkg

synth = pkg("synth")
F32 = np.float32


def _normal(B, n, seed, scale=1.5):
    return (np.random.RandomState(seed).standard_normal((B, n)) * scale).astype(F32)


@pytest.mark.parametrize("ratio", [1e-4, 0.5, 0.9, 0.995, 1.0])
@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_restatement_matches_numpy_quantile(kind, ratio):
    x = _normal(3, 1728, 5)
    if kind == "ties":
        x = (np.round(x * 2) / 2).astype(F32)       # a handful of levels: heavy ties
    got = ref.select(x, ratio)
    want = np.quantile(np.abs(x.astype(np.float64)), float(F32(ratio)), axis=1)
    rel = np.abs(got["s_raw"].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-30)
    print(f"{kind} ratio={ratio}: s_raw {got['s_raw']}, float64 quantile {want}, relative {rel.max():.1e}")
    assert rel.max() <= 1e-6
    assert (got["lo"] <= got["hi"]).all() and (got["s"] >= 1).all()


def test_single_value():
    for v in (0.25, -3.0):
        x = np.array([[v]], F32)
        r = ref.select(x, 0.995)
        assert ref.plan(0.995, 1) == (0, 0, F32(0))
        assert r["lo"][0] == abs(v) and r["hi"][0] == abs(v) and r["s"][0] == max(abs(v), 1.0)
        y, s = ref.threshold(x, 0.995)
        assert y[0, 0] == np.sign(v) * min(abs(v), s[0]) / s[0]


def test_ratio_one_takes_the_maximum():
    x = _normal(2, 193, 7)
    k, k2, frac = ref.plan(1.0, 193)
    assert (k, k2, frac) == (192, 192, F32(0))
    r = ref.select(x, 1.0)
    np.testing.assert_array_equal(r["lo"], np.abs(x).max(1))
    np.testing.assert_array_equal(r["hi"], r["lo"])
    y, s = ref.threshold(x, 1.0)
    assert np.abs(y).max() <= 1.0 and (np.abs(y).max(1) == 1.0).all()      # nothing is clipped, the largest maps to +-1


def test_tiny_ratio_takes_the_minimum():
    x = _normal(2, 193, 8)
    k, k2, frac = ref.plan(1e-6, 193)
    assert k == 0 and k2 == 1 and 0 < frac < 1e-3
    r = ref.select(x, 1e-6)
    srt = np.sort(np.abs(x), axis=1)
    np.testing.assert_array_equal(r["lo"], srt[:, 0])
    np.testing.assert_array_equal(r["hi"], srt[:, 1])


def test_below_one_is_the_static_clamp_bitwise():
    x = _normal(3, 1728, 9, scale=0.3)           # the 0.9 quantile of |x| ~ 0.5 < 1, yet some |x| > 1
    x[0, :4] = [1.5, -2.0, -0.0, 0.0]
    r = ref.select(x, 0.9)
    assert (r["s_raw"] < 1).all() and (r["s"] == 1).all() and np.abs(x).max() > 1
    y, _ = ref.threshold(x, 0.9)
    assert y.tobytes() == np.clip(x, F32(-1), F32(1)).tobytes()


@pytest.mark.parametrize("scale", [0.3, 1.5, 40.0])
def test_max_value_one_is_the_static_clamp_bitwise(scale):
    x = _normal(3, 1728, 10, scale=scale)
    x[1, :2] = [-0.0, 3e38]
    y, s = ref.threshold(x, 0.995, max_value=1.0)
    assert (s == 1).all()
    assert y.tobytes() == np.clip(x, F32(-1), F32(1)).tobytes()


def test_keys_order_is_total():
    x = np.array([[-0.0, 0.0, 1e-45, -1e-40, 1e-30, -3e38, np.inf, np.nan]], F32)
    k = ref.keys(x)[0]
    assert k[0] == k[1] == 0 and list(k[1:]) == sorted(k[1:]) and len(set(k[1:])) == 7
    r = ref.select(x, 1.0)                       # the largest key is the NaN: s_raw NaN -> s = 1
    assert np.isnan(r["s_raw"][0]) and r["s"][0] == 1


def test_loop_without_a_threshold_is_the_clamped_loop():
    """ratio None and max_value = 1 both give the static clamp's chain."""
    import fast_sampler_ref as fast
    sched = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
    co = fast.coefficients(sched, "dpmpp_2m", 5)
    noise = synth.synth_noise(5, 2, 3, 8, 8, 3)
    eps_fn = lambda x, nl: (np.sin(3 * x) * F32(2.0) + F32(nl)).astype(F32)
    off = ref.sample_loop(eps_fn, co, noise)
    one = ref.sample_loop(eps_fn, co, noise, 0.995, 1.0)
    on = ref.sample_loop(eps_fn, co, noise, 0.995)
    assert off["states"].tobytes() == one["states"].tobytes()
    assert (on["s"] > 1).any() and np.abs(on["final"] - off["final"]).max() > 1e-3
    assert np.abs(on["x0"]).max() <= 1.0


def _facade():
    opt = synth.yml_opt(8, 16, 20)
    opt["sr"]["model"]["unet"].update(inner_channel=32, channel_multiplier=[1, 2], res_blocks=1, attn_res=[8])
    opt["sr"]["model"]["diffusion"].update(image_size=16, conditional=True)
    netG = pkg().define_G(opt)
    netG.set_new_noise_schedule(opt["sr"]["model"]["beta_schedule"]["val"], ["cpu"])
    return netG


def test_facade_argument_checks():
    netG = _facade()
    keys = list(netG.state_dict())
    assert netG._dyn is None
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            netG.set_dynamic_threshold(bad)
    for bad in (0.5, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            netG.set_dynamic_threshold(0.995, max_value=bad)
    with pytest.raises(ValueError):
        netG.set_dynamic_threshold(None, max_value=2.0)
    assert netG._dyn is None                                        # a refused setting leaves the old one
    netG.set_dynamic_threshold(0.995)
    assert netG._dyn == (0.995, None)
    netG.set_dynamic_threshold(1.0, max_value=1.0)
    assert netG._dyn == (1.0, 1.0)
    netG.set_dynamic_threshold(ratio=0.9, max_value=float("inf"))
    assert netG._dyn == (0.9, float("inf"))
    # survives the sampler and the schedule, adds nothing to state_dict()
    netG.set_sampler("dpmpp_2m", steps=10)
    netG.set_new_noise_schedule({"schedule": "linear", "n_timestep": 30, "linear_start": 1e-4, "linear_end": 2e-2}, ["cpu"])
    assert netG._dyn == (0.9, float("inf")) and list(netG.state_dict()) == keys
    netG.set_dynamic_threshold(None)
    assert netG._dyn is None
