"""Train-mode Dropout, host side: the mask-aware aten oracle is pinned to vectors the reference itself
produced in train mode (tests/golden/make_golden_dropout.py), and the CPU twin of the device's mask stream
(tests/dropout_ref.py) has the properties the design claims. CPU only."""
import math

import numpy as np
import pytest

import dropout_ref as dr
import sr3_oracle_aten as aten
from conftest import cfg_from_meta, load_golden, pkg

synth = pkg("synth")

# the bars tests/test_oracle_golden.py holds the same oracle to without dropout: forward 2e-5, sampler 1e-4
TOL_FORWARD, TOL_SAMPLER = 2e-5, 1e-4


@pytest.fixture(scope="module")
def golden():
    import json
    g = load_golden("dropout_tiny.npz")
    g["metas"] = json.loads(str(g["metas"]))
    return g


def _case(golden, tag):
    m = golden["metas"][tag]
    cfg = cfg_from_meta(m)
    sd = aten.to_torch_state(synth.synth_state_dict(cfg, m["seed"]))
    return m, cfg, sd


@pytest.mark.parametrize("tag", ["a", "b"])
def test_masked_oracle_reproduces_the_reference_train_forward(golden, tag):
    import torch
    m, cfg, sd = _case(golden, tag)
    masks = dr.unpack(golden[tag + ".masks"], m["mask_shapes"])
    assert len(masks) == 8
    x, nl = torch.from_numpy(golden[tag + ".x"]), torch.from_numpy(golden[tag + ".noise_level"])
    with torch.no_grad():
        with dr.masked(masks, cfg.dropout):
            eps = aten.unet_forward(sd, cfg, x, nl).numpy()
        eps_eval = aten.unet_forward(sd, cfg, x, nl).numpy()
    e = np.abs(eps - golden[tag + ".eps_train"]).max()
    gap = np.abs(golden[tag + ".eps_train"] - golden[tag + ".eps_eval"]).max()
    print(f"case {tag}: masked oracle vs reference train {e:.2e}; reference train vs eval {gap:.3f}")
    assert e <= TOL_FORWARD
    assert np.abs(eps_eval - golden[tag + ".eps_eval"]).max() <= TOL_FORWARD
    assert gap > 0.1            # not a rounding-level difference: what the feature is about


def test_masked_oracle_reproduces_the_reference_train_loss(golden):
    import torch
    m, cfg, sd = _case(golden, "c")
    masks = dr.unpack(golden["c.masks"], m["mask_shapes"])
    lv = golden["c.levels"]
    s = pkg("diffusion").noise_coefficient(lv)
    x_noisy = lv[:, None, None, None] * golden["c.HR"] + s[:, None, None, None] * golden["c.noise"]
    np.testing.assert_array_equal(x_noisy.astype(np.float32), golden["c.x_noisy"])
    inp = torch.from_numpy(np.concatenate([golden["c.SR"], golden["c.x_noisy"]], axis=1))
    with torch.no_grad(), dr.masked(masks, cfg.dropout):
        x_recon = aten.unet_forward(sd, cfg, inp, torch.from_numpy(lv)).numpy()
    assert np.abs(x_recon - golden["c.x_recon"]).max() <= TOL_FORWARD
    loss = np.abs(golden["c.noise"].astype(np.float64) - x_recon).sum()
    assert abs(loss - float(golden["c.loss"])) <= TOL_FORWARD * x_recon.size


def test_masked_oracle_reproduces_the_reference_train_sampler(golden):
    import torch
    m, cfg, sd = _case(golden, "d")
    sch = aten.noise_schedule(m["schedule"])
    T, B = m["schedule"]["n_timestep"], m["B"]
    noise, cond = golden["d.noise"], torch.from_numpy(golden["d.cond"])
    img = torch.from_numpy(noise[0].copy())
    frames = []
    with torch.no_grad():
        for k, t in enumerate(reversed(range(T))):
            masks = dr.unpack(golden["d.masks"][k], m["mask_shapes"])
            nz = torch.from_numpy(noise[k + 1].copy()) if t > 0 else None
            with dr.masked(masks, cfg.dropout):
                img = aten.p_sample(sd, cfg, sch, img, t, cond, nz)
            frames.append(img.numpy().copy())
    ret = np.concatenate([golden["d.cond"]] + frames, axis=0)          # T = 4: every step is a frame (1 | T // 10 == 1)
    assert ret.shape == golden["d.ret_img"].shape
    assert np.abs(ret - golden["d.ret_img"]).max() <= TOL_SAMPLER


@pytest.mark.parametrize("p", [0.1, 0.2, 0.3, 0.37, 0.5])
def test_scale_is_what_torch_dropout_multiplies_by(p):
    import torch
    s = dr.scale(p)
    assert s == np.float32(1.0 / (1.0 - p))
    x = torch.ones(4096)
    y = torch.nn.functional.dropout(x, p, training=True)
    kept = y[y != 0]
    assert kept.numel() > 0 and bool((kept == float(s)).all())


def test_threshold_and_keep_probability():
    assert dr.threshold(0.1) == 6554 and dr.threshold(0.2) == 13107 and dr.threshold(0.5) == 32768
    assert dr.threshold(0.0) == 0
    assert dr.threshold(0.5 / 65536) == 0 and dr.threshold(1.5 / 65536) == 2      # ties go to the even neighbour
    assert abs((1 - dr.threshold(0.2) / 65536) - 0.80000305) < 1e-8


def test_field_to_channel_mapping():
    import philox
    seed, image, draw, layer, C, H, W = 0x1234567890abcdef, (7 << 32) | 5, 3, 2, 16, 3, 5
    f = dr.fields(seed, image, draw, layer, C, H, W)
    assert f.shape == (C, H, W) and f.max() <= 0xffff
    for (c, y, x) in [(0, 0, 0), (7, 0, 0), (8, 0, 0), (13, 2, 4), (5, 1, 3)]:
        octet = (y * W + x) * (C // 8) + c // 8
        r = philox.philox4x32_10(np.array([octet]), np.array([((layer + 1) << 24) | draw]), np.array([5]), np.array([7]),
                                 seed & 0xffffffff, seed >> 32)
        j = c % 8
        assert f[c, y, x] == (int(r[j >> 1][0]) >> (16 * (j & 1))) & 0xffff


def test_mask_depends_on_the_global_index_only():
    layers = [(32, 8, 8), (64, 4, 4)]
    whole = dr.batch_masks(11, 100, 0, layers, 4, 0.2)
    part = dr.batch_masks(11, 102, 0, layers, 2, 0.2)
    for w, q in zip(whole, part):
        np.testing.assert_array_equal(w[2:4], q)


def test_layers_draws_seeds_and_images_give_distinct_masks():
    base = dr.mask(5, 0, 0, 0, 32, 8, 8, 0.2)
    for other in (dr.mask(5, 0, 0, 1, 32, 8, 8, 0.2), dr.mask(5, 0, 1, 0, 32, 8, 8, 0.2),
                  dr.mask(6, 0, 0, 0, 32, 8, 8, 0.2), dr.mask(5, 1, 0, 0, 32, 8, 8, 0.2)):
        assert 0.2 < np.mean(base != other) < 0.45          # two independent p = 0.2 masks differ in 2 * 0.2 * 0.8 = 0.32


def test_counter_word_never_collides_with_the_noise_stream():
    for layer in (0, 1, 253):
        for draw in (0, 1, (1 << 24) - 1):
            assert dr.counter_c1(layer, draw) >> 24 == layer + 1 >= 1        # the noise stream's c1 is draw < 2^24
            assert dr.counter_c1(layer, draw) < 1 << 32
    with pytest.raises(ValueError):
        dr.counter_c1(254, 0)
    with pytest.raises(ValueError):
        dr.counter_c1(0, 1 << 24)


@pytest.mark.parametrize("p,seed", [(0.2, 1), (0.1, 2), (0.5, 3)])
def test_keep_fraction_of_one_layer(p, seed):
    n = 64 * 32 * 32
    q = 1 - dr.threshold(p) / 65536
    kept = int(dr.mask(seed, 0, 0, 0, 64, 32, 32, p).sum())
    sd = math.sqrt(n * q * (1 - q))
    print(f"p={p}: kept {kept} of {n}, expected {n * q:.1f} +- {sd:.1f}")
    assert abs(kept - n * q) <= 5 * sd
