"""The denoising loss on the host side (CPU only): the level draws of GaussianDiffusion.p_losses against the reference's,
and the fixture tests/golden/losses_tiny.npz (tests/golden/make_golden_losses.py: the reference's own p_losses) against
independent restatements, so that the GPU tests of tests/test_gpu_losses.py do not lean on a self-referential file."""
import ctypes
import os
import re

import numpy as np
import pytest

import sr3_oracle_aten as aten
from conftest import REPO, cfg_from_meta, load_golden, pkg

synth = pkg("synth")
schedule = pkg("schedule")


@pytest.fixture(scope="module")
def golden():
    return load_golden("losses_tiny.npz")


def _cases(g):
    return list(enumerate(g["cases"]))


def test_fixture_has_the_cases_the_loss_is_pinned_on(golden):
    got = [(m["loss_type"], m["conditional"], m["r"], m["B"]) for _, m in _cases(golden)]
    assert got == [("l1", True, 16, 3), ("l2", True, 16, 3), ("l1", True, 24, 2), ("l1", False, 16, 2)]
    assert (24 * 24) % 256 != 0
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "losses_tiny.npz")) < 512 * 1024


def test_draw_levels_reproduces_the_reference_draws(golden):
    """np.random.seed(k) + draw_levels == the t and the fp32 levels the reference drew inside p_losses under the same seed
    (diffusion.py:287-294), bit for bit."""
    draw_levels = pkg().draw_levels
    assert pkg("diffusion").draw_levels is draw_levels
    for i, m in _cases(golden):
        with np.errstate(divide="ignore", invalid="ignore"):
            bufs = schedule.schedule_buffers(m["schedule"])
        np.random.seed(m["np_seed"])
        t, lv = draw_levels(bufs["sqrt_alphas_cumprod_prev"], m["schedule"]["n_timestep"], m["B"])
        assert t == m["t"] and isinstance(t, int)
        assert lv.dtype == np.float32 and lv.shape == (m["B"],)
        assert lv.tobytes() == golden[f"c{i}.levels"].tobytes()
        lo, hi = sorted((bufs["sqrt_alphas_cumprod_prev"][t - 1], bufs["sqrt_alphas_cumprod_prev"][t]))
        assert (lv >= np.float32(lo)).all() and (lv <= np.float32(hi)).all()
        # the draws advance numpy's global stream exactly as the reference's two calls do
        after = np.random.random()
        np.random.seed(m["np_seed"])
        np.random.randint(1, m["schedule"]["n_timestep"] + 1)
        np.random.uniform(0.0, 1.0, size=m["B"])
        assert after == np.random.random()


def test_fixture_is_not_self_referential(golden):
    """x_noisy from the torch CPU expression of q_sample (bit-equal; its sqrt(1 - a^2) through numpy's correctly rounded
    fp32 sqrt: torch's CPU sqrt is 1 ulp off on some hosts, and the fixture comes from one where it is not); x_recon from
    the aten oracle on cat(SR, x_noisy) at the stored levels (2e-5: the forward bar of tests/test_oracle_golden.py); the
    stored loss — accumulated by torch in fp32 — from a float64 sum (1e-5 relative)."""
    import torch
    for i, m in _cases(golden):
        g = {k[len(f"c{i}."):]: v for k, v in golden.items() if k.startswith(f"c{i}.")}
        a = torch.from_numpy(g["levels"]).view(-1, 1, 1, 1)
        hr, noise = torch.from_numpy(g["HR"]), torch.from_numpy(g["noise"])
        s = torch.from_numpy(np.sqrt((1 - a ** 2).numpy()))
        assert s.dtype == torch.float32 and s.numpy().tobytes() == pkg("diffusion").noise_coefficient(g["levels"]).tobytes()
        x_noisy = a * hr + s * noise                                         # diffusion.py:279-282
        assert x_noisy.dtype == torch.float32
        assert x_noisy.numpy().tobytes() == g["x_noisy"].tobytes(), f"case {i}"
        cfg = cfg_from_meta(m)
        assert cfg.in_channel == (6 if m["conditional"] else 3)
        sd = aten.to_torch_state(synth.synth_state_dict(cfg, m["seed"]))
        x = torch.cat([torch.from_numpy(g["SR"]), x_noisy], dim=1) if m["conditional"] else x_noisy
        with torch.no_grad():
            eps = aten.unet_forward(sd, cfg, x, torch.from_numpy(g["levels"])).numpy()
        err = float(np.abs(eps - g["x_recon"]).max())
        d = g["noise"].astype(np.float64) - g["x_recon"].astype(np.float64)
        want = float(np.abs(d).sum() if m["loss_type"] == "l1" else (d * d).sum())
        rel = abs(want - float(g["loss"])) / want
        print(f"losses_tiny case {i}: max |aten - x_recon| = {err:.2e}, loss {float(g['loss']):.4f} vs float64 sum {want:.4f} "
              f"(rel {rel:.1e})")
        assert err <= 2e-5
        assert rel <= 1e-5


def test_facade_members_exist_without_a_gpu():
    """The reference's members are there on a CPU-only host: set_loss selects the loss, DictTensor has the reference's
    interface, and the evaluation itself refuses to run without the device (no CPU fallback)."""
    import torch
    P = pkg()
    opt = synth.yml_opt(8, 16, 100)
    opt["sr"]["model"]["unet"].update(inner_channel=32, channel_multiplier=[1, 2], res_blocks=1, attn_res=[8])
    opt["sr"]["model"]["diffusion"]["image_size"] = 16
    netG = P.define_G(opt)
    netG.set_new_noise_schedule(opt["sr"]["model"]["beta_schedule"]["val"], ["cpu"])
    x = {"HR": torch.zeros(1, 3, 16, 16), "SR": torch.zeros(1, 3, 16, 16)}
    with pytest.raises(NotImplementedError, match="set_loss"):
        netG(x)                                              # the reference has no loss_func before set_loss either
    for kind in ("l1", "l2"):
        netG.loss_type = kind
        netG.set_loss("cpu")
        assert netG.loss_func == kind
    netG.loss_type = "huber"
    with pytest.raises(NotImplementedError):
        netG.set_loss("cpu")
    with pytest.raises(NotImplementedError, match="no CPU"):
        netG(P.DictTensor(x))
    d = P.DictTensor({"HR": torch.zeros(1), "name": "a"})
    assert d.to("cpu") is d and d.data["name"] == "a" and d.data["HR"].device.type == "cpu"
    # the reference's whole interface (diffusion.py:323-344): indexing, assignment, keys, items, repr
    assert d["name"] == "a" and d["HR"] is d.data["HR"]
    d["SR"] = torch.ones(2)
    assert d.data["SR"].tolist() == [1.0, 1.0]
    assert list(d.keys()) == ["HR", "name", "SR"] and [k for k, _ in d.items()] == ["HR", "name", "SR"]
    assert d.keys() == d.data.keys() and repr(d) == str(d.data)
    assert len(netG.state_dict()) == len([k for k in netG.state_dict() if k.startswith("denoise_fn.")]) + 12


def test_abi_declares_the_loss_entry_points():
    header = open(os.path.join(REPO, "include", "sr3hip.h")).read()
    protos = pkg("_lib").PROTOTYPES
    for name, n_args in (("sr3_denoise_loss", 18), ("sr3_op_q_sample", 15)):
        assert re.search(r"\bint " + name + r"\(sr3_ctx \*ctx", header)
        res, args = protos[name]
        assert res is ctypes.c_int and len(args) == n_args
    assert "diffusion.py:275-282" in header and "diffusion.py:284-313" in header
    assert "kernels_loss.hip" in pkg("build").SOURCES
