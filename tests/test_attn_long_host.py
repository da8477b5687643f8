"""Pins both CPU oracles to tests/golden/unet_attn_long.npz (tests/golden/make_golden_attn.py): the reference's UNet
forward with attention over more than 1024 tokens (4624 at C = 32, 1156 in the mid block at C = 64). CPU only; bar
as in test_oracle_golden.py."""
import numpy as np

import sr3_oracle as oracle
import sr3_oracle_aten as aten
from conftest import cfg_from_meta, load_golden, pkg

synth = pkg("synth")
TOL = 2e-5


def test_fixture_attention_token_counts():
    g = load_golden("unet_attn_long.npz")
    cfg = cfg_from_meta(g["meta"])
    downs, mid, ups = oracle.unet_plan(cfg)
    r = g["x"].shape[-1]
    assert g["x"].shape == (1, 6, 68, 68) and r * r == 4624
    assert any(a for _, _, a in downs) and any(a for _, _, a in mid)
    assert (r // 2) ** 2 == 1156 and 4624 % 32 and 1156 % 32


def test_numpy_oracle_matches_reference_long_attention():
    g = load_golden("unet_attn_long.npz")
    cfg = cfg_from_meta(g["meta"])
    sd = synth.synth_state_dict(cfg, g["meta"]["seed"])
    eps = oracle.unet_forward(sd, cfg, g["x"], g["noise_level"])
    np.testing.assert_allclose(eps, g["eps"], atol=TOL, rtol=0)


def test_aten_oracle_matches_reference_long_attention():
    import torch
    g = load_golden("unet_attn_long.npz")
    cfg = cfg_from_meta(g["meta"])
    sd = aten.to_torch_state(synth.synth_state_dict(cfg, g["meta"]["seed"]))
    with torch.no_grad():
        eps = aten.unet_forward(sd, cfg, torch.from_numpy(g["x"]), torch.from_numpy(g["noise_level"])).numpy()
    np.testing.assert_allclose(eps, g["eps"], atol=TOL, rtol=0)
