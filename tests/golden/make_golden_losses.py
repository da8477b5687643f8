#!/usr/bin/env python3
"""Generates tests/golden/losses_tiny.npz: the reference's own denoising loss (GaussianDiffusion.forward -> p_losses,
model/sr/sr3_modules/diffusion.py:284-318) on tiny networks, with everything a test needs to follow it step by step.
Run from the repo root in the build container, next to make_golden.py (whose conventions this follows: the reference is
imported read-only, weights come from synth.synth_state_dict by seed and are not stored, torch's RNG calls are replaced
by a NoiseFeed slab, netG.eval()):

    python tests/golden/make_golden_losses.py

Per case `c<i>`: HR, SR, noise (what the reference's torch.randn_like returned), np_seed (np.random.seed before the
call), t and levels (the reference's two np.random draws: levels are the fp32 tensor it feeds the UNet), x_noisy and
x_recon (input channels [-3:] and output of denoise_fn, captured by wrapping it) and the loss. The reference's set_loss
calls .cuda(); loss_func is set directly instead.
"""
import json
import os

import numpy as np
import torch
from torch import nn

import make_golden as mg          # the shared helpers (and the sys.path set-up for the reference and the package)

synth, graph = mg.synth, mg.graph


class Capture(nn.Module):
    """denoise_fn wrapped: records the input and the output of the one forward p_losses runs."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.calls = inner, []

    def forward(self, x, level):
        y = self.inner(x, level)
        self.calls.append((x.numpy().copy(), level.numpy().copy(), y.numpy().copy()))
        return y


def gen_case(arrs, metas, i, cfg, sched, B, r, l, seed, loss_type, conditional, np_seed):
    netG = mg.build_ref(cfg, sched, seed, conditional)
    netG.loss_func = nn.L1Loss(reduction="sum") if loss_type == "l1" else nn.MSELoss(reduction="sum")
    cap = Capture(netG.denoise_fn)
    netG.denoise_fn = cap
    hr = synth.synth_cond(B, r, r // 2, seed + 1000)
    sr = synth.synth_cond(B, r, l, seed)
    noise = synth.synth_noise(1, B, 3, r, r, seed)
    x = {"HR": torch.from_numpy(hr), "SR": torch.from_numpy(sr)}
    np.random.seed(np_seed)
    with mg.NoiseFeed(noise) as nf:
        loss = netG(x)
        assert nf.k == 1, nf.k
    assert len(cap.calls) == 1
    xin, level, x_recon = cap.calls[0]
    # the draws the reference made, replayed from the same seed (diffusion.py:287-294)
    np.random.seed(np_seed)
    t = np.random.randint(1, netG.num_timesteps + 1)
    lv = np.random.uniform(netG.sqrt_alphas_cumprod_prev[t - 1], netG.sqrt_alphas_cumprod_prev[t], size=B)
    np.testing.assert_array_equal(torch.FloatTensor(lv).numpy(), level.reshape(-1))
    if conditional:
        np.testing.assert_array_equal(xin[:, :3], sr)
    p = f"c{i}."
    arrs.update({p + "HR": hr, p + "SR": sr, p + "noise": noise[0], p + "levels": level.reshape(-1).astype(np.float32),
                 p + "x_noisy": xin[:, -3:].copy(), p + "x_recon": x_recon, p + "loss": np.float32(loss.item())})
    metas.append(dict(json.loads(str(mg.meta(cfg))), B=B, r=r, l=l, seed=seed, loss_type=loss_type, conditional=conditional,
                      schedule=sched, np_seed=np_seed, t=int(t)))
    print(f"  case {i}: {loss_type} {'cond' if conditional else 'uncond'} {r}x{r} B={B} t={t} loss/elem "
          f"{loss.item() / x_recon.size:.4f}")


if __name__ == "__main__":
    tiny = synth.tiny_unet_config()
    tiny_u = graph.UNetConfig(in_channel=3, out_channel=3, inner_channel=32, channel_mults=(1, 2),
                              attn_res=(8,), res_blocks=1, dropout=0.0, image_size=16)      # sampler_uncond_tiny's
    s20 = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
    s10 = {"schedule": "cosine", "n_timestep": 10, "linear_start": 1e-4, "linear_end": 2e-2}
    arrs, metas = {}, []
    gen_case(arrs, metas, 0, tiny, s20, B=3, r=16, l=8, seed=21, loss_type="l1", conditional=True, np_seed=1)
    gen_case(arrs, metas, 1, tiny, s20, B=3, r=16, l=8, seed=21, loss_type="l2", conditional=True, np_seed=2)
    gen_case(arrs, metas, 2, tiny, s20, B=2, r=24, l=8, seed=22, loss_type="l1", conditional=True, np_seed=3)
    gen_case(arrs, metas, 3, tiny_u, s10, B=2, r=16, l=8, seed=23, loss_type="l1", conditional=False, np_seed=4)
    arrs["cases"] = np.array(json.dumps(metas))
    mg.save("losses_tiny.npz", **arrs)
