#!/usr/bin/env python3
"""Generates tests/golden/dropout_tiny.npz: the reference's own TRAIN-mode UNet — nn.Dropout active in every
ResnetBlock.block2 (model/sr/sr3_modules/unet.py:81-91,100-101) — on tiny networks, with the masks it drew. Run from the
repo root in the build container, next to make_golden.py (whose conventions this follows: the reference is imported
read-only, weights come from synth.synth_state_dict by seed and are not stored, torch's randn calls are replaced by a
NoiseFeed slab):

    python tests/golden/make_golden_dropout.py

The masks are recorded by a forward hook on each nn.Dropout as (out != 0) | (in == 0) — an element that was zero going
in says nothing about its keep bit and is recorded as kept, which gives the same product — in the order of the forward
(= named_modules() order: downs, mid, ups), concatenated as NCHW bytes and stored with np.packbits. torch's generator is
seeded per case, so a re-run reproduces the file.

Cases (all tiny_unet_config() with dropout set; 8 Dropout modules):
  a  UNet.forward, train mode, B = 2, 16x16, p = 0.2: x, noise_level, masks, eps_train, and eps_eval of the same net
  b  the same at 24x24 with p = 0.1 (an inexact scale)
  c  p_losses (l1), train mode, B = 3, 16x16, p = 0.2: HR, SR, noise, levels, masks, x_recon, loss
  d  super_resolution(continous=True), train mode, T = 4, B = 1, 16x16, p = 0.2: cond, noise, per-step masks, ret_img
"""
import dataclasses
import json

import numpy as np
import torch
from torch import nn

import make_golden as mg          # the shared helpers (and the sys.path set-up for the reference and the package)

synth = mg.synth


class MaskRecorder:
    """Forward hooks on every nn.Dropout of a module: one list of uint8 masks per forward, in call order."""

    def __init__(self, root):
        self.mods = [m for m in root.modules() if isinstance(m, nn.Dropout)]
        self.masks = []
        self.hooks = [m.register_forward_hook(self._hook) for m in self.mods]

    def _hook(self, mod, inp, out):
        self.masks.append(((out != 0) | (inp[0] == 0)).numpy().astype(np.uint8))

    def take(self):
        m, self.masks = self.masks, []
        return m

    def close(self):
        for h in self.hooks:
            h.remove()


def packed(masks):
    return np.packbits(np.concatenate([m.ravel() for m in masks]))


def with_dropout(cfg, p):
    return dataclasses.replace(cfg, dropout=p)


def gen_forward(arrs, metas, tag, p, B, r, seed, torch_seed):
    cfg = with_dropout(synth.tiny_unet_config(), p)
    sched = {"schedule": "linear", "n_timestep": 10, "linear_start": 1e-4, "linear_end": 2e-2}
    netG = mg.build_ref(cfg, sched, seed)
    unet = netG.denoise_fn
    x, nl = synth.synth_unet_input(cfg, B, r, r, seed)
    eps_eval = unet(torch.from_numpy(x), torch.from_numpy(nl)).numpy()
    rec = MaskRecorder(unet)
    unet.train()
    torch.manual_seed(torch_seed)
    eps_train = unet(torch.from_numpy(x), torch.from_numpy(nl)).numpy()
    masks = rec.take()
    rec.close()
    assert len(masks) == len(rec.mods) == 8, (len(masks), len(rec.mods))
    k = tag + "."
    arrs.update({k + "x": x, k + "noise_level": nl, k + "masks": packed(masks), k + "eps_train": eps_train,
                 k + "eps_eval": eps_eval})
    metas[tag] = dict(json.loads(str(mg.meta(cfg))), B=B, r=r, seed=seed, torch_seed=torch_seed,
                      mask_shapes=[list(m.shape) for m in masks])
    print(f"  case {tag}: p={p} {r}x{r} B={B} keep {np.mean(np.concatenate([m.ravel() for m in masks])):.4f} "
          f"train-eval max-abs {np.abs(eps_train - eps_eval).max():.3f} (range +-{np.abs(eps_eval).max():.2f})")


def gen_loss(arrs, metas, tag, p, B, r, l, seed, np_seed, torch_seed):
    cfg = with_dropout(synth.tiny_unet_config(), p)
    sched = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
    netG = mg.build_ref(cfg, sched, seed)
    netG.loss_func = nn.L1Loss(reduction="sum")
    captured = []
    hook = netG.denoise_fn.register_forward_hook(
        lambda mod, inp, out: captured.append((inp[0].numpy().copy(), inp[1].numpy().copy(), out.numpy().copy())))
    hr = synth.synth_cond(B, r, r // 2, seed + 1000)
    sr = synth.synth_cond(B, r, l, seed)
    noise = synth.synth_noise(1, B, 3, r, r, seed)
    rec = MaskRecorder(netG.denoise_fn)
    netG.train()
    np.random.seed(np_seed)
    torch.manual_seed(torch_seed)
    with mg.NoiseFeed(noise) as nf:
        loss = netG({"HR": torch.from_numpy(hr), "SR": torch.from_numpy(sr)})
        assert nf.k == 1, nf.k
    masks = rec.take()
    rec.close()
    hook.remove()
    assert len(masks) == 8 and len(captured) == 1
    xin, level, x_recon = captured[0]
    k = tag + "."
    arrs.update({k + "HR": hr, k + "SR": sr, k + "noise": noise[0], k + "levels": level.reshape(-1).astype(np.float32),
                 k + "x_noisy": xin[:, -3:].copy(), k + "masks": packed(masks), k + "x_recon": x_recon,
                 k + "loss": np.float32(loss.item())})
    metas[tag] = dict(json.loads(str(mg.meta(cfg))), B=B, r=r, l=l, seed=seed, np_seed=np_seed, torch_seed=torch_seed,
                      loss_type="l1", schedule=sched, mask_shapes=[list(m.shape) for m in masks])
    print(f"  case {tag}: l1 p={p} {r}x{r} B={B} loss/elem {loss.item() / x_recon.size:.4f}")


def gen_sampler(arrs, metas, tag, p, T, B, r, l, seed, torch_seed):
    cfg = with_dropout(synth.tiny_unet_config(), p)
    sched = {"schedule": "linear", "n_timestep": T, "linear_start": 1e-4, "linear_end": 2e-2}
    netG = mg.build_ref(cfg, sched, seed)
    cond = synth.synth_cond(B, r, l, seed)
    noise = synth.synth_noise(T, B, 3, r, r, seed)
    rec = MaskRecorder(netG.denoise_fn)
    netG.train()
    torch.manual_seed(torch_seed)
    with mg.NoiseFeed(noise) as nf:
        ret = netG.super_resolution(torch.from_numpy(cond), continous=True).numpy()
        assert nf.k == T, nf.k
    masks = rec.take()
    rec.close()
    assert len(masks) == 8 * T
    k = tag + "."
    # step k (t = T-1-k) drew masks[8k : 8k+8]
    arrs.update({k + "cond": cond, k + "noise": noise, k + "ret_img": ret,
                 k + "masks": np.stack([packed(masks[8 * s:8 * s + 8]) for s in range(T)])})
    metas[tag] = dict(json.loads(str(mg.meta(cfg))), B=B, r=r, l=l, seed=seed, torch_seed=torch_seed, schedule=sched,
                      mask_shapes=[list(m.shape) for m in masks[:8]])
    print(f"  case {tag}: sampler T={T} p={p} {r}x{r} B={B} final std {ret[-B:].std():.3f}")


if __name__ == "__main__":
    arrs, metas = {}, {}
    gen_forward(arrs, metas, "a", 0.2, B=2, r=16, seed=31, torch_seed=101)
    gen_forward(arrs, metas, "b", 0.1, B=2, r=24, seed=32, torch_seed=102)
    gen_loss(arrs, metas, "c", 0.2, B=3, r=16, l=8, seed=33, np_seed=4, torch_seed=103)
    gen_sampler(arrs, metas, "d", 0.2, T=4, B=1, r=16, l=8, seed=34, torch_seed=104)
    arrs["metas"] = np.array(json.dumps(metas))
    mg.save("dropout_tiny.npz", **arrs)
