#!/usr/bin/env python3
"""Generates tests/golden/warm_start_tiny.npz: the reference's own q_sample (model/sr/sr3_modules/diffusion.py:275-282)
of a start image at an intermediate level, followed by the reference's own p_sample steps (:182-187) from there: what
the sampler's warm start must reproduce. Run from the repo root in the build container, next to
make_golden.py (whose conventions this follows: the reference is imported read-only and at generation time only, weights
come from synth.synth_state_dict by seed and are not stored, torch's RNG calls are replaced by a NoiseFeed slab,
netG.eval()):

    python tests/golden/make_golden_warm_start.py

Config: synth.tiny_unet_config(), the T = 20 linear schedule of sampler_tiny.npz, B = 2, r = 16, l = 8. Per case
`s<s0>.<init>` with s0 in {1, 9, 20} and init in {"cond", "img"} (the conditioning image itself, or a second synthetic
image): the state q_sample(init, sqrt_alphas_cumprod_prev[s0], z) and the images after every step i of
reversed(range(s0)) with i % sample_inter == 0 (the loop of :208-211 cut to its last s0 iterations; the last frame, after
step 0, is the final result). z is slab 0 and the draw of step t slab s0 - t of synth.synth_noise(T, ...)[:s0]: the tests
regenerate them, and the images, from the same frozen streams.

To stay no larger than sampler_tiny.npz the arrays are stored sub-sampled: the states as every third element of the
flattened [B,3,r,r] array (`state_sub`: every lane of a 4-pixel run is visited), the frames as [..., ::2, ::2]
(`frames_sub`, as the large sampler fixtures store theirs). tests/test_warm_start_host.py pins the plain fp32 expression
a * x + s * z to `state_sub` bit for bit, so the GPU test can hold EVERY element of the device state to that expression.
"""
import json

import numpy as np
import torch

import make_golden as mg          # the shared helpers (and the sys.path set-up for the reference and the package)

synth = mg.synth
STATE_STRIDE, FRAME_STRIDE = 3, 2
START_STEPS = (1, 9, 20)


def gen_case(arrs, netG, s0, tag, init, cond, noise, T):
    B = init.shape[0]
    si = 1 | (T // 10)
    # one level for the whole batch, shaped as p_losses shapes its levels (:294-300); the fp32 cast is torch.FloatTensor's,
    # the one p_mean_variance applies to the level it feeds the UNet (:166-167)
    level = torch.FloatTensor([netG.sqrt_alphas_cumprod_prev[s0]]).repeat(B).view(-1, 1, 1, 1)
    state = netG.q_sample(torch.from_numpy(init), level, torch.from_numpy(noise[0].copy()))
    frames = []
    with mg.NoiseFeed(noise[1:s0]) as nf:
        img = state
        for i in reversed(range(0, s0)):
            img = netG.p_sample(img, i, condition_x=torch.from_numpy(cond))
            if i % si == 0:
                frames.append(img.numpy().copy())
        assert nf.k == s0 - 1, nf.k       # (step 0 draws nothing)
    p = f"s{s0}.{tag}."
    arrs[p + "state_sub"] = state.numpy().reshape(-1)[::STATE_STRIDE].copy()
    arrs[p + "frames_sub"] = np.stack(frames)[..., ::FRAME_STRIDE, ::FRAME_STRIDE].copy()
    print(f"  s0={s0:2d} init={tag:4s}: level {level.flatten()[0].item():.6f}, state std {state.std().item():.3f}, "
          f"{len(frames)} frames, final std {frames[-1].std():.3f}")


if __name__ == "__main__":
    tiny = synth.tiny_unet_config()
    s20 = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
    B, r, l, seed, T = 2, 16, 8, 5, 20                      # sampler_tiny.npz's network, schedule and conditioning
    netG = mg.build_ref(tiny, s20, seed)
    cond = synth.synth_cond(B, r, l, seed)
    img = synth.synth_cond(B, r, r // 2, seed + 1000)        # the second image: another smooth synthetic one
    noise = synth.synth_noise(T, B, 3, r, r, seed + 2000)
    arrs = {}
    for s0 in START_STEPS:
        for tag, init in (("cond", cond), ("img", img)):
            gen_case(arrs, netG, s0, tag, init, cond, noise[:s0], T)
    arrs["meta"] = mg.meta(tiny, B=B, r=r, l=l, seed=seed, img_seed=seed + 1000, img_l=r // 2, noise_seed=seed + 2000,
                           schedule=s20, conditional=True, start_steps=list(START_STEPS), inits=["cond", "img"],
                           state_stride=STATE_STRIDE, frame_stride=FRAME_STRIDE)
    mg.save("warm_start_tiny.npz", **arrs)
