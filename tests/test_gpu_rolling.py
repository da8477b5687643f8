"""The rolling-batch facade on the GPU (GaussianDiffusion.rolling -> rolling.RollingSampler): requests
with mixed strengths streamed through 4 slots against the single uniform call of each, byte for byte, and the restart of
the requests a range trip can have touched."""
import warnings

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
Sr3Error = pkg("_lib").Sr3Error
Sr3RangeWarning = pkg("_lib").Sr3RangeWarning
F32 = np.float32

TINY = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
SEED = 21
R, L = 16, 8


def _netG(opt, sd):
    import torch
    netG = pkg().define_G(opt).to("cuda:0")
    netG.load_state_dict({"denoise_fn." + k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    netG.set_new_noise_schedule(opt["sr"]["model"]["beta_schedule"]["val"], [0])
    return netG


def _tiny_netG():
    cfg = synth.tiny_unet_config()
    opt = {"phase": "val", "sr": {"model": {
        "which_model_G": "sr3",
        "unet": {"in_channel": 6, "out_channel": 3, "inner_channel": cfg.inner_channel,
                 "channel_multiplier": list(cfg.channel_mults), "attn_res": list(cfg.attn_res),
                 "res_blocks": cfg.res_blocks, "dropout": 0.0},
        "beta_schedule": {"train": TINY, "val": TINY},
        "diffusion": {"image_size": cfg.image_size, "channels": 3, "conditional": True}}}}
    return _netG(opt, synth.synth_state_dict(cfg, SEED))


def _expected_order(n_steps, slots):
    """completion order of requests pulled lazily into the lowest free slot: by step, then by slot"""
    rows, left, nxt, order = [None] * slots, [0] * slots, 0, []
    while nxt < len(n_steps) or any(r is not None for r in rows):
        for s in range(slots):
            if rows[s] is None and nxt < len(n_steps):
                rows[s], left[s] = nxt, n_steps[nxt]
                nxt += 1
        for s in range(slots):
            if rows[s] is not None:
                left[s] -= 1
                if left[s] == 0:
                    order.append(rows[s])
                    rows[s] = None
    return order


def test_stream_of_mixed_strengths_is_the_single_calls():
    import torch
    netG = _tiny_netG()
    netG.set_sampler("dpmpp_2m", steps=8)
    S, slots, seed = 8, 4, 1234
    strengths = [None, 0.5, 0.25, None, 0.25, 0.5, None, 0.5, 0.25, None]
    n = len(strengths)
    x = torch.from_numpy(synth.synth_cond(n, R, L, SEED)).cuda()
    img = torch.from_numpy(np.random.RandomState(SEED).uniform(-1, 1, (n, 3, R, R)).astype(F32)).cuda()
    # The guarantee is equality with a uniform call at the session's batch size (every step of the session runs at
    # B = slots): want4, the request repeated over 4 rows. want, the single B = 1 call the issue names, equals it on this
    # configuration only because the tiny UNet's conv plans do not vary over B = 1 and 4; on the yml UNet at 64 slots a
    # row is not the bytes of the B = 1 call.
    want, want4 = [], []
    for i, s in enumerate(strengths):
        x4, i4 = x[i:i + 1].expand(slots, -1, -1, -1).contiguous(), img[i:i + 1].expand(slots, -1, -1, -1).contiguous()
        if s is None:
            want.append(netG.super_resolution_batch(x[i:i + 1], seed=seed, image_offset=i)[0])
            want4.append(netG.super_resolution_batch(x4, seed=seed, image_offset=i)[0])
        else:
            want.append(netG.refine(x[i:i + 1], img[i:i + 1], s, seed=seed, image_offset=i)[0])
            want4.append(netG.refine(x4, i4, s, seed=seed, image_offset=i)[0])
    torch.cuda.synchronize()
    pulled = []

    def source():
        for i, s in enumerate(strengths):
            pulled.append(i)
            yield {"x_in_row": x[i], "init": None if s is None else img[i], "strength": s}

    with netG.rolling(slots, seed=seed) as rs:
        assert rs.S == S and rs.slots == slots
        got = list(rs.stream(source()))
        trace = list(rs.trace)
        assert rs.restarts == 0
    torch.cuda.synchronize()
    assert sorted(t for t, _ in got) == list(range(n))
    for t, image in got:
        for w, what in ((want4[t], "uniform call of 4"), (want[t], "single call")):
            assert image.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), \
                f"request {t} (strength {strengths[t]}) against the {what}: max abs difference {float((image - w).abs().max()):.3e}"
    n_steps = [S if s is None else max(1, round(s * S)) for s in strengths]
    assert [t for t, _ in got] == _expected_order(n_steps, slots) != list(range(n))
    # the slots were never idle while the source still had a request
    assert trace and all(live == slots or (queued == 0 and exhausted) for live, queued, exhausted in trace)
    assert sum(live for live, _, _ in trace) == sum(n_steps)
    # the default slot count
    with netG.rolling(seed=seed) as rs:
        assert rs.slots == min(64, netG._engine().max_batch(R, R))
    # the settings a row session does not carry are refused by name
    netG.set_feature_cache(2, 1)
    with pytest.raises(Sr3Error, match="set_feature_cache"):
        netG.rolling(slots)
    netG.set_feature_cache(None)
    netG.set_lr_consistency(torch.zeros(1, 3, L, L))
    with pytest.raises(Sr3Error, match="set_lr_consistency"):
        netG.rolling(slots)
    netG.set_lr_consistency(None)
    # and the uniform sampler is what it was
    again = netG.super_resolution_batch(x[:1], seed=seed, image_offset=0)[0]
    assert torch.equal(again, want[0])
    torch.cuda.synchronize()


def test_range_trip_restarts_the_requests_in_flight():
    """The input recipe of test_gpu_f16f8.py::test_fp8_range_falls_back_to_f16x3_first: a GroupNorm gamma at the 32x32
    level scaled so that activations pass the fp8 operand range (448) but not the fp16 range, at the batch (64) from
    which the fp8 path runs. A first wave is served in f16x3 and delivered; then the sampler is put in f16f8 and a second
    wave trips the check: those requests restart one arithmetic down and come back as the f16x3 bytes, restarts == 1,
    and what was delivered before stays what it was. Under the strict policy the check raises."""
    import torch
    cfg = synth.yml_unet_config(224)
    sd = synth.synth_state_dict(cfg, 3)
    name = next(k for k, v in sd.items() if k.startswith("downs.") and k.endswith("res_block.block2.block.0.weight") and v.shape == (256,))
    sd[name] = sd[name] * F32(400.0)
    netG = _netG(synth.yml_opt(16, 128, 3), sd)
    netG.eval()
    netG.denoise_fn.precision = "f16x3"
    B, seed, first_wave = 64, 7, 8
    x = torch.from_numpy(synth.synth_cond(B, 128, 16, 5)).cuda()
    want = netG.super_resolution_batch(x, seed=seed)
    eng = netG._engine()
    assert eng.fallback_calls() == 0
    rs = netG.rolling(B, seed=seed)
    for i in range(first_wave):
        rs.submit(x[i])
    first = rs.drain()
    assert [t for t, _ in first] == list(range(first_wave)) and rs.restarts == 0
    for t, image in first:
        assert torch.equal(image, want[t]), t
    kept = [image.clone() for _, image in first]
    rs.set_precision("f16f8")
    for i in range(first_wave, B):
        rs.submit(x[i])
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        rest = rs.drain()
    assert any(issubclass(w.category, Sr3RangeWarning) for w in rec)
    assert rs.restarts == 1 and rs.precision == "f16x3"
    assert [t for t, _ in rest] == list(range(first_wave, B))
    for t, image in rest:
        assert torch.equal(image, want[t]), t
    for (t, image), k in zip(first, kept):
        assert torch.equal(image, k), t
    rs.close()
    # strict: the same trip raises
    netG.denoise_fn.precision = "f16f8"
    netG.denoise_fn.strict_range = True
    with netG.rolling(B, seed=seed) as rs:
        assert rs.strict and rs.precision == "f16f8"
        rs.submit(x[0])
        with pytest.raises(Sr3Error, match="range"):
            rs.drain()
        assert rs.restarts == 0
    torch.cuda.synchronize()
