"""LR consistency and frames per request through the rolling-batch facade (GaussianDiffusion.rolling ->
rolling.RollingSampler): a stream of requests with and without an `lr`, some with `continous`, against
the single calls of each at B = slots, with and without set_lr_consistency, byte for byte; the consistency score of the
held results; and a range trip that restarts held requests."""
import warnings

import numpy as np
import pytest

import test_gpu_rolling as roll
from conftest import pkg
from test_gpu_lr_consistency import BAR_OP

pytestmark = pytest.mark.gpu
synth = pkg("synth")
Sr3Error = pkg("_lib").Sr3Error
Sr3RangeWarning = pkg("_lib").Sr3RangeWarning
F32 = np.float32
SEED, R, L = roll.SEED, roll.R, roll.L


def _bytes(t):
    return t.cpu().numpy().tobytes()


def test_stream_of_held_unheld_and_continous_requests_is_the_single_calls():
    import torch
    netG = roll._tiny_netG()
    netG.set_sampler("dpmpp_2m", steps=8)
    S, slots, seed = 8, 4, 1234
    #            lr     strength  continous
    plan = [(True, None, False), (False, None, False), (True, 0.5, False), (False, None, True), (True, None, True),
            (True, 0.25, True), (False, 0.5, False), (True, None, False), ("u8", None, False)]
    n = len(plan)
    x = torch.from_numpy(synth.synth_cond(n, R, L, SEED)).cuda()
    img = torch.from_numpy(np.random.RandomState(SEED).uniform(-1, 1, (n, 3, R, R)).astype(F32)).cuda()
    lr = torch.from_numpy(np.random.RandomState(SEED ^ 0x10C0).uniform(-1, 1, (n, 3, L, L)).astype(F32))
    u8 = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (1, L, L, 3)).astype(np.uint8))
    lr[n - 1] = pkg("diffusion").lr_to_tensor(u8)[0]
    # each request alone, repeated over the session's 4 rows (every step of the session runs at B = slots)
    want = []
    for i, (held, s, cont) in enumerate(plan):
        x4 = x[i:i + 1].expand(slots, -1, -1, -1).contiguous()
        i4 = img[i:i + 1].expand(slots, -1, -1, -1).contiguous()
        netG.set_lr_consistency(lr[i:i + 1] if held else None)
        kw = {} if s is None else {"init": i4, "start": s}
        if cont:
            out, frames = netG.sample_batch(x4, True, seed=seed, image_offset=i, **kw)
            want.append(torch.cat([x[i:i + 1], frames[:, 0]], dim=0))
            assert torch.equal(frames[-1, 0], out[0])
        else:
            want.append(netG.super_resolution_batch(x4, seed=seed, image_offset=i, **kw)[0])
    netG.set_lr_consistency(None)
    torch.cuda.synchronize()

    def source():
        for i, (held, s, cont) in enumerate(plan):
            rq = {"x_in_row": x[i], "init": None if s is None else img[i], "strength": s, "continous": cont}
            if held:
                rq["lr"] = u8[0] if held == "u8" else lr[i]
            yield rq

    with netG.rolling(slots, seed=seed) as rs:
        got = dict(rs.stream(source()))
        assert rs.restarts == 0
        # a later request with another LR size
        with pytest.raises(ValueError, match="one LR size"):
            rs.submit(x[0], lr=torch.zeros(3, 4, 4))
    torch.cuda.synchronize()
    assert sorted(got) == list(range(n))
    for i, (held, s, cont) in enumerate(plan):
        assert got[i].shape == want[i].shape and _bytes(got[i]) == _bytes(want[i]), \
            f"request {i} (lr {held}, strength {s}, continous {cont}): max abs difference {float((got[i] - want[i]).abs().max()):.3e}"
    # the held results downsample to their LR images, within the bar of the uniform test; the others do not
    final = torch.stack([got[i][-1] if plan[i][2] else got[i] for i in range(n)])
    score = pkg("validation").lr_consistency(netG, final, lr)["max_abs"]
    is_held = np.array([bool(p[0]) and p[1] is None for p in plan])         # (a warm start of few steps is held as well, but
    assert score[is_held].max() <= BAR_OP                                  #  only the full runs are scored against the bar)
    assert score[[i for i, p in enumerate(plan) if not p[0]]].min() > BAR_OP
    # a session begun without an lr is not armed: a later lr is refused, naming lr_size; lr_size arms it from the start
    with netG.rolling(slots, seed=seed) as rs:
        rs.submit(x[1], image_id=1)
        with pytest.raises(ValueError, match="lr_size"):
            rs.submit(x[0], lr=lr[0])
        assert _bytes(dict(rs.drain())[0]) == _bytes(want[1])
    with netG.rolling(slots, seed=seed, lr_size=(L, L)) as rs:
        rs.submit(x[1], image_id=1)
        rs.submit(x[0], lr=lr[0], image_id=0)
        out = dict(rs.drain())
        assert _bytes(out[0]) == _bytes(want[1]) and _bytes(out[1]) == _bytes(want[0])
    # the per-call setting is still refused by name, and the uniform sampler is what it was
    netG.set_lr_consistency(lr[:1])
    with pytest.raises(Sr3Error, match="set_lr_consistency"):
        netG.rolling(slots)
    netG.set_lr_consistency(None)
    x4 = x[1:2].expand(slots, -1, -1, -1).contiguous()
    assert torch.equal(netG.super_resolution_batch(x4, seed=seed, image_offset=1)[0], want[1])
    torch.cuda.synchronize()


def test_range_trip_restarts_a_held_request_with_its_lr_image():
    """The recipe of test_gpu_rolling.py::test_range_trip_restarts_the_requests_in_flight (activations beyond the fp8
    operand range at the batch from which the fp8 path runs): held requests served in f16f8 trip the check, restart in
    f16x3 and come back as the bytes of the uniform f16x3 call under set_lr_consistency; an unheld one next to them as
    those of the call without."""
    import torch
    cfg = synth.yml_unet_config(224)
    sd = synth.synth_state_dict(cfg, 3)
    name = next(k for k, v in sd.items() if k.startswith("downs.") and k.endswith("res_block.block2.block.0.weight") and v.shape == (256,))
    sd[name] = sd[name] * F32(400.0)
    netG = roll._netG(synth.yml_opt(16, 128, 3), sd)
    netG.eval()
    netG.denoise_fn.precision = "f16x3"
    B, seed, n = 64, 7, 8
    x = torch.from_numpy(synth.synth_cond(B, 128, 16, 5)).cuda()
    lr = torch.from_numpy(np.random.RandomState(11).uniform(-1, 1, (B, 3, 16, 16)).astype(F32))
    free = netG.super_resolution_batch(x, seed=seed)
    netG.set_lr_consistency(lr)
    held = netG.super_resolution_batch(x, seed=seed)
    netG.set_lr_consistency(None)
    assert float((held - free).abs().max()) > 1e-3
    rs = netG.rolling(B, seed=seed)
    rs.set_precision("f16f8")
    for i in range(n):
        rs.submit(x[i], **({} if i == 3 else {"lr": lr[i]}))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = dict(rs.drain())
    assert any(issubclass(w.category, Sr3RangeWarning) for w in rec)
    assert rs.restarts == 1 and rs.precision == "f16x3"
    for i in range(n):
        assert torch.equal(got[i], free[i] if i == 3 else held[i]), i
    rs.close()
    torch.cuda.synchronize()
