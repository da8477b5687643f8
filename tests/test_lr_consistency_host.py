"""Low-resolution consistency, host side: the operators of sr3_lr_operators_host against a float64
restatement of Pillow's real bicubic weights, the algebra of the pseudo-inverse, and the facade's argument handling.
Needs the built library, no GPU."""
import math

import numpy as np
import pytest

import lr_consistency_ref as ref
import pil_bicubic
from conftest import pkg

PAIRS = [(4, 16), (8, 16), (8, 24), (10, 24), (16, 128), (128, 1024)]


@pytest.fixture(scope="module", params=PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def ops(request):
    l, r = request.param
    A, P = pkg("engine").lr_operators(l, r)
    return l, r, A, P


def test_A_is_pillows_real_weights(ops):
    l, r, A, _ = ops
    want, bounds = ref.real_coeffs(r, l)
    assert A.shape == (l, r) and float(np.abs(A - want).max()) <= 1e-12
    # the zero pattern is the bounds of the fixed-point oracle (the same precompute_coeffs)
    b, _, ksize = pil_bicubic.precompute_coeffs(r, l)
    assert ksize == 2 * math.ceil(2 * r / l) + 1
    inside = np.zeros((l, r), dtype=bool)
    for i in range(l):
        assert tuple(b[i]) == tuple(bounds[i]) and b[i][1] <= ksize
        inside[i, b[i][0]:b[i][0] + b[i][1]] = True
    assert not A[~inside].any()
    # (inside its bounds a weight is zero only where the kernel has a root: the ends of the support)
    assert np.abs(A[inside]).max() > 0


def test_rows_of_A_sum_to_one(ops):
    l, _, A, _ = ops
    err = max(abs(math.fsum(A[i]) - 1.0) for i in range(l))
    print(f"max |row sum - 1| = {err:.2e}")
    assert err <= 1e-15


def test_P_is_the_pseudo_inverse(ops):
    l, r, A, P = ops
    assert P.shape == (r, l)
    e_inv = float(np.abs(A @ P - np.eye(l)).max())
    PA = P @ A
    e_sym = float(np.abs(PA - PA.T).max())
    e_idem = float(np.abs(PA @ PA - PA).max())
    e_ref = float(np.abs(P - ref.operators(l, r)[1]).max())
    cond = float(np.linalg.cond(A @ A.T))
    print(f"{l}->{r}: |AP - I| {e_inv:.1e}, P A symmetric {e_sym:.1e}, idempotent {e_idem:.1e}, |P - numpy| {e_ref:.1e}, cond(AA^T) {cond:.2f}")
    assert e_inv <= 1e-12 and e_sym <= 1e-12 and e_idem <= 1e-12 and e_ref <= 1e-12
    assert cond < 3.0


def test_operator_arguments_are_checked():
    Sr3Error = pkg("_lib").Sr3Error
    for l, r in ((0, 8), (8, 8), (16, 8)):
        with pytest.raises(Sr3Error):
            pkg("engine").lr_operators(l, r)


def test_reference_projection_is_consistent_and_idempotent():
    """The float64 reference the GPU tests are held to does what it says."""
    rs = np.random.RandomState(5)
    x = np.clip(rs.standard_normal((3, 3, 24, 24)), -1, 1)
    y = rs.uniform(-1, 1, (2, 3, 10, 10))
    p = ref.project(x, y, row_offset=1)
    assert ref.residual(p, y, row_offset=1)["max_abs"].max() <= 1e-13
    assert np.abs(ref.project(p, y, row_offset=1) - p).max() <= 1e-13
    np.testing.assert_allclose(ref.project(x, y, 1, 0.5), 0.5 * (x + p), rtol=0, atol=1e-15)
    assert ref.residual(x, y, row_offset=1)["max_abs"].min() > 0.1


def test_uint8_lr_maps_as_the_dataset_does():
    import torch
    diffusion = pkg("diffusion")
    u8 = np.arange(256, dtype=np.uint8)
    u8 = np.concatenate([u8, u8[::-1], np.roll(u8, 7)]).reshape(1, 16, 16, 3)
    u8 = np.concatenate([u8, 255 - u8])
    got = diffusion.lr_to_tensor(torch.from_numpy(u8))
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 16, 16) and got.is_contiguous()
    want = np.stack([pil_bicubic.to_tensor_pm1(u8[i]) for i in range(2)])
    np.testing.assert_array_equal(got.numpy(), want)
    f = torch.from_numpy(want)
    assert diffusion.lr_to_tensor(f) is f or torch.equal(diffusion.lr_to_tensor(f), f)
    for bad in (torch.zeros(2, 16, 16, 4, dtype=torch.uint8), torch.zeros(2, 3, 16, 16, dtype=torch.float64),
                torch.zeros(3, 16, 16)):
        with pytest.raises(RuntimeError):
            diffusion.lr_to_tensor(bad)


def test_facade_setting_is_configuration_only():
    import torch
    synth = pkg("synth")
    cfg = synth.tiny_unet_config()
    sched = {"schedule": "linear", "n_timestep": 12, "linear_start": 1e-4, "linear_end": 2e-2}
    opt = {"phase": "val", "sr": {"model": {
        "which_model_G": "sr3",
        "unet": {"in_channel": 6, "out_channel": 3, "inner_channel": cfg.inner_channel,
                 "channel_multiplier": list(cfg.channel_mults), "attn_res": list(cfg.attn_res),
                 "res_blocks": cfg.res_blocks, "dropout": 0.0},
        "beta_schedule": {"train": sched, "val": sched},
        "diffusion": {"image_size": cfg.image_size, "channels": 3, "conditional": True}}}}
    netG = pkg().define_G(opt)
    netG.set_new_noise_schedule(sched, torch.device("cpu"))
    keys = list(netG.state_dict())
    lr = torch.zeros(2, 3, 8, 8)
    netG.set_lr_consistency(lr, 0.75)
    assert netG._lr[1] == 0.75 and list(netG.state_dict()) == keys
    netG.set_sampler("ddim", steps=4)
    netG.set_new_noise_schedule(dict(sched, n_timestep=20), torch.device("cpu"))
    assert netG._lr is not None and netG._lr[0] is lr and list(netG.state_dict()) == keys
    netG.set_lr_consistency(lr, 0.0)
    assert netG._lr is None
    netG.set_lr_consistency(torch.zeros(2, 8, 8, 3, dtype=torch.uint8))
    assert tuple(netG._lr[0].shape) == (2, 3, 8, 8) and netG._lr[1] == 1.0
    netG.set_lr_consistency(None)
    assert netG._lr is None
    with pytest.raises(ValueError):
        netG.set_lr_consistency(lr, 1.5)
    with pytest.raises(RuntimeError):
        netG.set_lr_consistency(torch.zeros(2, 1, 8, 8))


def test_validate_batch_argument_checks():
    import torch
    validation = pkg("validation")
    sr = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match="hr"):
        validation.validate_batch(None, sr, None)
    with pytest.raises(ValueError, match="lr holds 3"):
        validation.validate_batch(None, sr, None, lr=torch.zeros(3, 3, 8, 8))
    with pytest.raises(ValueError, match="metrics"):
        validation.validate_batch(None, sr, None, lr=torch.zeros(2, 3, 8, 8), metrics="gpu")
    with pytest.raises(RuntimeError):
        validation.validate_batch(None, sr, None, lr=torch.zeros(2, 3, 8, 8, dtype=torch.float64))
