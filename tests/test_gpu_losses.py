"""The SR3 denoising loss on the device (sr3_denoise_loss / sr3_op_q_sample, GaussianDiffusion.q_sample / p_losses / forward,
validation.loss_by_level) against torch's CPU expressions, the library's own two-step path, float64 numpy sums, and the
reference's p_losses (tests/golden/losses_tiny.npz, made by tests/golden/make_golden_losses.py and pinned on the host by
tests/test_losses_host.py).

Bars. q_sample and the state the UNet reads are BIT-equal to their yardsticks (the same fp32 operations in the same order).
The reduction differs from a float64 numpy sum of the same fp32 terms only in summation order: 1e-12 relative (at most a few
thousand terms of one sign, each addition within 2^-53 relative). Against the reference the bar is the project's 1e-3 per
element (BASELINE.json north_star). In f32 a row's result does not depend on the batch it sits in, so rows of calls with
different batch sizes (a shard, a chunk, one level of loss_by_level) are held BIT-equal to the rows of the whole call.
"""
import warnings

import numpy as np
import pytest

from conftest import cfg_from_meta, load_golden, pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
validation = pkg("validation")
_lib = pkg("_lib")
Sr3Error, Sr3RangeWarning = _lib.Sr3Error, _lib.Sr3RangeWarning

MODES = ["f32", "f16x3", "f16f8"]
BAR = 1e-3
S20 = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}


def _opt(cfg, sched, conditional=True, dropout=0.0):
    return {"phase": "val", "sr": {"model": {
        "which_model_G": "sr3",
        "unet": {"in_channel": cfg.in_channel, "out_channel": cfg.out_channel, "inner_channel": cfg.inner_channel,
                 "channel_multiplier": list(cfg.channel_mults), "attn_res": list(cfg.attn_res),
                 "res_blocks": cfg.res_blocks, "dropout": dropout},
        "beta_schedule": {"train": sched, "val": sched},
        "diffusion": {"image_size": cfg.image_size, "channels": 3, "conditional": conditional}}}}


def _net(cfg, sched, seed, conditional=True, dropout=0.0, sd=None, loss="l1"):
    import torch
    netG = pkg().define_G(_opt(cfg, sched, conditional, dropout)).cuda()
    sd = synth.synth_state_dict(cfg, seed) if sd is None else sd
    netG.load_state_dict({"denoise_fn." + k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        netG.set_new_noise_schedule(sched, [0])
    netG.loss_type = loss
    netG.set_loss(0)
    netG.denoise_fn.precision = "f32"
    return netG.eval()


@pytest.fixture(scope="module")
def nets():
    """Networks by key, built on first use and closed with the module."""
    made = {}

    def get(key, build):
        if key not in made:
            made[key] = build()
        return made[key]
    yield get
    for n in made.values():
        if n.denoise_fn._engine is not None:
            n.denoise_fn._engine.close()


@pytest.fixture(scope="module")
def tiny(nets):
    return nets("tiny", lambda: _net(synth.tiny_unet_config(), S20, 21))


@pytest.fixture(scope="module")
def golden():
    return load_golden("losses_tiny.npz")


def _s_of(levels):
    """(a, s) as fp32 CPU tensors, s = sqrt(1 - a^2) in correctly rounded fp32 operations (diffusion.py:281; numpy, because
    torch's CPU sqrt is 1 ulp off on some hosts — the fixture comes from one where it is not)."""
    import torch
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.float32).reshape(-1))
    sv = np.sqrt(np.float32(1) - lv * lv)
    assert sv.dtype == np.float32 and sv.tobytes() == pkg("diffusion").noise_coefficient(lv).tobytes()
    return torch.from_numpy(lv), torch.from_numpy(sv)


def _unaligned(t):
    """The same values in a CUDA tensor that starts 4 bytes behind a 16-byte boundary (the kernels' scalar path)."""
    import torch
    flat = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda")
    v = flat[1:1 + t.numel()].view(t.shape).copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _raw(netG, hr, sr, levels, loss="l1", noise=None, per_source=False, seed=0, image_offset=0, row_offset=0,
         unaligned_out=False):
    """sr3_denoise_loss itself on torch tensors: (per_image fp64 [B], x_noisy [B,3,H,W], eps [B,3,H,W]) as numpy."""
    import torch
    unet = netG.denoise_fn
    eng = netG._engine()
    lv, sv = _s_of(levels)
    B = lv.numel()
    N, C, H, W = hr.shape
    lv, sv = lv.cuda(), sv.cuda()
    per = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    xn = torch.full((B, C, H, W), float("nan"), dtype=torch.float32, device="cuda")
    ep = torch.full((B, C, H, W), float("nan"), dtype=torch.float32, device="cuda")
    if unaligned_out:
        xn, ep = _unaligned(xn), _unaligned(ep)
    unet.ready()
    eng.denoise_loss(hr.data_ptr(), sr.data_ptr() if sr is not None else None, N, row_offset, lv.data_ptr(), sv.data_ptr(),
                     B, H, W, per.data_ptr(), loss, noise.data_ptr() if noise is not None else None, per_source, seed,
                     image_offset, xn.data_ptr(), ep.data_ptr())
    unet.finish()
    return per.cpu().numpy(), xn.cpu().numpy(), ep.cpu().numpy()


def _images(N, r, seed):
    import torch
    hr = torch.from_numpy(synth.synth_cond(N, r, max(r // 2, 2), seed + 1000)).cuda()
    sr = torch.from_numpy(synth.synth_cond(N, r, max(r // 4, 2), seed)).cuda()
    return hr, sr


def _host_sums(noise, eps, loss):
    d = noise.astype(np.float32) - eps.astype(np.float32)                    # fp32 difference, like torch
    terms = np.abs(d) if loss == "l1" else d * d                             # fp32 square
    assert terms.dtype == np.float32
    return terms.astype(np.float64).reshape(terms.shape[0], -1).sum(axis=1)


# ---- 1. q_sample ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(5, 7), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_q_sample_op_is_bit_equal_to_the_torch_expression(tiny, size):
    """B = 3 rows over N = 2 images from row_offset = 1, levels 1.0, near 0 and one between; 5x7 takes the scalar form of the
    kernel (H*W % 4 != 0), 16x16 the 16-byte one. Slab per row, slab per source image, and Philox against the slab
    sr3_philox_normal makes for the same (seed, image, draw 0)."""
    import torch
    H, W = size
    B, N, off = 3, 2, 1
    rs = np.random.RandomState(H * W)
    hr = rs.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)
    noise = rs.standard_normal((B, 3, H, W)).astype(np.float32)
    lv, sv = _s_of([1.0, 1e-4, 0.37])
    idx = [(off + b) % N for b in range(B)]
    a, s = lv.view(-1, 1, 1, 1), sv.view(-1, 1, 1, 1)

    def want(nz):
        return (a * torch.from_numpy(hr[idx]) + s * torch.from_numpy(nz)).numpy()          # diffusion.py:279-282

    eng = tiny.denoise_fn.engine()
    d_hr, d_lv, d_sv = torch.from_numpy(hr).cuda(), lv.cuda(), sv.cuda()

    def run(noise_t=None, per_source=False, seed=0, image_offset=0):
        out = torch.full((B, 3, H, W), float("nan"), dtype=torch.float32, device="cuda")
        tiny.denoise_fn.ready()
        eng.q_sample(d_hr.data_ptr(), N, off, d_lv.data_ptr(), d_sv.data_ptr(), B, 3, H, W, out.data_ptr(),
                     noise_t.data_ptr() if noise_t is not None else None, per_source, seed, image_offset)
        tiny.denoise_fn.finish()
        return out.cpu().numpy()

    got = run(torch.from_numpy(noise).cuda())
    assert got.tobytes() == want(noise).tobytes()
    assert got[0].tobytes() == hr[idx[0]].tobytes()                          # level 1.0: the image itself
    src = run(torch.from_numpy(noise[:N]).cuda(), per_source=True)
    assert src.tobytes() == want(noise[:N][idx]).tobytes()
    seed, io = 20261017, 5
    slab = np.stack([eng.philox_normal(seed, io + b, 0, 3 * H * W).reshape(3, H, W) for b in range(B)])
    assert run(None, seed=seed, image_offset=io).tobytes() == want(slab).tobytes()
    slab_src = np.stack([eng.philox_normal(seed, io + n, 0, 3 * H * W).reshape(3, H, W) for n in idx])
    assert run(None, per_source=True, seed=seed, image_offset=io).tobytes() == want(slab_src).tobytes()
    # the facade member: one level per image, the reference's call shape (diffusion.py:299-300)
    x = torch.from_numpy(hr[idx]).cuda()
    q = tiny.q_sample(x_start=x, continuous_sqrt_alpha_cumprod=lv.cuda().view(-1, 1, 1, 1), noise=torch.from_numpy(noise).cuda())
    assert q.is_cuda and q.cpu().numpy().tobytes() == want(noise).tobytes()
    with pytest.raises(Sr3Error, match="bad size"):
        eng.q_sample(d_hr.data_ptr(), 0, 0, d_lv.data_ptr(), d_sv.data_ptr(), B, 3, H, W, d_hr.data_ptr())
    with pytest.raises(Sr3Error, match="null"):
        eng.q_sample(None, N, 0, d_lv.data_ptr(), d_sv.data_ptr(), B, 3, H, W, d_hr.data_ptr())


# ---- 2. the fused state against the two-step path ---------------------------------------------------------------------
@pytest.mark.parametrize("r", [16, 24])
@pytest.mark.parametrize("mode", MODES)
def test_fused_state_equals_the_two_step_path_bitwise(tiny, mode, r):
    """eps of sr3_denoise_loss == denoise_fn(cat([sr, x_noisy_out]), levels) bit for bit: the state kernel leaves the same
    bits in the UNet's input (and in its packed split-f16 twin, which 16x16 has and 24x24 has not) as the layout change +
    packing of sr3_unet_forward, and the same kernels run on them."""
    import torch
    tiny.denoise_fn.precision = mode
    try:
        hr, sr = _images(2, r, r)
        B = 3
        noise = torch.from_numpy(synth.synth_noise(1, B, 3, r, r, r)[0]).cuda()
        levels = np.array([0.93, 0.41, 0.08], np.float32)
        per, xn, eps = _raw(tiny, hr, sr, levels, noise=noise, row_offset=1)
        idx = [(1 + b) % 2 for b in range(B)]
        x = torch.cat([sr[idx], torch.from_numpy(xn).cuda()], dim=1)
        two = tiny.denoise_fn(x, torch.from_numpy(levels).cuda().view(B, 1)).cpu().numpy()
        assert np.isfinite(eps).all() and eps.tobytes() == two.tobytes()
        a, s = (t.view(-1, 1, 1, 1) for t in _s_of(levels))
        want_xn = (a * hr[idx].cpu() + s * noise.cpu()).numpy()
        assert xn.tobytes() == want_xn.tobytes()
    finally:
        tiny.denoise_fn.precision = "f32"


# ---- 3. the reduction -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unaligned", [False, True], ids=["vec", "scalar"])
@pytest.mark.parametrize("loss", ["l1", "l2"])
def test_reduction_matches_float64_numpy_and_repeats_bitwise(tiny, loss, unaligned):
    """48x48: three blocks per image in the 16-byte form of the loss kernel, nine in the scalar form (tensors that do not
    start on 16 bytes)."""
    import torch
    r, B = 48, 3
    hr, sr = _images(2, r, 7)
    noise = torch.from_numpy(synth.synth_noise(1, B, 3, r, r, 7)[0]).cuda()
    if unaligned:
        noise = _unaligned(noise)
    levels = [0.9, 0.5, 0.2]
    per, xn, eps = _raw(tiny, hr, sr, levels, loss=loss, noise=noise, unaligned_out=unaligned)
    want = _host_sums(noise.cpu().numpy(), eps, loss)
    rel = np.abs(per - want) / want
    print(f"loss reduction {loss} {'scalar' if unaligned else 'vec'}: per_image {per}, rel to float64 numpy {rel.max():.2e}")
    assert np.isfinite(per).all() and (want > 0).all()
    assert rel.max() <= 1e-12
    per2, xn2, eps2 = _raw(tiny, hr, sr, levels, loss=loss, noise=noise, unaligned_out=unaligned)
    assert per.tobytes() == per2.tobytes() and eps.tobytes() == eps2.tobytes() and xn.tobytes() == xn2.tobytes()
    # both forms of the kernels compute the same state and the same terms
    if unaligned:
        per_v, xn_v, eps_v = _raw(tiny, hr, sr, levels, loss=loss, noise=noise.clone())
        assert xn.tobytes() == xn_v.tobytes() and eps.tobytes() == eps_v.tobytes()
        assert (np.abs(per - per_v) / want).max() <= 1e-12


def test_p_losses_is_the_fp32_of_the_per_image_sum(tiny):
    import torch
    hr, sr = _images(3, 16, 3)
    noise = torch.from_numpy(synth.synth_noise(1, 3, 3, 16, 16, 3)[0]).cuda()
    np.random.seed(11)
    loss = tiny.p_losses({"HR": hr, "SR": sr}, noise=noise)
    per = tiny.last_loss_per_image
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    assert loss.grad_fn is None and not loss.requires_grad
    assert per.dtype == torch.float64 and tuple(per.shape) == (3,) and per.is_cuda
    assert torch.equal(loss, per.sum().to(torch.float32))
    assert abs(float(loss) - per.cpu().numpy().sum()) <= 2.0 ** -23 * float(loss)       # one fp32 rounding
    # the levels are the reference's draws under the same np.random.seed
    np.random.seed(11)
    _, lv = pkg().draw_levels(tiny.sqrt_alphas_cumprod_prev, tiny.num_timesteps, 3)
    per_raw, _, _ = _raw(tiny, hr, sr, lv, noise=noise)
    assert per_raw.tobytes() == per.cpu().numpy().tobytes()


# ---- 4. against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_loss_matches_the_reference(nets, golden, case, mode):
    import torch
    m = golden["cases"][case]
    g = {k[len(f"c{case}."):]: v for k, v in golden.items() if k.startswith(f"c{case}.")}
    cfg = cfg_from_meta(m)
    netG = nets(("golden", m["seed"], m["conditional"], m["r"]),
                lambda: _net(cfg, m["schedule"], m["seed"], conditional=m["conditional"]))
    netG.loss_type = m["loss_type"]
    netG.set_loss(0)
    netG.denoise_fn.precision = mode
    try:
        hr, sr, noise = (torch.from_numpy(g[k]).cuda() for k in ("HR", "SR", "noise"))
        np.random.seed(m["np_seed"])
        loss = netG({"HR": hr, "SR": sr}, noise=noise)
        n_el = g["HR"].size
        err = abs(float(loss) - float(g["loss"])) / n_el
        per, xn, eps = _raw(netG, hr, sr if m["conditional"] else None, g["levels"], loss=m["loss_type"], noise=noise)
        e_eps = float(np.abs(eps - g["x_recon"]).max())
        print(f"losses_tiny case {case} [{mode}]: loss {float(loss):.4f} vs reference {float(g['loss']):.4f}: "
              f"|d| / (b c h w) = {err:.2e}; max |eps - x_recon| = {e_eps:.2e}")
        assert err <= BAR
        assert xn.tobytes() == g["x_noisy"].tobytes()                        # the reference's q_sample, bit for bit
        assert e_eps <= BAR
        assert per.tobytes() == netG.last_loss_per_image.cpu().numpy().tobytes()
    finally:
        netG.denoise_fn.precision = "f32"


# ---- 5. Philox --------------------------------------------------------------------------------------------------------
def test_philox_noise_equals_the_injected_stream_and_follows_image_offset(tiny):
    import torch
    r, B, seed = 16, 7, 424242
    hr, sr = _images(B, r, 9)
    levels = np.linspace(0.95, 0.05, B).astype(np.float32)
    eng = tiny._engine()
    per, xn, eps = _raw(tiny, hr, sr, levels, seed=seed)
    slab = np.stack([eng.philox_normal(seed, b, 0, 3 * r * r).reshape(3, r, r) for b in range(B)])
    per_s, xn_s, eps_s = _raw(tiny, hr, sr, levels, noise=torch.from_numpy(slab).cuda())
    assert xn.tobytes() == xn_s.tobytes() and eps.tobytes() == eps_s.tobytes() and per.tobytes() == per_s.tobytes()
    assert per.tobytes() != _raw(tiny, hr, sr, levels, seed=seed + 1)[0].tobytes()
    # the scalar form of the kernels draws the same stream
    per_u, xn_u, _ = _raw(tiny, hr, sr, levels, seed=seed, unaligned_out=True)
    assert xn_u.tobytes() == xn.tobytes() and (np.abs(per_u - per) / per).max() <= 1e-12
    # a shard: rows 5..6 as a call of their own with image_offset = 5
    per_o, xn_o, eps_o = _raw(tiny, hr[5:].contiguous(), sr[5:].contiguous(), levels[5:], seed=seed, image_offset=5)
    assert xn_o.tobytes() == xn[5:].tobytes()
    # f32: a row's result does not depend on the batch it sits in (the shard runs B = 2, the whole call B = 7)
    assert eps_o.tobytes() == eps[5:].tobytes() and per_o.tobytes() == per[5:].tobytes()
    # the same shard through % N: rows 5..6 of the 7 images from row_offset = 5, no copy of the images
    per_r, xn_r, _ = _raw(tiny, hr, sr, levels[5:], seed=seed, image_offset=5, row_offset=5)
    assert xn_r.tobytes() == xn[5:].tobytes() and per_r.tobytes() == per_o.tobytes()


# ---- 6. range policy --------------------------------------------------------------------------------------------------
def _overflow_net():
    """The network of tests/test_gpu_round3.py: downs.0 scaled so that its output leaves the fp16 range."""
    cfg = synth.tiny_unet_config()
    sd = synth.synth_state_dict(cfg, 77)
    sd["downs.0.weight"] = sd["downs.0.weight"] * np.float32(3e5)
    return cfg, sd


def test_range_policy_finishes_in_f32_and_strict_mode_raises(nets):
    import torch
    cfg, sd = _overflow_net()
    netG = nets("overflow", lambda: _net(cfg, S20, 77, sd=sd))
    hr, sr = _images(2, 16, 5)
    noise = torch.from_numpy(synth.synth_noise(1, 2, 3, 16, 16, 5)[0]).cuda()
    levels = [0.3, 0.7]
    netG.denoise_fn.strict_range = False
    netG.denoise_fn.precision = "f32"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        want = _raw(netG, hr, sr, levels, noise=noise)
    netG.denoise_fn.precision = "f16x3"
    before = netG._engine().fallback_calls()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = _raw(netG, hr, sr, levels, noise=noise)
    assert any(issubclass(w.category, Sr3RangeWarning) and "exact f32" in str(w.message) for w in rec)
    assert netG._engine().fallback_calls() == before + 1
    assert np.isfinite(got[0]).all()
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    netG.denoise_fn.strict_range = True
    try:
        with pytest.raises(Sr3Error, match="fp16 range"):
            _raw(netG, hr, sr, levels, noise=noise)
    finally:
        netG.denoise_fn.strict_range = False
        netG.denoise_fn.precision = "f32"


def test_fp8_range_steps_down_to_f16x3_first(nets):
    """The f16f8 -> f16x3 rung of the loss entry. The network of tests/test_gpu_f16f8.py::test_fp8_range_falls_back_to_f16x3_first
    (yml-224 UNet, one block2 GroupNorm gamma of the 32x32 level x 400: |activation| ~ 1e3, beyond the fp8 operand range of
    448 and far inside the fp16 range) on 128x128 images, at the smallest batch at which the f16f8 mode puts the 256 -> 256
    convs of that level on the fp8 path."""
    import torch
    cfg = synth.yml_unet_config(224)
    sd = synth.synth_state_dict(cfg, 3)
    name = next(k for k, v in sd.items() if k.startswith("downs.") and k.endswith("res_block.block2.block.0.weight") and v.shape == (256,))
    sd[name] = sd[name] * np.float32(400.0)
    netG = nets("fp8_overflow", lambda: _net(cfg, S20, 3, sd=sd))
    eng = netG._engine()
    B = next((b for b in range(1, 64) if eng.conv_f8_supported(b, 32, 32, 256, 256)), 64)
    assert eng.conv_f8_supported(B, 32, 32, 256, 256)                        # the fp8 path runs, or the test shows nothing
    hr, sr = _images(2, 128, 23)
    noise = torch.from_numpy(synth.synth_noise(1, B, 3, 128, 128, 23)[0]).cuda()
    levels = np.linspace(0.9, 0.1, B).astype(np.float32)
    unet = netG.denoise_fn
    unet.strict_range = False
    try:
        unet.precision = "f16x3"
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            want = _raw(netG, hr, sr, levels, noise=noise)
        unet.precision = "f16f8"
        before = eng.fallback_calls()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got = _raw(netG, hr, sr, levels, noise=noise)
        hits = [w for w in rec if issubclass(w.category, Sr3RangeWarning)]
        print(f"f16f8 loss at B = {B}: {len(hits)} range warning(s): {[str(w.message)[:90] for w in hits]}; "
              f"fallback_calls {before} -> {eng.fallback_calls()}")
        assert len(hits) == 1 and "f16x3" in str(hits[0].message)
        assert eng.fallback_calls() == before + 1
        assert np.isfinite(got[0]).all()
        for a, b in zip(got, want):                                          # per-image losses, x_noisy, eps
            assert a.tobytes() == b.tobytes()
        # the mode was put back: an in-range call (two rows: no conv on the fp8 path) passes without a warning, and the
        # same out-of-range call is caught and counted again
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            small = _raw(netG, hr, sr, levels[:2], noise=noise[:2].contiguous())
        assert np.isfinite(small[0]).all() and eng.fallback_calls() == before + 1
        with pytest.warns(Sr3RangeWarning, match="f16x3"):
            again = _raw(netG, hr, sr, levels, noise=noise)
        assert again[0].tobytes() == want[0].tobytes() and eng.fallback_calls() == before + 2
        unet.strict_range = True
        with pytest.raises(Sr3Error, match="fp8 range"):
            _raw(netG, hr, sr, levels, noise=noise)
    finally:
        unet.strict_range = False
        unet.precision = "f32"


def test_bad_arguments_raise(tiny):
    import torch
    hr, sr = _images(2, 16, 1)
    eng = tiny._engine()
    lv, sv = _s_of([0.5, 0.5])
    lv, sv = lv.cuda(), sv.cuda()
    per = torch.zeros(2, dtype=torch.float64, device="cuda")
    ok = dict(hr_ptr=hr.data_ptr(), cond_ptr=sr.data_ptr(), N=2, row_offset=0, level_ptr=lv.data_ptr(), s_ptr=sv.data_ptr(),
              B=2, H=16, W=16, per_image_ptr=per.data_ptr())
    for key in ("hr_ptr", "level_ptr", "s_ptr", "per_image_ptr"):
        with pytest.raises(Sr3Error, match="null"):
            eng.denoise_loss(**dict(ok, **{key: None}))
    with pytest.raises(Sr3Error, match="N=0"):
        eng.denoise_loss(**dict(ok, N=0))
    with pytest.raises(Sr3Error, match="loss_type"):
        _lib.check(eng.lib.sr3_denoise_loss(eng.ctx, hr.data_ptr(), sr.data_ptr(), 2, 0, lv.data_ptr(), sv.data_ptr(), None, 0,
                                            0, 0, 2, 16, 16, 2, per.data_ptr(), None, None))
    with pytest.raises(Sr3Error, match="unconditional"):
        eng.denoise_loss(**dict(ok, cond_ptr=None))
    eng.denoise_loss(**ok)                                                   # and the context still works
    assert np.isfinite(per.cpu().numpy()).all()
    # host tensors never reach the library: the facade refuses them
    with pytest.raises(RuntimeError, match="must be on"):
        tiny.p_losses({"HR": hr.cpu(), "SR": sr})
    with pytest.raises(RuntimeError, match="must be on"):
        tiny.q_sample(hr.cpu(), lv)
    with pytest.raises(RuntimeError, match="must be on"):
        validation.loss_by_level(tiny, hr.cpu(), sr, 2)


# ---- 7. the facade ----------------------------------------------------------------------------------------------------
def test_facade_call_forms(tiny, nets):
    import torch
    P = pkg()
    r = 16
    hr, sr = _images(2, r, 13)
    x = {"HR": hr, "SR": sr}
    np.random.seed(5)
    torch.manual_seed(1)
    a = tiny(x)
    np.random.seed(5)
    torch.manual_seed(1)
    b = tiny(P.DictTensor(dict(x)))
    assert a.dim() == 0 and b.dim() == 0 and torch.equal(a, b) and float(a) > 0
    torch.manual_seed(2)
    assert not torch.equal(tiny(x), a)                                       # another level draw / another Philox seed
    # sr_out=True: the reference's ret_img[-1] of super_resolution(x['SR'])
    torch.manual_seed(3)
    img = tiny(P.DictTensor(dict(x)), sr_out=True)
    torch.manual_seed(3)
    want = tiny.super_resolution(sr)
    assert tuple(img.shape) == (3, r, r) and torch.equal(img, want)
    # l2 through set_loss; anything else raises
    net2 = nets("tiny_l2", lambda: _net(synth.tiny_unet_config(), S20, 21, loss="l2"))
    noise = torch.from_numpy(synth.synth_noise(1, 2, 3, r, r, 13)[0]).cuda()
    np.random.seed(6)
    l2 = net2(x, noise=noise)
    np.random.seed(6)
    l1 = tiny(x, noise=noise)
    np.random.seed(6)
    _, lv = P.draw_levels(tiny.sqrt_alphas_cumprod_prev, 20, 2)
    per, _, eps = _raw(tiny, hr, sr, lv, noise=noise)
    assert (np.abs(net2.last_loss_per_image.cpu().numpy() - _host_sums(noise.cpu().numpy(), eps, "l2")) /
            _host_sums(noise.cpu().numpy(), eps, "l2")).max() <= 1e-12
    assert float(l1) != float(l2)
    net2.loss_type = "huber"
    with pytest.raises(NotImplementedError):
        net2.set_loss(0)
    net2.loss_type = "l2"


def test_chunked_batch_equals_the_unchunked_one(tiny):
    """max_chunk = 2 at B = 5: three calls of two rows (the last one padded) against one call of five; Philox and the
    injected slab."""
    import torch
    hr, sr = _images(5, 16, 17)
    noise = torch.from_numpy(synth.synth_noise(1, 5, 3, 16, 16, 17)[0]).cuda()
    for kw in (dict(noise=noise), dict(seed=99, image_offset=3)):
        np.random.seed(8)
        whole = tiny.p_losses({"HR": hr, "SR": sr}, **kw)
        per_w = tiny.last_loss_per_image.cpu().numpy()
        np.random.seed(8)
        parts = tiny.p_losses({"HR": hr, "SR": sr}, max_chunk=2, **kw)
        per_c = tiny.last_loss_per_image.cpu().numpy()
        print(f"chunked vs unchunked per-image sums ({'slab' if 'noise' in kw else 'philox'}): {per_c} vs {per_w}")
        assert per_c.shape == (5,) and per_c.tobytes() == per_w.tobytes()
        assert torch.equal(whole, parts)


def test_train_mode_warns_once_that_dropout_is_the_identity(nets):
    import torch
    netG = nets("dropout", lambda: _net(synth.tiny_unet_config(), S20, 21, dropout=0.1))
    hr, sr = _images(1, 16, 2)
    netG.train()
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            np.random.seed(1)
            a = netG({"HR": hr, "SR": sr}, seed=4)
            np.random.seed(1)
            b = netG({"HR": hr, "SR": sr}, seed=4)
        hits = [w for w in rec if issubclass(w.category, UserWarning) and "dropout" in str(w.message)]
        assert len(hits) == 1 and torch.equal(a, b)
    finally:
        netG.eval()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        np.random.seed(1)
        assert torch.equal(netG({"HR": hr, "SR": sr}, seed=4), a)           # eval(): the same loss, no warning


# ---- 8. loss_by_level -------------------------------------------------------------------------------------------------
def test_loss_by_level_equals_separate_calls_and_keys_noise_by_source_image(tiny):
    import torch
    K, N, r = 4, 3, 16
    hr, sr = _images(N, r, 19)
    noise = torch.from_numpy(synth.synth_noise(1, N, 3, r, r, 19)[0]).cuda()
    res = validation.loss_by_level(tiny, hr, sr, K, noise=noise)
    prev = np.asarray(tiny.sqrt_alphas_cumprod_prev)[1:]
    assert res["levels"].dtype == np.float32 and res["levels"].tobytes() == prev[[0, 6, 13, 19]].astype(np.float32).tobytes()
    assert res["per_image"].shape == (K, N) and res["per_image"].dtype == np.float64 and res["loss"].shape == (K,)
    np.testing.assert_array_equal(res["loss"], res["per_image"].sum(axis=1) / (N * 3 * r * r))
    for k in range(K):
        per, _, _ = _raw(tiny, hr, sr, [res["levels"][k]] * N, noise=noise)
        assert per.tobytes() == res["per_image"][k].tobytes(), k
    assert (res["loss"][:-1] != res["loss"][1:]).all()
    # Philox: image i meets the stream (seed, i) at every level — the curve equals the one of the injected slab
    seed = 777
    eng = tiny._engine()
    slab = np.stack([eng.philox_normal(seed, i, 0, 3 * r * r).reshape(3, r, r) for i in range(N)])
    a = validation.loss_by_level(tiny, hr, sr, res["levels"], seed=seed)
    b = validation.loss_by_level(tiny, hr, sr, res["levels"], noise=torch.from_numpy(slab).cuda())
    assert a["per_image"].tobytes() == b["per_image"].tobytes()
    rows = tiny._loss_rows(hr, sr, torch.zeros(K * N), "l1", noise_per_source=True, seed=seed, want=("x_noisy",))
    xn = rows["x_noisy"].cpu().numpy().reshape(K, N, 3, r, r)               # level 0: x_noisy = 0 * x + 1 * noise
    for k in range(K):
        assert np.array_equal(xn[k], slab), k
    # chunked: the rows of a level may straddle two calls
    c = validation.loss_by_level(tiny, hr, sr, res["levels"], noise=noise, max_chunk=5)
    assert c["per_image"].tobytes() == res["per_image"].tobytes()
