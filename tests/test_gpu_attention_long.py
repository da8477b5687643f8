"""Self-attention over more than 1024 tokens (the streaming core): the op against a float64 oracle,
the forced streaming entry against the tiled core on the same shapes, the reference-made fixture of a UNet whose
attention runs over 4624 and 1156 tokens, the yml UNets at output sizes whose attention level passes 1024 tokens,
sampler runs of the fixture's config, and the largest batch sr3_max_batch reports at 1024 x 1024."""
import numpy as np
import pytest

import fast_sampler_ref as ref
import sr3_oracle as oracle
import sr3_oracle_aten as aten
from conftest import cfg_from_meta, load_golden, pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
schedule = pkg("schedule")
samplers = pkg("samplers")
OP_TOL = 2e-5           # test_gpu_ops.test_attention's bar
UNET_TOL = 1e-4         # test_gpu_unet's bar
BAR = 1e-3              # the sampler tests' bar


def _rand(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


def _attention64(qkv, rows=512):
    """softmax(q k^T / sqrt(C)) v in float64, 512 query rows at a time."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    q, k, v = (qkv[..., i * C:(i + 1) * C].astype(np.float64) for i in range(3))
    out = np.empty((B, N, C))
    for b in range(B):
        for r0 in range(0, N, rows):
            s = q[b, r0:r0 + rows] @ k[b].T / np.sqrt(C)
            s = np.exp(s - s.max(-1, keepdims=True))
            out[b, r0:r0 + rows] = (s / s.sum(-1, keepdims=True)) @ v[b]
    return out


@pytest.fixture(scope="module")
def eng():
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    e.load_state_dict(synth.synth_state_dict(e.cfg, 11))
    yield e
    e.close()


@pytest.mark.parametrize("B,N,C", [(1, 1025, 32), (2, 1300, 64), (1, 2304, 512), (2, 4096, 256), (1, 8192, 64)])
def test_op_attention_long(eng, B, N, C):
    qkv = _rand(np.random.RandomState(B * 7 + N + C), B, N, 3 * C)
    got = eng.op_attention(qkv)
    err = np.abs(got - _attention64(qkv)).max()
    print(f"B={B} N={N} C={C}: max abs err {err:.2e}")
    assert err <= OP_TOL
    # every precision mode runs the exact-f32 streaming core over 1024 tokens
    eng.set_precision("f16x3")
    try:
        np.testing.assert_array_equal(eng.op_attention(qkv), got)
    finally:
        eng.set_precision("f32")


def test_op_attention_long_peaked_softmax(eng):
    """N = 4096: a sharply peaked query row, a query whose scores are all equal (across every tile boundary), one key
    dominating a late tile for one query (its running max jumps), and a key raised for every query."""
    B, N, C = 1, 4096, 128
    rs = np.random.RandomState(5)
    qkv = _rand(rs, B, N, 3 * C)
    qkv[0, 5, :C] *= 40.0
    qkv[0, 7, :C] = 0.0
    qv = qkv[0, 100, :C]
    qkv[0, 3001, C:2 * C] = 40.0 * np.sqrt(C) * qv / np.dot(qv, qv)     # score 40 for query 100
    qkv[0, 2050, C:2 * C] += 0.5
    got = eng.op_attention(qkv)
    want = _attention64(qkv)
    err = np.abs(got - want).max()
    print(f"peaked N={N}: max abs err {err:.2e}")
    assert err <= 5e-5            # test_gpu_ops.test_attention_peaked_softmax's bar
    np.testing.assert_allclose(got[0, 7], qkv[0, :, 2 * C:].astype(np.float64).mean(0), atol=2e-5, rtol=0)


@pytest.mark.parametrize("N", [1, 31, 33, 1024])
@pytest.mark.parametrize("B,C", [(2, 64), (1, 512), (3, 160)])
def test_forced_streaming_entry(eng, B, N, C):
    """sr3_op_attention_stream at token counts the tiled core also takes: both against the oracle and each other."""
    qkv = _rand(np.random.RandomState(N + C), B, N, 3 * C)
    got = eng.op_attention(qkv, streaming=True)
    tiled = eng.op_attention(qkv)
    want = _attention64(qkv)
    assert np.abs(got - want).max() <= OP_TOL
    assert np.abs(tiled - want).max() <= OP_TOL
    assert np.abs(got - tiled).max() <= OP_TOL


def test_streaming_core_rejects_unsupported_channels(eng):
    Sr3Error = pkg("_lib").Sr3Error
    with pytest.raises(Sr3Error, match="512"):
        eng.op_attention(np.zeros((1, 8, 3 * 544), np.float32), streaming=True)
    with pytest.raises(Sr3Error, match="512"):
        eng.op_attention(np.zeros((1, 1100, 3 * 544), np.float32))


@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16f8"])
def test_unet_forward_fixture_long_attention(prec):
    """tests/golden/unet_attn_long.npz: the reference's forward at 68 x 68 with attention over 4624 tokens (C = 32)
    and over 1156 tokens in the mid block (C = 64)."""
    g = load_golden("unet_attn_long.npz")
    cfg = cfg_from_meta(g["meta"])
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(synth.synth_state_dict(cfg, g["meta"]["seed"]))
    e.set_precision(prec)
    eps = e.unet_forward_np(g["x"], g["noise_level"])
    err = np.abs(eps - g["eps"]).max()
    print(f"unet_attn_long [{prec}]: max abs err vs reference {err:.3e}")
    assert err < UNET_TOL
    np.testing.assert_array_equal(e.unet_forward_np(g["x"], g["noise_level"]), eps)
    e.close()


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("image_size,r", [(224, 576), (128, 512)])
def test_yml_unet_large_outputs(image_size, r, prec):
    """The yml UNet at 576^2 (mid-block attention over 36 x 36 = 1296 tokens, C = 512) and the image_size=128 variant
    at 512^2 (attention over 64 x 64 = 4096 tokens at C = 512), B = 1, against the aten oracle on the CPU with the
    same synthetic weights."""
    import torch
    cfg = synth.yml_unet_config(image_size)
    sd = synth.synth_state_dict(cfg, 31)
    rs = np.random.RandomState(r + image_size)
    x = rs.standard_normal((1, 6, r, r)).astype(np.float32)
    nl = np.array([0.42], np.float32)
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_precision(prec)
    got = e.unet_forward_np(x, nl)
    e.close()
    with torch.no_grad():
        want = aten.unet_forward(aten.to_torch_state(sd), cfg, torch.from_numpy(x), torch.from_numpy(nl)).numpy()
    err = np.abs(got - want).max()
    print(f"yml image_size={image_size} at {r}^2 [{prec}]: max abs err vs aten oracle {err:.3e}")
    assert err < UNET_TOL


@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16f8"])
def test_sampler_long_attention(prec):
    """T = 3 DDPM of the fixture's config at 68 x 68, B = 2, injected noise, against the oracle's p_sample_loop."""
    cfg = cfg_from_meta(load_golden("unet_attn_long.npz")["meta"])
    sd = synth.synth_state_dict(cfg, 23)
    B, r, T = 2, 68, 3
    sched = {"schedule": "linear", "n_timestep": T, "linear_start": 1e-4, "linear_end": 2e-2}
    cond = synth.synth_cond(B, r, 17, 23)
    noise = synth.synth_noise(T, B, 3, r, r, 23)
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_precision(prec)
    with np.errstate(divide="ignore", invalid="ignore"):
        e.set_schedule(schedule.schedule_buffers(sched))
        want_f, want_fr = oracle.p_sample_loop(sd, cfg, oracle.noise_schedule(sched), cond, noise)
    got_f, got_fr = e.sample_np(cond, noise=noise, frames=True)
    e.close()
    err = np.abs(got_fr - want_fr).reshape(want_fr.shape[0], -1).max(1)
    print(f"ddpm T={T} at {r}^2 [{prec}]: per-frame max abs err {np.array2string(err, precision=2)}")
    assert err.max() <= BAR
    assert np.abs(got_f - want_f).max() <= BAR


def test_ddim_long_attention():
    """DDIM at S = 2 over the same shape against the few-step restatement."""
    cfg = cfg_from_meta(load_golden("unet_attn_long.npz")["meta"])
    sd = synth.synth_state_dict(cfg, 29)
    B, r, S = 2, 68, 2
    sched = {"schedule": "linear", "n_timestep": 20, "linear_start": 1e-4, "linear_end": 2e-2}
    cond = synth.synth_cond(B, r, 17, 29)
    noise = synth.synth_noise(S, B, 3, r, r, 29)
    with np.errstate(divide="ignore", invalid="ignore"):
        bufs = schedule.schedule_buffers(sched)
    want_f, want_fr = ref.sample_loop(sd, cfg, sched, cond, noise, "ddim", S, 0.0)
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(sd)
    e.set_sampler_schedule(samplers.sampler_tables(bufs, "ddim", S, 0.0))
    got_f, got_fr = e.sample_np(cond, noise=noise, frames=True)
    e.close()
    err = np.abs(got_fr - want_fr).reshape(want_fr.shape[0], -1).max(1)
    print(f"ddim S={S} at {r}^2: per-frame max abs err {np.array2string(err, precision=2)}")
    assert err.max() <= BAR


def test_yml_unet_1024_at_max_batch():
    """The yml UNet at 1024^2 (mid block over 64 x 64 = 4096 tokens) with B = sr3_max_batch(1024, 1024): the call
    runs, and its image 0 equals a B = 1 run to test_gpu_sweep's bar."""
    cfg = synth.yml_unet_config(224)
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(synth.synth_state_dict(cfg, 37))
    Bmax = e.max_batch(1024, 1024)
    assert Bmax >= 1
    rs = np.random.RandomState(37)
    x = rs.standard_normal((Bmax, 6, 1024, 1024)).astype(np.float32)
    nl = rs.uniform(0.05, 1.0, Bmax).astype(np.float32)
    full = e.unet_forward_np(x, nl)
    alone = e.unet_forward_np(x[:1], nl[:1])
    e.close()
    assert np.isfinite(full).all()
    d = float(np.abs(full[0] - alone[0]).max())
    print(f"1024^2: B = {Bmax}, image 0 vs B = 1: {d:.2e}")
    assert d <= 2e-5
