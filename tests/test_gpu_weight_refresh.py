"""The device route of the weight refresh (sr3_load_weights_dev) against the host route (sr3_load_weight +
prepare_fused). Both routes perform the same arithmetic in the same order, so every comparison here is BITWISE: the kernel
layouts an engine keeps of every parameter (Engine.read_weight_layout), the split-f16 scales, and the outputs of the
forward and of the sampler. There is no tolerance anywhere in this file.

Shapes: every forward that only has to make the engines build their on-demand layouts (fused products, F8C copies) runs one
image at 16x16, the smallest size the five-level configs take. The rows of test_forward_* are the issue's."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")
schedule = pkg("schedule")
engine_mod = pkg("engine")
Engine = engine_mod.Engine

SEEDS = {"tiny": 41, "B": 42, "C": 43, "D": 44, "yml224": 45}
LAYOUTS = sorted(Engine.WEIGHT_LAYOUTS, key=Engine.WEIGHT_LAYOUTS.get)


def _cfg(name):
    if name == "tiny":
        return synth.tiny_unet_config()
    if name.startswith("yml"):
        return synth.yml_unet_config(int(name[3:]))
    return synth.sweep_unet_config(name)


@functools.lru_cache(maxsize=None)
def _weights(name):
    return synth.synth_state_dict(_cfg(name), SEEDS[name])


def _host_engine(cfg, sd):
    e = Engine(cfg, 0)
    e.load_state_dict(sd)
    assert e.weights_missing() == 0
    return e


def _device_load(e, sd, names=None):
    """One load_weights_device call for `names` (default: every parameter) from CUDA tensors."""
    names = [n for n, _ in e.param_list()] if names is None else list(names)
    tensors = [(n, torch.from_numpy(sd[n]).cuda()) for n in names]
    assert e.load_weights_device(tensors) == len(names)
    e.synchronize()


def _device_engine(cfg, sd):
    e = Engine(cfg, 0)
    _device_load(e, sd)
    assert e.weights_missing() == 0
    return e


def _tiny_forward(e, cfg, seed, prec="f16f8"):
    x, nl = synth.synth_unet_input(cfg, 1, 16, 16, seed)
    e.set_precision(prec)
    return e.unet_forward_np(x, nl.reshape(-1))


def _compare_layouts(h, d, what):
    """Every layout of every parameter: the same size in both engines, the same bytes, the same unscale factor."""
    seen = {k: 0 for k in LAYOUTS}
    for name, _ in h.param_list():
        assert h.weight_unscale(name) == d.weight_unscale(name), (what, name)
        for lay in LAYOUTS:
            a, b = h.read_weight_layout(name, lay), d.read_weight_layout(name, lay)
            assert (a is None) == (b is None), (what, name, lay)
            if a is None:
                continue
            assert a.size == b.size, (what, name, lay, a.size, b.size)
            if not np.array_equal(a, b):
                bad = np.flatnonzero(a != b)
                raise AssertionError(f"{what}: {name} [{lay}]: {bad.size} of {a.size} bytes differ, first at {bad[0]}")
            seen[lay] += 1
    return seen


def _mutations(cfg_name, sd):
    """The in-place changes of the issue, as {name: new array}: three conv tensors scaled by 1.5 (the first conv, the final
    conv and an Upsample conv: the edge layouts and the phase planes), a fused conv2 with max|w| < 2^-5 (its res_conv is
    NOT refreshed: the partner is split again with the common exponent), an identity-skip conv2 with max|w| < 2^-5 where the
    configuration has one (the k <= 15 rule), a res_conv weight and a res_conv bias alone, one conv tensor of zeros and
    one of negative values only."""
    names = list(sd)
    convs = [n for n in names if sd[n].ndim == 4]
    out = {}
    ups = [n for n in convs if n.startswith("ups.") and n.endswith(".conv.weight")]
    for n in (convs[0], convs[-1], ups[0]):
        out[n] = sd[n] * np.float32(1.5)
    c2 = [n for n in convs if n.endswith(".block2.block.3.weight")]
    has_res = lambda n: n.replace("block2.block.3.weight", "res_conv.weight") in sd
    fused = [n for n in c2 if has_res(n)]
    ident = [n for n in c2 if not has_res(n) and sd[n].shape[0] <= 128 and sd[n].shape[0] % 32 == 0]
    small = lambda a: (a / np.abs(a).max() * np.float32(0.03)).astype(np.float32)       # max|w| = 0.03 < 2^-5
    out[fused[0]] = small(sd[fused[0]])
    if ident:
        out[ident[0]] = small(sd[ident[0]])
    if len(fused) > 1:
        out[fused[1].replace("block2.block.3.weight", "res_conv.weight")] = \
            sd[fused[1].replace("block2.block.3.weight", "res_conv.weight")] * np.float32(3.0)
        out[fused[-1].replace("block2.block.3.weight", "res_conv.bias")] = \
            sd[fused[-1].replace("block2.block.3.weight", "res_conv.bias")] + np.float32(0.25)
    c1 = [n for n in convs if n.endswith(".block1.block.3.weight")]
    out[c1[0]] = np.zeros_like(sd[c1[0]])
    out[c1[-1]] = -np.abs(sd[c1[-1]]) - np.float32(1e-3)
    assert all(np.isfinite(v).all() and v.dtype == np.float32 for v in out.values())
    assert (out[c1[-1]] < 0).all() and np.abs(out[fused[0]]).max() < 2.0 ** -5
    return out


@pytest.mark.parametrize("name", ["tiny", "B", "C", "D", "yml224"])
def test_every_layout_of_every_parameter(name):
    cfg, sd = _cfg(name), _weights(name)
    h, d = _host_engine(cfg, sd), _device_engine(cfg, sd)
    np.testing.assert_array_equal(_tiny_forward(h, cfg, 1), _tiny_forward(d, cfg, 1))
    seen = _compare_layouts(h, d, f"{name}, full load")
    print(f"{name}: layouts compared after the full load: {seen}")
    expect = {"tiny": ("conv_in", "final_mfma", "ident"), "B": (), "C": ("ident", "wino", "conv_in", "final_mfma", "final_valu"),
              "D": ("wino", "final_mfma", "final_valu"), "yml224": ("wino", "conv_in", "final_mfma", "final_valu")}[name]
    for lay in ("plain", "split", "f8", "fused_bias") + expect:
        assert seen[lay], (lay, seen)

    new = _mutations(name, sd)
    sd2 = dict(sd)
    sd2.update(new)
    _device_load(d, sd2, list(new))
    for n, v in new.items():
        h.load_weight(n, v)
    np.testing.assert_array_equal(_tiny_forward(h, cfg, 2), _tiny_forward(d, cfg, 2))
    seen = _compare_layouts(h, d, f"{name}, partial refresh")
    print(f"{name}: layouts compared after refreshing {len(new)} tensors: {seen}")
    if name == "C":
        # the identity-skip conv2 with max|w| = 0.03 would scale by 2^16: capped to 2^15, which the identity matrix holds
        idn = [n for n in new if n.endswith("block2.block.3.weight") and d.read_weight_layout(n, "ident") is not None]
        assert idn and d.weight_unscale(idn[0]) == 2.0 ** -15
    h.close()
    d.close()


ROWS = [("D", (4, 32, 32), ("f32", "f16x3", "f16f8")), ("C", (2, 64, 96), ("f32", "f16x3")), ("C", (32, 64, 64), ("f32",))]


@pytest.mark.parametrize("name", ["D", "C"])
def test_forward_equal_and_refresh_under_use(name):
    """The issue's forward rows, then a refresh of the engine that ran them against a fresh host-loaded engine."""
    cfg, sd = _cfg(name), _weights(name)
    h, d = _host_engine(cfg, sd), _device_engine(cfg, sd)
    rows = [(shape, modes) for c, shape, modes in ROWS if c == name]
    for (B, H, W), modes in rows:
        x, nl = synth.synth_unet_input(cfg, B, H, W, SEEDS[name] + B)
        if B == 32:
            assert engine_mod.conv_plan(B, H, W, 64, 64, precision="f32", stats=True)["needs_wino_frag"]
        for prec in modes:
            h.set_precision(prec)
            d.set_precision(prec)
            np.testing.assert_array_equal(h.unet_forward_np(x, nl.reshape(-1)), d.unet_forward_np(x, nl.reshape(-1)),
                                          err_msg=f"{name} {B}x{H}x{W} [{prec}]")
    if name == "C":
        frag = [n for n, _ in d.param_list() if d.read_weight_layout(n, "wino_frag") is not None]
        assert frag, "the one-pass Winograd kernel's fragment-major copies were not made"
    h.close()
    # every tensor changes; the engine that ran the rows above (workspace, on-demand layouts) is refreshed in one call
    sd2 = {k: (v * np.float32(0.75) if v.ndim == 4 else v + np.float32(0.01)) for k, v in sd.items()}
    _device_load(d, sd2)
    fresh = _host_engine(cfg, sd2)
    (B, H, W), modes = rows[-1]
    x, nl = synth.synth_unet_input(cfg, B, H, W, SEEDS[name] + B)
    for prec in modes:
        fresh.set_precision(prec)
        d.set_precision(prec)
        np.testing.assert_array_equal(fresh.unet_forward_np(x, nl.reshape(-1)), d.unet_forward_np(x, nl.reshape(-1)),
                                      err_msg=f"after the refresh: {name} {B}x{H}x{W} [{prec}]")
    _compare_layouts(fresh, d, f"{name}, refresh under use")
    fresh.close()
    d.close()


@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16f8"])
def test_sampler_after_refresh_of_an_engine_with_captured_graphs(prec):
    """B = 2, T = 4 on the tiny configuration with a fixed seed: the engine samples (its step graph is captured from the
    second step on), is refreshed on the device, and samples again — equal to a fresh host-loaded engine. A graph that
    survived the refresh would replay the old w_unscale scalars."""
    cfg, sd = _cfg("tiny"), _weights("tiny")
    bufs = schedule.schedule_buffers({"schedule": "linear", "n_timestep": 4, "linear_start": 1e-4, "linear_end": 0.3})
    cond = synth.synth_cond(2, 16, 8, 3)

    def sample(e):
        e.set_precision(prec)
        with np.errstate(divide="ignore", invalid="ignore"):
            e.set_schedule(bufs)
        return e.sample_np(cond, seed=1234)

    d = _device_engine(cfg, sd)
    h = _host_engine(cfg, sd)
    first = sample(d)
    np.testing.assert_array_equal(first, sample(h))
    h.close()
    sd2 = dict(sd)
    for n, v in sd.items():
        if v.ndim == 4:
            sd2[n] = v * np.float32(4.0)          # another exponent for every conv
    _device_load(d, sd2, [n for n, v in sd.items() if v.ndim == 4])
    fresh = _host_engine(cfg, sd2)
    got, want = sample(d), sample(fresh)
    assert not np.array_equal(got, first)
    np.testing.assert_array_equal(got, want)
    fresh.close()
    d.close()


def _unet(cfg):
    return pkg("unet").UNet(in_channel=cfg.in_channel, out_channel=cfg.out_channel, inner_channel=cfg.inner_channel,
                            norm_groups=cfg.norm_groups, channel_mults=cfg.channel_mults, attn_res=cfg.attn_res,
                            res_blocks=cfg.res_blocks, dropout=cfg.dropout, image_size=cfg.image_size)


def test_tied_facade_refreshes_exactly_what_the_optimiser_changed():
    cfg, sd = _cfg("tiny"), _weights("tiny")
    m = _unet(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.cuda()
    f = _unet(cfg).cuda()
    f.tie_weights(m)
    assert f.weight_sync == "device"
    x, nl = synth.synth_unet_input(cfg, 2, 16, 16, 9)
    x, nl = torch.from_numpy(x).cuda(), torch.from_numpy(nl).cuda()

    def fresh_host_route():
        u = _unet(cfg)
        u.load_state_dict({k: v.detach().cpu().float() for k, v in m.state_dict().items()})
        u.cuda()
        assert u.weight_sync == "host"
        y = u(x, nl)
        assert u.last_refreshed_on_device == [] and len(u.last_refreshed) == len(sd)
        return y.cpu().numpy()

    y0 = f(x, nl).cpu().numpy()
    assert sorted(f.last_refreshed_on_device) == sorted(sd)
    np.testing.assert_array_equal(y0, fresh_host_route())
    f(x, nl)
    assert f.last_refreshed == []

    # an optimiser step on exactly three parameters of the module that owns them
    params = dict(m.named_parameters())
    three = ["downs.0.weight", [n for n in params if n.endswith("res_conv.weight")][0],
             [n for n in params if n.endswith("block2.block.0.bias")][0]]
    g = torch.Generator(device="cuda").manual_seed(5)
    for n in three:
        params[n].grad = torch.randn(params[n].shape, device="cuda", generator=g)
    torch.optim.SGD(m.parameters(), lr=0.05).step()
    y1 = f(x, nl).cpu().numpy()
    assert sorted(f.last_refreshed) == sorted(three) == sorted(f.last_refreshed_on_device)
    assert not np.array_equal(y1, y0)
    np.testing.assert_array_equal(y1, fresh_host_route())

    # a parameter moved to the CPU and one cast to fp64 take the host route, and the result still matches
    moved = [n for n in params if n.endswith("block1.block.3.weight")][0]
    cast = [n for n in params if n.endswith("block2.block.3.bias")][0]
    with torch.no_grad():
        params[moved].data = (params[moved].data * 1.25).cpu()
        params[cast].data = (params[cast].data + 0.5).double()
    y2 = f(x, nl).cpu().numpy()
    assert sorted(f.last_refreshed) == sorted([moved, cast]) and f.last_refreshed_on_device == []
    assert not np.array_equal(y2, y1)
    np.testing.assert_array_equal(y2, fresh_host_route())


def test_refresh_allocates_nothing_after_the_first():
    cfg, sd = _cfg("yml224"), _weights("yml224")
    e = Engine(cfg, 0)
    names = [n for n, _ in e.param_list()]
    tensors = [(n, torch.from_numpy(sd[n]).cuda()) for n in names]
    e.load_weights_device(tensors)
    _tiny_forward(e, cfg, 1)
    sizes = []
    for _ in range(2):
        e.load_weights_device(tensors)
        _tiny_forward(e, cfg, 1)
        sizes.append(e.device_bytes())
    assert sizes[0] == sizes[1], sizes
    e.close()


def test_routes_mixed_on_one_engine():
    """Both routes on the same engine: prepare_fused has to run for blocks whose tensors came by the device route (whose
    host copies were dropped), and a device refresh has to re-split a partner that came by the host route."""
    name = "C"
    cfg, sd = _cfg(name), _weights(name)
    h = _host_engine(cfg, sd)
    d = Engine(cfg, 0)
    names = [n for n, _ in d.param_list()]
    _device_load(d, sd, names[0::2])            # every block gets tensors from both routes
    for n in names[1::2]:
        d.load_weight(n, sd[n])
    assert d.weights_missing() == 0
    np.testing.assert_array_equal(_tiny_forward(h, cfg, 1), _tiny_forward(d, cfg, 1))
    _compare_layouts(h, d, "alternating routes")

    new = _mutations(name, sd)
    for i, (n, v) in enumerate(new.items()):    # the changes of the first test, alternating routes again
        h.load_weight(n, v)
        if i % 2:
            d.load_weight(n, v)
        else:
            _device_load(d, {n: v}, [n])
    np.testing.assert_array_equal(_tiny_forward(h, cfg, 2), _tiny_forward(d, cfg, 2))
    _compare_layouts(h, d, "alternating routes, partial refresh")
    # and back: the host-loaded ones by the device route, the others by the host route
    for i, (n, v) in enumerate(new.items()):
        w = (v * np.float32(0.5)).astype(np.float32)
        h.load_weight(n, w)
        if i % 2:
            _device_load(d, {n: w}, [n])
        else:
            d.load_weight(n, w)
    np.testing.assert_array_equal(_tiny_forward(h, cfg, 3), _tiny_forward(d, cfg, 3))
    _compare_layouts(h, d, "alternating routes, swapped")
    h.close()
    d.close()
