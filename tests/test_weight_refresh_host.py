"""UNet.tie_weights / GaussianDiffusion.tie_weights on CPU modules: parameter sharing, key order and the errors. No GPU
and no library call (the device route itself: tests/test_gpu_weight_refresh.py)."""
import pytest
import torch
from torch import nn

from conftest import pkg

synth = pkg("synth")


def _unet(cfg):
    return pkg("unet").UNet(in_channel=cfg.in_channel, out_channel=cfg.out_channel, inner_channel=cfg.inner_channel,
                            norm_groups=cfg.norm_groups, channel_mults=cfg.channel_mults, attn_res=cfg.attn_res,
                            res_blocks=cfg.res_blocks, dropout=cfg.dropout, image_size=cfg.image_size)


def test_tie_weights_shares_the_parameter_objects_and_keeps_the_key_order():
    cfg = synth.tiny_unet_config()
    f, m = _unet(cfg), _unet(cfg)
    keys = list(f.state_dict())
    assert f.weight_sync == "host"
    f.tie_weights(m)
    assert f.weight_sync == "device"
    mine, theirs = dict(f.named_parameters()), dict(m.named_parameters())
    assert list(mine) == list(theirs) == keys == list(f.state_dict()) == list(m.state_dict())
    assert all(mine[k] is theirs[k] for k in keys)
    # what an optimiser does to the module is what the tied model holds, version counter included
    before = mine[keys[0]]._version
    with torch.no_grad():
        theirs[keys[0]].add_(1.0)
    assert mine[keys[0]]._version == before + 1
    assert torch.equal(f.state_dict()[keys[3]], m.state_dict()[keys[3]])
    with pytest.raises(ValueError):
        f.set_weight_sync("pinned")


def test_tie_weights_raises_on_a_missing_key_and_on_a_shape_mismatch():
    cfg = synth.tiny_unet_config()
    f, m = _unet(cfg), _unet(cfg)
    own = dict(f.named_parameters())
    name = [k for k in own if k.endswith("res_conv.weight")][0]
    parts = name.split(".")
    holder = m
    for p_ in parts[:-1]:
        holder = holder._modules[p_]
    saved = holder._parameters.pop(parts[-1])
    with pytest.raises(KeyError, match="res_conv.weight"):
        f.tie_weights(m)
    holder.register_parameter(parts[-1], nn.Parameter(saved.detach()[:, :-1].clone()))
    with pytest.raises(ValueError, match="res_conv.weight"):
        f.tie_weights(m)
    # a failed call ties nothing
    assert all(p is own[k] for k, p in f.named_parameters()) and f.weight_sync == "host"


def test_diffusion_tie_weights_goes_through_the_denoise_fn_prefix():
    cfg = synth.tiny_unet_config()
    diffusion = pkg("diffusion")
    ours = diffusion.GaussianDiffusion(_unet(cfg), image_size=16)

    class RefNetG(nn.Module):               # a trainer's module: the UNet under denoise_fn, and parameters of its own
        def __init__(self, unet):
            super().__init__()
            self.denoise_fn = unet
            self.other = nn.Parameter(torch.zeros(3))

    ref = RefNetG(_unet(cfg))
    ours.tie_weights(ref)
    a, b = dict(ours.denoise_fn.named_parameters()), dict(ref.denoise_fn.named_parameters())
    assert list(a) == list(b) and all(a[k] is b[k] for k in a)
    assert ours.denoise_fn.weight_sync == "device"
