"""The one-pass Winograd kernel reads its own fragment-major copy of the transformed weights (ConvParams::w_wino_f):
  * near the block-count gate (B = 8 at 128x128, B = 16 at 64x64) its error against a float64 oracle stays within twice
    the direct kernel's, with residual, FeatureWiseAffine bias and both levels;
  * the engine makes the copy on the device when a workspace plan first runs a conv at a one-pass shape, and
    sr3_load_weight refreshes it: new weights loaded after a forward give bit for bit the forward of an engine that
    had them from the start."""
import json

import numpy as np
import pytest

from conftest import REPO, pkg
from test_gpu_winograd_fused import CHECK_IMAGES, _OPS_CHILD, _child

pytestmark = pytest.mark.gpu

# (B, H, W, C0, C1, Cout, resid, chan_bias): smallest batches the one-pass kernel takes at each level
GATE_SHAPES = [
    (8, 128, 128, 64, 0, 64, 1, 1), (8, 128, 128, 192, 0, 64, 0, 1),
    (16, 64, 64, 128, 0, 128, 1, 0), (16, 64, 64, 64, 0, 128, 0, 1), (16, 64, 64, 384, 0, 128, 1, 1),
]


def test_fused_winograd_gate_batches_error_vs_direct(tmp_path):
    images = sorted(set(min(i, 7) for i in CHECK_IMAGES))
    src = _OPS_CHILD.format(root=REPO, shapes=GATE_SHAPES, images=images)
    errs = {}
    for off in (False, True):
        line = [l for l in _child(tmp_path, src, off, "gate_%d" % off).splitlines() if l.startswith("ERRS")][-1]
        errs[off] = json.loads(line[5:])
    for shape, wino, direct in zip(GATE_SHAPES, errs[False], errs[True]):
        print(f"{shape}: winograd {wino:.3e}  direct {direct:.3e}  ratio {wino / direct:.2f}")
    for shape, wino, direct in zip(GATE_SHAPES, errs[False], errs[True]):
        assert wino <= 2.0 * direct, (shape, wino, direct)


def test_fused_weights_follow_a_reload():
    synth, Engine = pkg("synth"), pkg("engine").Engine
    cfg = synth.yml_unet_config(128)
    B = 16
    x = synth.synth_noise(1, B, 6, 128, 128, 4)[0]
    nl = np.linspace(0.2, 0.9, B).astype(np.float32)
    e = Engine(cfg, 0)
    e.set_precision("f32")
    e.load_state_dict(synth.synth_state_dict(cfg, 9))
    first = e.unet_forward_np(x, nl)                  # plans the workspace: copies made from the loaded weights
    e.load_state_dict(synth.synth_state_dict(cfg, 10))
    reloaded = e.unet_forward_np(x, nl)
    e.close()
    f = Engine(cfg, 0)
    f.set_precision("f32")
    f.load_state_dict(synth.synth_state_dict(cfg, 10))
    fresh = f.unet_forward_np(x, nl)
    f.close()
    assert np.isfinite(reloaded).all()
    assert not np.array_equal(first, reloaded)
    assert np.array_equal(reloaded, fresh)
