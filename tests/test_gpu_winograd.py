"""Winograd F(2x2, 3x3) form of the exact-f32 3x3 convs (kernels_wino.hip): error against a float64 oracle no worse
than twice the direct kernel's on the same data, the whole UNet forward (fused 1x1 res_conv, residual, FeatureWiseAffine
bias, fused GroupNorm statistics of the next GroupNorm) against the direct path, and batch invariance.
The direct kernel's figures come from a child process with SR3_NO_WINOGRAD=1 (the switch is read once per process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, pkg

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, Cout, resid, chan_bias): every 3x3 stride-1 conv shape of the yml UNet at <= 32x32 pixels, B = 64
YML_SHAPES = [
    (64, 8, 8, 1024, 512, 0, 1), (64, 8, 8, 512, 512, 1, 0),
    (64, 16, 16, 1024, 512, 0, 1), (64, 16, 16, 256, 512, 0, 0), (64, 16, 16, 512, 512, 1, 1), (64, 16, 16, 768, 512, 0, 0),
    (64, 32, 32, 128, 256, 0, 1), (64, 32, 32, 256, 256, 1, 0), (64, 32, 32, 384, 256, 0, 0), (64, 32, 32, 512, 256, 0, 1),
    (64, 32, 32, 768, 256, 1, 1),
]
CHECK_IMAGES = [0, 63]      # rows compared against the float64 oracle (the arithmetic of a row does not depend on B)

_OPS_CHILD = r'''
import importlib, json, sys
import numpy as np
sys.path.insert(0, {root!r})
name = "3d-super-resolution-face-reconstruction_amd"
synth = importlib.import_module(name + ".synth")
Engine = importlib.import_module(name + ".engine").Engine
e = Engine(synth.tiny_unet_config(), 0)
e.set_precision("f32")
out = []
for (B, H, W, Cin, Cout, rs_, cb_) in {shapes!r}:
    rs = np.random.RandomState(Cin * 7 + Cout + H)
    x = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    cb = rs.standard_normal((B, Cout)).astype(np.float32) if cb_ else None
    res = rs.standard_normal((B, H, W, Cout)).astype(np.float32) if rs_ else None
    got = e.op_conv2d(x, w, b, chan_bias=cb, resid=res)
    err = 0.0
    for i in {images!r}:
        xp = np.pad(x[i].astype(np.float64), ((1, 1), (1, 1), (0, 0)))
        want = np.zeros((H * W, Cout))
        for dy in range(3):
            for dx in range(3):
                want += xp[dy:dy + H, dx:dx + W].reshape(-1, Cin) @ w[:, :, dy, dx].T.astype(np.float64)
        want = want.reshape(H, W, Cout) + b
        if cb is not None: want = want + cb[i]
        if res is not None: want = want + res[i]
        err = max(err, float(np.abs(got[i] - want).max()))
    out.append(err)
e.close()
print("ERRS", json.dumps(out))
'''

_FWD_CHILD = r'''
import importlib, sys
import numpy as np
sys.path.insert(0, {root!r})
name = "3d-super-resolution-face-reconstruction_amd"
synth = importlib.import_module(name + ".synth")
Engine = importlib.import_module(name + ".engine").Engine
cfg = synth.yml_unet_config(224)
e = Engine(cfg, 0)
e.load_state_dict(synth.synth_state_dict(cfg, 9))
e.set_precision("f32")
B = 64
x = synth.synth_noise(1, B, 6, 128, 128, 4)[0]
nl = np.linspace(0.2, 0.9, B).astype(np.float32)
np.save({path!r}, e.unet_forward_np(x, nl))
e.close()
'''


def _child(tmp_path, src, env_off, tag):
    script = tmp_path / f"{tag}.py"
    script.write_text(src)
    env = dict(os.environ)
    if env_off:
        env["SR3_NO_WINOGRAD"] = "1"
    else:
        env.pop("SR3_NO_WINOGRAD", None)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout


def test_winograd_op_error_vs_direct(tmp_path):
    src = _OPS_CHILD.format(root=REPO, shapes=YML_SHAPES, images=CHECK_IMAGES)
    errs = {}
    for off in (False, True):
        line = [l for l in _child(tmp_path, src, off, "ops_%d" % off).splitlines() if l.startswith("ERRS")][-1]
        errs[off] = json.loads(line[5:])
    for shape, wino, direct in zip(YML_SHAPES, errs[False], errs[True]):
        print(f"{shape}: winograd {wino:.3e}  direct {direct:.3e}  ratio {wino / direct:.2f}")
    for shape, wino, direct in zip(YML_SHAPES, errs[False], errs[True]):
        assert wino <= 2.0 * direct, (shape, wino, direct)


def test_winograd_unet_forward_matches_direct(tmp_path):
    """128x128 yml UNet forward at B = 64 (levels 32, 16, 8 in Winograd form): res_conv as the fused 1x1 term, residuals,
    FeatureWiseAffine biases, and every GroupNorm behind a Winograd conv fed by its fused statistics."""
    outs = {}
    for off in (False, True):
        path = str(tmp_path / ("fwd_%d.npy" % off))
        _child(tmp_path, _FWD_CHILD.format(root=REPO, path=path), off, "fwd_%d" % off)
        outs[off] = np.load(path)
    d = float(np.abs(outs[False] - outs[True]).max())
    print("forward max |winograd - direct| =", d)
    assert d <= 2e-5


@pytest.fixture(scope="module")
def eng():
    synth = pkg("synth")
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    e.set_precision("f32")
    yield e
    e.close()


def test_winograd_batch_invariance(eng):
    rs = np.random.RandomState(3)
    B, H, W, Cin, Cout = 64, 16, 16, 512, 512
    x = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    full = eng.op_conv2d(x, w, b)
    for i in (0, 17, 63):
        alone = eng.op_conv2d(x[i:i + 1], w, b)      # (one image: 64 tiles, below WINO_MIN_TILES: the direct kernel)
        assert np.abs(full[i] - alone[0]).max() <= 2e-5
    rep = eng.op_conv2d(np.repeat(x[5:6], B, axis=0), w, b)
    assert all(np.array_equal(rep[0], rep[i]) for i in range(1, B))
