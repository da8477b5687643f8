"""One-pass Winograd F(2x2, 3x3) kernel of the exact-f32 3x3 convs at 64x64 and 128x128 pixels (kernels_wino.hip,
wino_fused_kernel): error against a float64 oracle no worse than twice the direct kernel's on every such shape of the yml
UNet at B = 64, batch invariance and replicated rows. The fused 1x1 term and the fused GroupNorm statistics at these
levels are covered by the UNet forward of test_gpu_winograd.py against SR3_NO_WINOGRAD=1.
Concatenated inputs (x || skip) reach a conv as ONE tensor: the GroupNorm apply pass that writes the conv's input
concatenates them (the engine and op_conv2d alike), and the one-pass kernel takes no second tensor. The x1 shapes below
check that route against the oracle.
The direct kernel's figures come from a child process with SR3_NO_WINOGRAD=1 (the switch is read once per process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, pkg

pytestmark = pytest.mark.gpu

# (B, H, W, C0, C1, Cout, resid, chan_bias): the 3x3 stride-1 conv shapes of the yml UNet at 64x64 and 128x128 pixels
# (without the 6 -> 64 input conv, which stays direct), B = 64; C1 > 0: input given as x0 || x1
YML_SHAPES = [
    (64, 128, 128, 64, 0, 64, 1, 0), (64, 128, 128, 128, 0, 64, 0, 1), (64, 128, 128, 192, 0, 64, 1, 1),
    (64, 64, 64, 64, 0, 128, 0, 1), (64, 64, 64, 128, 0, 128, 1, 0), (64, 64, 64, 192, 0, 128, 0, 1),
    (64, 64, 64, 256, 0, 128, 1, 1), (64, 64, 64, 384, 0, 128, 0, 0),
    (64, 64, 64, 128, 64, 128, 0, 1), (64, 128, 128, 128, 64, 64, 1, 0),
]
CHECK_IMAGES = [0, 63]

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
for (B, H, W, C0, C1, Cout, rs_, cb_) in {shapes!r}:
    Cin = C0 + C1
    rs = np.random.default_rng(Cin * 7 + Cout + H + C1)
    x = rs.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    cb = rs.standard_normal((B, Cout), dtype=np.float32) if cb_ else None
    res = rs.standard_normal((B, H, W, Cout), dtype=np.float32) if rs_ else None
    if C1:
        got = e.op_conv2d(np.ascontiguousarray(x[..., :C0]), w, b, x1=np.ascontiguousarray(x[..., C0:]), chan_bias=cb, resid=res)
    else:
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


def test_fused_winograd_op_error_vs_direct(tmp_path):
    src = _OPS_CHILD.format(root=REPO, shapes=YML_SHAPES, images=CHECK_IMAGES)
    errs = {}
    for off in (False, True):
        line = [l for l in _child(tmp_path, src, off, "ops_%d" % off).splitlines() if l.startswith("ERRS")][-1]
        errs[off] = json.loads(line[5:])
    for shape, wino, direct in zip(YML_SHAPES, errs[False], errs[True]):
        print(f"{shape}: winograd {wino:.3e}  direct {direct:.3e}  ratio {wino / direct:.2f}")
    for shape, wino, direct in zip(YML_SHAPES, errs[False], errs[True]):
        assert wino <= 2.0 * direct, (shape, wino, direct)


@pytest.fixture(scope="module")
def eng():
    synth = pkg("synth")
    e = pkg("engine").Engine(synth.tiny_unet_config(), 0)
    e.set_precision("f32")
    yield e
    e.close()


@pytest.mark.parametrize("H, Cin, Cout", [(64, 128, 128), (128, 64, 64)])
def test_fused_winograd_batch_invariance(eng, H, Cin, Cout):
    rs = np.random.default_rng(5)
    B = 64
    x = rs.standard_normal((B, H, H, Cin), dtype=np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rs.standard_normal(Cout).astype(np.float32)
    full = eng.op_conv2d(x, w, b)
    for i in (0, 17, 63):
        alone = eng.op_conv2d(x[i:i + 1], w, b)      # (one image: too few blocks for the one-pass kernel: direct)
        assert np.abs(full[i] - alone[0]).max() <= 2e-5
    rep = eng.op_conv2d(np.repeat(x[5:6], B, axis=0), w, b)
    assert all(np.array_equal(rep[0], rep[i]) for i in range(1, B))
