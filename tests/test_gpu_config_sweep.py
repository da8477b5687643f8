"""UNet forward on configurations and input shapes no fixture reaches, against the float64 run of the aten oracle
(oracle/sr3_oracle_aten.unet_forward(dtype=torch.float64); pinned to reference-made forwards of the same
configurations by tests/test_oracle_golden.py::test_sweep_configs_match_reference).

What the rows are for (kernel names: profiles/r10_sweep_kernel_trace.txt lists what this file launches):
  A  norm_groups 8 over 32/64/96 channels: 160- and 96+64-channel concatenations whose 20-channel groups straddle the
     two sources of the two-source GroupNorm routes; 96-channel convs; attention over 240 and 960 tokens at 48x80
     (tiled core; in the f16 modes 960 tokens is the f32 core between split-f16 convs) and over 3840 tokens at 96x160
     (streaming core)
  B  inner_channel 96, norm_groups 16: groups of 6 and 12 channels, 192-channel attention, one ResnetBlock per level
  C  multipliers (1,1,2,2,4): identity-skip ResnetBlocks on the down path, five levels, three ResnetBlocks per level;
     B = 32 at 64x64 is exactly WINO_FUSED_MIN_BLOCKS blocks of the one-pass Winograd kernel (32 * 32 * 1 * 1) in f32
  D  unconditional (in_channel == out_channel); B = 4 at 32x32 is exactly WINO_MIN_TILES tiles at the 16x16 level
  yml 224 at 96x96, 192x64, 64x128 and yml 128 at 256x256 / 192x256: non-square and non-power-of-two levels of the yml
     ladder (24x24, 12x12, 6x6; 48x16, 12x4; F8C at 16x32), attention over 1024 and 768 tokens

Bars are the project's: f32 and f16x3 1e-4 max-abs (tests/test_gpu_unet.py, TOL), f16f8 5e-4 (tests/test_gpu_f16f8.py);
an image forwarded alone equals the same image of the batch to 2e-5 (tests/test_gpu_sweep.py). Outputs are O(1)
(max |y| ~ 3, std ~ 0.6); the float32 CPU oracle is within 2.4e-6 of the float64 one on these cases."""
import functools

import numpy as np
import pytest
import torch

import sr3_oracle_aten as aten
from conftest import pkg

pytestmark = pytest.mark.gpu
synth = pkg("synth")

TOL = {"f32": 1e-4, "f16x3": 1e-4, "f16f8": 5e-4}
ALONE_TOL = 2e-5

ALL3 = ("f32", "f16x3", "f16f8")
F2 = ("f32", "f16x3")
# config, (B, H, W), distinct images (None: every image is its own), modes
ROWS = [
    ("A", (3, 48, 80), None, ALL3),
    ("A", (64, 48, 80), None, ALL3),
    ("A", (2, 96, 160), None, ALL3),            # 3840 tokens at the 48x80 level: streaming core
    ("B", (5, 24, 40), None, F2),
    ("B", (48, 24, 40), None, F2),
    ("C", (2, 64, 96), None, F2),
    ("C", (32, 64, 64), None, F2),
    ("D", (4, 32, 32), None, ALL3),
    ("D", (40, 32, 32), None, ALL3),
    ("yml224", (20, 96, 96), None, F2),
    ("yml224", (12, 192, 64), None, F2),
    ("yml224", (64, 64, 128), 2, ("f16f8", "f16x3")),      # two distinct images, alternating
    ("yml128", (1, 256, 256), None, ALL3),
    ("yml128", (1, 192, 256), None, ALL3),
]
CASES = [(c, s, d, m) for c, s, d, modes in ROWS for m in modes]
SEEDS = {"A": 31, "B": 32, "C": 33, "D": 34, "yml224": 35, "yml128": 36}


def _cfg(name):
    if name.startswith("yml"):
        return synth.yml_unet_config(int(name[3:]))
    return synth.sweep_unet_config(name)


@functools.lru_cache(maxsize=None)
def _weights(name):
    return synth.synth_state_dict(_cfg(name), SEEDS[name])


@functools.lru_cache(maxsize=None)
def _inputs(name, shape, distinct):
    """x, per-image noise levels, and the float64 oracle's output for the distinct images of the row."""
    cfg = _cfg(name)
    B, H, W = shape
    n = distinct or B
    x, nl = synth.synth_unet_input(cfg, n, H, W, SEEDS[name] + B)
    sd64 = aten.to_torch_state(_weights(name), torch.float64)
    with torch.no_grad():
        want = aten.unet_forward(sd64, cfg, torch.from_numpy(x), torch.from_numpy(nl), dtype=torch.float64).numpy()
    assert want.dtype == np.float64
    return x, nl.reshape(-1), want


@pytest.mark.parametrize("name,shape,distinct,prec", CASES,
                         ids=[f"{c}-{s[0]}x{s[1]}x{s[2]}-{m}" for c, s, _, m in CASES])
def test_forward_against_float64_oracle(name, shape, distinct, prec):
    cfg = _cfg(name)
    B, H, W = shape
    x, nl, want = _inputs(name, shape, distinct)
    if distinct:
        idx = np.arange(B) % distinct
        x, nl, want = x[idx], nl[idx], want[idx]
    e = pkg("engine").Engine(cfg, 0)
    e.load_state_dict(_weights(name))
    assert e.weights_missing() == 0
    e.set_precision(prec)
    got = e.unet_forward_np(x, nl)
    again = e.unet_forward_np(x, nl)
    alone = [(i, e.unet_forward_np(x[i:i + 1], nl[i:i + 1])[0]) for i in sorted({0, B - 1})]
    assert e.fallback_calls() == 0
    e.close()
    err = np.abs(got - want).reshape(B, -1).max(1)                   # every image of the batch
    d_alone = [float(np.abs(a - got[i]).max()) for i, a in alone]
    print(f"config {name} B={B} {H}x{W} [{prec}]: max abs err vs float64 oracle {err.max():.3e} (image {int(err.argmax())}); "
          f"alone vs batch {max(d_alone):.3e}")
    assert got.shape == want.shape and np.isfinite(got).all()
    assert err.max() <= TOL[prec], (name, shape, prec, err)
    np.testing.assert_array_equal(again, got)                        # a second call reproduces the first bit for bit
    if distinct:
        for i in range(distinct, B):                                 # replicated images: bit-identical outputs
            np.testing.assert_array_equal(got[i], got[i % distinct], err_msg=f"replica {i}")
    assert max(d_alone) <= ALONE_TOL, (name, shape, prec, d_alone)
