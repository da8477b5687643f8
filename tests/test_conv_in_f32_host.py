"""The gate of the exact-f32 first-conv kernel (sr3_conv_in_f32_gate = conv_in_f32_gate of csrc/conv_plan.hip, what
run_unet_body's M_CONV_IN case and sr3_op_conv_in_f32 ask): over a grid of (Cin, Cout, H, W, precision) and both values of
SR3_NO_CONV_IN_F32 its answer is conv_in_supported's shape rule, restated here, and the precision rule (exact f32 only).
Host arithmetic only: no GPU. The switch is read once per process, so each value runs in a process of its own."""
import itertools
import json
import os
import subprocess
import sys

import pytest

from conftest import pkg

CINS = (1, 3, 6, 8, 9, 32)
COUTS = (16, 32, 48, 64, 96, 128)
SIZES = ((16, 16), (8, 32), (16, 48), (48, 80), (128, 128), (32, 24), (8, 16), (24, 24), (4, 64), (16, 8), (1, 256), (17, 16))
GRID = list(itertools.product(CINS, COUTS, SIZES, (0, 1, 2)))


def supported(cin, cout, h, w):
    """conv_in_supported (csrc/kernels_edge.hip)"""
    return cin <= 8 and cout in (32, 64) and w % 16 == 0 and (h * w) % 256 == 0


def answers():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = lib_mod.load()
    return [int(lib.sr3_conv_in_f32_gate(cin, cout, h, w, prec)) for cin, cout, (h, w), prec in GRID]


@pytest.mark.parametrize("switch", [None, "0", "1"], ids=["unset", "0", "1"])
def test_gate_is_the_shape_rule_the_precision_rule_and_the_switch(switch):
    env = dict(os.environ)
    env.pop("SR3_NO_CONV_IN_F32", None)
    if switch is not None:
        env["SR3_NO_CONV_IN_F32"] = switch
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = [int(switch != "1" and prec == 0 and supported(cin, cout, h, w)) for cin, cout, (h, w), prec in GRID]
    assert len(got) == len(GRID) and got == want, [g for g, a, b in zip(GRID, got, want) if a != b][:10]
    if switch != "1":           # the grid holds both answers, and the shapes the configurations run
        assert 0 < sum(want) < len(want)
        for cin, cout, hw in ((6, 64, (128, 128)), (6, 32, (16, 16)), (6, 32, (48, 80))):
            assert got[GRID.index((cin, cout, hw, 0))] == 1 and got[GRID.index((cin, cout, hw, 1))] == 0


if __name__ == "__main__":
    print(json.dumps(answers()))
