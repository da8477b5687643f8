#!/usr/bin/env python3
"""The exact-f32 first conv alone: conv_in_f32_kernel (Engine.op_conv_in_f32) against the generic implicit-GEMM kernel
on the 32 padded input channels (Engine.op_conv2d), the launch it replaces, alternating in one process.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/conv_in_bench.py [--shape 64 128 128 6 64]
    python3 tools/conv_in_bench.py --trace DIR/.../*_kernel_trace.csv

The single-op entry points own their buffers (upload, launch, read back), so the kernels' durations come from the
kernel trace of the run, not from a host timer: the second form groups the trace's dispatches of the two kernels into
the rounds of the first and prints mean / min / max per kernel and round."""
import argparse
import csv
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "3d-super-resolution-face-reconstruction_amd"
NEW, OLD = "conv_in_f32_kernel", "conv_igemm_dma_f32"


def run(shape, iters, rounds):
    engine = importlib.import_module(PKG + ".engine")
    synth = importlib.import_module(PKG + ".synth")
    B, H, W, Cin, Cout = shape
    rs = np.random.RandomState(0)
    state = rs.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    bias = rs.standard_normal(Cout).astype(np.float32)
    s32 = np.zeros((B, H, W, 32), np.float32)
    s32[..., :Cin] = state
    w32 = np.zeros((Cout, 32, 3, 3), np.float32)
    w32[:, :Cin] = w
    e = engine.Engine(synth.tiny_unet_config(), 0)
    try:
        for r in range(rounds):
            for i in range(iters):
                a = e.op_conv_in_f32(state, w, bias)["out"]
                b, _ = e.op_conv2d(s32, w32, bias, return_stats=True)
            print(f"round {r}: {iters} x ({NEW}, generic); max |new - generic| {float(np.abs(a - b).max()):.3e}", flush=True)
    finally:
        e.close()


def summarise(path, iters):
    rows = list(csv.DictReader(open(path)))
    for key in (NEW, OLD):
        d = [(int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
             for r in rows if key in r["Kernel_Name"]]
        d.sort()
        ms = [x[1] for x in d]
        for r in range(0, len(ms), iters):
            part = ms[r:r + iters]
            print(f"{key:22s} round {r // iters}: n {len(part):3d}  mean {np.mean(part):.4f} ms  min {min(part):.4f}  max {max(part):.4f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[64, 128, 128, 6, 64], metavar=("B", "H", "W", "Cin", "Cout"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--trace", default="", help="a *_kernel_trace.csv of an earlier run: print the per-round durations")
    a = ap.parse_args()
    if a.trace:
        summarise(a.trace, a.iters)
    else:
        run(tuple(a.shape), a.iters, a.rounds)
