#!/usr/bin/env python3
"""Kernel micro-benchmark for the implicit-GEMM conv (development tool; run on the GPU box):
    python tools/conv_bench.py [--iters N] [--set main|wino3|up2|rows|gnres] [--only i,j,...] [--repeat R]
Prints ms and TFLOP/s per shape of the B=64, 128x128 SR3 step (--set wino3: every distinct shape of its three-pass
Winograd convs, timed from U on: the position GEMMs + output transform, in whichever form the plan takes).
--set up2: the four Upsample convs of the step, and the 64 -> 128 one at B = 4 and 16, in the form the plan takes, as
four phase convs (SR3_NO_UP2_WINO=1) and as sub-pixel Winograd wherever its preconditions hold (SR3_UP2_WINO_FORCE=1):
one child process per form (the switches are read once per process), the forms alternating, --repeat rounds.
--set rows: every distinct 3x3 shape of the step's 32x32 and 16x16 levels from the RAW input on (GroupNorm apply pass + conv),
in the parent's three-pass forms (SR3_NO_WINO_FUSED_ROWS=1) and on the one-pass kernel with 2 | 4 tile rows per block
(SR3_WINO_FUSED_ROWS_FORCE=1), alternating in the same way: the table that sets WINO_FUSED_ROWS_MIN_BLOCKS.
--set gnres: the eleven ResnetBlocks of the step whose block1 GroupNorm pass also multiplies the 1x1 res_conv
(gn_res1x1_kernel): the pair it replaces (apply pass on the engine's route, with its finalize launch where that route has
one, + the 1x1 side launch) against finalize + the kernel, alternating in ONE process, --repeat rounds: the table that
sets the level gate of gn_res1x1_gate (a level is adopted where every shape is at or under 0.9 of the pair)."""
import argparse
import importlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
PKG = "3d-super-resolution-face-reconstruction_amd"

# B, H, W, C0, C1, Cout, ks, stride, up2, mode, resid, chan_bias
MAIN = [
    (64, 128, 128, 64, 0, 64, 3, 1, 0, 2, 1, 0),
    (64, 128, 128, 64, 0, 64, 3, 1, 0, 0, 0, 0),
    (64, 128, 128, 128, 64, 64, 3, 1, 0, 2, 0, 1),
    (64, 64, 64, 128, 0, 128, 3, 1, 0, 2, 1, 0),
    (64, 64, 64, 128, 0, 128, 3, 1, 0, 0, 0, 0),
    (64, 32, 32, 256, 0, 256, 3, 1, 0, 2, 1, 0),
    (64, 16, 16, 512, 0, 512, 3, 1, 0, 2, 1, 0),
    (64, 16, 16, 512, 0, 512, 3, 1, 0, 0, 0, 0),
    (64, 8, 8, 512, 0, 512, 3, 1, 0, 2, 1, 0),
    (64, 16, 16, 512, 0, 512, 3, 1, 1, 0, 0, 0),
    (64, 64, 64, 128, 0, 128, 3, 1, 1, 0, 0, 0),
    (64, 128, 128, 64, 0, 3, 3, 1, 0, 2, 0, 0),
    (64, 128, 128, 32, 0, 64, 3, 1, 0, 0, 0, 0),
    (64, 16, 16, 1024, 0, 512, 3, 1, 0, 0, 0, 0),
    (64, 32, 32, 768, 0, 256, 3, 1, 0, 0, 0, 0),
    # the remaining 3x3 stride-1 shapes of the 64x64 and 128x128 levels (Winograd one-pass kernel; x || skip inputs)
    (64, 128, 128, 128, 0, 64, 3, 1, 0, 2, 0, 1),
    (64, 64, 64, 64, 0, 128, 3, 1, 0, 2, 0, 1),
    (64, 64, 64, 128, 64, 128, 3, 1, 0, 2, 0, 1),
    (64, 64, 64, 128, 128, 128, 3, 1, 0, 2, 0, 1),
    (64, 64, 64, 256, 128, 128, 3, 1, 0, 2, 0, 1),
]

# the three-pass Winograd shapes of the step: 32x32 (-> 256), 16x16 (-> 512), 8x8 (-> 512); Cin of x || skip inputs in C0
WINO3 = [(64, 32, 32, cin, 0, 256, 3, 1, 0, 2, 1, 1) for cin in (128, 256, 384, 512, 768)] + \
        [(64, 16, 16, cin, 0, 512, 3, 1, 0, 2, 1, 1) for cin in (256, 512, 768, 1024)] + \
        [(64, 8, 8, cin, 0, 512, 3, 1, 0, 2, 1, 1) for cin in (512, 1024)]

# the Upsample convs of the step (8 -> 16, 16 -> 32, 32 -> 64, 64 -> 128), then the last one at B = 4 and 16
UP2 = [(64, 8, 8, 512, 0, 512, 3, 1, 1, 0, 0, 0), (64, 16, 16, 512, 0, 512, 3, 1, 1, 0, 0, 0), (64, 32, 32, 256, 0, 256, 3, 1, 1, 0, 0, 0),
       (64, 64, 64, 128, 0, 128, 3, 1, 1, 0, 0, 0), (4, 64, 64, 128, 0, 128, 3, 1, 1, 0, 0, 0), (16, 64, 64, 128, 0, 128, 3, 1, 1, 0, 0, 0)]
UP2_FORMS = [("plan", {}), ("phase", {"SR3_NO_UP2_WINO": "1"}), ("wino", {"SR3_UP2_WINO_FORCE": "1"})]

# the three-pass shapes of the 32x32 and 16x16 levels, in both forms of the plan
ROWS = WINO3[:9]
ROWS_FORMS = [("three-pass", {"SR3_NO_WINO_FUSED_ROWS": "1"}), ("rows", {"SR3_WINO_FUSED_ROWS_FORCE": "1"})]
FORMS = {"up2": UP2_FORMS, "rows": ROWS_FORMS}

# B, H = W, C0, C1, Cout of the blocks gn_res1x1_gate takes at B = 64: the 128x128, 64x64 and 32x32 levels
GNRES = [(64, 128, 128, 64, 64), (64, 128, 64, 64, 64), (64, 64, 64, 0, 128), (64, 64, 256, 128, 128), (64, 64, 128, 128, 128),
         (64, 64, 128, 64, 128), (64, 32, 128, 0, 256), (64, 32, 512, 256, 256), (64, 32, 256, 256, 256), (64, 32, 256, 128, 256)]


def gnres_main(e, args):
    shapes = GNRES if not args.only else [GNRES[int(i)] for i in args.only.split(",")]
    for rnd in range(args.repeat):
        for (B, hw, C0, C1, Cout) in shapes:
            pair, one, route = e.bench_gn_res1x1(B, hw, hw, C0, C1, Cout, args.iters)
            fl = 2.0 * B * hw * hw * Cout * (C0 + C1)
            gb = 4.0 * B * hw * hw * (2 * (C0 + C1) + Cout) / 1e9
            print(f"round {rnd + 1} B{B} {hw}x{hw} cin{C0}+{C1} cout{Cout}: pair {pair:7.4f} ms (apply route {route})  one {one:7.4f} ms  "
                  f"ratio {one / pair:5.3f}   [one: {fl / one / 1e9:6.1f} TFLOP/s, {gb / one:5.2f} TB/s]", flush=True)


def forms_parent(args):
    """one child per form and round; nothing here touches the GPU"""
    forms = FORMS[args.set]
    switches = {k for _, env_add in forms for k in env_add}
    for rnd in range(args.repeat):
        for form, env_add in forms:
            env = {k: v for k, v in os.environ.items() if k not in switches}
            env.update(env_add)
            cmd = [sys.executable, os.path.abspath(__file__), "--set", args.set, "--child", form, "--iters", str(args.iters),
                   "--precision", args.precision] + (["--only", args.only] if args.only else [])
            print(f"# round {rnd + 1}, form '{form}' {env_add}", flush=True)
            r = subprocess.run(cmd, env=env, timeout=600)
            if r.returncode != 0:       # (a fault or a hang ends the whole run: nothing more is started on the GPU)
                sys.exit(f"child for form '{form}' ended with {r.returncode}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--set", type=str, default="main", choices=["main", "wino3", "up2", "rows", "gnres"])
    ap.add_argument("--repeat", type=int, default=2, help="--set up2 | rows | gnres: rounds over the forms")
    ap.add_argument("--child", type=str, default="", help=argparse.SUPPRESS)
    ap.add_argument("--only", type=str, default="", help="comma list of shape indices")
    ap.add_argument("--precision", type=str, default="f32", choices=["f32", "f16x3", "f16f8"])
    args = ap.parse_args()
    if args.set in FORMS and not args.child:
        forms_parent(args)
        sys.exit(0)
    if os.environ.get("SR3_LIB"):       # timing experiments with an alternative build of the library
        importlib.import_module(PKG + "._lib").LIB_PATH = os.path.abspath(os.environ["SR3_LIB"])
    synth = importlib.import_module(PKG + ".synth")
    Engine = importlib.import_module(PKG + ".engine").Engine
    e = Engine(synth.tiny_unet_config(), 0)
    e.set_precision(args.precision)
    if args.set == "gnres":
        gnres_main(e, args)
        e.close()
        sys.exit(0)
    table = {"wino3": WINO3, "up2": UP2, "rows": ROWS}.get(args.set, MAIN)
    shapes = table if not args.only else [table[int(i)] for i in args.only.split(",")]
    for (B, H, W, C0, C1, Cout, ks, st, up, mode, rs, cb) in shapes:
        n0 = e.up2_wino_launches() if args.set == "up2" else e.wino_fused_rows_launches() if args.set == "rows" else 0
        ms, ams = e.bench_conv(B, H, W, C0, C1, Cout, ks, st, up, mode, rs, cb, args.iters)
        Ho, Wo = (H * (2 if up else 1)) // st, (W * (2 if up else 1)) // st
        fl = 2.0 * B * Ho * Wo * Cout * ks * ks * (C0 + C1)
        tail = f"(gn_apply {ams:.4f} ms)"
        if args.set == "up2":           # which kernel ran, and its rate on the MACs it executes (16 | 9 of the 36)
            wino = e.up2_wino_launches() > n0
            tail = f"[{args.child}: {'wino_up2_kernel' if wino else 'phase convs'}, {fl * (9 if wino else 16) / 36 / ms / 1e9:6.2f} TFLOP/s executed]"
        if args.set == "rows":          # from the raw input: the apply pass (writes U | the activated tensor) + the conv
            rows = e.wino_fused_rows_launches() > n0
            tail = f"[{args.child}: {'wino_fused_kernel<R>' if rows else 'three-pass'}; apply pass {ams:.4f} ms, pass + conv {ms + ams:8.4f} ms]"
        print(f"B{B} {H}x{W} cin{C0}+{C1} cout{Cout} k{ks} s{st} u{up} mode{mode} res{rs} cb{cb}: "
              f"{ms:8.4f} ms  {fl / ms / 1e9:7.2f} TFLOP/s   {tail}", flush=True)
    e.close()
