"""Low-resolution consistency at the headline shape (B = 64, 16 -> 128, yml UNet, T = 1000): the sampler
step with the feature off and on, alternating inside one process (off is the step of the commit before the feature: the
same kernels, the same graphs), and the projection op alone in both forms with its achieved bandwidth. The difference of
a precision counts as signal by the rule of finding 82: every run with the feature slower than every run without it by at
least five times the spread of the runs without. Prints one JSON object. Standalone: bench.py is not involved.

    python tools/consistency_bench.py [--batch 64] [--rounds 5] [--steps 10] [--precisions f32,f16f8] [--op-iters 50]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
PKG = "3d-super-resolution-face-reconstruction_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--lres", type=int, default=16)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of the per-step timing")
    ap.add_argument("--steps", type=int, default=10, help="steps per timed run")
    ap.add_argument("--precisions", default="f32,f16f8")
    ap.add_argument("--op-iters", type=int, default=50)
    a = ap.parse_args()
    import torch

    synth = importlib.import_module(PKG + ".synth")
    schedule = importlib.import_module(PKG + ".schedule")
    Engine = importlib.import_module(PKG + ".engine").Engine
    B, r, l, T = a.batch, a.res, a.lres, a.T
    cfg = synth.yml_unet_config(224)
    eng = Engine(cfg, 0)
    eng.load_state_dict(synth.synth_state_dict(cfg, 0))
    eng.set_schedule(schedule.schedule_buffers({"schedule": "linear", "n_timestep": T, "linear_start": 1e-6, "linear_end": 1e-2}))
    cond = torch.from_numpy(synth.synth_cond(B, r, l, 0)).cuda()
    lr = (torch.rand((B, 3, l, l), device="cuda") * 2 - 1).contiguous()
    out = torch.empty((B, 3, r, r), device="cuda")
    torch.cuda.synchronize()

    def time_steps(on):
        """seconds per step over a.steps consecutive steps from the start of the loop (graph replays)"""
        eng.set_lr_consistency(lr.data_ptr() if on else None, B, l, l, 0, 1.0)
        eng.sample_begin(cond.data_ptr(), B, r, r, None, 7, 0)
        for t in range(T - 1, T - 3, -1):           # eager first step + graph capture
            eng.sample_step(t, None)
        eng.synchronize()
        t0 = time.perf_counter()
        for t in range(T - 3, T - 3 - a.steps, -1):
            eng.sample_step(t, None)
        eng.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        eng.sample_end(out.data_ptr())
        eng.synchronize()
        return dt

    step_ms = {}
    for prec in [p for p in a.precisions.split(",") if p]:
        eng.set_precision(prec)
        for on in (False, True):                    # warm-up: both graphs of this precision
            time_steps(on)
        runs = {False: [], True: []}
        for _ in range(a.rounds):
            for on in (False, True):
                runs[on].append(time_steps(on) * 1e3)
        off, on = runs[False], runs[True]
        spread = max(off) - min(off)
        gap = min(on) - max(off)
        step_ms[prec] = {"off_ms": [round(x, 3) for x in off], "on_ms": [round(x, 3) for x in on],
                         "median_off_ms": round(statistics.median(off), 3), "median_on_ms": round(statistics.median(on), 3),
                         "difference_ms": round(statistics.median(on) - statistics.median(off), 3),
                         "spread_off_ms": round(spread, 3), "gap_ms": round(gap, 3), "signal": bool(gap >= 5 * spread)}
    eng.set_lr_consistency(None)

    # the op alone: reads and writes X once (the operators and the intermediates stay in cache / LDS in the best case)
    x = torch.randn((B, 3, r, r), device="cuda").clamp_(-1, 1).contiguous()
    moved = 2 * x.numel() * 4 + lr.numel() * 4
    op = {}
    for form in ("lds", "scratch"):
        try:
            for _ in range(5):
                eng.lr_project(x.data_ptr(), B, 3, r, r, lr.data_ptr(), B, l, l, 0, 1.0, form)
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.op_iters):
                eng.lr_project(x.data_ptr(), B, 3, r, r, lr.data_ptr(), B, l, l, 0, 1.0, form)
            eng.synchronize()
            us = (time.perf_counter() - t0) / a.op_iters * 1e6
            op[form] = {"us": round(us, 1), "min_bytes": moved, "GBps_of_min_bytes": round(moved / us * 1e-3, 1)}
        except Exception as e:          # (the LDS form does not exist above its plane size)
            op[form] = {"error": str(e)}
    sc_s = torch.empty(B, dtype=torch.float64, device="cuda")
    sc_m = torch.empty(B, dtype=torch.float32, device="cuda")
    eng.lr_residual(x.data_ptr(), B, 3, r, r, lr.data_ptr(), B, l, l, 0, sc_s.data_ptr(), sc_m.data_ptr())
    eng.synchronize()
    eng.close()
    print(json.dumps({"tool": "consistency_bench", "device": torch.cuda.get_device_name(0),
                      "shape": {"B": B, "lres": l, "res": r, "T": T, "unet": "yml image_size=224"},
                      "step_ms": step_ms, "project_op": op, "residual_after_op_max_abs": float(sc_m.max().item())}))


if __name__ == "__main__":
    main()
