"""Few-step samplers at the headline shape (B = 64, 16 -> 128, yml UNet, T = 1000): the sampler step of ddpm / ddim /
dpmpp_2m in the same process (their update kernels differ only by the x0 history), and whole sr3_sample calls at
S in {20, 50, 100} against the T = 1000 DDPM call, each with its fixed cost beyond S steps at the per-step time
(`fixed_ms`: workspace / graph reuse, the segment guard's ten boundary synchronisations in split-f16 modes). Prints one
JSON object. Standalone: bench.py is not involved.

    python tools/sampler_bench.py [--batch 64] [--rounds 5] [--steps 10] [--call-precisions f32,f16f8]
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
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of the per-step timing")
    ap.add_argument("--steps", type=int, default=10, help="steps per timed run")
    ap.add_argument("--step-precisions", default="f32,f16f8")
    ap.add_argument("--call-precisions", default="f32,f16f8")
    ap.add_argument("--call-steps", default="20,50,100")
    a = ap.parse_args()
    import torch

    synth = importlib.import_module(PKG + ".synth")
    schedule = importlib.import_module(PKG + ".schedule")
    samplers = importlib.import_module(PKG + ".samplers")
    Engine = importlib.import_module(PKG + ".engine").Engine
    B, r, T = a.batch, a.res, a.T
    cfg = synth.yml_unet_config(224)
    eng = Engine(cfg, 0)
    eng.load_state_dict(synth.synth_state_dict(cfg, 0))
    bufs = schedule.schedule_buffers({"schedule": "linear", "n_timestep": T, "linear_start": 1e-6, "linear_end": 1e-2})
    cond = torch.from_numpy(synth.synth_cond(B, r, a.lres, 0)).cuda()
    out = torch.empty((B, 3, r, r), device="cuda")
    torch.cuda.synchronize()

    def use(kind, S=None):
        if kind == "ddpm":
            eng.set_schedule(bufs)
        else:
            eng.set_sampler_schedule(samplers.sampler_tables(bufs, kind, S, 0.0))

    def time_steps(kind, S):
        """seconds per step over a.steps consecutive steps from the start of the loop (graph replays)"""
        use(kind, S)
        n = T if kind == "ddpm" else S
        eng.sample_begin(cond.data_ptr(), B, r, r, None, 7, 0)
        for t in range(n - 1, n - 3, -1):          # eager first step + graph capture
            eng.sample_step(t, None)
        eng.synchronize()
        t0 = time.perf_counter()
        for t in range(n - 3, n - 3 - a.steps, -1):
            eng.sample_step(t, None)
        eng.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        eng.sample_end(out.data_ptr())
        eng.synchronize()
        return dt

    S_step = max(a.steps + 3, 50)
    step_ms = {}
    for prec in [p for p in a.step_precisions.split(",") if p]:
        eng.set_precision(prec)
        kinds = ("ddpm", "ddim", "dpmpp_2m")
        for k in kinds:                               # warm-up: graphs of this precision
            time_steps(k, S_step)
        runs = {k: [] for k in kinds}
        for _ in range(a.rounds):
            for k in kinds:
                runs[k].append(time_steps(k, S_step) * 1e3)
        med = {k: statistics.median(v) for k, v in runs.items()}
        step_ms[prec] = {k: {"median_ms": round(med[k], 3), "runs_ms": [round(x, 3) for x in runs[k]],
                             "vs_ddpm": round(med[k] / med["ddpm"] - 1.0, 4)} for k in kinds}

    calls = {}
    for prec in [p for p in a.call_precisions.split(",") if p]:
        eng.set_precision(prec)
        res = {}
        for kind, S in [("dpmpp_2m", int(s)) for s in a.call_steps.split(",")] + [("ddpm", T)]:
            use(kind, S)
            eng.sample(cond.data_ptr(), B, r, r, out.data_ptr(), None, 5, 0)   # warm-up call (graph, workspace)
            eng.synchronize()
            t0 = time.perf_counter()
            eng.sample(cond.data_ptr(), B, r, r, out.data_ptr(), None, 5, 0)
            eng.synchronize()
            sec = time.perf_counter() - t0
            res[f"{kind}_S{S}"] = {"s": round(sec, 3), "ms_per_step": round(sec / S * 1e3, 3),
                                   "finite": bool(torch.isfinite(out).all())}
            if prec in step_ms:   # fixed per-call cost: the call minus S steps at the measured per-step time
                res[f"{kind}_S{S}"]["fixed_ms"] = round(sec * 1e3 - S * step_ms[prec][kind]["median_ms"], 1)
        ddpm = res[f"ddpm_S{T}"]["s"]
        for v in res.values():
            v["speedup_vs_ddpm_T"] = round(ddpm / v["s"], 2)
        calls[prec] = res
    eng.close()
    print(json.dumps({"tool": "sampler_bench", "device": torch.cuda.get_device_name(0),
                      "shape": {"B": B, "lres": a.lres, "res": r, "T": T, "unet": "yml image_size=224"},
                      "step_ms": step_ms, "whole_call": calls}))


if __name__ == "__main__":
    main()
