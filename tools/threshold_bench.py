"""Dynamic thresholding of the x0 prediction at the headline shape (yml UNet, 16 -> 128, T = 1000): the
sampler step of dpmpp_2m (S = 10) and ddpm with the feature off and on in the same process, interleaved, at B = 64 and
B = 1; and the selection kernels alone through sr3_op_abs_quantile, with the bandwidth they achieve against the bytes
they must read (4 passes x 4 n bytes per image). Prints one JSON object. Standalone: bench.py is not involved.

    python tools/threshold_bench.py [--batches 64,1] [--rounds 5] [--precisions f32,f16f8] [--blocks N]

--blocks N pins the blocks that share one image in the selection (SR3_THRESHOLD_BLOCKS; 1: a single block per image).
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
RATIO = 0.995
PASSES = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--lres", type=int, default=16)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of the per-step timing")
    ap.add_argument("--steps", type=int, default=7, help="steps per timed run (dpmpp_2m S = 10 has 8 after its two warm-up steps)")
    ap.add_argument("--precisions", default="f32,f16f8")
    ap.add_argument("--select-shapes", default="64x49152,1x49152,1x196608,1x3145728", help="BxN of the selection alone")
    ap.add_argument("--select-iters", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=0)
    a = ap.parse_args()
    if a.blocks:
        os.environ["SR3_THRESHOLD_BLOCKS"] = str(a.blocks)      # (read once, when the library first plans a selection)
    import torch

    synth = importlib.import_module(PKG + ".synth")
    schedule = importlib.import_module(PKG + ".schedule")
    samplers = importlib.import_module(PKG + ".samplers")
    Engine = importlib.import_module(PKG + ".engine").Engine
    r, T = a.res, a.T
    cfg = synth.yml_unet_config(224)
    eng = Engine(cfg, 0)
    eng.load_state_dict(synth.synth_state_dict(cfg, 0))
    bufs = schedule.schedule_buffers({"schedule": "linear", "n_timestep": T, "linear_start": 1e-6, "linear_end": 1e-2})

    def time_steps(kind, S, B, cond, out, on):
        """seconds per step over a.steps consecutive steps from the start of the loop (graph replays)"""
        if kind == "ddpm":
            eng.set_schedule(bufs)
        else:
            eng.set_sampler_schedule(samplers.sampler_tables(bufs, kind, S, 0.0))
        eng.set_dynamic_threshold(RATIO if on else None)
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

    cases = [("dpmpp_2m", 10), ("ddpm", T)]
    step_ms = {}
    for B in [int(b) for b in a.batches.split(",") if b]:
        cond = torch.from_numpy(synth.synth_cond(B, r, a.lres, 0)).cuda()
        out = torch.empty((B, 3, r, r), device="cuda")
        torch.cuda.synchronize()
        for prec in [p for p in a.precisions.split(",") if p]:
            eng.set_precision(prec)
            keys = [(k, S, on) for k, S in cases for on in (False, True)]
            for k, S, on in keys:                      # warm-up: workspace and graphs of this precision and batch
                time_steps(k, S, B, cond, out, on)
            runs = {key: [] for key in keys}
            for _ in range(a.rounds):
                for key in keys:
                    runs[key].append(time_steps(key[0], key[1], B, cond, out, key[2]) * 1e3)
            res = {}
            for k, S in cases:
                off, on = runs[(k, S, False)], runs[(k, S, True)]
                m_off, m_on = statistics.median(off), statistics.median(on)
                res[f"{k}_S{S}"] = {"off_ms": round(m_off, 4), "on_ms": round(m_on, 4), "delta_us": round((m_on - m_off) * 1e3, 1),
                                    "delta_rel": round(m_on / m_off - 1.0, 5), "off_runs_ms": [round(x, 4) for x in off],
                                    "on_runs_ms": [round(x, 4) for x in on]}
            step_ms[f"B{B}_{prec}"] = res
    eng.set_dynamic_threshold(None)

    select = {}
    for spec in [s for s in a.select_shapes.split(",") if s]:
        B, n = (int(v) for v in spec.split("x"))
        x = torch.randn((B, n), device="cuda") * 1.5
        o = torch.empty((3, B), device="cuda")
        torch.cuda.synchronize()
        call = lambda: eng.abs_quantile(x.data_ptr(), B, n, RATIO, None, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
        for _ in range(3):
            call()
        eng.synchronize()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(a.select_iters):
                call()
            eng.synchronize()
            runs.append((time.perf_counter() - t0) / a.select_iters * 1e6)
        us = statistics.median(runs)
        must_read = PASSES * 4 * n * B
        select[spec] = {"us": round(us, 1), "runs_us": [round(v, 1) for v in runs], "bytes_read": must_read,
                        "GBps": round(must_read / us * 1e-3, 1), "s": [round(float(v), 4) for v in o[2][:2].cpu()]}
    eng.close()
    print(json.dumps({"tool": "threshold_bench", "device": torch.cuda.get_device_name(0), "ratio": RATIO,
                      "blocks_per_image": a.blocks or "auto",
                      "shape": {"lres": a.lres, "res": r, "T": T, "unet": "yml image_size=224"},
                      "step_ms": step_ms, "select_alone": select}))


if __name__ == "__main__":
    main()
