"""Warm start of the sampler (sr3_sample_from) at the headline shape (B = 64, 16 -> 128, yml UNet,
T = 1000, the reference's DDPM loop): whole calls begun from the conditioning image, noised to the level of s0 / S in
--fractions, against the full call from pure noise in the same process — wall time per call, its ratio to the full
call, and how far the result is from the full run's (max-abs and PSNR over the batch, same seed: the noise draws of the
steps both calls run are the same ones). One process, no reference needed. Prints one JSON object.

The weights are synthetic: the distances say how far apart the two calls land, not how good either image is — sample
quality at a given strength is a property of a trained checkpoint and is not established by this tool.

    python tools/warm_start_bench.py [--batch 64] [--T 1000] [--precision f32] [--fractions 0.1,0.25,0.5,0.75,1.0]
                                     [--sampler ddpm|ddim|dpmpp_2m --steps S]
"""
import argparse
import importlib
import json
import os
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
    ap.add_argument("--precision", default="f32", choices=["f32", "f16x3", "f16f8"])
    ap.add_argument("--sampler", default="ddpm", choices=["ddpm", "ddim", "dpmpp_2m"])
    ap.add_argument("--steps", type=int, default=None, help="S of a few-step sampler (default: T)")
    ap.add_argument("--fractions", default="0.1,0.25,0.5,0.75,1.0", help="s0 / S of the warm calls")
    a = ap.parse_args()
    import torch

    synth = importlib.import_module(PKG + ".synth")
    schedule = importlib.import_module(PKG + ".schedule")
    samplers = importlib.import_module(PKG + ".samplers")
    metrics = importlib.import_module(PKG + ".metrics")
    Engine = importlib.import_module(PKG + ".engine").Engine
    B, r, T = a.batch, a.res, a.T
    cfg = synth.yml_unet_config(224)
    eng = Engine(cfg, 0)
    eng.load_state_dict(synth.synth_state_dict(cfg, 0))
    eng.set_precision(a.precision)
    bufs = schedule.schedule_buffers({"schedule": "linear", "n_timestep": T, "linear_start": 1e-6, "linear_end": 1e-2})
    if a.sampler == "ddpm":
        eng.set_schedule(bufs)
        S = T
    else:
        S = a.steps or T
        eng.set_sampler_schedule(samplers.sampler_tables(bufs, a.sampler, S, 0.0))
    cond = torch.from_numpy(synth.synth_cond(B, r, a.lres, 0)).cuda()
    full, out = torch.empty((B, 3, r, r), device="cuda"), torch.empty((B, 3, r, r), device="cuda")
    torch.cuda.synchronize()
    seed = 5

    def call(dst, s0=None):
        t0 = time.perf_counter()
        if s0 is None:
            eng.sample(cond.data_ptr(), B, r, r, dst.data_ptr(), None, seed, 0)
        else:
            eng.sample(cond.data_ptr(), B, r, r, dst.data_ptr(), None, seed, 0, init_ptr=cond.data_ptr(), start_step=s0)
        eng.synchronize()
        return time.perf_counter() - t0

    call(out, min(S, 4))                    # warm-up: workspace, the eager first step, the captured graph
    sec_full = call(full)
    rows = []
    for frac in [float(x) for x in a.fractions.split(",") if x]:
        s0 = max(1, min(S, int(round(frac * S))))
        sec = call(out, s0)
        d = (out - full).abs().max().item()
        rows.append({"s0": s0, "s0_over_S": round(s0 / S, 4), "s": round(sec, 3), "vs_full": round(sec / sec_full, 4),
                     "ms_per_step": round(sec / s0 * 1e3, 3), "max_abs_vs_full": round(d, 4),
                     "psnr_vs_full": metrics.batch_psnr_stats(out.cpu().numpy(), full.cpu().numpy()),
                     "finite": bool(torch.isfinite(out).all())})
    sec_full2 = call(out)                   # the full call again: the spread of the yardstick itself
    same = bool(torch.equal(out, full))
    eng.close()
    print(json.dumps({"tool": "warm_start_bench", "device": torch.cuda.get_device_name(0),
                      "shape": {"B": B, "lres": a.lres, "res": r, "T": T, "unet": "yml image_size=224"},
                      "sampler": a.sampler, "S": S, "precision": a.precision,
                      "full_call": {"s": round(sec_full, 3), "again_s": round(sec_full2, 3), "bit_equal_again": same,
                                    "ms_per_step": round(sec_full / S * 1e3, 3)},
                      "warm_calls": rows}))


if __name__ == "__main__":
    main()
