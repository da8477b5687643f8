"""Feature cache of the sampler (sr3_set_feature_cache; DeepCache) at the headline shape (B = 64,
16 -> 128, yml UNet, T = 1000, the reference's DDPM loop), in one process:

  steps   ms per whole step and per shallow step of depth 1 and 2 in every arithmetic mode (step API, captured graphs,
          a host clock around --step-count steps that end in a device synchronise), and shallow / whole
  calls   whole calls with interval in --intervals: wall time, its ratio to the interval-1 call of the same run (the
          sampler as it is without the feature), and max-abs / PSNR of the result against that call's, same seed
  few     the same calls with --sampler/--steps (default dpmpp_2m, S = 20)
  families event-timed ms, launches and counted conv FLOPs per kernel family of a whole and of a shallow step (no graph)
  fixture on tests/golden/sampler_cfg2_16_128_T1000.npz (B = 1, injected noise, a run of the reference itself): the
          distance of every setting's result from the reference's own

Prints one JSON object. The weights are synthetic: the distances say how far the calls land from each other, not how
good either image is — sample quality with the cache on is a property of a trained checkpoint and is not established by
this tool.

    python tools/feature_cache_bench.py [--batch 64] [--T 1000] [--intervals 1,2,3,5,10] [--depth 1]
                                        [--call-precisions f32,f16f8] [--fixture-precisions f32]
                                        [--sampler dpmpp_2m --steps 20]
                                        [--sections steps,families,calls,few,fixture]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
PKG = "3d-super-resolution-face-reconstruction_amd"
MODES = ("f32", "f16x3", "f16f8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--lres", type=int, default=16)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--intervals", default="1,2,3,5,10")
    ap.add_argument("--depth", type=int, default=1, help="depth of the whole calls")
    ap.add_argument("--call-precisions", default="f32,f16f8")
    ap.add_argument("--sampler", default="dpmpp_2m", choices=["ddim", "dpmpp_2m"])
    ap.add_argument("--steps", type=int, default=20, help="S of the few-step calls")
    ap.add_argument("--step-count", type=int, default=30, help="steps in one timed window")
    ap.add_argument("--fixture-precisions", default="f32")
    ap.add_argument("--sections", default="steps,families,calls,few,fixture")
    a = ap.parse_args()
    import torch

    synth = importlib.import_module(PKG + ".synth")
    schedule = importlib.import_module(PKG + ".schedule")
    samplers = importlib.import_module(PKG + ".samplers")
    metrics = importlib.import_module(PKG + ".metrics")
    Engine = importlib.import_module(PKG + ".engine").Engine
    B, r, T = a.batch, a.res, a.T
    intervals = [int(x) for x in a.intervals.split(",") if x]
    if intervals[0] != 1:
        intervals.insert(0, 1)
    sections = set(a.sections.split(","))
    cfg = synth.yml_unet_config(224)
    sched_opt = {"schedule": "linear", "n_timestep": T, "linear_start": 1e-6, "linear_end": 1e-2}
    bufs = schedule.schedule_buffers(sched_opt)
    res = {"tool": "feature_cache_bench", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "lres": a.lres, "res": r, "T": T, "unet": "yml image_size=224"},
           "flop_share": {"d1": 0.21, "d2": 0.45}}

    eng = Engine(cfg, 0)
    eng.load_state_dict(synth.synth_state_dict(cfg, 0))
    cond = torch.from_numpy(synth.synth_cond(B, r, a.lres, 0)).cuda()
    full, out = torch.empty((B, 3, r, r), device="cuda"), torch.empty((B, 3, r, r), device="cuda")
    seed = 5

    def window(n, t0):
        """n steps t0, t0 - 1, ... of the live call; ms per step"""
        eng.synchronize()
        c0 = time.perf_counter()
        for k in range(n):
            eng.sample_step(t0 - k, None)
        eng.synchronize()
        return (time.perf_counter() - c0) / n * 1e3

    if "steps" in sections:
        eng.set_schedule(bufs)
        n = min(a.step_count, (T - 8) // 2)
        rows = {}
        for mode in MODES:
            eng.set_precision(mode)
            eng.set_feature_cache(None)
            eng.sample_begin(cond.data_ptr(), B, r, r, None, seed, 0)
            window(3, T - 1)                                # the eager first step, the capture, one replay
            whole = window(n, T - 4)
            row = {"whole_ms": round(whole, 3)}
            for d in (1, 2):
                eng.set_feature_cache(10 ** 6, d)           # one whole step, then shallow steps only
                eng.sample_begin(cond.data_ptr(), B, r, r, None, seed, 0)
                window(4, T - 1)                            # whole | shallow eager, capture, replay
                ms = window(n, T - 5)
                w, s = eng.feature_cache_steps()
                assert (w, s) == (1, n + 3), (w, s)
                row[f"shallow_d{d}_ms"] = round(ms, 3)
                row[f"shallow_d{d}_over_whole"] = round(ms / whole, 4)
            eng.set_feature_cache(None)
            eng.sample_begin(cond.data_ptr(), B, r, r, None, seed, 0)
            window(1, T - 1)
            row["whole_again_ms"] = round(window(n, T - 2), 3)      # the spread of the yardstick itself
            rows[mode] = row
        res["steps"] = rows

    if "families" in sections:
        # per kernel family (conv, GroupNorm, attention, embedding, the rest), every launch bracketed by events and no
        # graph: what a whole step and a shallow step spend where, and the FLOPs the engine counts for their convs
        eng.set_schedule(bufs)
        n, fam = 10, {}
        for mode in [m for m in a.call_precisions.split(",") if m]:
            eng.set_precision(mode)
            row = {}
            for label, d in (("whole", 0), ("shallow_d1", 1), ("shallow_d2", 2)):
                eng.set_feature_cache(10 ** 6 if d else None, max(d, 1))
                eng.sample_begin(cond.data_ptr(), B, r, r, None, seed, 0)
                eng.sample_step(T - 1, None)                # the whole step that fills the cache
                eng.profile_reset()
                eng.profile_enable(True)
                for k in range(n):
                    eng.sample_step(T - 2 - k, None)
                prof = eng.profile_get()
                eng.profile_enable(False)
                row[label] = {k: {"ms": round(v["ms"] / n, 3), "launches": int(v["launches"] // n),
                                  "gflop": round(v["flops"] / n / 1e9, 1)} for k, v in prof.items()}
                row[label]["total_ms"] = round(sum(v["ms"] for v in prof.values()) / n, 3)
            fam[mode] = row
        eng.set_feature_cache(None)
        res["families_event_timed"] = fam

    def calls(S):
        """whole calls over `intervals` in the engine's current schedule and arithmetic"""
        def call(dst):
            t0 = time.perf_counter()
            eng.sample(cond.data_ptr(), B, r, r, dst.data_ptr(), None, seed, 0)
            eng.synchronize()
            return time.perf_counter() - t0

        rows, base = [], None
        for n in intervals:
            eng.set_feature_cache(n, a.depth)
            if n == 1 or len(rows) == 1:                    # warm-up of the whole / the shallow graph of this mode
                eng.sample(cond.data_ptr(), B, r, r, out.data_ptr(), None, seed, 0, init_ptr=cond.data_ptr(),
                           start_step=min(S, 6))
                eng.synchronize()
            sec = call(full if n == 1 else out)
            if n == 1:
                base = sec
            dst = full if n == 1 else out
            rows.append({"interval": n, "depth": a.depth, "s": round(sec, 3), "vs_interval_1": round(sec / base, 4),
                         "steps": list(eng.feature_cache_steps()), "ms_per_step": round(sec / S * 1e3, 3),
                         "max_abs_vs_interval_1": round((dst - full).abs().max().item(), 4),
                         "psnr_vs_interval_1": metrics.batch_psnr_stats(dst.cpu().numpy(), full.cpu().numpy()),
                         "finite": bool(torch.isfinite(dst).all()), "fallbacks": eng.fallback_calls()})
        eng.set_feature_cache(None)
        sec2 = call(out)
        return {"calls": rows, "interval_1_again_s": round(sec2, 3), "bit_equal_again": bool(torch.equal(out, full))}

    for mode in [m for m in a.call_precisions.split(",") if m]:
        eng.set_precision(mode)
        if "calls" in sections:
            eng.set_schedule(bufs)
            res.setdefault("ddpm_calls", {})[mode] = calls(T)
        if "few" in sections:
            eng.set_sampler_schedule(samplers.sampler_tables(bufs, a.sampler, a.steps, 0.0))
            res.setdefault("few_step_calls", {"sampler": a.sampler, "S": a.steps})[mode] = calls(a.steps)
    eng.close()

    if "fixture" in sections:
        z = np.load(os.path.join(ROOT, "tests", "golden", "sampler_cfg2_16_128_T1000.npz"), allow_pickle=False)
        m = json.loads(str(z["meta"]))
        graph = importlib.import_module(PKG + ".graph")
        fcfg = graph.UNetConfig(in_channel=m["in_channel"], out_channel=m["out_channel"], inner_channel=m["inner_channel"],
                                norm_groups=m["norm_groups"], channel_mults=tuple(m["channel_mults"]),
                                attn_res=tuple(m["attn_res"]), res_blocks=m["res_blocks"], dropout=m["dropout"],
                                image_size=m["image_size"])
        fT, fr_ = m["schedule"]["n_timestep"], m["r"]
        e = Engine(fcfg, 0)
        e.load_state_dict(synth.synth_state_dict(fcfg, m["seed"]))
        e.set_schedule(schedule.schedule_buffers(m["schedule"]))
        noise = e.to_device(synth.synth_noise(fT, m["B"], 3, fr_, fr_, m["seed"]))
        dc, do = e.to_device(z["cond"]), e.buffer(m["B"] * 3 * fr_ * fr_)
        rows = []
        for mode in [x for x in a.fixture_precisions.split(",") if x]:
            e.set_precision(mode)
            for d in (1, 2):
                for n in intervals:
                    if n == 1 and d == 2:
                        continue
                    e.set_feature_cache(n, d)
                    e.sample(dc.ptr, m["B"], fr_, fr_, do.ptr, noise.ptr, 0, 0)
                    got = do.download((m["B"], 3, fr_, fr_))
                    rows.append({"precision": mode, "interval": n, "depth": d,
                                 "max_abs_vs_reference": round(float(np.abs(got - z["final"]).max()), 6),
                                 "psnr_vs_reference": metrics.batch_psnr_stats(got, z["final"])})
        e.close()
        res["fixture_cfg2_16_128_T1000"] = rows
    print(json.dumps(res))


if __name__ == "__main__":
    main()
