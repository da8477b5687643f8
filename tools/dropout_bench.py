"""What train-mode Dropout (sr3_set_dropout) costs in the sampler step: B = 64 at 128 x 128, yml UNet, the
three arithmetic modes, dropout off and on in the SAME process and interleaved round by round (boxes differ by up to 20 %;
only numbers of one process compare).

Per mode:
  step_off_ms / step_on_ms   ms per sampler step through the captured step graph (wall clock around `--steps` steps between
                             two stream synchronisations), median over `--reps` rounds, with the min / max of the rounds
  on_minus_off_ms            median and quartiles of the PAIRED differences (off and on of the same round, back to back)
  gn_off_ms / gn_on_ms       the event-timed GroupNorm / apply family per step (sr3_profile_get, every kernel launched
                             individually: no graph) — the family the masked passes belong to — and its launches per step

Prints one JSON object. Standalone: bench.py is not involved.

    python tools/dropout_bench.py [--res 128] [--batch 64] [--steps 20] [--reps 7] [--p 0.2] [--modes f32,f16x3,f16f8]
"""
import argparse
import dataclasses
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
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--lres", type=int, default=16)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--p", type=float, default=0.2)
    ap.add_argument("--modes", default="f32,f16x3,f16f8")
    a = ap.parse_args()
    synth, schedule, engine = (importlib.import_module(PKG + "." + m) for m in ("synth", "schedule", "engine"))
    B, r, T = a.batch, a.res, 1000
    cfg = dataclasses.replace(synth.yml_unet_config(224), dropout=a.p)
    e = engine.Engine(cfg, 0)
    e.load_state_dict(synth.synth_state_dict(cfg, 0))
    e.set_schedule(schedule.schedule_buffers({"schedule": "linear", "n_timestep": T, "linear_start": 1e-6, "linear_end": 1e-2}))
    cond = e.to_device(synth.synth_cond(B, r, a.lres, 0))

    def steps(n, t0):
        for k in range(n):
            e.sample_step(t0 - k)

    def timed(on, n):
        e.set_dropout(on, 1234, 0)
        steps(3, T - 1)                         # eager first step + capture + one replay
        e.synchronize()
        t = time.perf_counter()
        steps(n, T - 4)
        e.synchronize()
        return (time.perf_counter() - t) * 1e3 / n

    def family(on, n):
        e.set_dropout(on, 1234, 0)
        e.profile_enable(True)
        steps(2, T - 1)
        e.profile_reset()
        steps(n, T - 3)
        g = e.profile_get()["groupnorm"]
        e.profile_enable(False)
        return round(g["ms"] / n, 4), g["launches"] // n

    result = {"tool": "dropout_bench", "shape": {"batch": B, "res": r, "unet": "yml image_size=224", "p": a.p},
              "steps": a.steps, "reps": a.reps, "modes": {}}
    for mode in a.modes.split(","):
        e.set_precision(mode)
        e.sample_begin(cond.ptr, B, r, r, None, 7, 0)
        off, on = [], []
        for rep in range(a.reps + 1):
            t_off, t_on = timed(False, a.steps), timed(True, a.steps)
            if rep:                             # (round 0 warms both graphs)
                off.append(t_off)
                on.append(t_on)
        d = sorted(y - x for x, y in zip(off, on))
        q = statistics.quantiles(d, n=4) if len(d) >= 4 else [d[0], statistics.median(d), d[-1]]
        gn_off, n_off = family(False, 5)
        gn_on, n_on = family(True, 5)
        e.range_check() if mode != "f32" else None
        result["modes"][mode] = {
            "step_off_ms": round(statistics.median(off), 3), "step_off_range": [round(min(off), 3), round(max(off), 3)],
            "step_on_ms": round(statistics.median(on), 3), "step_on_range": [round(min(on), 3), round(max(on), 3)],
            "on_minus_off_ms": {"median": round(statistics.median(d), 3), "quartiles": [round(q[0], 3), round(q[2], 3)]},
            "gn_off_ms": gn_off, "gn_on_ms": gn_on, "gn_launches_off": n_off, "gn_launches_on": n_on}
    e.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
