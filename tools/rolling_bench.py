"""The rolling-batch sampler (sr3_rows_*) at 16 -> 128 with the yml UNet, everything in one process:

  step      B = 64, every row live: ms per rolling step against ms per uniform step in f32 and f16f8, as alternating
            blocks of --block steps (one synchronisation per block), --rounds rounds; the median of each, their ratio, and
            the uniform step's own spread over its rounds, which is what the ratio is judged against; the HIP-event time
            per kernel family of both forms (a profiled pass of its own), which says where a difference sits
  stream    --requests single-image requests at T = --T, all waiting at time zero, served three ways: through 64 slots
            (rows; a finished row is retired and its slot refilled at once), one by one at B = 1, and in held-back
            uniform batches of 64: images per second and seconds to the first result
  mixed     64 requests whose strengths are drawn from {0.25, 0.5, 1.0}: one rolling session against one uniform
            warm-start call per strength (each at the batch of its own group)

--lr holds EVERY request to an LR image (LR consistency per row: sr3_rows_lr_consistency / sr3_rows_admit_lr) and
compares with the uniform forms under sr3_set_lr_consistency: the like-for-like pair of the armed rolling step.
SR3_LIB=<another build of the library> (read by _lib.py) runs the tool on that build (without --lr: an A/B of the
unarmed step against the build of an earlier commit).

Synthetic weights: times only. One JSON object on the last line.

    python tools/rolling_bench.py [--precision f16f8] [--T 100] [--requests 256] [--rounds 5] [--block 20] [--skip stream,mixed] [--lr]
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
SLOTS, R, L = 64, 128, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16f8", choices=["f32", "f16x3", "f16f8"], help="arithmetic of stream and mixed")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--skip", default="", help="comma list of step, stream, mixed")
    ap.add_argument("--lr", action="store_true", help="hold every request to an LR image (both the rolling and the uniform forms)")
    a = ap.parse_args()
    skip = set(x for x in a.skip.split(",") if x)
    import numpy as np
    import torch

    synth = importlib.import_module(PKG + ".synth")
    schedule = importlib.import_module(PKG + ".schedule")
    Engine = importlib.import_module(PKG + ".engine").Engine
    cfg = synth.yml_unet_config(224)
    eng = Engine(cfg, 0)
    eng.load_state_dict(synth.synth_state_dict(cfg, 0))
    seed = 5
    cond = torch.from_numpy(synth.synth_cond(SLOTS, R, L, 0)).cuda()
    out = torch.empty((SLOTS, 3, R, R), device="cuda")
    lr = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (SLOTS, 3, L, L)).astype(np.float32)).cuda() if a.lr else None
    torch.cuda.synchronize()

    def hold_uniform(on, offset=0):
        """the per-call setting of the uniform forms (row b of a call at image offset k is held to lr[(k + b) % SLOTS]);
        off before every row session, which refuses it"""
        if lr is not None:
            eng.set_lr_consistency(lr.data_ptr() if on else None, SLOTS, L, L, offset, 1.0)

    def rows_begin():
        hold_uniform(False)
        eng.rows_begin(SLOTS, R, R, seed)
        if lr is not None:
            eng.rows_lr_consistency(L, L)

    def lr_kw(i):
        return {} if lr is None else {"lr": lr[i % SLOTS].data_ptr()}

    def set_T(T):
        eng.set_schedule(schedule.schedule_buffers({"schedule": "linear", "n_timestep": T, "linear_start": 1e-6, "linear_end": 1e-2}))

    def admit_all(B, start=None, ids=None):
        for s in range(B):
            i = s if ids is None else ids[s]
            if start is None:
                eng.rows_admit(s, cond[i % SLOTS].data_ptr(), i, **lr_kw(i))
            else:
                eng.rows_admit(s, cond[i % SLOTS].data_ptr(), i, init_ptr=cond[i % SLOTS].data_ptr(), start_step=start, **lr_kw(i))

    res = {"tool": "rolling_bench", "device": torch.cuda.get_device_name(0), "lr_consistency": bool(a.lr),
           "library": os.environ.get("SR3_LIB") or "in-tree",
           "shape": {"slots": SLOTS, "lres": L, "res": R, "unet": "yml image_size=224"}}

    # ---- step: rolling against uniform, all rows live --------------------------------------------------------------
    if "step" not in skip:
        T = 1000
        set_T(T)
        res["step"] = {}
        for prec in ("f32", "f16f8"):
            eng.set_precision(prec)
            n = a.block

            def uniform_block():
                hold_uniform(True)
                eng.sample_begin(cond.data_ptr(), SLOTS, R, R, None, seed, 0)
                for t in range(T - 1, T - 4, -1):       # eager step, capture, one replay
                    eng.sample_step(t)
                eng.synchronize()
                t0 = time.perf_counter()
                for t in range(T - 4, T - 4 - n, -1):
                    eng.sample_step(t)
                eng.synchronize()
                return (time.perf_counter() - t0) / n * 1e3

            def rolling_block():
                rows_begin()
                admit_all(SLOTS)
                for _ in range(3):
                    eng.rows_step()
                eng.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    eng.rows_step()
                eng.synchronize()
                ms = (time.perf_counter() - t0) / n * 1e3
                eng.rows_end()
                return ms

            uniform_block(); rolling_block()            # warm-up: workspace, both graphs
            u, r = [], []
            for _ in range(a.rounds):
                u.append(uniform_block())
                r.append(rolling_block())
            fam = {}
            for name, block in (("uniform", uniform_block), ("rolling", rolling_block)):
                eng.profile_enable(True)
                eng.profile_reset()
                block()
                p = eng.profile_get()
                eng.profile_enable(False)
                fam[name] = {k: round(v["ms"] / (n + 3), 4) for k, v in p.items()}
            um, rm = statistics.median(u), statistics.median(r)
            res["step"][prec] = {"uniform_ms": [round(x, 4) for x in u], "rolling_ms": [round(x, 4) for x in r],
                                 "uniform_median": round(um, 4), "rolling_median": round(rm, 4),
                                 "ratio": round(rm / um, 5),
                                 "uniform_spread": round((max(u) - min(u)) / um, 5),
                                 "within_uniform_spread": bool(min(u) <= rm <= max(u)),
                                 "family_ms_per_step_profiled": fam}

    eng.set_precision(a.precision)
    T, N = a.T, a.requests
    set_T(T)

    # ---- stream: N requests waiting at time zero ---------------------------------------------------------------------
    if "stream" not in skip:
        one = torch.empty((3, R, R), device="cuda")
        # warm-up of the three workspaces' graphs happens inside each timing's first steps; the workspace changes between
        # the forms (B = 64 | 1), so each form is timed after a short run of its own
        def rolling_stream():
            rows_begin()
            nxt, done, first = 0, 0, None
            held = [None] * SLOTS
            t0 = time.perf_counter()
            while done < N:
                for s in range(SLOTS):
                    if held[s] is None and nxt < N:
                        eng.rows_admit(s, cond[nxt % SLOTS].data_ptr(), nxt, **lr_kw(nxt))
                        held[s] = nxt
                        nxt += 1
                eng.rows_step()
                retired = 0
                for s in range(SLOTS):
                    if held[s] is not None and eng.rows_position(s) == 0:
                        eng.rows_retire(s, out[s].data_ptr())
                        held[s] = None
                        retired += 1
                done += retired
                if retired and a.precision != "f32":
                    eng.range_check()           # what RollingSampler.poll does before it hands results out
                if retired and first is None:
                    eng.synchronize()
                    first = time.perf_counter() - t0
            eng.synchronize()
            sec = time.perf_counter() - t0
            eng.rows_end()
            return sec, first

        def uniform_batches():
            t0, first = time.perf_counter(), None
            for k in range(0, N, SLOTS):
                hold_uniform(True, k)
                eng.sample(cond.data_ptr(), SLOTS, R, R, out.data_ptr(), None, seed, k)
                if first is None:
                    eng.synchronize()
                    first = time.perf_counter() - t0
            eng.synchronize()
            return time.perf_counter() - t0, first

        def one_by_one():
            t0, first = time.perf_counter(), None
            for k in range(N):
                hold_uniform(True, k)
                eng.sample(cond[k % SLOTS].data_ptr(), 1, R, R, one.data_ptr(), None, seed, k)
                if first is None:
                    eng.synchronize()
                    first = time.perf_counter() - t0
            eng.synchronize()
            return time.perf_counter() - t0, first

        res["stream"] = {"precision": a.precision, "T": T, "requests": N, "arrival": "all waiting at time zero"}
        hold_uniform(True)
        eng.sample(cond.data_ptr(), SLOTS, R, R, out.data_ptr(), None, seed, 0)     # warm-up at B = 64 (both graphs below)
        rows_begin(); admit_all(SLOTS)
        for _ in range(3):
            eng.rows_step()
        eng.rows_end()
        eng.synchronize()
        for name, fn in (("rolling_64_slots", rolling_stream), ("uniform_batches_of_64", uniform_batches)):
            sec, first = fn()
            res["stream"][name] = {"s": round(sec, 3), "images_per_s": round(N / sec, 2), "first_result_s": round(first, 3)}
        hold_uniform(True)
        eng.sample(cond.data_ptr(), 1, R, R, one.data_ptr(), None, seed, 0)         # warm-up at B = 1
        eng.synchronize()
        sec, first = one_by_one()
        res["stream"]["one_by_one_B1"] = {"s": round(sec, 3), "images_per_s": round(N / sec, 2), "first_result_s": round(first, 3)}

    # ---- mixed strengths -----------------------------------------------------------------------------------------------
    if "mixed" not in skip:
        rs = np.random.RandomState(3)
        strengths = rs.choice([0.25, 0.5, 1.0], SLOTS)
        starts = [max(1, int(round(float(s) * T))) for s in strengths]

        def rolling_mixed():
            rows_begin()
            t0 = time.perf_counter()
            for s in range(SLOTS):
                eng.rows_admit(s, cond[s].data_ptr(), s, init_ptr=cond[s].data_ptr(), start_step=starts[s], **lr_kw(s))
            steps = 0
            while eng.rows_step():
                steps += 1
            for s in range(SLOTS):
                eng.rows_retire(s, out[s].data_ptr())
            eng.synchronize()
            sec = time.perf_counter() - t0
            eng.rows_end()
            return sec, steps

        def uniform_per_strength():
            t0 = time.perf_counter()
            for s0 in sorted(set(starts)):
                rows = [i for i in range(SLOTS) if starts[i] == s0]
                c = cond[rows].contiguous()
                if lr is not None:      # (the group's own LR rows, in its order)
                    y = lr[rows].contiguous()
                    eng.set_lr_consistency(y.data_ptr(), len(rows), L, L, 0, 1.0)
                eng.sample(c.data_ptr(), len(rows), R, R, out.data_ptr(), None, seed, 0, init_ptr=c.data_ptr(), start_step=s0)
            eng.synchronize()
            return time.perf_counter() - t0

        rolling_mixed(); uniform_per_strength()          # warm-up: the workspaces and graphs of every batch size
        r_sec, r_steps = rolling_mixed()
        u_sec = uniform_per_strength()
        r_sec2, _ = rolling_mixed()
        res["mixed"] = {"precision": a.precision, "T": T, "requests": SLOTS,
                        "per_strength": {str(s0): starts.count(s0) for s0 in sorted(set(starts))},
                        "rolling_s": round(r_sec, 3), "rolling_again_s": round(r_sec2, 3), "rolling_steps": r_steps,
                        "uniform_calls_s": round(u_sec, 3), "uniform_steps": int(sum(sorted(set(starts)))),
                        "rolling_over_uniform": round(r_sec / u_sec, 4)}
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
