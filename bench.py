#!/usr/bin/env python3
"""Headline benchmark: SR images/sec for the full SR3 p_sample_loop (16->128) on MI355X.

    python bench.py --gpus 1 --steps K --warmup W [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is ONE p_sample step (UNet forward + DDPM update, reference diffusion.py:182-187) over
one batch of B images per GPU; an image needs T such steps, so
    value [img/s] = n_gpus * B / (T * seconds_per_step).
Every step costs the same (the step index only changes scalars), so K timed steps measure the
loop; `--steps T` times the whole loop. Workload = BASELINE.json configs[1]:
sr_sr3_VGGF2_16_128, batch 64 per GPU, T = 1000, yml-literal UNet (92.6 M parameters,
89.0 GFLOP per image per step), synthetic conditioning images and synthetic weights.
Inputs are resident in HBM before the timed region. Multi-GPU: the batch is sharded (weak
scaling, 64 images per GPU), no collective inside the loop, one RCCL all-gather of the finished
images at the end of the timed region.

A plain run sets up, warms up, times the K steps, writes `--dump-outputs` if asked and prints the JSON line: the
headline (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`) and the workload's `config`. The
headline is measured in the REFERENCE's arithmetic: fp32 operands, fp32 accumulation (`--precision f32`,
v_mfma_f32_32x32x2_f32; reference unet.py:235-265 / diffusion.py:164-187 compute in plain fp32). The library's faster
split-f16 arithmetics are reported next to it under `--full`, never as `value`.

`--full` runs everything else after the timed region and adds to the line (`--no-alt`, `--no-cpu-baseline`,
`--no-full-loop` leave parts out)
  roofline     the conv implicit-GEMM kernel family of the headline mode: algorithmic FLOPs / HIP-event time per
               launch against the dense MFMA peak of the mode's instruction — 157.3 TFLOP/s (f32-input MFMA) for f32,
               2500 TFLOP/s (f16 MFMA) for the split-f16 modes (f16f8 is priced against the f16 peak too) — plus
               `executed_frac` (MFMA work issued: 3 MFMA MACs per product in f16x3, 16/36 of the MACs on the sub-pixel
               Upsample convs) and `traffic` (HBM bytes per conv launch from the committed PMC summary of that mode)
  alt_precisions  one FULL block per other arithmetic mode of the same library measured in the same run: ms per step,
               img/s, its own `roofline` object and its own `parity` (below)
  parity       max-abs of the GPU against the CPU oracle on the cpu_baseline sample, with the sample REPLICATED to the
               benchmark batch (B = 64) so that every mode runs the kernels it runs in the timed region (f16f8 takes
               its fp8 path only at full batch); every replica is compared
  full_loop    ONE whole sr3_sample call (T steps, intermediate frames recorded) timed end to end in the headline
               mode (and in the fastest alternative mode): the sustained rate next to the K-step figure;
               `fallback_calls` must stay 0 (no range-policy replay hidden in the figure)
  cpu_baseline oracle/sr3_oracle_aten.py (the build's restatement on torch's CPU operators — what the
               reference's CPU path runs on) timed on this host on a bounded sample ("port-aten").
None of it touches the timed steps, `value` or what `--dump-outputs` writes.

`--dump-outputs DIR` writes what the timed path returned after its last timed step — the images sr3_sample_end hands
the caller (all ranks' images, gathered, with N > 1) — to DIR/images.npy in float32. The inputs are seeded, so two
builds run with the same arguments can be compared output for output. Beyond 64 MB a fixed, seeded sample of the
images is written instead, with their batch indices in DIR/images_index.npy.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

# the host driver of this pool only supports dmabuf IPC: RCCL (and any cross-process CUDA-tensor
# sharing) needs this before the HSA runtime starts; already exported on the benchmark boxes
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = "3d-super-resolution-face-reconstruction_amd"
sys.path.insert(0, ROOT)

# MI355X_MICROARCH.md, dense peaks: v_mfma_f32_32x32x2_f32 (= f32 vector peak) and f16/bf16 MFMA
PEAK_TFLOPS = {"f32": 157.3, "f16x3": 2500.0, "f16f8": 2500.0}      # (f16f8 priced against the f16 peak too)
DTYPE = {"f32": "f32 (fp32 operands, fp32 accumulate: the reference's arithmetic)", "f16x3": "f16x3-split (hi+lo fp16 operands, 3 MFMA per product, fp32 accumulate)",
         "f16f8": "f16x3-split with the two correction products of the 32x32 / 16x16-pixel convs on the fp8 MFMA (e4m3, fp32 accumulate)"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU")
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--lres", type=int, default=16)
    ap.add_argument("--T", type=int, default=1000, help="diffusion steps per image (BASELINE configs[1]: 1000)")
    ap.add_argument("--image-size", type=int, default=224, help="UNet image_size key: 224 = yml-literal, 128 = 6 attention modules")
    ap.add_argument("--precision", default="f32", choices=["f32", "f16x3", "f16f8"],
                    help="arithmetic of the HEADLINE: f32 = the reference's (default); the split-f16 modes are "
                         "reported as alt_precisions (--full)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure the roofline pass, the other arithmetic modes, the whole-loop "
                         "call, the CPU baseline and the GPU-vs-CPU parity (a plain run measures the headline only)")
    ap.add_argument("--no-alt", action="store_true", help="with --full: skip the measurement of the other arithmetic modes")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the parity")
    ap.add_argument("--no-full-loop", action="store_true", help="with --full: skip the timed whole-loop sr3_sample call (N=1 only)")
    ap.add_argument("--cpu-batch", type=int, default=4)
    ap.add_argument("--cpu-steps", type=int, default=32)
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write the images of the last timed step to DIR/images.npy (float32, at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_BYTES = 64 << 20


def dump_outputs(path, images):
    """--dump-outputs: `images` [N,3,r,r] as DIR/images.npy (float32). Over DUMP_BYTES, a fixed, seeded sample of the
    images (ascending batch index) is written, and its indices as DIR/images_index.npy (float64)."""
    os.makedirs(path, exist_ok=True)
    a = np.ascontiguousarray(images, dtype=np.float32)
    files = {}
    if a.nbytes > DUMP_BYTES:
        n = a.shape[0]
        keep = (DUMP_BYTES - 8 * n) // a[0].nbytes       # room for the index file
        idx = np.sort(np.random.RandomState(0).choice(n, keep, replace=False))
        a = a[idx]
        np.save(os.path.join(path, "images_index.npy"), idx.astype(np.float64))
        files["images_index"] = [int(idx.shape[0])]
    np.save(os.path.join(path, "images.npy"), a)
    files["images"] = list(a.shape)
    return files


def cpu_baseline(cfg, sd, sched_opt, args, synth):
    """CPU baseline on a bounded sample of the same workload. Returns (record, sample) where `sample` holds the
    inputs and the CPU result so that every GPU arithmetic mode can be checked against it (gpu_parity).

    The timed code is oracle/sr3_oracle_aten.py: the build's own restatement of the reference's sampler on torch's
    CPU operators (F.conv2d / F.group_norm / bmm) — the operator library the reference's CPU path itself runs on
    (nn.Conv2d / nn.GroupNorm, unet.py:62,84,87) — pinned to the reference-made fixtures by
    tests/test_oracle_golden.py. Never the reference's files (they do not exist on the GPU box)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import sr3_oracle_aten as aten      # checker / baseline only
    B, r, T, K = args.cpu_batch, args.res, args.T, args.cpu_steps
    cond = synth.synth_cond(B, r, args.lres, 4242)
    noise = synth.synth_noise(K + 1, B, 3, r, r, 4242)
    sch = aten.noise_schedule(sched_opt)
    tsd = aten.to_torch_state(sd)
    tc = torch.from_numpy(cond)
    x = torch.from_numpy(noise[0].copy())
    # intra-op threads: torch's default (one per logical CPU) oversubscribes these small convolutions on a 128-core
    # host (measured: 0.55 s per image-step with 128 threads, slower than 8 vCPUs), so one untimed step is run per
    # candidate count and the fastest is used for the timed sample — a baseline tuned in the CPU's favour
    default_threads = torch.get_num_threads()
    trial = {}
    with torch.no_grad():
        aten.p_sample(tsd, cfg, sch, x, T - 1, tc, torch.from_numpy(noise[1].copy()))      # untimed warm-up (thread pool, allocator)
        for n in sorted({n for n in (8, 16, 32, 64, default_threads) if n <= default_threads}):
            torch.set_num_threads(n)
            aten.p_sample(tsd, cfg, sch, x, T - 1, tc, torch.from_numpy(noise[1].copy()))
            ts = time.perf_counter()
            aten.p_sample(tsd, cfg, sch, x, T - 1, tc, torch.from_numpy(noise[1].copy()))
            trial[n] = time.perf_counter() - ts
        threads = min(trial, key=trial.get)
        torch.set_num_threads(threads)
        t0 = time.perf_counter()
        for k in range(K):
            x = aten.p_sample(tsd, cfg, sch, x, T - 1 - k, tc, torch.from_numpy(noise[k + 1].copy()))
        dt = time.perf_counter() - t0
        # one UNet evaluation (diffusion.py:170) mid-schedule on the same inputs: the denoiser's own output, before the
        # clamp of the update step (which hides most of an arithmetic's error in the first steps of a chain)
        t_mid = T // 2
        nl_mid = float(np.float32(sch["sqrt_alphas_cumprod_prev"][t_mid + 1]))
        eps_want = aten.unet_forward(tsd, cfg, torch.cat([tc, torch.from_numpy(noise[0])], dim=1),
                                     torch.full((B, 1), nl_mid, dtype=torch.float32)).numpy()
    base = {
        "value": B / (T * dt / K), "unit": "img/s", "cores": int(threads), "kind": "port-aten",
        "host_cpus": os.cpu_count(), "thread_trials_s_per_step": {str(k): round(v, 3) for k, v in trial.items()},
        "sample": (f"{K} p_sample steps of B={B} at {r}x{r} with oracle/sr3_oracle_aten.py (torch {torch.__version__} CPU "
                   f"operators, {threads} intra-op threads = the fastest of {sorted(trial)} on one untimed step each, {dt:.1f} s), scaled to T={T}"),
        "provenance": ("the reference's own torch-CPU path measured by the survey in the build container (8 vCPU): "
                       "0.25 s per image-step at 128x128 => ~0.004 img/s at T=1000 (BASELINE.md section 2); "
                       "the reference itself cannot run on the GPU box"),
    }
    return base, {"cond": cond, "noise": noise, "want": x.numpy(), "K": K, "eps_want": eps_want, "nl_mid": nl_mid}


def gpu_parity(eng, torch, sample, args, precision, batch):
    """The CPU sample's K steps on the GPU in `precision`, with the sample replicated to `batch` images (replica j of
    sample image i is batch row j * b + i, same injected noise) so that the kernels of the timed region run — the
    f16f8 mode takes its fp8 path only where conv_f8_supported(batch, ...) — and EVERY replica is compared."""
    metrics = importlib.import_module(PKG + ".metrics")
    cond, noise, want, K = sample["cond"], sample["noise"], sample["want"], sample["K"]
    b, r, T = cond.shape[0], args.res, args.T
    rep = max(1, batch // b)
    B = rep * b
    dc = torch.from_numpy(cond).cuda().repeat(rep, 1, 1, 1).contiguous()
    dn = torch.from_numpy(noise).cuda().repeat(1, rep, 1, 1, 1).contiguous()     # [K+1][B][3][r][r]
    out = torch.empty((B, 3, r, r), dtype=torch.float32, device="cuda")
    prev = eng.precision
    eng.set_precision(precision)
    fb0 = eng.fallback_calls()
    torch.cuda.synchronize()
    slab = B * 3 * r * r * 4
    eng.sample_begin(dc.data_ptr(), B, r, r, dn.data_ptr())
    for k in range(K):
        eng.sample_step(T - 1 - k, dn.data_ptr() + (k + 1) * slab)
    eng.sample_end(out.data_ptr())
    eng.synchronize()
    got = out.cpu().numpy().reshape(rep, b, 3, r, r)
    # the denoiser's output itself (one UNet forward at the mid-schedule noise level, same replication)
    xin = torch.cat([dc, dn[0]], dim=1).contiguous()
    nl = torch.full((B,), sample["nl_mid"], dtype=torch.float32, device="cuda")
    eps = torch.empty((B, 3, r, r), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.unet_forward(xin.data_ptr(), nl.data_ptr(), B, r, r, eps.data_ptr())
    eng.synchronize()
    eps_err = float(np.abs(eps.cpu().numpy().reshape(rep, b, 3, r, r) - sample["eps_want"][None]).max())
    eng.set_precision(prev)
    err = np.abs(got - want[None]).max(axis=(1, 2, 3, 4))          # per replica
    st = metrics.batch_psnr_stats(got.reshape(B, 3, r, r), np.tile(want, (rep, 1, 1, 1)))
    # psnr_db: mean over the images that differ after uint8 rounding (null if none differs — JSON has
    # no Infinity); identical_after_rounding counts the images whose PSNR is infinite
    return {"max_abs": float(err.max()), "max_abs_best_replica": float(err.min()), "batch": B, "replicas": rep,
            "unet_forward_max_abs": eps_err, "unet_forward_rms": float(np.sqrt(np.mean(sample["eps_want"] ** 2))),
            "psnr_db": st["mean_db"], "identical_after_rounding": st["identical"], "images": st["n"], "steps": K,
            "tolerance": 1e-3, "vs": "oracle/sr3_oracle_aten.py on the cpu_baseline sample",
            "fallback_calls": eng.fallback_calls() - fb0}


def full_loop(eng, torch, B, r, T, cond, sec_per_step, precision):
    """One whole p_sample_loop through sr3_sample (T steps, frames recorded like continous=True)."""
    out = torch.empty((B, 3, r, r), dtype=torch.float32, device="cuda")
    frames = torch.empty((eng.num_frames(), B, 3, r, r), dtype=torch.float32, device="cuda")
    prev = eng.precision
    eng.set_precision(precision)
    fb0 = eng.fallback_calls()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.sample(cond.data_ptr(), B, r, r, out.data_ptr(), None, 7, 0, frames.data_ptr())
    eng.synchronize()
    dt = time.perf_counter() - t0
    fb = eng.fallback_calls() - fb0
    eng.set_precision(prev)
    ok = bool(torch.isfinite(out).all().item()) and float(out.abs().max().item()) <= 1.0
    # a range-policy replay (f16f8 -> f16x3 -> f32 segments) would be correct but slower and would make this figure a
    # mixture of arithmetics: it must not happen silently
    assert fb == 0, f"full_loop in {precision}: {fb} range-policy fallback(s) inside the timed call"
    return {"precision": precision, "fallback_calls": fb,
            "seconds": dt, "img_per_s": B / dt, "T": T, "frames": int(frames.shape[0]), "batch": B,
            "ms_per_step": dt / T * 1e3,
            "vs_step_extrapolation_pct": 100.0 * (dt / (T * sec_per_step) - 1.0),
            "finite_and_clamped": ok,
            "note": "one sr3_sample call: init + T steps (hipGraph replay) + frame copies + final copy, host-timed"}


def pmc_summary(precision):
    """The committed rocprofv3 PMC summary of this arithmetic mode (tools/pmc_summary.py; counters collected and
    corrected as MI355X_MICROARCH.md prescribes, separate --pmc passes); None if there is none."""
    path = os.path.join(ROOT, "profiles", f"pmc_latest_{precision}.json")
    try:
        with open(path) as f:
            return json.load(f)
    except Exception:
        return None


def pmc_traffic(precision):
    """HBM bytes of the conv family per sampler step (PMC FETCH_SIZE / WRITE_SIZE passes)"""
    d = pmc_summary(precision)
    try:
        return d["per_step"]["conv_igemm"]["hbm_bytes"]
    except Exception:
        return None


def pmc_mfma_busy(precision):
    """SQ_VALU_MFMA_BUSY_CYCLES over the SIMD cycles of the conv family (north_star's 'MFMA utilisation', target >= 0.40)"""
    d = pmc_summary(precision)
    try:
        return d["sq"]["conv_igemm"]["mfma_busy_frac_of_simd_cycles"]
    except Exception:
        return None


def main():
    args = parse()
    # Exactly ONE line may reach stdout (the JSON record). librccl prints a version banner to fd 1 when its first
    # communicator is created (seen with SR3_FORCE_COLLECTIVE=1 on one GPU), so fd 1 is pointed at stderr for the
    # whole run and the record is written to the saved descriptor at the end.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    distm = importlib.import_module(PKG + ".dist")
    synth = importlib.import_module(PKG + ".synth")
    graph = importlib.import_module(PKG + ".graph")
    schedule = importlib.import_module(PKG + ".schedule")
    Engine = importlib.import_module(PKG + ".engine").Engine

    # RCCL over xGMI in production; SR3_DIST_BACKEND=gloo rehearses the N > 1 control flow (barriers,
    # max-over-ranks timing, gather, rank-0 report) where fewer GPUs than ranks exist
    backend = os.environ.get("SR3_DIST_BACKEND", "nccl")
    rank, world, local = distm.init_from_env(backend)
    if backend != "nccl":
        local = local % max(1, torch.cuda.device_count())
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with torch.distributed.run", file=sys.stderr)
        if world == 1 and args.gpus > 1:
            sys.exit(2)
    torch.cuda.set_device(local)
    B, r, T, K, W = args.batch, args.res, args.T, args.steps, args.warmup

    cfg = synth.yml_unet_config(args.image_size)
    sched_opt = {"schedule": "linear", "n_timestep": T, "linear_start": 1e-6, "linear_end": 1e-2}
    sd = synth.synth_state_dict(cfg, 2024)
    eng = Engine(cfg, local)
    eng.load_state_dict(sd)
    eng.set_schedule(schedule.schedule_buffers(sched_opt))
    eng.set_precision(args.precision)
    stream = torch.cuda.current_stream(local)
    eng.set_stream(stream.cuda_stream)

    # inputs resident in HBM: this rank's shard of the global batch (weak scaling)
    a, _ = distm.shard_bounds(B * world, world, rank)
    cond = torch.from_numpy(synth.synth_cond(B, r, args.lres, 1000 + rank)).cuda()
    out = torch.empty((B, 3, r, r), dtype=torch.float32, device="cuda")
    # SR3_FORCE_COLLECTIVE=1: the collective branch runs with one rank too (world-size-1 RCCL all-gather inside
    # the timed region, exactly as at N > 1) — exercises librccl on a single-GPU box
    collective = world > 1 or distm.force_collective()
    gathered = torch.empty((B * world, 3, r, r), dtype=torch.float32, device="cuda") if collective else None

    def run_steps(n, t_start):
        t = t_start
        for _ in range(n):
            eng.sample_step(t, None)         # device Philox noise
            t = t - 1 if t > 0 else T - 1
        return t

    def barrier():
        if collective:
            dist.barrier()
        torch.cuda.synchronize()

    eng.sample_begin(cond.data_ptr(), B, r, r, None, seed=7, image_offset=a)
    t_next = run_steps(W, T - 1)
    barrier()
    t0 = time.perf_counter()
    t_next = run_steps(K, t_next)
    eng.sample_end(out.data_ptr())
    eng.synchronize()        # explicit: the library may run on its own stream, the collective must see `out`
    if collective:
        if backend == "nccl":
            dist.all_gather_into_tensor(gathered, out)
        else:
            gathered = distm.all_gather_images(out.cpu(), B * world)
    barrier()
    dt = time.perf_counter() - t0
    if collective:
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        if world == 1 and rank == 0 and backend == "nccl":
            assert torch.equal(gathered, out), "world-size-1 all-gather must be the identity"
    sec_per_step = dt / K
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, (gathered if collective else out).cpu().numpy())

    # ---- per-mode blocks (rank 0): the headline mode first, then the other arithmetic modes of the same library
    def roofline_block(precision, steps, t_from, sec_step):
        """Conv family of `precision`: the same `steps` steps again with a HIP-event pair around every launch (events
        on the library's stream; a second pass so that event overhead never touches `value`)."""
        eng.profile_reset()
        eng.profile_enable(True)
        t_after = run_steps(steps, t_from)
        prof = eng.profile_get()
        if os.environ.get("SR3_PROFILE_CSV") and precision == args.precision:
            eng.profile_dump_csv(os.environ["SR3_PROFILE_CSV"])
        eng.profile_enable(False)
        conv = prof["conv_igemm"]
        n = max(1, conv["launches"])
        sec = conv["ms"] * 1e-3
        achieved = conv["flops"] / sec / 1e12 if sec > 0 else 0.0
        peak = PEAK_TFLOPS[precision]
        # MFMA work actually issued by the family: the sub-pixel Upsample convs execute 16/36 of their
        # algorithmic MACs, split-f16 issues 3 MFMA MACs per executed product
        up_alg = graph.upsample_flops_per_image(cfg, r, r) * B * steps
        executed = (conv["flops"] - up_alg * (20.0 / 36.0)) * (1.0 if precision == "f32" else 3.0)
        f8c_alg = 0.0
        if precision == "f16f8":
            # convs on the fp8 correction path issue 2/3 of f16x3's MFMA cycles (two f16 MFMAs + one fp8 MFMA of twice the
            # cycles instead of six): counted in f16-MFMA cycle equivalents
            f8c_alg = sum(2.0 * hh * ww * co * ci * 9 for hh, ww, ci, co in graph.resblock_conv3x3_shapes(cfg, r, r)
                          if eng.conv_f8_supported(B, hh, ww, co, ci)) * B * steps
            executed -= f8c_alg
        traffic = pmc_traffic(precision)
        note = {"f32": "Exact-f32 MFMA (v_mfma_f32_32x32x2_f32): the reference's arithmetic.",
                "f16x3": "Every executed MAC costs 3 f16 MFMA MACs (hi*hi + hi*lo + lo*hi); matrix-pipe busy: profiles/README.md.",
                "f16f8": ("executed_* in f16-MFMA cycle equivalents: 3 per product, 2 per product in the convs on the fp8 "
                          "correction path (f8c_flop_share of the family's algorithmic FLOPs).")}[precision]
        return t_after, {
            "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
            "traffic": (traffic / (n / steps)) if traffic else None,
            "traffic_unit": "HBM bytes per conv launch (rocprofv3 PMC summary profiles/pmc_latest_%s.json)" % precision,
            "mfma_pipe_busy": pmc_mfma_busy(precision),
            "mfma_pipe_busy_note": ("SQ_VALU_MFMA_BUSY_CYCLES / SIMD cycles over the conv family, from the same committed PMC summary "
                                    "(north_star's MFMA-utilisation target: >= 0.40)"),
            "executed_frac": (executed / sec / 1e12) / peak if sec > 0 else 0.0,
            "executed_mfma_tflops": executed / sec / 1e12 if sec > 0 else 0.0,
            "f8c_flop_share": f8c_alg / conv["flops"] if conv["flops"] else 0.0,
            "note": ("achieved = algorithmic conv FLOPs (the reference's conv arithmetic, SURVEY 8d) / HIP-event time per "
                     "logical conv; the Upsample convs execute 16/36 of their algorithmic MACs (sub-pixel phases). " + note),
            "kernel": "conv family: conv3x3_halo_h3<...> + conv_igemm_dma_f32<...> (all tile shapes)",
            "launches_per_step": n / steps, "avg_launch_ms": conv["ms"] / n, "flop_per_launch": conv["flops"] / n,
            "family_ms_per_step": {k: v["ms"] / steps for k, v in prof.items()},
            "whole_step_frac": (B * graph.flops_per_image(cfg, r, r) / sec_step / 1e12) / peak,
            "event_timed_step_ms": sum(v["ms"] for v in prof.values()) / steps,
        }

    roof = None
    alts = {}
    if rank == 0 and args.full:
        t_next, roof = roofline_block(args.precision, K, t_next, sec_per_step)
    if rank == 0 and args.full and not args.no_alt:
        t_a = t_next
        for other in [m for m in ("f32", "f16x3", "f16f8") if m != args.precision]:
            eng.set_precision(other)
            t_a = run_steps(max(1, W), t_a)
            torch.cuda.synchronize()
            ta0 = time.perf_counter()
            t_a = run_steps(K, t_a)
            torch.cuda.synchronize()
            sa = (time.perf_counter() - ta0) / K
            t_a, ra = roofline_block(other, min(K, 10), t_a, sa)
            alts[other] = {"precision": other, "dtype": DTYPE[other], "ms_per_step": sa * 1e3,
                           "img_per_s_1gpu": B / (T * sa), "roofline": ra}
        eng.set_precision(args.precision)
    if rank == 0:
        lo_hi = f"{args.lres}->{r}"
        res = {
            "metric": f"SR images/sec (full p_sample_loop, {lo_hi})",
            "value": world * B / (T * sec_per_step), "unit": "img/s",
            "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": sec_per_step * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPE[args.precision], "precision": args.precision, "data": "synthetic",
            "config": {"workload": f"sr_sr3_VGGF2_{args.lres}_{r} p_sample_loop, yml UNet image_size={args.image_size}",
                       "batch_per_gpu": B, "global_batch": B * world, "T": T,
                       "gflop_per_image_step": graph.flops_per_image(cfg, r, r) / 1e9,
                       "step": "one p_sample step (UNet forward + DDPM update) over the per-GPU batch",
                       "stages_not_run": ("BASELINE configs[4]'s MICA / FLAME stage is outside this path (SURVEY 8: untouched "
                                          "PyTorch encoder; FLAME assets and loguru absent): SR stage only"),
                       "parallelism": f"batch-sharded x{world}, one all-gather at the end" +
                                      (" (SR3_FORCE_COLLECTIVE: world-size-1 RCCL all-gather executed)" if collective and world == 1 else "")},
        }
        if args.full:
            res["roofline"] = roof
            res["alt_precisions"] = alts
        if args.full and world == 1 and not args.no_full_loop:
            res["full_loop"] = full_loop(eng, torch, B, r, T, cond, sec_per_step, args.precision)
            if alts:
                fastest = min(alts, key=lambda m: alts[m]["ms_per_step"])
                alts[fastest]["full_loop"] = full_loop(eng, torch, B, r, T, cond, alts[fastest]["ms_per_step"] * 1e-3, fastest)
        if args.full and not args.no_cpu_baseline and world == 1:
            base, sample = cpu_baseline(cfg, sd, sched_opt, args, synth)
            res["cpu_baseline"] = base
            res["parity"] = dict(gpu_parity(eng, torch, sample, args, args.precision, B), precision=args.precision)
            for m in alts:
                alts[m]["parity"] = gpu_parity(eng, torch, sample, args, m, B)
        res["fallback_calls"] = eng.fallback_calls()
        if dumped is not None:
            res["dumped_outputs"] = {"dir": args.dump_outputs, "shapes": dumped}
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(res, allow_nan=False) + "\n").encode())
    if collective:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()


if __name__ == "__main__":
    main()
