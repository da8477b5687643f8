#!/usr/bin/env python3
"""Summarises rocprofv3 CSV output of `bench.py` runs into profiles/ (development tool).

    python tools/pmc_summary.py gpurun_out profiles/r01

Reads gpurun_out/p_stats (kernel-trace --stats), p_fetch (--pmc FETCH_SIZE), p_write
(--pmc WRITE_SIZE), p_sq (SQ counters) and writes <prefix>_kernel_stats.csv and
<prefix>_pmc_summary.json. HBM bytes follow MI355X_MICROARCH.md §HBM: FETCH_SIZE and WRITE_SIZE
are in KiB; on gfx950 FETCH_SIZE counts half of a wide coalesced read, so reads = 2*FETCH_SIZE*1024.
"""
import csv
import glob
import json
import shutil
import sys
from collections import defaultdict


def family(name):
    for key, fam in (("gn_wino_input", "gn_apply"),     # (the apply pass that writes a Winograd conv's transformed input)
                     ("conv_igemm", "conv_igemm"), ("conv3x3_halo", "conv_igemm"), ("conv_splitk", "conv_igemm"), ("wino_", "conv_igemm"),
                     ("conv_in_kernel", "conv_igemm"), ("final_conv", "conv_igemm"),
                     ("gn_partial", "gn_stats"), ("gn_finalize", "gn_stats"),
                     ("gn_apply", "gn_apply"), ("attention", "attention"), ("noise_embed", "embed"),
                     ("ddpm_update", "update"),
                     # runtime copy / fill kernels and the call's own set-up: ONCE per process or per call (the 266
                     # copyBuffer launches of a bench run are the staged host-to-device uploads of the 349 weight
                     # tensors, all in front of the first step; the fills zero the workspace) — never part of a step
                     ("__amd_rocclr_", "setup_once"), ("pack_state", "setup_once"), ("init_state", "setup_once"),
                     ("nchw_to_nhwc", "setup_once"),
                     # PER-CALL work: the final copy-out and, in the split-f16 modes, sr3_sample's checkpoint copies of the
                     # sampler state at every segment boundary (~10 per call) — not part of a step, but not
                     # "once" either: reported as a family of its own
                     ("nhwc_to_nchw", "per_call_copies")):
        if key in name:
            return fam
    return "other"


def load(d, pat):
    f = glob.glob(f"{d}/*/*{pat}")
    return list(csv.DictReader(open(f[0]))) if f else []


def main(src, prefix):
    out = {}
    ks = glob.glob(f"{src}/p_stats/*/*kernel_stats.csv")
    if ks:
        shutil.copy(ks[0], prefix + "_kernel_stats.csv")
    trace = load(f"{src}/p_stats", "kernel_trace.csv")
    dur = defaultdict(lambda: [0, 0.0])
    for r in trace:
        fam = family(r["Kernel_Name"])
        dur[fam][0] += 1
        dur[fam][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
    out["kernel_trace_ms"] = {k: {"launches": v[0], "total_ms": v[1], "avg_ms": v[1] / v[0]} for k, v in dur.items()}
    for tag, cname in (("p_fetch", "FETCH_SIZE"), ("p_write", "WRITE_SIZE")):
        acc = defaultdict(lambda: [0, 0.0])
        for r in load(f"{src}/{tag}", "counter_collection.csv"):
            if r["Counter_Name"] == cname:
                fam = family(r["Kernel_Name"])
                acc[fam][0] += 1
                acc[fam][1] += float(r["Counter_Value"])
        out[cname + "_KiB"] = {k: {"launches": v[0], "sum": v[1]} for k, v in acc.items()}
    hbm = {}
    for fam in out.get("FETCH_SIZE_KiB", {}):
        f, w = out["FETCH_SIZE_KiB"][fam], out.get("WRITE_SIZE_KiB", {}).get(fam, {"sum": 0, "launches": 1})
        n = max(1, f["launches"])
        hbm[fam] = {"read_bytes_per_launch": 2 * f["sum"] * 1024 / n, "write_bytes_per_launch": w["sum"] * 1024 / max(1, w["launches"])}
        hbm[fam]["bytes_per_launch"] = hbm[fam]["read_bytes_per_launch"] + hbm[fam]["write_bytes_per_launch"]
    out["hbm"] = hbm
    # one ddpm_update launch per sampler step: per-step totals (a logical conv of the engine can be
    # several device launches: 4 sub-pixel phases of an upsample conv, split-K + reduce)
    steps = max(1, out["kernel_trace_ms"].get("update", {}).get("launches", 1))
    out["steps"] = steps
    out["per_step"] = {fam: {"ms": v["total_ms"] / steps, "device_launches": v["launches"] / steps,
                             "hbm_bytes": (hbm.get(fam, {}).get("bytes_per_launch", 0.0) *
                                           out.get("FETCH_SIZE_KiB", {}).get(fam, {}).get("launches", 0)) /
                                          max(1, out["kernel_trace_ms"].get("update", {}).get("launches", 1))}
                       for fam, v in out["kernel_trace_ms"].items() if fam != "setup_once"}
    if "setup_once" in out["kernel_trace_ms"]:
        out["setup_once"] = dict(out["kernel_trace_ms"]["setup_once"],
                                 note="runtime copies / fills (weight upload, workspace zeroing) and per-call layout kernels: "
                                      "once per process or call, all outside the sampler steps")
    sq = defaultdict(lambda: defaultdict(float))
    for r in load(f"{src}/p_sq", "counter_collection.csv"):
        sq[family(r["Kernel_Name"])][r["Counter_Name"]] += float(r["Counter_Value"])
    for fam, c in sq.items():
        if c.get("GRBM_GUI_ACTIVE"):
            c["mfma_busy_frac_of_simd_cycles"] = c.get("SQ_VALU_MFMA_BUSY_CYCLES", 0) / 1024 / (c["GRBM_GUI_ACTIVE"] / 8)
    out["sq"] = {k: dict(v) for k, v in sq.items()}
    json.dump(out, open(prefix + "_pmc_summary.json", "w"), indent=1)
    print(json.dumps({"hbm": hbm, "mfma_busy": {k: v.get("mfma_busy_frac_of_simd_cycles") for k, v in out["sq"].items()},
                      "trace": out["kernel_trace_ms"]}, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
