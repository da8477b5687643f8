#!/bin/bash
# One-call evidence collection for a round (run through gpurun): kernel stats + PMC passes in the three arithmetic modes,
# the per-shape conv table, the default bench line with the full loop, every BASELINE config on one GPU, and the
# config-3 kernel stats.
#   bash tools/collect_round.sh OUT_DIR
# Outputs under OUT_DIR (created); summarise with tools/pmc_summary.py and copy into profiles/.
set -e
O=${1:?usage: bash tools/collect_round.sh OUT_DIR}
mkdir -p "$O"
bash tools/profile_round.sh f16f8 "$O" > "$O"/pr_f16f8.log 2>&1
bash tools/profile_round.sh f16x3 "$O" > "$O"/pr_f16x3.log 2>&1
bash tools/profile_round.sh f32 "$O" > "$O"/pr_f32.log 2>&1
python tools/step_profile.py --batch 64 --steps 20 --precision f16f8 --csv "$O"/conv_shapes_f16f8.csv > "$O"/sp64.txt 2>&1
python tools/step_profile.py --batch 64 --steps 20 --precision f16x3 --csv "$O"/conv_shapes_f16x3.csv >> "$O"/sp64.txt 2>&1
python tools/step_profile.py --batch 64 --steps 10 --precision f32 --csv "$O"/conv_shapes_f32.csv >> "$O"/sp64.txt 2>&1
python bench.py --full > "$O"/bench_full.log 2>&1
: > "$O"/configs.txt
run_cfg() { echo "== bench.py $*" >> "$O"/configs.txt; python bench.py "$@" --full --no-cpu-baseline 2>/dev/null | tail -n 1 >> "$O"/configs.txt; }
run_cfg --batch 4 --res 16 --lres 8 --T 100 --steps 100
run_cfg --image-size 128
run_cfg --lres 8
run_cfg --batch 32 --lres 32 --T 100 --steps 50
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
rm -rf "$O"/prof_cfg3
rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/prof_cfg3 -- python3 bench.py --image-size 128 --steps 5 --warmup 1 --full --no-alt --no-cpu-baseline --no-full-loop > "$O"/cfg3.log 2>&1
# the "other" kernels of a step (copies / fills): with and without hipGraph replay
rm -rf "$O"/prof_nograph
SR3_NO_GRAPH=1 rocprofv3 --kernel-trace --stats --output-format csv -d "$O"/prof_nograph -- python3 bench.py --steps 5 --warmup 1 --full --no-alt --no-cpu-baseline --no-full-loop > "$O"/nograph.log 2>&1
(python tools/step_profile.py --batch 1 --steps 30; python tools/step_profile.py --batch 4 --steps 30; python tools/step_profile.py --batch 4 --res 16 --lres 8 --T 100 --steps 30) > "$O"/small_batch.txt 2>&1
tail -n 1 "$O"/bench_full.log | cut -c1-300
