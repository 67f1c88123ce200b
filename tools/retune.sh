#!/bin/bash
# Re-measure the per-shape (tile config, split-K) tables of the three bench workloads on the GPU box.
# usage: tools/retune.sh [fp32|bf16x3] [out_dir]   -> <out_dir>/tuned_<mode>_*.json (merge with tools/merge_tuned.py)
MODE=${1:-bf16x3}
O=${2:-${TMPDIR:-/tmp}/ppy_retune}; mkdir -p $O
export PPYOLO_HIP_MATH=$MODE
python bench.py --full --autotune --save-tuning $O/tuned_${MODE}_r50.json --no-cpu-baseline --no-alt-math > $O/bench_${MODE}_r50_tune.json 2> $O/bench_${MODE}_r50_tune.err
python bench.py --full --workload r18vd_416 --autotune --save-tuning $O/tuned_${MODE}_r18_416.json --no-cpu-baseline --no-alt-math > $O/bench_${MODE}_r18_416_tune.json 2>/dev/null
python bench.py --full --workload r18vd_320 --batch 1 --autotune --save-tuning $O/tuned_${MODE}_r18_320b1.json --no-cpu-baseline --no-alt-math > $O/bench_${MODE}_r18_320b1_tune.json 2>/dev/null
python bench.py --full --workload r18vd_320 --autotune --save-tuning $O/tuned_${MODE}_r18_320.json --no-cpu-baseline --no-alt-math > $O/bench_${MODE}_r18_320_tune.json 2>/dev/null
for f in $O/bench_${MODE}_*_tune.json; do python -c "import json,sys; d=json.load(open('$f')); print('$f', d['value'], d['roofline']['achieved'], d['roofline']['frac'])"; done
