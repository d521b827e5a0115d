#!/bin/bash
# rocprofv3 kernel trace of a short bench (graph mode) for per-shape durations.  Usage: bash scripts/gpu_rocprof_short.sh <tag> <precision>
tag=${1:-x}; prec=${2:-bf16x3}
ROOT=$(cd "$(dirname "$0")/.." && pwd)      # the repository; results go to $OUT (a directory, relative to it or absolute)
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
: "${OUT:?set OUT to the directory the results go to}"; mkdir -p "$OUT"
rocprofv3 --kernel-trace -d $OUT/prof_$tag -o short -- python bench.py --full --steps 1 --warmup 0 --ddim-steps 12 --precision $prec --no-cpu-baseline --no-roofline > $OUT/short_$tag.json 2> $OUT/short_$tag.err
python scripts/rocprof_shapes.py $OUT/prof_$tag/short_results.db 12 > $OUT/shapes_rocprof_$tag.txt
rm -f $OUT/prof_$tag/short_results.db
python bench.py --full --steps 2 --warmup 1 --precision $prec --no-cpu-baseline > $OUT/bench_$tag.json 2> $OUT/bench_$tag.err
python -c "
import json; d=json.load(open('$OUT/bench_$tag.json')); print('VALUE', d['value'], d['ms_per_step']); print(json.dumps(d['roofline'])[:1200])"
head -50 $OUT/shapes_rocprof_$tag.txt
