#!/bin/bash
# Run on an MI355X: rocprofv3 evidence for the two secondary workloads -- BASELINE configs[2] (HiFi-GAN
# 64 x 1024 frames) and configs[4] on one GPU (inpaint + image-to-audio): kernel trace + stats of the bench command itself,
# then HBM-side FETCH_SIZE / WRITE_SIZE in their own passes (kernel trace only, as the MI355X guide prescribes).
# Usage: bash scripts/gpu_profile_secondary.sh <tag> [precision]
tag=${1:-r3}; prec=${2:-bf16x3}
ROOT=$(cd "$(dirname "$0")/.." && pwd)      # the repository; results go to $OUT (a directory, relative to it or absolute)
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
: "${OUT:?set OUT to the directory the results go to}"; mkdir -p "$OUT"
for wl in ${WORKLOADS:-hifigan64 mixed}; do
  if [ $wl = mixed ]; then steps="--steps 1 --warmup 1"; pmc_args="--steps 1 --warmup 0 --ddim-steps 4 --no-graph"; else steps="--steps 2 --warmup 1"; pmc_args="--steps 1 --warmup 0"; fi
  timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_${tag}_$wl -o bench -- python bench.py --full --workload $wl $steps --precision $prec --no-cpu-baseline > $OUT/${tag}_${wl}_bench_under_rocprof.json 2> $OUT/${tag}_${wl}_prof.err
  python scripts/prof_summary.py $OUT/prof_${tag}_$wl/bench_results.db > $OUT/${tag}_${wl}_kernel_stats.txt
  rm -rf $OUT/prof_${tag}_$wl
  out=$OUT/${tag}_${wl}_pmc_fetch_write.txt
  echo "# rocprofv3 --kernel-trace --pmc <set> -- python bench.py --workload $wl $pmc_args --no-roofline --no-cpu-baseline   (sums over the launches of each kernel; FETCH_SIZE / WRITE_SIZE in KiB-units as rocprofv3 reports them; on gfx950 FETCH_SIZE counts half the bytes of wide streaming reads -- double it)" > $out
  for set in "FETCH_SIZE GRBM_GUI_ACTIVE" "WRITE_SIZE GRBM_GUI_ACTIVE"; do
    n=$(echo $set | cut -d_ -f1)
    timeout 600 rocprofv3 --kernel-trace --pmc $set -d $OUT/pmc_${tag}_${wl}_$n -o pmc -- python bench.py --workload $wl $pmc_args --precision $prec --no-roofline --no-cpu-baseline > $OUT/pmc_${tag}_${wl}_$n.log 2>&1
    echo "== $set" >> $out
    python scripts/pmc_summary.py $OUT/pmc_${tag}_${wl}_$n/pmc_results.db 80 | grep -v "^# columns" >> $out 2>&1
    rm -rf $OUT/pmc_${tag}_${wl}_$n
  done
  # third pass: matrix-pipe occupancy; then the per-launch table bench.py's `secondary` rooflines read (profiles/pmc_traffic.json)
  timeout 600 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE -d $OUT/pmc_${tag}_${wl}_SQ -o pmc -- python bench.py --workload $wl $pmc_args --precision $prec --no-roofline --no-cpu-baseline > $OUT/pmc_${tag}_${wl}_SQ.log 2>&1
  echo "== SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE" >> $out
  python scripts/pmc_summary.py $OUT/pmc_${tag}_${wl}_SQ/pmc_results.db 80 | grep -v "^# columns" >> $out 2>&1
  rm -rf $OUT/pmc_${tag}_${wl}_SQ
  if [ $wl = mixed ]; then units=4; else units=1; fi
  python scripts/pmc_traffic_json.py $out $prec $units profiles/pmc_traffic.json --section $wl && cp profiles/pmc_traffic.json $OUT/${tag}_pmc_traffic.json
  head -12 $OUT/${tag}_${wl}_kernel_stats.txt | cut -c1-170
done
