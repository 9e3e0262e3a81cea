#!/bin/bash
# On an MI355X: parity tests + smoke + short bench (+ optional rocprof).  Everything is logged under $LOG_DIR (default bench_out/).
# usage: [LOG_DIR=dir] scripts/gpu_check.sh [tests|bench|prof|all]
set -u
what=${1:-all}
cd "$(dirname "$0")/.."
LOG=$(realpath -m "${LOG_DIR:-bench_out}")
mkdir -p "$LOG"
rocminfo 2>/dev/null | grep -E "Marketing Name|gfx|Compute Unit" | head -6 > "$LOG/device.txt"
if [[ $what == tests || $what == all ]]; then
  timeout -k 10 1500 python -m pytest tests -m gpu -q --timeout=600 -p no:cacheprovider > "$LOG/pytest_gpu.log" 2>&1
  rc=$?; echo "pytest exit $rc" >> "$LOG/pytest_gpu.log"
  tail -40 "$LOG/pytest_gpu.log"
  [[ $rc == 0 ]] || exit $rc
  timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" > "$LOG/smoke.log" 2>&1
  rc=$?; echo "smoke exit $rc" >> "$LOG/smoke.log"
  tail -5 "$LOG/smoke.log"
  [[ $rc == 0 ]] || exit $rc
fi
if [[ $what == bench || $what == all ]]; then
  timeout -k 10 600 python bench.py --full --steps 2 --warmup 1 --detail-file "$LOG/bench_detail.json" > "$LOG/bench.log" 2> "$LOG/bench.err"
  rc=$?; echo "bench exit $rc"; tail -3 "$LOG/bench.log"; tail -5 "$LOG/bench.err"
  [[ $rc == 0 ]] || exit $rc
fi
if [[ $what == prof || $what == all ]]; then
  R=$(pwd)
  ( cd /tmp && timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$LOG/prof" -o r1 -- python "$R/bench.py" --full --steps 1 --warmup 1 --no-cpu-baseline --detail-file "$LOG/prof_bench_detail.json" > "$LOG/prof_bench.log" 2> "$LOG/prof_bench.err" )
  echo "prof exit $?"
  find "$LOG/prof" -name "*stats*" | head
fi
