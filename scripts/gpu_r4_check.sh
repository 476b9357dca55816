#!/bin/bash
# Round-4 check: the whole -m gpu suite, smoke, the driver's bench command (with the C3/C4/C5 legs).
set -u
cd "$(dirname "$0")/.."
O=${OUT_DIR:-gpu_results}   # output folder, relative to the repository root
mkdir -p $O
export TMPDIR=/tmp
STAGES="${*:-tests smoke bench}"
for s in $STAGES; do
  case $s in
    tests)
      timeout 1500 python -m pytest tests -m gpu -q -x --timeout=900 2>&1 | tail -40 > $O/tests.log
      echo "== tests =="; tail -15 $O/tests.log ;;
    new)
      timeout 900 python -m pytest tests/test_gpu_distributed.py tests/test_gpu_kernels.py tests/test_gpu_backward.py tests/test_gpu_baseline_configs.py -m gpu -q --timeout=600 -k "rccl or nan or pose_score_bwd or mlp2_pool or vertical_pool or matching_dim_64 or c4_exhaustive" -s 2>&1 | tail -60 > $O/tests_new.log
      echo "== new tests =="; grep -E "passed|failed|RCCL1_OK|\[dist\]|Error|assert" $O/tests_new.log | head -30 ;;
    smoke)
      timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
      echo "== smoke =="; tail -3 $O/smoke.log ;;
    bench)
      T0=$SECONDS
      SNAP_BENCH_DUMP=$O/launches.json timeout 1200 python bench.py --full > $O/bench.log 2>$O/bench.err
      echo "== bench == wall $((SECONDS - T0)) s"; tail -c 6000 $O/bench.log; tail -5 $O/bench.err ;;
    trace)
      # kernel trace of 3 steps: GPU busy / idle time per step (tools/trace_gaps.py)
      rm -rf $O/trace
      (cd /tmp && timeout 600 rocprofv3 --kernel-trace --output-format csv -d "$OLDPWD/$O/trace" -o snap -- \
        python "$OLDPWD/bench.py" --steps 3 --warmup 2 --no-cpu-baseline --no-extra-legs) > $O/trace.log 2>&1
      f=$(find $O/trace -name '*kernel_trace.csv' | head -1)
      echo "== trace =="; tail -2 $O/trace.log | cut -c1-400
      [ -n "$f" ] && python tools/trace_gaps.py "$f" > $O/trace_gaps.txt && cat $O/trace_gaps.txt && rm -rf $O/trace ;;
  esac
done
