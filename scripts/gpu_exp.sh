#!/bin/bash
# Tuning experiments: bench under env-knob variants; prints conv time per variant.
cd "$(dirname "$0")/.."
O=${OUT_DIR:-gpu_results}   # output folder, relative to the repository root
mkdir -p $O
for v in "$@"; do
  env $v timeout 600 python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline > $O/exp.log 2>&1
  python - "$v" "$O/exp.log" <<'PY'
import json, sys
line = [l for l in open(sys.argv[2]) if l.startswith('{')]
if not line:
    print(sys.argv[1], 'FAILED'); print(open(sys.argv[2]).read()[-800:])
else:
    r = json.loads(line[-1])
    k = r['kernels']
    print(sys.argv[1], 'scenes/s', r['value'], 'ms', r['ms_per_step'], '| conv', k['conv_igemm']['ms'], 'TF', k['conv_igemm']['tflops'],
          '| lift', k['lift_pool']['ms'], 'gn', k['group_norm_stats']['ms'], 'pose', k['pose_score']['ms'], 'sim', k['sim_softmax']['ms'], 'ransac', k['ransac_sample']['ms'])
PY
done
