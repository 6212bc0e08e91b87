#!/bin/bash
# Same-box A/B of training steps: bench.py --workload $WORKLOAD alternating over the variants given
# as arguments, ROUNDS times.  A variant is a library path, optionally followed by env settings:
#   bash tools/ab_train.sh ab/head.so ab/cur.so "ab/cur.so LG_SKF_EXACT=1"
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
mkdir -p gpurun_out
variants=("$@")
for r in $(seq 1 ${ROUNDS:-2}); do
  for v in "${variants[@]}"; do
    read -r lib envs <<< "$v"
    env LIGHTGLUE_MI355X_LIB=$(realpath "$lib") $envs timeout -k 10 300 python3 bench.py --workload ${WORKLOAD:-train} --steps ${STEPS:-5} --warmup 2 --cpu-budget 0 > gpurun_out/ab_train_run.log 2>&1 || { echo "$v failed"; tail -5 gpurun_out/ab_train_run.log; exit 1; }
    python3 - "$v" <<'PY'
import json, sys
r = json.loads([l for l in open("gpurun_out/ab_train_run.log") if l.startswith("{")][0])
print(f"{sys.argv[1]:40s} {r['value']:8.2f} pairs/s  {r['ms_per_step']:7.1f} ms/step", flush=True)
PY
  done
done
