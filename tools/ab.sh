#!/bin/bash
# A/B of two libmpcx builds on one box (alternating runs): tools/ab.sh LIB_A LIB_B "bench args" reps
set -uo pipefail
A=$1; B=$2; ARGS=$3; R=${4:-2}
mkdir -p gpurun_out/ab
for i in $(seq 1 "$R"); do
  for L in "$A" "$B"; do
    n=$(basename "$L" .so)
    MPCX_LIB=$L MPCX_ALLOW_STALE_LIB=1 timeout -k 10 200 python3 bench.py --full $ARGS --no-cpu --no-roofline \
      > gpurun_out/ab/${n}_$i.json 2> gpurun_out/ab/${n}_$i.err || exit 1
    python3 -c "import json,sys;d=json.loads([l for l in open('gpurun_out/ab/${n}_$i.json') if l.startswith('{')][-1]);print('$n', d['value'], d['lockstep']['value'], d['solve_kernel']['us_per_ipm_iteration'])"
  done
done
