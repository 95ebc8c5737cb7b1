#!/bin/bash
# Alternating A/B of a variant library (tools/prof_lib/<v>/libpet_hip.so) against the built one on ONE box:
#   bash tools/debug/ab_bench.sh <v> [pairs = 4]   -> ms per step of every run (bench.py --steps 20 --warmup 5)
# Every run has a time limit of its own; the first run that fails ends the script (the built library is put back).
set -o pipefail
V=$1; PAIRS=${2:-4}
cp metatrain_amd/lib/libpet_hip.so /tmp/lib_base.so
trap 'cp /tmp/lib_base.so metatrain_amd/lib/libpet_hip.so' EXIT
for p in $(seq $PAIRS); do
  for v in base $V; do
    if [ $v = base ]; then cp /tmp/lib_base.so metatrain_amd/lib/libpet_hip.so; else cp tools/prof_lib/$v/libpet_hip.so metatrain_amd/lib/libpet_hip.so; fi
    timeout -k 10 200 python bench.py --steps 20 --warmup 5 --no-extras --no-cpu-baseline $AB_ARGS 2>/dev/null | python3 -c "
import sys, json
d=json.loads([l for l in sys.stdin if l.startswith('{')][-1])
print('   $v ms_per_step', round(d['ms_per_step'],3), flush=True)
" || { echo "run of $v failed: stopping"; exit 1; }
  done
done
