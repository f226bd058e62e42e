#!/bin/bash
# Does a monitoring loop (rocm-smi polled back to back, as a bench driver's GPU-busy sampler does) stretch the FIRST call of a workload?
# The first call allocates (hipMalloc / hipFree = driver ioctls); the kernels do not.  VERDICT r4 weak 4: driver 441 ms vs builder 80 ms.
# usage: scripts/smi_interference.sh <out-dir> [runs (3)]
set -u
cd "$(dirname "$0")/.."
OUT=${1:-gpurun_out/r05}; RUNS=${2:-3}
mkdir -p "$OUT"
one() {  # $1 = tag
  python bench.py --full --configs motif3 --steps 3 --warmup 1 --traffic off --no-cpu-baseline --no-standins --detail "$OUT/smi_$1.json" > /dev/null 2> "$OUT/smi_$1.err"
  python - "$OUT/smi_$1.json" "$1" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
for c in d["configs"][1:]:
    print(sys.argv[2], c["workload"], "first_call_ms", c["first_call_ms"], "kernel_ms", c["kernel_ms_avg"], c["setup_ms"])
PY
}
for i in $(seq 1 "$RUNS"); do one "quiet$i"; done
( while true; do rocm-smi --showuse --showmemuse --showpower > /dev/null 2>&1; done ) &
SMI=$!
sleep 1
for i in $(seq 1 "$RUNS"); do one "polled$i"; done
kill $SMI 2>/dev/null; wait $SMI 2>/dev/null
echo done
