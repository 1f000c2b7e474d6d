#!/bin/bash
# the bench with everything it can measure (--full: roofline, extras, cpu baseline), timed; plans measured on the way are kept
# usage: tools/gpu_bench_full.sh [output directory, default bench_full]
out=${1:-bench_full}
mkdir -p $out
export UD_GEMM_TUNE_CACHE=$PWD/$out/plans.json
t0=$(date +%s)
python bench.py --full > $out/bench_full.json 2> $out/bench_full.err
echo "bench exit $? in $(( $(date +%s) - t0 )) s"
python3 - <<PY
import json
d=json.loads(open("$out/bench_full.json").read().strip().splitlines()[-1])
print({k:d[k] for k in ("value","ms_per_step")})
for e in d.get("extra",[]): print(e)
r=d["roofline"]; print({k:r[k] for k in ("achieved","peak","frac","launches_per_step","traffic")}); print(r["kernel"][:40]); print(r["families"])
print(d.get("cpu_baseline"))
PY
