#!/bin/bash
# Three arms of the fp32 bench on the SAME GPU box, alternating (tools/ab_bench.sh conventions: IDN_LIB, plain bench runs,
# one timeout per run, stop at the first failure):
#   off     the shipped library with the colour gate switched off (IDN_COLOUR_GATE=0)
#   <tagA>  ideal-nerf_amd/libidealnerf_<tagA>.so, gate on          (e.g. the parent commit's build)
#   new     the shipped ideal-nerf_amd/libidealnerf.so, gate on
# Usage: tools/ab_gate_arms.sh <tagA> [reps=3] [outdir=bench_outputs]      (the log is <outdir>/ab_gate_arms.log)
set -e -o pipefail
A=$1; REPS=${2:-3}; OUT=${3:-bench_outputs}; LOG=$OUT/ab_gate_arms.log
mkdir -p "$OUT"
: > "$LOG"
NEW="$PWD/ideal-nerf_amd/libidealnerf.so"
for rep in $(seq 1 "$REPS"); do
  for arm in off "$A" new; do
    case $arm in
      off) env="IDN_COLOUR_GATE=0 IDN_LIB=$NEW" ;;
      new) env="IDN_COLOUR_GATE=1 IDN_LIB=$NEW" ;;
      *)   env="IDN_COLOUR_GATE=1 IDN_LIB=$PWD/ideal-nerf_amd/libidealnerf_$arm.so" ;;
    esac
    env $env timeout -k 10 200 python bench.py --gpus 1 --steps 8 --warmup 2 > "$OUT/ab_tmp.json" 2> "$OUT/ab_err.log"
    python - "$rep" "$arm" "$OUT/ab_tmp.json" <<'PY' | tee -a "$LOG"
import json, sys
d = json.loads([l for l in open(sys.argv[3]) if l.startswith("{")][-1])
print(f"rep {sys.argv[1]} arm {sys.argv[2]:7s} value {d['value']:.5e} ray-samples/s  ms_per_step {d['ms_per_step']:.3f}  "
      f"mlp_kernel_ms {d['per_rank']['mlp_kernel_ms'][0]:.3f}  launches {d['roofline']['launches']}", flush=True)
PY
  done
done
