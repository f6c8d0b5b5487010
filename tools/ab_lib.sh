#!/bin/bash
# dev (GPU box): same-lease A/B of two builds of libcodd_hip.so: alternating bench.py runs, in-tree library vs $1
# usage: [ARGS="--precision fp32"] tools/ab_lib.sh ab/libcodd_hip_old.so [pairs] [steps]
# Every bench run has its own time limit; the first run that fails (a fault, a time limit) ends the script.
old=$1; n=${2:-3}; steps=${3:-100}
run() {  # $1 = value of CODD_LIB_AB ("" = the in-tree library)
  CODD_LIB_AB=$1 timeout -k 10 ${AB_TIMEOUT:-300} python bench.py --full --steps $steps --no-cpu-baseline --no-pmc-traffic --fp32-steps 0 --two-video-steps 0 $ARGS 2>/dev/null |
    python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['roofline']['ms_per_frame'], d['epe_vs_synthetic_gt'])"
}
set -o pipefail
for i in $(seq 1 $n); do
  a=$(run $PWD/$old) && b=$(run "") || { echo "pair $i: a bench run failed (rc $?); stopping"; exit 1; }
  echo "pair $i: old [$a]   new [$b]   (frames/s, conv_bf16 family ms/frame by HIP events, epe)"
done
