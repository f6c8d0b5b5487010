#!/bin/bash
# dev aid: autotune N times, keep every tune db with its frames/s under $OUT (default tune_search/)
# usage: [OUT=dir] tools/tune_search.sh [N]
O=${OUT:-tune_search}
mkdir -p $O
for i in $(seq 1 ${1:-6}); do
  rm -f $O/db_$i.json
  python bench.py --full --no-cpu-baseline --retune --tune-db $O/db_$i.json 2>/dev/null | tail -1 | python3 -c "
import sys,json; d=json.loads(sys.stdin.read()); print($i, d['value'], d['roofline']['frac'])" | tee -a $O/results.txt
done
