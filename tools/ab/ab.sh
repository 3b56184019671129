#!/bin/bash
# usage: ab.sh B libA.so libB.so ...   -> alternates the builds 3 times on this box, prints value per run
# (AB_ARGS: further bench.py arguments, e.g. "--paths 4"; AB_ROUNDS: rounds instead of 3).  A run that fails ends the script.
set -o pipefail
B=$1; shift
for r in $(seq 1 ${AB_ROUNDS:-3}); do
  for L in "$@"; do
    FSGM_LIB_PATH=$PWD/$L timeout -k 10 300 python bench.py --steps 10 --warmup 2 --full --no-cpu-baseline --frames-per-gpu $B $AB_ARGS 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$L', '%.4g'%d['value'], '%.3f ms'%d['ms_per_step'], 'checked', d.get('checked'))" || exit 1
  done
done
