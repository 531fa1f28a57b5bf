#!/bin/bash
# quick GPU check: the given pytest selection, then N benches (train + DDIM-50 + CFG lines); logs go to OUT
#   scripts/gpu_check.sh "PYTEST SELECTION" [N] [OUT]
set -e -o pipefail
SEL="$1"; NB="${2:-2}"; O="${3:-/tmp/dmc_gpu_check}"
mkdir -p "$O"
timeout -k 10 500 python -u -m pytest -x -q --timeout 200 --timeout-method thread $SEL > "$O/chk.log" 2>&1 || { tail -40 "$O/chk.log"; exit 1; }
tail -2 "$O/chk.log"
for i in $(seq $NB); do
  timeout -k 10 200 python -u bench.py --full --steps 30 --warmup 5 --no-cpu --no-extra --no-dit --no-roofline > "$O/b.json" 2>/dev/null
  python3 -c "import json, sys; d=json.load(open(sys.argv[1])); print('train', d['value'], 'ddim50', d.get('ddim50',{}).get('value'), 'cfg', d.get('ddim50_cfg',{}).get('value'))" "$O/b.json"
done
