#!/bin/bash
# the 2048^3 deposit with its accumulation / its stores switched off (dbg_tsc 0..3): gpu_deposit_ablate.sh OUTDIR
cd "$(dirname "$0")/.." || exit 1
O=${1:?usage: gpu_deposit_ablate.sh OUTDIR}; mkdir -p "$O"
for o in 0 1 2 3; do
  timeout -k 10 200 python3 bench.py --full --workload pk --nmesh 2048 --steps 3 --warmup 1 --no-cpu --option dbg_tsc=$o > "$O/tsc_$o.json" 2>/dev/null
  python3 - "$O/tsc_$o.json" $o <<'PY'
import json,sys
o=sys.argv[2]
d=json.load(open(sys.argv[1]))
k=d['kernels_ms']
print('dbg_tsc',o,'step',round(d['ms_per_step'],2),'deposit',k.get('tsc_tile_deposit'),'fine',k.get('tsc_lines_fine'))
PY
done
