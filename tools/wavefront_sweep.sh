#!/bin/bash
# wavefront mode (HRT_FUSED=0) on C4 at 16 spp: hipGraph replay off / on.
# Usage: tools/wavefront_sweep.sh <outdir>
OUT=${1:-gpurun_out/wavefront}; mkdir -p $OUT
for graph in 0 1; do
  HRT_FUSED=0 HRT_WAVEFRONT_GRAPH=$graph HRT_BENCH_NO_TIMING=1 python3 bench.py --full --steps 3 --warmup 1 --spp 16 --no-alt-builder --cpu-seconds 6 > $OUT/wf_$graph.json 2> $OUT/wf_$graph.err
  python3 -c "
import json
try:
    d=json.loads(open('$OUT/wf_$graph.json').read().strip().splitlines()[-1]); print('wavefront graph=$graph :', d['value'], 'Mrays/s', d['ms_per_step'], 'ms; parity', d.get('parity', {}).get('linear_radiance_bit_exact'))
except Exception as e: print('wavefront graph=$graph FAILED', e)
" | tee -a $OUT/wavefront.txt
done
