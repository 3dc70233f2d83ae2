#!/bin/bash
# The 16-frame flow_fix headline with the coupled two-stream split off / on (VFACE_SPLIT_COUPLED), interleaved.
# usage (on an MI355X): bash tools/ab_flow_fix_streams.sh <out-prefix>
out=${1:?usage: ab_flow_fix_streams.sh <out-prefix>}
for v in 0 1 0 1; do
VFACE_SPLIT_COUPLED=$v python bench.py --full --frames 16 --fusion flow_fix --steps 20 --warmup 3 --no-extras --no-cpu-baseline --inv-steps 0 > ${out}_$v.json 2>> ${out}.err
python - <<PY
import json
d=json.loads(open("${out}_$v.json").read().strip().splitlines()[-1])
print("coupled=$v", round(d["value"],3), "f/s", round(d["ms_per_step"],2), "ms/step streams", d["config"]["launch_streams"], "overlap", d["config"]["launch_stream_overlap"], "bits", d["config"]["timed_region_bits_equal_kernel_by_kernel"], flush=True)
PY
done
