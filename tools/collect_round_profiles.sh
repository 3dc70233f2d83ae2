#!/bin/bash
# End-of-round profile collection: rocprofv3 kernel statistics of the bench with two / one launch sequences, the HBM traffic
# summary (tools/traffic.sh) and the per-launch step trace, all into <out-dir>.
# usage (on an MI355X, from the repo root): bash tools/collect_round_profiles.sh <out-dir>
set -o pipefail
export TMPDIR=/tmp; R=$PWD; O=$(realpath -m "${1:?usage: collect_round_profiles.sh <out-dir>}"); mkdir -p $O
rm -rf $O/stats1 $O/stats2; cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats2 -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --inv-steps 0 --no-extras > $O/stats2.json 2> $O/stats2.log
cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats1 -- python3 $R/bench.py --full --streams 1 --steps 5 --warmup 2 --no-cpu-baseline --inv-steps 0 --no-extras > $O/stats1.json 2> $O/stats1.log
cd $R && bash tools/traffic.sh $O/hbm_traffic.json --steps 3 --warmup 1 --no-cpu-baseline --inv-steps 0 --no-extras > $O/traffic.log 2>&1
cd $R && python3 tools/step_trace.py --frames 32 --fusion fft --reps 3 > $O/step_trace.txt 2>&1
ls $O; tail -3 $O/traffic.log
