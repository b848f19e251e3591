#!/bin/bash
# The judged measurements of a build, in one box session: counter passes of the four bench workloads (atrium with the L1 / L2 passes),
# rocprofv3 kernel stats + trace of the bench command itself, and the full bench line (tools/final_bench.sh).   usage: bash tools/final_profiles.sh <label>
# afterwards: python tools/collect_profiles.py <label> r03; cp out/<label>/final_bench.json profiles/r03_final_bench.json ...
L=${1:-final}; R=$GRAFT_REPO_ROOT; cd $R; mkdir -p gpurun_out/$L
make -s -C oracle
HPRT_L1_PASSES=1 bash tools/counters_passes.sh $L atrium > gpurun_out/$L/passes_atrium.log 2>&1; tail -c 300 gpurun_out/$L/passes_atrium.log; echo
for w in killeroo-simple living-room instanced-10m; do bash tools/counters_passes.sh $L $w > gpurun_out/$L/passes_$w.log 2>&1; grep -h "rc=" gpurun_out/$L/passes_$w.log | cut -c1-150; done
bash tools/final_bench.sh $L
