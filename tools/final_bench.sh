#!/bin/bash
# After tools/final_profiles.sh + tools/collect_profiles.py (so that the committed counter summary carries this build's stamp): the
# bench command under rocprofv3 (kernel stats + trace of its own launches) and the full bench line (bench.py --full).
# usage: bash tools/final_bench.sh <label> [output root, default out]   — everything goes to <output root>/<label>/ in the repository
L=${1:-final}; R=$(cd "$(dirname "$0")/.." && pwd); O=$R/${2:-out}/$L
cd $R; mkdir -p $O
make -s -C oracle
(cd /tmp && export TMPDIR=/tmp && timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $O/bench_command -- python3 $R/bench.py --steps 3 --warmup 1 --full --no-secondary --no-cpu-baseline > $O/bench_command.log 2>&1; echo "bench command rc=$?")
timeout -k 10 900 python3 bench.py --full > $O/final_bench.log 2>&1; echo "bench rc=$?"
grep '^{' $O/final_bench.log | tail -1 > $O/final_bench.json
grep '^{' $O/bench_command.log | tail -1 > $O/bench_command_line.json
python3 -c "
import json
j=json.load(open('$O/final_bench.json'))
r=j['roofline']
print('headline', j['ms_per_step'], 'ms', j['value'], 'Mrays/s', r['kernel'], r.get('bound'), r.get('bound_candidates'), 'stale', r.get('counters_stale'), 'frac', r.get('frac'), 'avg_launch_ms', r.get('avg_launch_ms'), 'rocprof', r.get('rocprof_avg_launch_ms'))
for s in j['secondary']: print(s['workload'][:40], s['ms_per_step'], s['mrays_per_s'], s.get('gpu_over_cpu'), s['roofline'].get('bound_candidates'))
print('cpu', j['cpu_baseline']['value'] if j.get('cpu_baseline') else None, j.get('gpu_over_cpu'))
"
