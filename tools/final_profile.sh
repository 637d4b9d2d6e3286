#!/bin/bash
# rocprofv3 kernel trace (+stats) of the default bench command; summary goes to profiles/ via tools/rocpd_summary.py
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${BENCH_OUT:-bench_out}; mkdir -p "$out"       # where the runs' lines and logs go
timeout 400 rocprofv3 --kernel-trace --stats -d $out/prof_$1 -o $1 -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-gaf > $out/prof_$1.log 2>&1
tail -1 $out/prof_$1.log | head -c 600
