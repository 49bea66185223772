#!/bin/bash
# One bench.py --full run (PMC + CPU leg included) from the repository root; record and log go to OUTDIR:  bash tools/r03_bench_only.sh OUTDIR
O=${1:?usage: tools/r03_bench_only.sh OUTDIR}; mkdir -p "$O" && python bench.py --full > "$O/bench.json" 2> "$O/bench.err"; tail -c 200 "$O/bench.err"
