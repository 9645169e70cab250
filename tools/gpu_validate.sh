#!/bin/bash
export TMPDIR=/tmp
out=${1:?usage: tools/gpu_validate.sh OUTPUT_DIR}
mkdir -p "$out"
timeout 1500 python -m pytest tests -x -q -m gpu > "$out/validate_tests.log" 2>&1
echo "all gpu tests rc=$?"; tail -5 "$out/validate_tests.log"
python bench.py --full > "$out/validate_bench.json" 2> "$out/validate_bench.err"; echo "bench rc=$?"; cat "$out/validate_bench.json"
python bench.py --steps 20 --warmup 5 > "$out/validate_bench_driver_flags.json" 2>/dev/null; cut -c1-400 "$out/validate_bench_driver_flags.json"
python3 tools/prof_head.py r02 headline C2 FWD C4 C5 READS > "$out/validate_prof.log" 2>&1; echo "prof rc=$?"
cat gpurun_out/head_counters.json | head -40
for c in C2 FWD C4 C5 READS; do echo "== $c"; cat gpurun_out/r02_$c.txt; done
