#!/bin/bash
# full GPU verification (gpurun): the -m gpu test suite, smoke(), the default bench line, and (with "profile") the rocprofv3
# kernel stats + PMC passes of tools/profile.sh for the headline datapath.  Results go to $OUT (default: out/)
OUT=${OUT:-out}
mkdir -p "$OUT"
timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -40 > "$OUT/check_tests.log"
timeout 200 python __graft_entry__.py smoke > "$OUT/check_smoke.log" 2>&1
timeout 900 python bench.py --full > "$OUT/check_bench.json" 2> "$OUT/check_bench.err"
tail -6 "$OUT/check_tests.log"; tail -3 "$OUT/check_smoke.log"; tail -c 600 "$OUT/check_bench.err"; head -c 1500 "$OUT/check_bench.json"
if [ "$1" == "profile" ]; then bash tools/profile.sh fp16x3 > "$OUT/check_profile.log" 2>&1; tail -5 "$OUT/check_profile.log"; fi
