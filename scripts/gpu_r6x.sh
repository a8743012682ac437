#!/bin/bash
# Final round-6 evidence: the driver's default bench line with every leg (--full), then the whole GPU suite.
cd "$(dirname "$0")/.."; O=${OUT_DIR:-bench_out}; mkdir -p "$O"
timeout -k 10 600 python3 -u bench.py --full --steps 20 --warmup 5 > "$O/r6x_bench.json" 2> "$O/r6x_bench.err"
rc=$?; echo "bench rc $rc"; tail -c 1500 "$O/r6x_bench.json"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 1500 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$O/r6x_suite.log" 2>&1
rc=$?; tail -3 "$O/r6x_suite.log"; exit $rc
