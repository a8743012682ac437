#!/bin/bash
# The driver's default bench line with every leg (--full), untraced (the traced run faulted inside tts_parler_generate).
cd "$(dirname "$0")/.."; O=${OUT_DIR:-bench_out}; mkdir -p "$O"
export TTS_HIP_CRASH_HANDLER=1
timeout -k 10 600 python3 -u bench.py --full --steps 20 --warmup 5 > "$O/r6i_bench.json" 2> "$O/r6i_bench.err"
rc=$?; echo "bench rc $rc"; tail -c 3000 "$O/r6i_bench.err"; tail -c 2500 "$O/r6i_bench.json"
exit $rc
