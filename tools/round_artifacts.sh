#!/bin/bash
# Produces the evidence files of a round on the GPU box (run from the repo root): tools/round_artifacts.sh [OUT]
#   OUT/bench.json.log      the JSON line of an un-profiled default bench.py --full run
#   OUT/prof/               rocprofv3 --kernel-trace --stats of the same command (no CPU baseline, no host->host legs)
#   OUT/pmc/                PMC passes (tools/pmc_passes.sh) + summary.txt + traffic.json
# OUT (a directory relative to the repo root, bench_out by default) is scratch: copy what should be judged into
# profiles/ afterwards.
set -u
ROOT=$(pwd)
OUT=${1:-bench_out}
mkdir -p "$OUT"
timeout -k 10 420 python3 bench.py --full --steps 20 --warmup 3 > "$OUT/bench.json.log" 2> "$OUT/bench.err" || { echo "bench failed"; tail -5 "$OUT/bench.err"; exit 1; }
tail -c 600 "$OUT/bench.json.log"; echo
rm -rf "$OUT/prof"
(cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/$OUT/prof" -- python3 "$ROOT/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline --h2h-frames 0 > "$ROOT/$OUT/prof.log" 2>&1) || { echo "rocprofv3 stats failed"; tail -5 "$OUT/prof.log"; exit 1; }
echo "stats done"
rm -rf "$OUT/pmc"
timeout -k 10 600 bash tools/pmc_passes.sh "$OUT/pmc" > "$OUT/pmc_passes.log" 2>&1 || { echo "pmc failed"; tail -5 "$OUT/pmc_passes.log"; exit 1; }
python3 tools/pmc_summary.py "$OUT/pmc" > "$OUT/pmc/summary.txt"
python3 tools/make_traffic_json.py "$OUT/pmc" "$OUT/pmc/traffic.json" > /dev/null
grep -c . "$OUT/pmc/summary.txt"
