#!/bin/bash
# GPU tests (not -x: all failures at once), then the full bench unless pytest did not end normally.
# usage: tools/gpu_session.sh <outdir> <tag> [pytest args...]
out=$1; tag=$2; shift 2
mkdir -p "$out"
timeout -k 10 1000 python -m pytest tests -m gpu -q --durations=12 "$@" > "$out/${tag}_tests.log" 2>&1
rc=$?
echo "pytest rc=$rc" >> "$out/${tag}_tests.log"
tail -n 30 "$out/${tag}_tests.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 400 python bench.py --full > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err"
echo "bench rc=$?"; head -c 3000 "$out/${tag}_bench.json"
