#!/bin/bash
# dev: the whole GPU suite, then the full bench.  usage: tools/gpu_step.sh OUTDIR
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(realpath -m "${1:?usage: tools/gpu_step.sh OUTDIR}")
mkdir -p "$OUT"
cd "$REPO"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT/gputests.log" 2>&1
rc=$?
echo "tests rc=$rc"; tail -3 "$OUT/gputests.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 700 python -u bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
rc2=$?
echo "bench rc=$rc2"; tail -3 "$OUT/bench.err"; cat "$OUT/bench.json"
exit $rc2
