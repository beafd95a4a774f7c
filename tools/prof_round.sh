#!/bin/bash
# Round-end evidence: decoder HBM traffic (PMC passes, tools/pmc_bench.sh) and a
# rocprofv3 kernel-trace --stats run of the full bench command.
# usage: tools/prof_round.sh TAG OUTDIR   (writes OUTDIR/pmc_TAG, OUTDIR/stats_TAG)
REPO=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:?usage: tools/prof_round.sh TAG OUTDIR}
OUT=$(realpath -m "${2:?usage: tools/prof_round.sh TAG OUTDIR}")
mkdir -p "$OUT"
cd "$REPO"
bash tools/pmc_bench.sh "$OUT/pmc_$TAG" > "$OUT/pmc_$TAG.log" 2>&1
echo "pmc rc=$?"; tail -5 "$OUT/pmc_$TAG.log"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$OUT/stats_$TAG" -o st --output-format csv -- python3 "$REPO/bench.py" --full > "$OUT/stats_$TAG.json" 2> "$OUT/stats_$TAG.err"
echo "stats rc=$?"; tail -c 600 "$OUT/stats_$TAG.json"
