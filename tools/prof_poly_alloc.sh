#!/bin/bash
# tools/prof_poly_alloc.sh OUTDIR -- rocprofv3 --kernel-trace --stats of the poly bank's note events, one run per
# configuration of tools/explore_poly_alloc.py, plus one un-profiled run of all of them.  Run from the repo root on a
# machine with an MI355X; everything is written under OUTDIR (summary: profiles/poly_alloc_costs.txt).
set -e
[ $# -eq 1 ] || { echo "usage: $0 OUTDIR" >&2; exit 2; }
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
REPO=$PWD
cd /tmp
timeout -k 10 300 python3 "$REPO/tools/explore_poly_alloc.py" > "$OUT/unprofiled.jsonl"
for L in 18 22; do
  for MIX in silent full; do
    for E in 1 64 1024; do
      timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/n${L}_${MIX}_e${E}" \
        -- python3 "$REPO/tools/explore_poly_alloc.py" --one $L $MIX $E > "$OUT/n${L}_${MIX}_e${E}.json"
    done
  done
done
find "$OUT" -name "*kernel_stats.csv" | sort
