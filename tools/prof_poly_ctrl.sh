#!/bin/bash
# tools/prof_poly_ctrl.sh OUTDIR [MAIN_TREE] -- the poly bank's controllers under rocprofv3 --kernel-trace --stats,
# one run per configuration of tools/explore_poly_ctrl.py, after un-profiled runs of all of them.  MAIN_TREE: another
# built tree (e.g. the parent commit) whose unbent block is timed alternately with this one's in the same call.
# Run from the repo root on a machine with an MI355X; everything is written under OUTDIR.
set -e
[ $# -ge 1 ] || { echo "usage: $0 OUTDIR [MAIN_TREE]" >&2; exit 2; }
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
REPO=$PWD
MAIN=${2:+$(cd "$2" && pwd)}
cd /tmp
for k in 1 2; do
  timeout -k 10 300 python3 "$REPO/tools/explore_poly_ctrl.py" >> "$OUT/unprofiled.jsonl"
  [ -z "$MAIN" ] || timeout -k 10 120 python3 "$REPO/tools/explore_poly_ctrl.py" --root "$MAIN" >> "$OUT/unprofiled.jsonl"
done
for C in "block64 18" "block64_bent 18" "sound_off 18" "sound_off 22" "pedal_up_128 18"; do
  set -- $C
  timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/$1_$2" \
    -- python3 "$REPO/tools/explore_poly_ctrl.py" --one $1 $2 > "$OUT/$1_$2.json"
done
if [ -n "$MAIN" ]; then
  timeout -k 10 180 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/main_block64_18" \
    -- python3 "$REPO/tools/explore_poly_ctrl.py" --root "$MAIN" --one block64 18 > "$OUT/main_block64_18.json"
fi
find "$OUT" -name "*kernel_stats.csv" | sort
