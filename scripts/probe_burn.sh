#!/bin/sh
# The measurements of the fusion burn (scripts/probe_burn.py), one process per precision, each under rocprofv3
# --kernel-trace --stats (no counters; the program after --) and its own time limit:
# scripts/probe_burn.sh <outdir> [particles] [grid] [precisions].  <outdir>/time_<precision>.txt is the probe's JSON line,
# <outdir>/<precision>/ the profiler's tables; the summary of both and every dispatch of the deciding pass, the generation pass,
# the compaction, fusion_tally_kernel and remove_move_kernel go to stdout (profiles/burn_kernel_stats.txt is a copy).  Stops at
# the first step that fails.
OUT=$1; N=${2:-500000000}; GRID=${3:-256}; PRECISIONS=${4:-fp32 fp64}
mkdir -p "$OUT" || exit 1
for P in $PRECISIONS; do
    timeout -k 10 540 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/$P" -o "$P" -- \
        python3 scripts/probe_burn.py --particles "$N" --grid "$GRID" --precision "$P" > "$OUT/time_$P.txt" 2>&1 || { tail -20 "$OUT/time_$P.txt"; exit 1; }
    echo "== $P"
    grep '^{' "$OUT/time_$P.txt"
    STATS=$(find "$OUT/$P" -name '*kernel_stats.csv' | head -1)
    [ -n "$STATS" ] && grep -E 'Name|burn_|fusion_tally|pair_count|pair_scan|pair_fill|renumber_count|load_scan|remove_m|ionize_|iota3' "$STATS" | cut -c1-260
    TRACE=$(find "$OUT/$P" -name '*kernel_trace.csv' | head -1)
    [ -n "$TRACE" ] && python3 - "$TRACE" <<'PY'
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
for r in rows:
    name = r["Kernel_Name"]
    if "burn_" in name or "fusion_tally" in name or "remove_move" in name or "remove_mark" in name or "ionize_decide" in name or "ionize_generate" in name:
        print("dispatch %-64s %10.3f ms  grid %s" % (name[:64], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6, r.get("Grid_Size", r.get("Grid_Size_X", "?"))))
PY
done
