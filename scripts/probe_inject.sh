#!/bin/sh
# The measurements of the particle sources (scripts/probe_inject.py), one process per precision, each under
# rocprofv3 --kernel-trace --stats (no counters; the program after --) and its own time limit:
# scripts/probe_inject.sh <outdir> [particles] [grid] [big].  <outdir>/time_<precision>.txt is the probe's JSON line,
# <outdir>/<precision>/ the profiler's tables; the summary of both and every dispatch of the generation kernel and of the
# loader's go to stdout (profiles/inject_kernel_stats.txt is a copy).  Stops at the first step that fails.
OUT=$1; N=${2:-500000000}; GRID=${3:-256}; BIG=${4:-50000000}
mkdir -p "$OUT" || exit 1
for P in fp32 fp64; do
    timeout -k 10 540 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/$P" -o "$P" -- \
        python3 scripts/probe_inject.py --particles "$N" --grid "$GRID" --big "$BIG" --precision "$P" > "$OUT/time_$P.txt" 2>&1 || { tail -20 "$OUT/time_$P.txt"; exit 1; }
    echo "== $P"
    grep '^{' "$OUT/time_$P.txt"
    STATS=$(find "$OUT/$P" -name '*kernel_stats.csv' | head -1)
    [ -n "$STATS" ] && grep -E 'Name|inject_kernel|reserve_copy|init3|load_slots|remove_|load_scan|push3_|bin3_|sort_scatter|fft|gradient|kspace|iota3' "$STATS" | cut -c1-260
    TRACE=$(find "$OUT/$P" -name '*kernel_trace.csv' | head -1)
    [ -n "$TRACE" ] && python3 - "$TRACE" <<'PY'
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
for r in rows:
    name = r["Kernel_Name"]
    if "inject_kernel" in name or "load_slots_kernel" in name or "reserve_copy" in name:
        print("dispatch %-60s %10.3f ms  grid %s" % (name[:60], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6, r.get("Grid_Size", r.get("Grid_Size_X", "?"))))
PY
done
