#!/bin/sh
# The measurements of the absorbing particle sinks (scripts/probe_remove.py), one process per precision, each
# under rocprofv3 --kernel-trace --stats (no counters; the program after --) and its own time limit:
# scripts/probe_remove.sh <outdir> [particles] [grid].  <outdir>/time_<precision>.txt is the probe's JSON line,
# <outdir>/<precision>/ the profiler's tables; the summary of both goes to stdout (profiles/remove_kernel_stats.txt is a copy).
# Stops at the first step that fails.
OUT=$1; N=${2:-500000000}; GRID=${3:-256}
mkdir -p "$OUT" || exit 1
for P in fp32 fp64; do
    timeout -k 10 540 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/$P" -o "$P" -- \
        python3 scripts/probe_remove.py --particles "$N" --grid "$GRID" --precision "$P" > "$OUT/time_$P.txt" 2>&1 || { tail -20 "$OUT/time_$P.txt"; exit 1; }
    echo "== $P"
    grep '^{' "$OUT/time_$P.txt"
    STATS=$(find "$OUT/$P" -name '*kernel_stats.csv' | head -1)
    [ -n "$STATS" ] && grep -E 'Name|remove_|renumber_|select_kernel|load_scan|push3_|bin3_|sort_scatter|fft|gradient|kspace|iota3' "$STATS" | cut -c1-260
done
