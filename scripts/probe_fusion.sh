#!/bin/sh
# The fusion yield tally's measurements (scripts/probe_fusion.py), fp32 and fp64: first the whole applications from HIP events
# in a run without a profiler, then the same script under rocprofv3 (kernel trace and stats only, no counters) for the
# kernels' own times: scripts/probe_fusion.sh <outdir> [particles] [grid].  Stops at the first step that fails.
OUT=$1; N=${2:-500000000}; GRID=${3:-256}
mkdir -p "$OUT" || exit 1
TRACES=$(mktemp -d) || exit 1      # the traces themselves are large and stay out of <outdir>
trap 'rm -rf "$TRACES"' EXIT
for P in fp32 fp64; do
    timeout -k 10 300 python3 scripts/probe_fusion.py --precision $P --particles "$N" --grid "$GRID" > "$OUT/$P.events.txt" 2>&1 || { tail -20 "$OUT/$P.events.txt"; exit 1; }
    tail -1 "$OUT/$P.events.txt"
    timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACES/$P" -o k -- \
        python3 scripts/probe_fusion.py --precision $P --particles "$N" --grid "$GRID" --calls 2 > "$OUT/$P.trace_run.txt" 2>&1 || { tail -20 "$OUT/$P.trace_run.txt"; exit 1; }
    find "$TRACES/$P" -name "*kernel_stats.csv" -exec cp {} "$OUT/$P.kernel_stats.csv" \;
    grep -E "Name|pair_|fusion_|push" "$OUT/$P.kernel_stats.csv"
done
