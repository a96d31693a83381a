#!/bin/sh
# Kernel times of the selection pass beside the histogram pass, fp32 and fp64, each in a rocprofv3 run of its own (kernel trace
# and stats only, no counters): scripts/probe_select.sh <outdir> [particles] [grid].  Stops at the first step that fails.
OUT=$1; N=${2:-500000000}; GRID=${3:-256}
mkdir -p "$OUT" || exit 1
TRACES=$(mktemp -d) || exit 1      # the traces themselves are large and stay out of <outdir>
for P in fp32 fp64; do
    timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACES/$P" -o k -- \
        python3 scripts/probe_select.py run --precision $P --particles "$N" --grid "$GRID" --labels "$OUT/$P.labels.json" > "$OUT/$P.run.txt" 2>&1 || { tail -20 "$OUT/$P.run.txt"; exit 1; }
    python3 scripts/probe_select.py report --trace "$TRACES/$P" --labels "$OUT/$P.labels.json" > "$OUT/$P.report.txt" || exit 1
    cat "$OUT/$P.report.txt"
    find "$TRACES/$P" -name "*kernel_stats.csv" -exec cp {} "$OUT/$P.kernel_stats.csv" \;
done
