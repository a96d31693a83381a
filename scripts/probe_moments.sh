#!/bin/sh
# Kernel times of the moment passes beside the parent's push / density kernels, one rocprofv3 run (kernel trace and stats
# only, no counters) per precision and field mode: scripts/probe_moments.sh <outdir> [particles] [grid] ["fp32 fp64"] ["poisson_fft yee"].
# Stops at the first step that fails.
OUT=$1; N=${2:-500000000}; GRID=${3:-256}; PRECS=${4:-fp32 fp64}; SOLVERS=${5:-poisson_fft yee}
mkdir -p "$OUT" || exit 1
TRACES=$(mktemp -d) || exit 1      # the traces themselves are large and stay out of <outdir>
for S in $SOLVERS; do
for P in $PRECS; do
    timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$TRACES/$S.$P" -o k -- \
        python3 scripts/probe_moments.py run --precision $P --solver $S --particles "$N" --grid "$GRID" --labels "$OUT/$S.$P.labels.json" > "$OUT/$S.$P.run.txt" 2>&1 || { tail -20 "$OUT/$S.$P.run.txt"; exit 1; }
    python3 scripts/probe_moments.py report --trace "$TRACES/$S.$P" --labels "$OUT/$S.$P.labels.json" > "$OUT/$S.$P.report.txt" || { cat "$OUT/$S.$P.report.txt"; exit 1; }
    cat "$OUT/$S.$P.report.txt"
    find "$TRACES/$S.$P" -name "*kernel_stats.csv" -exec cp {} "$OUT/$S.$P.kernel_stats.csv" \;
done
done
