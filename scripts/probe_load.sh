#!/bin/sh
# The loader's measurements (scripts/probe_load.py): the kernel's ulp deviations, then the three timings of DESIGN.md 4.15 —
# load(), the setRange uploads of the same population, a plain fill of the six arrays — and the two-pass form, fp32 and fp64:
# then the profiled load (fpic_load_profile) against load() and the uploads in one run, and the radial load
# (fpic_load_radial) against load() and a three-table profiled load in another:
# scripts/probe_load.sh <outdir> [particles] [grid].  Stops at the first step that fails.
OUT=$1; N=${2:-500000000}; GRID=${3:-256}
mkdir -p "$OUT" || exit 1
timeout -k 10 300 python3 scripts/probe_load.py ulps > "$OUT/ulps.txt" 2>&1 || { tail -20 "$OUT/ulps.txt"; exit 1; }
cat "$OUT/ulps.txt"
timeout -k 10 900 python3 scripts/probe_load.py time --particles "$N" --grid "$GRID" > "$OUT/time.txt" 2>&1 || { tail -20 "$OUT/time.txt"; exit 1; }
cat "$OUT/time.txt"
timeout -k 10 900 python3 scripts/probe_load.py profile --particles "$N" --grid "$GRID" > "$OUT/profile.txt" 2>&1 || { tail -20 "$OUT/profile.txt"; exit 1; }
cat "$OUT/profile.txt"
timeout -k 10 900 python3 scripts/probe_load.py radial --particles "$N" --grid "$GRID" > "$OUT/radial.txt" 2>&1 || { tail -20 "$OUT/radial.txt"; exit 1; }
cat "$OUT/radial.txt"
