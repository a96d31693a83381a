#!/bin/sh
# The collision operator's measurements (scripts/probe_collide.py): the three reference passes and every case of DESIGN.md
# 4.16, fp32 and fp64: scripts/probe_collide.sh <outdir> [particles] [grid].  Stops at the first step that fails.
OUT=$1; N=${2:-500000000}; GRID=${3:-256}
mkdir -p "$OUT" || exit 1
timeout -k 10 900 python3 scripts/probe_collide.py --particles "$N" --grid "$GRID" > "$OUT/time.txt" 2>&1 || { tail -20 "$OUT/time.txt"; exit 1; }
cat "$OUT/time.txt"
