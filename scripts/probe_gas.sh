#!/bin/sh
# The measurements of the windowed background collisions (scripts/probe_gas.py), fp32 and fp64:
# scripts/probe_gas.sh <outdir> [particles] [grid].  First the host's own choices beside the reference passes
# (fpic_collide's null pass, one sub-step's push, count() over v2), then each form forced by FPIC_GAS_FORMS in a process of
# its own (the switch is read once): 4 the wave-shared loop, 8 the LDS queue, 1 the word first, 2 the window first.  Stops at the first step that fails.
OUT=$1; N=${2:-500000000}; GRID=${3:-256}
mkdir -p "$OUT" || exit 1
timeout -k 10 600 python3 scripts/probe_gas.py --particles "$N" --grid "$GRID" --references > "$OUT/time_0.txt" 2>&1 || { tail -20 "$OUT/time_0.txt"; exit 1; }
cat "$OUT/time_0.txt"
for FORMS in 4 8 1 2; do
    FPIC_GAS_FORMS=$FORMS timeout -k 10 600 python3 scripts/probe_gas.py --particles "$N" --grid "$GRID" > "$OUT/time_$FORMS.txt" 2>&1 || { tail -20 "$OUT/time_$FORMS.txt"; exit 1; }
    cat "$OUT/time_$FORMS.txt"
done
