"""Kernel times of the fluid moment passes (fpic_moments) beside the parent kernels that do comparable work, on ONE state:
a box of --grid^3 nodes with one thermal species of --particles.  Two modes:

  run      build the state (torch on the device, uploaded in blocks), call moments("n") and moments("order2") once on the
           species as loaded (the flat pass), then precalc() and --steps step()s (electrostatic: push3_tiles_kernel per
           sub-step; full EM, --solver yee: em_push_tiles_kernel) and --calls times each: density() (full EM:
           em_rho_tiles_kernel), moments "n", "order1", "order2" (the tiled pass).  Meant to run under
           `rocprofv3 --kernel-trace --stats --output-format csv` (scripts/probe_moments.sh); writes the order of the calls
           to --labels.
  report   reads the kernel trace of such a run and the labels, and prints per case: calls, launches per call, mean / min /
           max kernel time per call, LDS (or global) atomics per second; and the yardstick kernels' times.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

MOMENTS = {"n": 1, "order1": 4, "order2": 10}
C = 2.998e8


def run(args):
    import numpy as np
    import torch
    import fusionpic as fp
    n, grid, vth = args.particles, args.grid, 1e-3
    L = grid * 3e-4
    dt = 0.5 / (C * np.sqrt(3.0) * grid / L) if args.solver == "yee" else 1e-11
    spec = dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=dt, nparticles=0, count=n, particle_mass=9.109e-31,
                particle_charge=-1.602e-19, geometry="cart3d", solver=args.solver, macro_weight=1.0)
    sim = fp.makeCylindricalParticlePusher(spec, precision=args.precision)
    dev = torch.device("cuda", 0)
    T = torch.float32 if args.precision == "fp32" else torch.float64
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    block = 1 << 24
    for first in range(0, n, block):
        m = min(block, n - first)
        pos = torch.rand((m, 3), dtype=T, device=dev, generator=gen) * (L * 0.999)
        vel = torch.randn((m, 3), dtype=T, device=dev, generator=gen) * vth
        torch.cuda.synchronize()
        sim.setRange(first, position=pos, velocity=vel)
    del pos, vel
    torch.cuda.empty_cache()
    order = []

    def call(which, path):
        m = sim.moments(which)
        total = (int((m["N"] >> 32).sum()) << 32) + int((m["N"] & 0xFFFFFFFF).sum())    # (beyond int64 above 2^21 particles)
        assert m["rejected"] == 0 and total == n << 42
        order.append([which, path, m["spilled"]])
        return m

    call("n", "flat")
    call("order2", "flat")
    sim.precalc()
    sim.step(args.steps)
    for rep in range(args.calls + 1):      # (the first round warms every shape up; the report drops it)
        if args.solver == "yee":
            sim.density()
        for which in MOMENTS:
            call(which, "tiled")
    with open(args.labels, "w") as f:
        json.dump(dict(order=order, particles=n, grid=grid, precision=args.precision, calls=args.calls, solver=args.solver, steps=args.steps), f)
    sim.destroy()
    print("ran %d rounds of %d calls on %d particles, %s, %s" % (args.calls + 1, len(MOMENTS), n, args.precision, args.solver))


def report(args):
    meta = json.load(open(args.labels))
    files = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    mom, other = [], {}
    for r in csv.DictReader(open(files[0])):
        name, t = r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if "mom_tiles_kernel" in name or "mom_flat_kernel" in name:
            mom.append((int(r["Start_Timestamp"]), t, name))
        elif "push3_tiles_kernel" in name or "em_rho_tiles_kernel" in name or "em_push_tiles_kernel" in name:
            other.setdefault(name, []).append(t)
    mom.sort()
    n = meta["particles"]
    calls = len(meta["order"])
    flat_launches = sum(1 for m in mom if "mom_flat_kernel" in m[2])
    tiled_calls = [o for o in meta["order"] if o[1] == "tiled"]
    tiled_launches = [m for m in mom if "mom_tiles_kernel" in m[2]]
    # launches per tiled call: the same for every round (sweeps of n + order1 + order2)
    rounds = meta["calls"] + 1
    per_round = len(tiled_launches) // rounds
    assert per_round * rounds == len(tiled_launches) and flat_launches == 2, (len(tiled_launches), rounds, flat_launches)
    print("%s, %s, %d^3 nodes, %d particles, %d calls of each request after %d steps; spilled of the last order2 call: %d"
          % (meta["precision"], meta["solver"], meta["grid"], n, meta["calls"], meta["steps"], meta["order"][-1][2]))
    print("%-28s %5s %8s %10s %10s %10s %12s" % ("case", "calls", "launches", "mean ms", "min ms", "max ms", "atomics/s"))
    flat = [m for m in mom if "mom_flat_kernel" in m[2]]
    for (which, _, _), m in zip(meta["order"][:2], flat):
        print("%-28s %5d %8d %10.3f %10.3f %10.3f %12.3g" % ("flat " + which, 1, 1, m[1] * 1e-6, m[1] * 1e-6, m[1] * 1e-6, 8.0 * MOMENTS[which] * n / (m[1] * 1e-9)))
    # sweeps per request in launch order: found from the round's launches by the known split (sweeps(n) = 1, the rest by size)
    sweeps = {}
    rest = per_round - 1
    # order1 and order2 take ceil(4 / fit) and ceil(10 / fit) sweeps for the same fit: try the fits
    for fit in range(1, 11):
        s1, s2 = -(-4 // fit), -(-10 // fit)
        if s1 + s2 == rest:
            sweeps = {"n": 1, "order1": s1, "order2": s2}
            break
    assert sweeps, per_round
    at = 0
    times = {}
    for rnd in range(rounds):
        for which in MOMENTS:
            t = sum(m[1] for m in tiled_launches[at:at + sweeps[which]])
            at += sweeps[which]
            if rnd:
                times.setdefault(which, []).append(t)
    for which, t in times.items():
        mean = sum(t) / len(t)
        print("%-28s %5d %8d %10.3f %10.3f %10.3f %12.3g" % ("tiled " + which, len(t), sweeps[which], mean * 1e-6, min(t) * 1e-6, max(t) * 1e-6, 8.0 * MOMENTS[which] * n / (mean * 1e-9)))
    print("yardsticks (every launch of the run but the first of each kernel):")
    for name, t in sorted(other.items()):
        t = t[1:] if len(t) > 1 else t
        print("  %5d launches  mean %10.3f ms  min %10.3f ms  max %10.3f ms  %s" % (len(t), sum(t) / len(t) * 1e-6, min(t) * 1e-6, max(t) * 1e-6, name[:150]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "report"])
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--solver", default="poisson_fft")
    ap.add_argument("--particles", type=int, default=500_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--labels", default="mom_labels.json")
    ap.add_argument("--trace", default=".")
    a = ap.parse_args()
    run(a) if a.mode == "run" else report(a)
