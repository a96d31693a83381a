"""Kernel times of the modes diagnostic's partial pass (fpic_modes_*) beside the energy row's field pass on ONE state, and
what recording costs a run.  The box of scripts/probe_series.py: --grid^3 nodes, one thermal species of --particles (the
passes read grids only, so the default population is small).  Three modes:

  run      the electrostatic box after precalc(), then --calls + 1 rounds of: energy() (the yardstick: diag_field_kernel reads
           the same node records once), modes() with 16, 64 and 256 wave vectors of ex ey ez phi, and with 16 of all eight
           quantities; then step(3) and the same rounds again; then a full-EM box of the same grid (the node-centred B
           exists there) with 16 wave vectors of all eight.  Meant to run under `rocprofv3 --kernel-trace --stats
           --output-format csv` (scripts/probe_modes.sh); writes the order of the calls to --labels.
  report   reads the kernel trace of such a run and the labels, and prints per state and case: dispatches, mean / min / max
           kernel time of the partial pass and the ratio to the yardstick of the same state.
  cost     wall time of --substeps sub-steps of the self-consistent box with recordModes(every = 1, 16 wave vectors of ex ey
           ez phi) against the same sub-steps without, alternating, --calls times each, on one handle (no profiler).
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

from probe_series import build  # noqa: E402

E4 = ("ex", "ey", "ez", "phi")
ALL = ("ex", "ey", "ez", "phi", "bx", "by", "bz", "rho")
CASES = [("E x 16", 16, E4), ("E x 64", 64, E4), ("E x 256", 256, E4), ("all 8 x 16", 16, ALL)]


def wave_vectors(n, grid):
    import numpy as np
    rng = np.random.default_rng(5)
    seen = set()
    while len(seen) < n:
        seen.add(tuple(int(x) for x in rng.integers(-(grid // 2), grid // 2 + 1, 3)))
    return np.array(sorted(seen), dtype=np.int32)


def build_em(args, n=2_000_000):
    """the full-EM box of the same grid, its time step inside the lattice's stability bound"""
    import numpy as np
    import fusionpic as fp
    grid = args.grid
    dx = 3e-4
    L = grid * dx
    spec = dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=0.5 * dx / (2.998e8 * 3 ** 0.5), nparticles=0, count=n,
                particle_mass=9.109e-31, particle_charge=-1.602e-19, geometry="cart3d", solver="yee", macro_weight=1.0)
    sim = fp.makeCylindricalParticlePusher(spec, precision=args.precision)
    rng = np.random.default_rng(3)
    sim.set(position=rng.random((n, 3)) * (L * 0.999), velocity=rng.normal(0, 1e-3, (n, 3)))
    return sim


def run(args):
    import numpy as np
    order = []
    sim, L = build(args, "poisson_fft")
    sim.precalc()
    for state in ("after precalc", "after 3 steps"):
        if state == "after 3 steps":
            sim.step(3)
        for rep in range(args.calls + 1):      # (the first round of a state warms every shape up; the report drops it)
            sim.energy()
            order.append([state, "energy field pass", rep == 0])
            for label, n, fields in CASES:
                got = sim.modes(wave_vectors(n, args.grid), fields)
                assert np.isfinite(got["ex"]).all()
                order.append([state, label, rep == 0])
    sim.destroy()
    em = build_em(args)
    em.precalc()
    em.step(1)
    em.density()
    for rep in range(args.calls + 1):
        em.energy()
        order.append(["full EM", "energy field pass", rep == 0])
        got = em.modes(wave_vectors(16, args.grid), ALL)
        assert np.isfinite(got["bx"]).all() and np.isfinite(got["rho"]).all()
        order.append(["full EM", "all 8 x 16", rep == 0])
    em.destroy()
    with open(args.labels, "w") as f:
        json.dump(dict(order=order, grid=args.grid, precision=args.precision, calls=args.calls), f)
    print("ran %d calls, %s" % (len(order), args.precision))


def report(args):
    meta = json.load(open(args.labels))
    files = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if "diag_field_kernel" in name or "modes_partial_kernel" in name:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name))
    rows.sort()
    assert len(rows) == len(meta["order"]), (len(rows), len(meta["order"]))
    times = {}
    for (state, label, warm), (_, dur, name) in zip(meta["order"], rows):
        assert ("diag_field_kernel" if label.startswith("energy") else "modes_partial_kernel") in name, (label, name)
        if not warm:
            times.setdefault((state, label), []).append(dur)
    print("%s, %d^3 nodes" % (meta["precision"], meta["grid"]))
    print("%-16s %-18s %5s %10s %10s %10s %10s" % ("state", "case", "calls", "mean ms", "min ms", "max ms", "x field"))
    for state in ("after precalc", "after 3 steps", "full EM"):
        base = sum(times[(state, "energy field pass")]) / len(times[(state, "energy field pass")])
        for label in ["energy field pass"] + [c[0] for c in CASES]:
            if (state, label) not in times:
                continue
            t = times[(state, label)]
            mean = sum(t) / len(t)
            print("%-16s %-18s %5d %10.3f %10.3f %10.3f %10.2f" % (state, label, len(t), mean * 1e-6, min(t) * 1e-6, max(t) * 1e-6, mean / base))


def cost(args):
    import numpy as np
    sim, L = build(args, "poisson_fft")
    modes = wave_vectors(16, args.grid)
    sim.precalc()
    sim.substeps(12)          # past the first binning
    sim.sync()
    res = {"off": [], "on": []}
    for rep in range(args.calls):
        for mode in ("off", "on"):
            sim.recordModes(1 if mode == "on" else 0, args.substeps, modes, E4)
            sim.sync()
            t0 = time.perf_counter()
            sim.substeps(args.substeps)
            sim.sync()
            res[mode].append(time.perf_counter() - t0)
            if mode == "on":
                hist, dropped = sim.modesHistory()
                assert len(hist["substep"]) == args.substeps and dropped == 0
    sim.destroy()
    off, on = np.array(res["off"]), np.array(res["on"])
    print("%s, %d^3 nodes, %d particles, %d sub-steps per run, %d alternating runs each" % (args.precision, args.grid, args.particles, args.substeps, args.calls))
    print("not recording       ms per sub-step: %s  (median %.3f)" % (" ".join("%.3f" % (1e3 * x / args.substeps) for x in off), 1e3 * np.median(off) / args.substeps))
    print("recording 16 modes  ms per sub-step: %s  (median %.3f)" % (" ".join("%.3f" % (1e3 * x / args.substeps) for x in on), 1e3 * np.median(on) / args.substeps))
    print("ratio of the medians %.4f" % (np.median(on) / np.median(off)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "report", "cost"])
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--particles", type=int, default=20_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--substeps", type=int, default=100)
    ap.add_argument("--labels", default="modes_labels.json")
    ap.add_argument("--trace", default=".")
    a = ap.parse_args()
    {"run": run, "report": report, "cost": cost}[a.mode](a)
