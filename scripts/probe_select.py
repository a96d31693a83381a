"""Kernel times of the particle selection's pass (fpic_select) beside the histogram pass on ONE state: a box of --grid^3 nodes
with one thermal species of --particles, as loaded (upload order) and after --steps steps (tile order, the slots permuted).
Two modes:

  run      build the state (torch on the device, uploaded in blocks), then per state --calls times each: the histogram of vx
           with 1024 bins (the yardstick: the same 4 / 8 bytes per slot), the count query with one term on vx, the delivering
           pass for a vx window holding about 1e-3 of the particles, the same window with every = (1000, 0) (which adds the id
           stream), and a delivering request of three terms (x, vx, v2).  Meant to run under `rocprofv3 --kernel-trace --stats
           --output-format csv` (scripts/probe_select.sh); writes the order of the calls to --labels.
  report   reads the kernel trace of such a run and the labels, and prints per state and case: dispatches, mean / min / max
           kernel time, bytes streamed per slot and per second, the rows matched, and the count query's ratio to the yardstick.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

VTH = 1e-3
WINDOW = (0.0, 2.5066e-3 * VTH)      # about 1e-3 of a normal distribution: width * pdf(0) = 2.5066e-3 * 0.39894
CASES = [  # label, kind, where, every, capacity, arrays streamed per slot, id stream
    ("hist vx 1024 (yardstick)", "hist", None, None, 0, 1, 0),
    ("count, vx", "count", {"vx": (-4 * VTH, 4 * VTH)}, None, 0, 1, 0),
    ("deliver, vx window 1e-3", "select", {"vx": WINDOW}, None, 1 << 20, 1, 0),
    ("deliver, same, every (1000, 0)", "select", {"vx": WINDOW}, (1000, 0), 1 << 20, 1, 1),
    ("deliver, x vx v2", "select", {"x": (0.25, 0.30), "vx": (0.0, 0.5 * VTH), "v2": (None, 3 * VTH ** 2)}, None, 1 << 24, 4, 0),
]


def run(args):
    import torch
    import fusionpic as fp
    n, grid = args.particles, args.grid
    L = grid * 3e-4
    spec = dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=1e-11, nparticles=0, count=n, particle_mass=9.109e-31,
                particle_charge=-1.602e-19, geometry="cart3d", solver="none", macro_weight=1.0)
    sim = fp.makeCylindricalParticlePusher(spec, precision=args.precision)
    dev = torch.device("cuda", 0)
    T = torch.float32 if args.precision == "fp32" else torch.float64
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    block = 1 << 24
    for first in range(0, n, block):
        m = min(block, n - first)
        pos = torch.rand((m, 3), dtype=T, device=dev, generator=gen) * (L * 0.999)
        vel = torch.randn((m, 3), dtype=T, device=dev, generator=gen) * VTH
        torch.cuda.synchronize()
        sim.setRange(first, position=pos, velocity=vel)
    del pos, vel
    torch.cuda.empty_cache()
    order, matched = [], {}

    def call(state, case):
        label, kind, where, every, capacity, _, _ = case
        if kind == "hist":
            h = sim.histogram("vx", 1024, (-4 * VTH, 4 * VTH))
            m = int(h["counts"].sum())
        elif kind == "count":
            m = sim.count(where)
        else:
            r = sim.select(where, every=every, capacity=capacity)
            assert r["ids"] is not None and len(r["ids"]) == r["matched"], (label, r["matched"])
            m = r["matched"]
        order.append([state, label])
        matched[state + " | " + label] = m

    for state in ("as loaded", "after %d steps" % args.steps):
        if state != "as loaded":
            sim.precalc()
            sim.step(args.steps)
        for rep in range(args.calls + 1):      # (the first round warms every shape up; the report drops it)
            for case in CASES:
                call(state, case)
        assert matched[state + " | " + CASES[0][0]] == matched[state + " | " + CASES[1][0]]      # the yardstick's bins hold what the count query counts
    with open(args.labels, "w") as f:
        json.dump(dict(order=order, matched=matched, particles=n, grid=grid, precision=args.precision, calls=args.calls, steps=args.steps), f)
    sim.destroy()
    print("ran 2 states x %d rounds of %d calls on %d particles, %s" % (args.calls + 1, len(CASES), n, args.precision))


def report(args):
    meta = json.load(open(args.labels))
    files = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if "hist_kernel" in name or "select_kernel" in name:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name))
    rows.sort()
    assert len(rows) == len(meta["order"]), (len(rows), len(meta["order"]))
    kinds = {c[0]: c[1] for c in CASES}
    times, seen = {}, {}
    for (state, label), row in zip(meta["order"], rows):
        want = "hist_kernel" if kinds[label] == "hist" else ("true>" if kinds[label] == "select" else "false>")
        assert want in row[2] and ("hist_kernel" in row[2]) == (kinds[label] == "hist"), (label, row)
        seen[(state, label)] = seen.get((state, label), 0) + 1
        if seen[(state, label)] > 1:           # the first round warms up
            times.setdefault((state, label), []).append(row[1])
    size = 4 if meta["precision"] == "fp32" else 8
    n = meta["particles"]
    for state in dict.fromkeys(s for s, _ in meta["order"]):
        print("%s, %d^3 nodes, %d particles, %s" % (meta["precision"], meta["grid"], n, state))
        print("%-32s %5s %10s %10s %10s %8s %10s %10s" % ("case", "calls", "mean ms", "min ms", "max ms", "B/slot", "read TB/s", "matched"))
        means = {}
        for label, _, _, _, _, arrays, idstream in CASES:
            t = times[(state, label)]
            means[label] = mean = sum(t) / len(t)
            bytes_per = arrays * size + 4 * idstream
            print("%-32s %5d %10.3f %10.3f %10.3f %8d %10.2f %10d" % (label, len(t), mean * 1e-6, min(t) * 1e-6, max(t) * 1e-6, bytes_per,
                                                                     n * bytes_per / (mean * 1e-9) * 1e-12, meta["matched"][state + " | " + label]))
        ratio = means[CASES[1][0]] / means[CASES[0][0]]
        print("count query / yardstick = %.3f (the bar: within 1.25) -> %s\n" % (ratio, "met" if ratio <= 1.25 else "MISSED"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "report"])
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--particles", type=int, default=500_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--labels", default="select_labels.json")
    ap.add_argument("--trace", default=".")
    a = ap.parse_args()
    run(a) if a.mode == "run" else report(a)
