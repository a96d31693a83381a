"""Kernel times of the series diagnostic's tracer pass (fpic_series_*) beside the histogram pass on ONE state, and what
recording costs a run.  A box of --grid^3 nodes with one thermal species of --particles.  Three modes:

  run      build the state (torch on the device, uploaded in blocks), then --calls + 1 rounds of: histogram vx / 1024 bins (the
           yardstick: the same 4 bytes per slot through the same launch shape, one LDS operation per slot), series() with 16,
           4096 and 65536 tracers, series() with 16 points; then step(3) (the species is binned, slots are in tile order) and
           the same rounds again.  Meant to run under `rocprofv3 --kernel-trace --stats --output-format csv`
           (scripts/probe_series.sh); writes the order of the calls to --labels.
  report   reads the kernel trace of such a run and the labels, and prints per state and case: dispatches, mean / min / max
           kernel time, the ratio to the yardstick of the same state, and the filter's load at 65536 tracers.
  cost     wall time of --substeps sub-steps of the self-consistent box with recordSeries(every = 1, 16 points + 16 tracers)
           against the same sub-steps without, alternating, --calls times each, on one handle (no profiler).
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

TRACERS = (16, 4096, 65536)


def build(args, solver):
    import torch
    import fusionpic as fp
    n, grid, vth = args.particles, args.grid, 1e-3
    L = grid * 3e-4
    spec = dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=1e-11, nparticles=0, count=n, particle_mass=9.109e-31,
                particle_charge=-1.602e-19, geometry="cart3d", solver=solver, macro_weight=1.0)
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
    return sim, L


def filter_load(ids, n):
    """(bits of the filter, fraction of the slots that are no tracer and pass it) for a request of these ids among n:
    fes_series_core.hpp's size rule and placement (a word by the hash's top bits, three bits of it by the fields below)"""
    import numpy as np
    log2 = 10
    while log2 < 19 and (1 << log2) < 256 * len(ids):
        log2 += 1
    shift = 32 - (log2 - 5)

    def place(x):
        h = (x.astype(np.uint64) * 0x9E3779B1) & 0xFFFFFFFF
        mask = (1 << ((h >> (shift - 5)) & 31)) | (1 << ((h >> (shift - 10)) & 31)) | (1 << ((h >> (shift - 15)) & 31))
        return (h >> shift).astype(np.int64), mask.astype(np.uint32)

    words = np.zeros(1 << (log2 - 5), dtype=np.uint32)
    w, mask = place(ids)
    np.bitwise_or.at(words, w, mask)
    others = np.setdiff1d(np.random.default_rng(1).integers(0, n, 2_000_000), ids)
    w, mask = place(others)
    return 1 << log2, float(((words[w] & mask) == mask).mean())


def run(args):
    import numpy as np
    sim, L = build(args, "none")
    n, vth = args.particles, 1e-3
    rng = np.random.default_rng(7)
    ids = {m: rng.choice(n, m, replace=False).astype(np.uint32) for m in TRACERS}
    pts = rng.random((16, 3)) * L
    order = []
    for state in ("upload order", "after 3 steps"):
        if state == "after 3 steps":
            sim.step(3)
        for rep in range(args.calls + 1):      # (the first round of a state warms every shape up; the report drops it)
            h = sim.histogram("vx", 1024, (-4 * vth, 4 * vth))
            assert int(h["counts"].sum()) + h["outside"] == n
            order.append([state, "hist vx 1024", rep == 0])
            for m in TRACERS:
                rows = sim.series(tracers=ids[m])["tracers"]
                assert (rows[:, 6] == 1).all()
                order.append([state, "tracers %d" % m, rep == 0])
            assert (sim.series(points=pts)["points"][:, 7] == 1).all()
            order.append([state, "points 16", rep == 0])
    bits, load = filter_load(ids[65536], n)
    with open(args.labels, "w") as f:
        json.dump(dict(order=order, particles=n, grid=args.grid, precision=args.precision, calls=args.calls, filter_bits=bits, filter_load=load), f)
    sim.destroy()
    print("ran 2 x %d rounds of %d calls on %d particles, %s" % (args.calls + 1, 2 + len(TRACERS), n, args.precision))


def report(args):
    meta = json.load(open(args.labels))
    files = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if "hist_kernel" in name or "series_tracers_kernel" in name or "series_points_kernel" in name:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name))
    rows.sort()
    assert len(rows) == len(meta["order"]), (len(rows), len(meta["order"]))
    times = {}
    for (state, label, warm), (_, dur, name) in zip(meta["order"], rows):
        want = "hist_kernel" if label.startswith("hist") else ("series_tracers_kernel" if label.startswith("tracers") else "series_points_kernel")
        assert want in name, (label, name)
        if not warm:
            times.setdefault((state, label), []).append(dur)
    n = meta["particles"]
    print("%s, %d^3 nodes, %d particles; the filter of 65536 tracers: %d bits, %.1f %% of the slots that are no tracer pass it (and take the search)"
          % (meta["precision"], meta["grid"], n, meta["filter_bits"], 100 * meta["filter_load"]))
    print("%-16s %-16s %5s %10s %10s %10s %10s %10s" % ("state", "case", "calls", "mean ms", "min ms", "max ms", "x hist", "id TB/s"))
    for state in ("upload order", "after 3 steps"):
        base = sum(times[(state, "hist vx 1024")]) / len(times[(state, "hist vx 1024")])
        for label in ["hist vx 1024"] + ["tracers %d" % m for m in TRACERS] + ["points 16"]:
            t = times[(state, label)]
            mean = sum(t) / len(t)
            bw = "%10.2f" % (n * 4 / (mean * 1e-9) * 1e-12) if not label.startswith("points") else "%10s" % "-"
            print("%-16s %-16s %5d %10.3f %10.3f %10.3f %10.2f %s" % (state, label, len(t), mean * 1e-6, min(t) * 1e-6, max(t) * 1e-6, mean / base, bw))


def cost(args):
    import numpy as np
    sim, L = build(args, "poisson_fft")
    rng = np.random.default_rng(9)
    pts, ids = rng.random((16, 3)) * L, rng.choice(args.particles, 16, replace=False)
    sim.precalc()
    sim.substeps(12)          # past the first binning
    sim.sync()
    res = {"off": [], "on": []}
    for rep in range(args.calls):
        for mode in ("off", "on"):
            sim.recordSeries(1 if mode == "on" else 0, args.substeps, points=pts, tracers=ids)
            sim.sync()
            t0 = time.perf_counter()
            sim.substeps(args.substeps)
            sim.sync()
            res[mode].append(time.perf_counter() - t0)
            if mode == "on":
                hist, dropped = sim.seriesHistory()
                assert len(hist["substep"]) == args.substeps and dropped == 0 and (hist["tracers"][:, :, 6] == 1).all()
    sim.destroy()
    off, on = np.array(res["off"]), np.array(res["on"])
    print("%s, %d^3 nodes, %d particles, %d sub-steps per run, %d alternating runs each" % (args.precision, args.grid, args.particles, args.substeps, args.calls))
    print("not recording    ms per sub-step: %s  (median %.3f)" % (" ".join("%.3f" % (1e3 * x / args.substeps) for x in off), 1e3 * np.median(off) / args.substeps))
    print("recording 16+16  ms per sub-step: %s  (median %.3f)" % (" ".join("%.3f" % (1e3 * x / args.substeps) for x in on), 1e3 * np.median(on) / args.substeps))
    print("ratio of the medians %.4f" % (np.median(on) / np.median(off)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "report", "cost"])
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--particles", type=int, default=500_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--substeps", type=int, default=100)
    ap.add_argument("--labels", default="series_labels.json")
    ap.add_argument("--trace", default=".")
    a = ap.parse_args()
    {"run": run, "report": report, "cost": cost}[a.mode](a)
