"""Kernel times of the phase-space histogram pass (fpic_histogram) beside the energy pass on ONE state: a box of
--grid^3 nodes with a thermal species and a cold beam of --particles each.  Two modes:

  run      build the state (torch on the device, uploaded in blocks; --binned: then sorted into tile order), then --calls times each: energy(), vx / 1024 bins on
           the thermal species, the same on the cold beam, (x, vx) / 128 x 128, 512 x 512 and 2048 x 2048 on the thermal
           species.  Meant to run under `rocprofv3 --kernel-trace --stats --output-format csv` (scripts/probe_hist.sh);
           writes the order of the calls to --labels.
  report   reads the kernel trace of such a run and the labels, and prints per case: dispatches, mean / min / max kernel
           time, bytes read per particle and per second.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

CASES = [  # label, axes, bins, range, species, arrays read per particle
    ("vx 1024, thermal", "vx", 1024, None, 0, 1),
    ("vx 1024, cold beam", "vx", 1024, None, 1, 1),
    ("(x, vx) 128 x 128, thermal", ("x", "vx"), (128, 128), None, 0, 2),
    ("(x, vx) 512 x 512, thermal", ("x", "vx"), (512, 512), None, 0, 2),
    ("(x, vx) 2048 x 2048, thermal", ("x", "vx"), (2048, 2048), None, 0, 2),
]


def run(args):
    import numpy as np
    import torch
    import fusionpic as fp
    n, grid, vth = args.particles, args.grid, 1e-3
    L = grid * 3e-4
    spec = dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=1e-11, nparticles=0, count=n, particle_mass=9.109e-31,
                particle_charge=-1.602e-19, geometry="cart3d", solver="none", macro_weight=1.0)
    sim = fp.makeCylindricalParticlePusher(spec, precision=args.precision)
    beam = sim.addSpecies(9.109e-31, -1.602e-19, n)
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
        vel[:] = torch.tensor([0.5 * vth, 0.0, 0.0], dtype=T, device=dev)
        torch.cuda.synchronize()
        sim.setRange(first, position=pos, velocity=vel, species=beam)
    del pos, vel
    torch.cuda.empty_cache()
    if args.binned:        # tile order, as a stepped run holds its particles: the lanes of a wave share a tile
        sim.sort()
    rng = (-4 * vth, 4 * vth)
    order = []

    def call(case):
        label, axes, bins, _, species, _ = case
        r = rng if isinstance(axes, str) else ((0.0, 1.0), rng)
        h = sim.histogram(axes, bins, r, species=species)
        order.append(label)
        return h

    for rep in range(args.calls + 1):      # (the first round warms every shape up; the report drops it)
        e = sim.energy()
        order.append("energy")
        for case in CASES:
            h = call(case)
            assert int(h["counts"].sum()) + h["outside"] == n == int(e["count"][case[4]])
    thermal, cold = call(CASES[0]), call(CASES[1])
    with open(args.labels, "w") as f:
        json.dump(dict(order=order, particles=n, grid=grid, precision=args.precision, calls=args.calls, species=2, binned=args.binned,
                       thermal_outside=thermal["outside"], thermal_nonzero_bins=int(np.count_nonzero(thermal["counts"])),
                       cold_nonzero_bins=int(np.count_nonzero(cold["counts"]))), f)
    sim.destroy()
    print("ran %d rounds of %d calls on 2 x %d particles, %s" % (args.calls + 1, 1 + len(CASES), n, args.precision))


def report(args):
    meta = json.load(open(args.labels))
    files = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"]
        if "hist_kernel" in name or "diag_particles_kernel" in name:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name))
    rows.sort()
    at, times = 0, {}
    for i, label in enumerate(meta["order"]):
        warm = i < 1 + len(CASES) or i >= len(meta["order"]) - 2      # the first round, and the two calls that only count bins
        if label == "energy":            # one pass per species: thermal first, then the beam
            for sp in ("thermal", "cold beam"):
                assert "diag_particles_kernel" in rows[at][2], rows[at]
                if not warm:
                    times.setdefault("energy pass, " + sp, []).append(rows[at][1])
                at += 1
        else:
            assert "hist_kernel" in rows[at][2], (label, rows[at])
            if not warm:
                times.setdefault(label, []).append(rows[at][1])
            at += 1
    assert at == len(rows), (at, len(rows))
    size = 4 if meta["precision"] == "fp32" else 8
    arrays = {"energy pass, thermal": 3, "energy pass, cold beam": 3}
    arrays.update({c[0]: c[5] for c in CASES})
    n = meta["particles"]
    print("%s, %d^3 nodes, %d particles per species, %s; thermal vx / 1024: %d bins hit, %d outside; cold beam: %d bin hit"
          % (meta["precision"], meta["grid"], n, "binned (tile order)" if meta.get("binned") else "upload order", meta["thermal_nonzero_bins"], meta["thermal_outside"], meta["cold_nonzero_bins"]))
    print("%-32s %5s %10s %10s %10s %8s %10s" % ("case", "calls", "mean ms", "min ms", "max ms", "B/part", "read TB/s"))
    for label in ["energy pass, thermal", "energy pass, cold beam"] + [c[0] for c in CASES]:
        t = times[label]
        mean = sum(t) / len(t)
        print("%-32s %5d %10.3f %10.3f %10.3f %8d %10.2f" % (label, len(t), mean * 1e-6, min(t) * 1e-6, max(t) * 1e-6, arrays[label] * size,
                                                          n * arrays[label] * size / (mean * 1e-9) * 1e-12))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "report"])
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--particles", type=int, default=500_000_000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--binned", action="store_true", help="sort() the particles into tile order after the upload")
    ap.add_argument("--labels", default="hist_labels.json")
    ap.add_argument("--trace", default=".")
    a = ap.parse_args()
    run(a) if a.mode == "run" else report(a)
