"""Measurements of the windowed background collisions (fpic_gas): a box of --grid^3 nodes with --particles particles, solver
'none', per precision, on a species sorted by fpic_sort (the ids are read).  ELASTIC throughout.
  flat_P        a flat two-node table on the whole box at P_max = 1e-3, 1e-2, 1e-1 and 1;
  window_0.01   a 4096-node table in a window of 0.375 of the box (0.75 x 1 x 0.5) with three 1025-node tapers at P_max = 1e-2;
  --references  beside them in the same run: fpic_collide's null-collision ELASTIC at P_max = 1e-2, one sub-step's push and
                count() over v2.
HIP events on the handle's stream, one warm-up, the median of --calls repetitions; every call takes a new epoch.  The form
that runs is the host's choice, or what FPIC_GAS_FORMS forces (fes_gas.inc.hpp; read once: one process per value —
scripts/probe_gas.sh runs them all).  Prints one JSON line per precision."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

P_MAX = (1e-3, 1e-2, 1e-1, 1.0)
C = 2.998e8
BACKGROUND = dict(drift=(0.0, 0.0, 0.01), vth=1e-3)
G_LO, G_HI, TAU = 0.0, 0.1, 1e-11


def box_spec(grid, n, L):
    return dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=1e-11, nparticles=0, count=n, particle_mass=9.109e-31,
                particle_charge=-1.602e-19, geometry="cart3d", solver="none", macro_weight=1.0)


def timed(torch, stream, calls, fn):
    """median, least and largest milliseconds of fn() between two events on `stream`, after one warm-up"""
    ms = []
    for rep in range(calls + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if rep:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def bound(sigma, g_lo, g_hi):
    """max_k max(S[k], S[k+1]) g_{k+1}: the interval-wise candidate bound of the header"""
    n = len(sigma)
    dg = (g_hi - g_lo) / (n - 1)
    return max(max(sigma[k], sigma[k + 1]) * (g_hi if k == n - 2 else g_lo + (k + 1) * dg) for k in range(n - 1))


def density_for(p, sigma):
    x = 50.0 if p == 1.0 else -math.log1p(-p)
    return x / (C * TAU * bound(sigma, G_LO, G_HI))


def main(args):
    import numpy as np
    import torch
    import fusionpic as fp
    n, grid = args.particles, args.grid
    L = grid * 3e-4
    stream = torch.cuda.Stream()
    flat = np.array([3.0e-19, 3.0e-19])                  # (arrays, so that the wrapper converts nothing between the two events)
    g = np.linspace(G_LO, G_HI, 4096)
    long_table = 1.0e-19 + 2.0e-19 * np.exp(-0.5 * ((g - 0.012) / 0.002) ** 2)            # a resonance near the beam's speed
    tapers = tuple(np.sin(math.pi * np.linspace(0.0, 1.0, 1025)) ** 2 for _ in range(3))
    window = dict(lo=(L / 8, 0.0, L / 4), hi=(7 * L / 8, L, 3 * L / 4))
    out = {"particles": n, "grid": grid, "calls": args.calls, "forms": os.environ.get("FPIC_GAS_FORMS", "0")}
    for precision in ("fp32", "fp64"):
        sim = fp.makeCylindricalParticlePusher(box_spec(grid, n, L), precision=precision)
        sim.setStream(stream.cuda_stream)
        sim.load(**BACKGROUND)
        sim.precalc()
        res = {}
        if args.references:
            res["push"] = timed(torch, stream, args.calls, lambda: sim.substeps(1))
        else:
            sim.substeps(1)                     # (the first push bins the species; fpic_sort leaves it sorted by cell)
        sim.sort()
        epoch = [0]
        last = []

        def once(**kw):
            epoch[0] += 1
            last.append(sim.collideGas("elastic", epoch=epoch[0], mass_ratio=1.0, tau=TAU, g_lo=G_LO, g_hi=G_HI, **BACKGROUND, **kw))

        for p in P_MAX:
            t = timed(torch, stream, args.calls, lambda: once(density=density_for(p, flat), sigma=flat))
            res["flat_%g" % p] = t + (last[-1]["candidates"], last[-1]["collided"])
        t = timed(torch, stream, args.calls, lambda: once(density=density_for(1e-2, long_table), sigma=long_table, taper=tapers, **window))
        res["window_0.01"] = t + (last[-1]["candidates"], last[-1]["collided"])
        if args.references:
            def null():
                epoch[0] += 1
                sim.collide("elastic", epoch=epoch[0], nu_tau=0.005, sigma_tau=1.0, g_max=-math.log1p(-1e-2) - 0.005, mass_ratio=1.0, **BACKGROUND)
            res["collide_null_0.01"] = timed(torch, stream, args.calls, null)
            res["count_v2"] = timed(torch, stream, args.calls, lambda: sim.count({"v2": (0.0, 1e-4)}))
            res["flat_0.01_over_collide_null"] = res["flat_0.01"][0] / res["collide_null_0.01"][0]
        res["sorted_1e-2_faster_than_1"] = res["flat_0.01"][0] < res["flat_1"][0]
        sim.destroy()
        del sim
        torch.cuda.empty_cache()
        out[precision] = res
        print("forms", out["forms"], precision, json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=500000000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--references", action="store_true")
    main(ap.parse_args())
