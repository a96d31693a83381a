"""Measurements of the fusion yield tally (fpic_fusion): a box of --grid^3 nodes with --particles deuterons and as many
tritons at 10 keV, solver 'none', one precision per run (--precision), a Gamow-form table of 4096 points over 0.5 .. 500 keV.
In the same run: one sub-step's push of the box, then — freshly sorted (fpic_sort) and after --drift in-place sub-steps, when
particles sit in the slots of tiles they have left — fusionYield of the deuterons with themselves and with the tritons and,
beside each, collidePair of the same kind on the same state.  HIP events on the handle's stream, one warm-up, the median of
--calls repetitions; every call takes a new epoch.  The whole application is timed here (for the call form that includes
zeroing the cell grid and copying the table; the cell grid is not read back); the kernels of an application are cut from a
rocprofv3 kernel trace of this same run by scripts/probe_fusion.sh (pair_count_lds_kernel, pair_scan_kernel,
pair_fill_lds_kernel, fusion_tally_kernel, pair_collide_kernel).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

MD, MT, QP, KEV, C = 3.3435837724e-27, 5.0073567446e-27, 1.602176634e-19, 1.602176634e-16, 2.998e8


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


def main(args):
    import torch
    import fusionpic as fp
    n, grid = args.particles, args.grid
    L = grid * 3e-4
    vth = [float(np.sqrt(10.0 * KEV / m) / C) for m in (MD, MT)]
    stream = torch.cuda.Stream()
    W = 1e20 * L ** 3 / n                      # a density of 1e20 per cubic metre
    spec = dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=1e-11, nparticles=0, count=n, particle_mass=MD, particle_charge=QP,
                geometry="cart3d", solver="none", macro_weight=W)
    sim = fp.makeCylindricalParticlePusher(spec, precision=args.precision)
    sim.setStream(stream.cuda_stream)
    assert sim.addSpecies(MT, QP, n) == 1
    sim.load(species=0, seed=1, vth=vth[0])
    sim.load(species=1, seed=2, vth=vth[1])
    tables = {}
    for name, mb in (("like", MD), ("unlike", MT)):
        S, g_lo, g_hi = fp.sigma_table(lambda e: 1e-24 / e * np.exp(-34.38 / np.sqrt(e)), MD, mb, 0.5, 500.0)
        tables[name] = dict(sigma=S, g_lo=g_lo, g_hi=g_hi)
    res = {"particles": n, "grid": grid, "calls": args.calls, "precision": args.precision, "forms": os.environ.get("FPIC_PAIR_FORMS", "default")}
    epoch = [0]

    def tally(name, a, b):
        epoch[0] += 1
        return sim.fusionYield(a, b, tau=1e-9, epoch=epoch[0], **tables[name])

    def collide(a, b):
        epoch[0] += 1
        return sim.collidePair(a, b, log_lambda=10.0, tau=1e-15, epoch=epoch[0])     # (a short tau: the state barely changes)

    sim.precalc()
    res["push"] = timed(torch, stream, args.calls, lambda: sim.substeps(1))
    for order in ("sorted", "drifted"):
        if order == "sorted":
            sim.sort()
        else:
            sim.substeps(args.drift)
        for name, (a, b) in (("like", (0, None)), ("unlike", (0, 1))):
            last = []
            t = timed(torch, stream, args.calls, lambda: last.append(tally(name, a, b)))
            got = {k: v for k, v in last[-1].items() if k != "reactions_exact"}
            res["%s_fusion_%s" % (order, name)] = t + (got,)
            last = []
            t = timed(torch, stream, args.calls, lambda: last.append(collide(a, b)))
            res["%s_pair_%s" % (order, name)] = t + (last[-1],)
            res["%s_%s_fusion_over_pair" % (order, name)] = res["%s_fusion_%s" % (order, name)][0] / t[0]
    sim.destroy()
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--particles", type=int, default=500000000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--drift", type=int, default=8)
    main(ap.parse_args())
