"""Measurements of the fusion product spectrum (fpic_fusion_spectrum): a box of --grid^3 nodes with --particles deuterons and as
many tritons at 10 keV, solver 'none', one precision per run (--precision), a Gamow-form table of 4096 points over 0.5 .. 500
keV.  In the same run: one sub-step's push of the box, then — freshly sorted (fpic_sort) and after --drift in-place sub-steps,
when particles sit in the slots of tiles they have left — for the deuterons with the tritons: fusionYield, and beside it on the
same state fusionSpectrum of the same request on the centre-of-mass axis, on the neutron's axis with isotropic emission and on
the neutron's axis along a line of sight, --bins bins each (256; with 1 every pair of a workgroup adds to one entry).  HIP
events on the handle's stream, one warm-up, the median of --calls repetitions; every call takes a new epoch.  The whole
application is timed (for the call form that includes zeroing the slot's words and copying the table; the counts and the
words are read back: 8 + (bins + 2) x 2 words).  Prints one JSON line with the times (median, least, largest; ms), the ratios
of each spectrum to the tally, and the counts of the last call of each kind; the identity with the tally of the same epoch is
asserted on one more fusionYield per case."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

MD, MT, MN, MA, QP, KEV, C = 3.3435837724e-27, 5.0073567446e-27, 1.67492749804e-27, 6.6446573357e-27, 1.602176634e-19, 1.602176634e-16, 2.998e8


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
    S, g_lo, g_hi = fp.sigma_table(lambda e: 1e-24 / e * np.exp(-34.38 / np.sqrt(e)), MD, MT, 0.5, 500.0)
    table = dict(sigma=S, g_lo=g_lo, g_hi=g_hi, tau=1e-9)
    neutron = dict(axis="product", bins=args.bins, lo=12000.0 * fp.KEV, hi=16200.0 * fp.KEV, q_value=17590.0 * fp.KEV, product_mass=MN, other_mass=MA)
    kinds = {"cm": dict(axis="cm", bins=args.bins, lo=0.0, hi=300.0 * fp.KEV), "product_isotropic": neutron, "product_sight": dict(neutron, los=(1.0, 2.0, -2.0))}
    res = {"particles": n, "grid": grid, "calls": args.calls, "precision": args.precision, "bins": args.bins}
    epoch = [0]

    def tally():
        epoch[0] += 1
        return sim.fusionYield(0, 1, epoch=epoch[0], **table)

    def spectrum(kind):
        epoch[0] += 1
        return sim.fusionSpectrum(0, 1, epoch=epoch[0], **table, **kinds[kind])

    sim.precalc()
    res["push"] = timed(torch, stream, args.calls, lambda: sim.substeps(1))
    for order in ("sorted", "drifted"):
        if order == "sorted":
            sim.sort()
        else:
            sim.substeps(args.drift)
        last = []
        t_tally = timed(torch, stream, args.calls, lambda: last.append(tally()))
        res["%s_tally" % order] = t_tally + ({k: v for k, v in last[-1].items() if k != "reactions_exact"},)
        for kind in kinds:
            last = []
            t = timed(torch, stream, args.calls, lambda: last.append(spectrum(kind)))
            got = last[-1]
            res["%s_%s" % (order, kind)] = t + ({k: got[k] for k in ("pairs", "below", "above", "cells", "reactions", "unit_exponent")},
                                                dict(under=float(got["under"]), over=float(got["over"]), inside=float(sum(got["bins"]))))
            res["%s_%s_over_tally" % (order, kind)] = t[0] / t_tally[0]
            same = sim.fusionYield(0, 1, epoch=epoch[0], **table)          # the identity, at this size
            assert sum(got["bins"]) + got["under"] + got["over"] == same["reactions_exact"] and got["pairs"] == same["pairs"], (order, kind)
    sim.destroy()
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--particles", type=int, default=500000000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--drift", type=int, default=8)
    ap.add_argument("--bins", type=int, default=256)
    main(ap.parse_args())
