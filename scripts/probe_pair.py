"""Measurements of the binary collision operator (fpic_pair): a box of --grid^3 nodes with --particles electrons and as many
protons, solver 'none', one precision per run (--precision).  In the same run: count() over v2 (streams the three velocity
arrays) and one sub-step's push of the box, then collidePair of the electrons with themselves and with the protons — in the
caller's order (as loaded: slot = id), freshly sorted (fpic_sort) and after --drift in-place sub-steps, when particles sit in the slots of tiles they have left.  HIP events
on the handle's stream, one warm-up, the median of --calls repetitions; every call takes a new epoch.  The whole application
is timed here; the four kernels of an application are cut from a rocprofv3 kernel trace of this same run by
scripts/probe_pair.sh (pair_count_kernel, pair_scan_kernel, pair_fill_kernel, pair_collide_kernel).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

ME, QE, MP = 9.109e-31, -1.602e-19, 1.673e-27


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
    vth = 1e-3
    stream = torch.cuda.Stream()
    # the weight at which a thermal pair of a cell with n / grid^3 particles has the variance 0.01
    per_cell = max(1.0, n / grid ** 3)
    k1 = (QE * QE) ** 2 * 10.0 * 1e-11 / (8 * 3.141592653589793 * 8.8541878128e-12 ** 2 * (ME / 2) ** 2 * 2.998e8 ** 3 * (L / grid) ** 3)
    W = 0.01 * vth ** 3 / (k1 * per_cell)
    spec = dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=1e-11, nparticles=0, count=n, particle_mass=ME, particle_charge=QE,
                geometry="cart3d", solver="none", macro_weight=W)
    sim = fp.makeCylindricalParticlePusher(spec, precision=args.precision)
    sim.setStream(stream.cuda_stream)
    assert sim.addSpecies(MP, -QE, n) == 1
    sim.load(species=0, seed=1, vth=vth)
    sim.load(species=1, seed=2, vth=vth / 40)
    res = {"particles": n, "grid": grid, "calls": args.calls, "precision": args.precision}
    res["count_v2"] = timed(torch, stream, args.calls, lambda: sim.count({"v2": (0.0, 1e-4)}))
    epoch = [0]

    def once(a, b):
        epoch[0] += 1
        return sim.collidePair(a, b, log_lambda=10.0, epoch=epoch[0])

    for order in ("identity", "sorted", "drifted"):
        if order == "identity":             # (as loaded: slot = id, the cells of neighbouring slots unrelated)
            pass
        elif order == "sorted":
            sim.precalc()
            res["push"] = timed(torch, stream, args.calls, lambda: sim.substeps(1))
            sim.sort()
        else:
            sim.substeps(args.drift)
        for name, (a, b) in (("like", (0, None)), ("unlike", (0, 1))):
            last = []
            t = timed(torch, stream, args.calls, lambda: last.append(once(a, b)))
            res["%s_%s" % (order, name)] = t + (last[-1],)
    for key in [k for k in res if k.endswith("like")]:
        res[key + "_share_of_push"] = res[key][0] / res["push"][0]
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
