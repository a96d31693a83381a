"""Measurements of the absorbing particle sinks (fpic_remove, fpic_renumber): a box of --grid^3 nodes with
--particles thermal particles of one species, the electrostatic solver, one precision per process (--precision).
  nothing_*     an application that removes nothing, one term on x, beside count() with the same term (the bar: 1.25 x), on the
                species as loaded and after 3 sub-steps;
  remove_F      a removing application at the fraction F = 1e-4, 1e-2, 0.5 of the particles held then (a slab in x), the whole
                synchronous call — mark, scan, move, tally, the re-deposit and the solve —, and what follows it: the sub-step
                that re-bins (forced by the removal) beside an ordinary sub-step's push, and the re-deposit + solve alone
                (precalc() on the same state);
  renumber      fpic_renumber of the thinned species.
HIP events on the handle's stream around the calls (the calls wait for the device themselves), one warm-up and the median of
--calls repetitions where a call can be repeated; a removing call is made once.  Run under rocprofv3 --kernel-trace --stats
(scripts/probe_remove.sh) the kernels' own times are beside it.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))


def box_spec(grid, n, L):
    return dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=1e-11, nparticles=0, count=n, particle_mass=9.109e-31,
                particle_charge=-1.602e-19, geometry="cart3d", solver="poisson_fft", macro_weight=1.0)


def timed(torch, stream, calls, fn):
    """median, least and largest milliseconds of fn() between two events on `stream`, after one warm-up (calls = 0: one call, no warm-up)"""
    ms = []
    for rep in range(calls + 1 if calls else 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if rep or not calls:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main(args):
    import torch
    import fusionpic as fp
    n, grid = args.particles, args.grid
    L = grid * 3e-4
    stream = torch.cuda.Stream()
    sim = fp.makeCylindricalParticlePusher(box_spec(grid, n, L), precision=args.precision)
    sim.setStream(stream.cuda_stream)
    sim.load(vth=0.01)
    sim.precalc()
    res = {"particles": n, "grid": grid, "calls": args.calls, "precision": args.precision}
    empty = {"x": (2.0, 3.0)}       # a stored position lies in [0, 1): nobody

    def nothing(tag):
        res["nothing_" + tag] = timed(torch, stream, args.calls, lambda: sim.remove(where=empty))
        res["count_" + tag] = timed(torch, stream, args.calls, lambda: sim.count(empty))
        res["ratio_" + tag] = res["nothing_" + tag][0] / res["count_" + tag][0]

    nothing("loaded")
    res["push_first"] = timed(torch, stream, 0, lambda: sim.substeps(1))      # (bins the species)
    sim.substeps(2)
    nothing("stepped")
    res["push"] = timed(torch, stream, args.calls, lambda: sim.substeps(1))
    for fraction, lo in ((1e-4, 0.2), (1e-2, 0.3), (0.5, 0.5)):
        got = []
        t = timed(torch, stream, 0, lambda: got.append(sim.remove(where={"x": (lo, lo + fraction)})))
        res["remove_%g" % fraction] = t + (got[0]["scanned"], got[0]["removed"])
        res["redeposit_solve_after_%g" % fraction] = timed(torch, stream, 0, sim.precalc)
        res["rebinning_push_after_%g" % fraction] = timed(torch, stream, 0, lambda: sim.substeps(1))
        sim.substeps(1)
    out = []
    res["renumber"] = timed(torch, stream, 0, lambda: out.append(sim.renumber())) + (out[0] if out else 0,)
    sim.destroy()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=500000000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--precision", default="fp32")
    main(ap.parse_args())
