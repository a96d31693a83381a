"""Measurements of the prescribed external forces (fpic_force): a box of --grid^3 nodes with --particles particles, solver
'none', per precision.  The yardstick in the same box and run is RELAX of fpic_collide (relax_kernel: the same launch shape,
three arrays read and written); then fpic_force on the whole box with one wave (the plain instance: six arrays read, three
written), with one uniform wave, and in a window with three 1025-node tapers and four waves (the windowed instance), first in
the caller's order, then after one sub-step and fpic_sort.  HIP events on the handle's stream, one warm-up, the median of
--calls repetitions; every call is synchronous and ends with the copy of its ten tally words.  Prints one JSON line per
precision: milliseconds (median, least, largest), the particles kicked, and the bytes per second the pass achieved — the
bytes the rule needs (six loads per visited particle and three stores per kicked one, sizeof(T) each) over the median."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))

FOUR = [dict(amp=(1.5e4, 0.0, -0.7e4), mode=(1, 0, 0), nu=0.013, phase=0.1), dict(amp=(0.0, 2.0e4, 0.3e4), mode=(0, 2, -1), nu=-0.27),
        dict(amp=(0.4e4, 0.4e4, 0.4e4), mode=(3, 1, 2), phase=0.625), dict(amp=(-1.0e4, 0.2e4, 0.0), mode=(-2, 0, 5), nu=1.75, phase=-0.3)]


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


def main(args):
    import numpy as np
    import torch
    import fusionpic as fp
    n, grid = args.particles, args.grid
    L = grid * 3e-4
    stream = torch.cuda.Stream()
    x = np.linspace(0.0, 1.0, fp.FORCE_TABLE_MAX)
    taper = np.sin(np.pi * x) ** 2
    cases = {
        "whole_one_wave": dict(waves=FOUR[:1]),
        "whole_uniform": dict(waves=[dict(amp=(1.0e4, 0.0, 0.0), nu=0.01)]),
        "window_tapers_four_waves": dict(waves=FOUR, lo=(L / 4, 0.0, L / 8), hi=(3 * L / 4, L, 7 * L / 8), taper=(taper, taper, taper)),
    }
    out = {"particles": n, "grid": grid, "calls": args.calls}
    for precision in ("fp32", "fp64"):
        size = 4 if precision == "fp32" else 8
        sim = fp.makeCylindricalParticlePusher(box_spec(grid, n, L), precision=precision)
        sim.setStream(stream.cuda_stream)
        sim.load(drift=(0.0, 0.0, 0.01), vth=1e-3)
        res = {}
        epoch = [0]

        def relax():
            epoch[0] += 1
            return sim.collide("relax", nu_tau=0.1, epoch=epoch[0], drift=(0.0, 0.0, 0.01), vth=1e-3)

        for order in ("identity", "sorted"):
            if order == "sorted":               # (the first push bins the species; fpic_sort leaves it sorted by cell)
                sim.precalc()
                sim.substeps(1)
                sim.sort()
            res["%s_relax" % order] = timed(torch, stream, args.calls, relax)
            for name, request in cases.items():
                last = []
                t = timed(torch, stream, args.calls, lambda: last.append(sim.force(**request)))
                kicked = last[-1]["kicked"]
                moved = (6 * n + 3 * kicked) * size
                res["%s_%s" % (order, name)] = t + (kicked, moved / (t[0] * 1e-3))
        sim.destroy()
        del sim
        torch.cuda.empty_cache()
        res["whole_one_wave_over_relax"] = res["sorted_whole_one_wave"][0] / res["sorted_relax"][0]
        out[precision] = res
        print(precision, json.dumps(res), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=500000000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    main(ap.parse_args())
