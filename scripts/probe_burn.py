"""Measurements of the fusion burn (fpic_burn): a box of --grid^3 nodes with --particles deuterons and as
many tritons, the electrostatic solver, one precision per process (--precision).  For P_max = 1e-4, 1e-3, 1e-2 (the
probability of a pair at the table's last speed in a cell of the mean population), with one flat table:
  tally_P        fpic_fusion on the same state (the pass the deciding pass is held against: the bar is 1.25 x its launch, read
                 from the profiler's table — both kernels run in this process);
  burn_P         the whole synchronous fpic_burn with ready fields: both cell indices, the deciding pass, the 8-byte read-back,
                 the scan, the generation pass, both compactions and the settling; M = its events;
  remove_P       fpic_remove of about M deuterons by id (remove_move_kernel, which the compaction is held against);
  ionize_P       fpic_ionize of the alphas' species on a gas whose density gives about M events (the whole call of the
                 family that showed the placement).
HIP events on the handle's stream around the calls (the calls wait for the device themselves); the median of --calls
repetitions after one warm-up where a call can be repeated, one call where it changes a species.  Run under rocprofv3
--kernel-trace --stats (scripts/probe_burn.sh) the kernels' own times are beside it.  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))
C = 2.998e8
MD, MT, MA, MN, QP = 3.3435837724e-27, 5.0073567446e-27, 6.6446573357e-27, 1.67492749804e-27, 1.602176634e-19


def box_spec(grid, n, L, W):
    return dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=1e-11, nparticles=0, count=n, particle_mass=MD, particle_charge=QP,
                geometry="cart3d", solver="poisson_fft", macro_weight=W)


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
    L, W = grid * 3e-4, 1e6
    dv = (L / grid) ** 3
    stream = torch.cuda.Stream()
    sim = fp.makeCylindricalParticlePusher(box_spec(grid, n, L, W), precision=args.precision)
    sim.setStream(stream.cuda_stream)
    assert sim.addSpecies(MT, QP, n) == 1 and sim.addSpecies(MA, 2 * QP, 1000) == 2 and sim.addSpecies(MD, QP, 1000) == 3
    sim.load(seed=7, stream=1, vth=0.003)
    sim.load(species=1, seed=8, stream=2, vth=0.0025)
    sim.load(species=2, seed=9, stream=3, vth=0.01)
    sim.load(species=3, seed=10, stream=4, vth=0.001)
    room = n // 20 + 1024
    sim.reserve(2, 1000 + 2 * room)
    sim.reserve(3, 1000 + room)
    sigma, g_lo, g_hi = [5e-28] * 16, 0.0, 0.03
    mean = n / float(grid) ** 3
    res = {"particles": n, "grid": grid, "calls": args.calls, "precision": args.precision, "per_cell": mean}
    sim.precalc()
    sim.substeps(3)
    res["push"] = timed(torch, stream, args.calls, lambda: sim.substeps(1))
    for k, p_max in enumerate((1e-4, 1e-3, 1e-2)):
        tau = p_max * dv / (W * mean * sigma[0] * g_hi * C)
        table = dict(sigma=sigma, g_lo=g_lo, g_hi=g_hi, tau=tau)
        res["tally_%g" % p_max] = timed(torch, stream, args.calls, lambda: sim.fusionYield(0, 1, seed=31 + k, **table))
        got = []
        res["burn_%g" % p_max] = timed(torch, stream, 0, lambda: got.append(sim.burn(0, 1, products=(2, None), other_mass=MN, q_value=2.818e-12, seed=41 + k, **table)))
        m = got[0]["burnt"]
        res["events_%g" % p_max] = {key: got[0][key] for key in ("pairs", "below", "above", "cells", "overfull_cells", "accepted", "blocked", "saturated", "burnt")}
        res["next_substep_after_burn_%g" % p_max] = timed(torch, stream, 0, lambda: sim.substeps(1))
        sim.substeps(2)
        now = sim.population(0)["n"]
        mod = max(2, int(round(now / max(m, 1))))
        gone = []
        res["remove_%g" % p_max] = timed(torch, stream, 0, lambda: gone.append(sim.remove(species=0, every=(mod, 1))))
        res["removed_%g" % p_max] = gone[0]["removed"]
        sim.substeps(2)
        # about m events among the alphas' species would need that many alphas: the deuterons stand in as projectiles
        p_ion = min(0.5, 5.0 * m / max(sim.population(0)["n"], 1))
        density = -math.log1p(-p_ion) / (C * 1e-9 * 3e-19 * 0.02)
        ion = []
        try:
            res["ionize_%g" % p_max] = timed(torch, stream, 0, lambda: ion.append(sim.ionize(species=0, electron=3, ion=2, g_threshold=0.0001, density=density, tau=1e-9,
                                                                                          sigma=[3e-19] * 16, g_lo=0.0001, g_hi=0.02, vth=0.0005, seed=51 + k)))
            res["ionised_%g" % p_max] = ion[0]["ionised"]
        except fp.FusionPicError as e:                                         # (the comparison is lost, the burner's figures are not)
            res["ionize_%g" % p_max] = str(e)
        sim.substeps(2)
    res["population"] = [sim.population(s) for s in range(4)]
    sim.destroy()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=500000000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--precision", default="fp32")
    main(ap.parse_args())
