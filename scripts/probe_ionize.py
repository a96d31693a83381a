"""Measurements of the electron-impact ionisation (fpic_ionize): a box of --grid^3 nodes with --particles
thermal electrons and a few ions, the electrostatic solver, one precision per process (--precision).  For P_max = 1e-3, 1e-2,
1e-1, with one flat table and one window:
  gas_P          fpic_gas ELASTIC over the electrons (the pass the deciding pass is held against: the bar is 1.25 x its launch,
                 read from the profiler's table — both kernels run in this process);
  ionize_P       the whole synchronous fpic_ionize with ready fields: the deciding pass, the 8-byte read-back, the scan, the
                 generation pass, and the settling (which bins both targets again, deposits and solves); M = its events;
  inject_P       fpic_inject of M particles into the electrons, the call that pays the same re-binning;
  next_substep_* the sub-step that follows either; push: an ordinary sub-step.
HIP events on the handle's stream around the calls (the calls wait for the device themselves); the median of --calls
repetitions after one warm-up where a call can be repeated, one call where it grows a species.  Run under rocprofv3
--kernel-trace --stats (scripts/probe_ionize.sh) the kernels' own times are beside it.  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))
C = 2.998e8


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
    assert sim.addSpecies(1.67e-27, 1.602e-19, 1000) == 1
    sim.load(seed=7, stream=1, vth=0.05)
    sim.load(species=1, seed=8, stream=2, vth=0.0005)
    room = n // 10 + 1024
    sim.reserve(0, n + 2 * room)
    sim.reserve(1, 1000 + room)
    sigma, g_lo, g_hi, tau = [3e-19] * 16, 0.01, 0.5, 1e-9
    window = dict(lo=(L / 8, 0.0, 0.0), hi=(7 * L / 8, L, L))            # 0.75 of the box: the word is tested first
    table = dict(sigma=sigma, g_lo=g_lo, g_hi=g_hi, tau=tau, vth=0.001, **window)
    res = {"particles": n, "grid": grid, "calls": args.calls, "precision": args.precision}
    sim.precalc()
    sim.substeps(3)
    res["push"] = timed(torch, stream, args.calls, lambda: sim.substeps(1))
    at = [n]
    for k, p_max in enumerate((1e-3, 1e-2, 1e-1)):
        density = -math.log1p(-p_max) / (C * tau * sigma[0] * g_hi)
        res["gas_%g" % p_max] = timed(torch, stream, args.calls, lambda: sim.collideGas("elastic", density=density, seed=11 + k, **table))
        got = []
        res["ionize_%g" % p_max] = timed(torch, stream, 0, lambda: got.append(sim.ionize(species=0, ion=1, g_threshold=g_lo, density=density, seed=21 + k, **table)))
        m = got[0]["ionised"]
        res["events_%g" % p_max] = {key: got[0][key] for key in ("candidates", "below", "above", "ionised")}
        res["next_substep_after_ionize_%g" % p_max] = timed(torch, stream, 0, lambda: sim.substeps(1))
        sim.substeps(2)

        def inject():
            sim.inject("volume", first=at[0], count=m, seed=7, stream=1, vth=0.05)
            at[0] += m
        res["inject_%g" % p_max] = timed(torch, stream, 0, inject)
        res["next_substep_after_inject_%g" % p_max] = timed(torch, stream, 0, lambda: sim.substeps(1))
        sim.substeps(2)
    res["population"] = [sim.population(0), sim.population(1)]
    sim.destroy()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=500000000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--precision", default="fp32")
    main(ap.parse_args())
