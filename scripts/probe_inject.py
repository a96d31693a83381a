"""Measurements of the particle sources (fpic_reserve, fpic_inject): a box of --grid^3 nodes with --particles
thermal particles of one species, the electrostatic solver, one precision per process (--precision).
  reserve        fpic_reserve from --particles to 1.1 x that (a second, untimed call then makes the room the rest needs);
  load_big       fpic_load over --big = 5e7 particles of the species, beside
  generate_big   fpic_inject of --big particles while the fields are not ready: the generation launch, the combining launch and
                 the other set's id pass, no deposit — the kernels' own times are the profiler's (the bar: the generation launch at
                 most 1.25 x the loader's launch over the same count);
  inject_C       the whole synchronous call with ready fields for C = 5e4, 5e6, --big: generation, tally, the re-deposit (which
                 bins the whole species first) and the solve; beside it what follows — the re-deposit + solve alone (precalc() on
                 the same state) and the next sub-step — an ordinary sub-step's push, and a removing fpic_remove of about C.
HIP events on the handle's stream around the calls (the calls wait for the device themselves), one warm-up and the median of
--calls repetitions where a call can be repeated; an injecting call is made once.  Run under rocprofv3 --kernel-trace --stats
(scripts/probe_inject.sh) the kernels' own times are beside it.  Prints one JSON line."""
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
    n, grid, big = args.particles, args.grid, args.big
    L = grid * 3e-4
    stream = torch.cuda.Stream()
    sim = fp.makeCylindricalParticlePusher(box_spec(grid, n, L), precision=args.precision)
    sim.setStream(stream.cuda_stream)
    kw = dict(seed=7, stream=1, vth=0.01)
    sim.load(**kw)
    res = {"particles": n, "grid": grid, "calls": args.calls, "precision": args.precision, "big": big}
    res["reserve"] = timed(torch, stream, 0, lambda: sim.reserve(0, n + n // 10))
    sim.reserve(0, n + n // 10 + (args.calls + 2) * big + 5050000 + 1024)
    res["load_big"] = timed(torch, stream, args.calls, lambda: sim.load(first=0, count=big, **kw))
    at = [n]

    def generate():
        sim.inject("volume", first=at[0], count=big, **kw)
        at[0] += big

    res["generate_big"] = timed(torch, stream, args.calls, generate)
    sim.precalc()
    res["push_first"] = timed(torch, stream, 0, lambda: sim.substeps(1))      # (bins the species)
    sim.substeps(2)
    res["push"] = timed(torch, stream, args.calls, lambda: sim.substeps(1))
    for count in (50000, 5000000, big):
        def inject():
            sim.inject("volume", first=at[0], count=count, **kw)
            at[0] += count
        res["inject_%g" % count] = timed(torch, stream, 0, inject)
        res["redeposit_solve_after_%g" % count] = timed(torch, stream, 0, sim.precalc)
        res["next_substep_after_%g" % count] = timed(torch, stream, 0, lambda: sim.substeps(1))
        sim.substeps(1)
        held = sim.population()["n"]
        got = []
        res["remove_%g" % count] = timed(torch, stream, 0, lambda: got.append(sim.remove(where={"x": (0.3, 0.3 + count / held)}))) + (got[0]["removed"],)
        sim.substeps(2)
    res["population"] = sim.population()
    sim.destroy()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=500000000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--big", type=int, default=50000000)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--precision", default="fp32")
    main(ap.parse_args())
