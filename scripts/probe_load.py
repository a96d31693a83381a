"""Measurements of the particle loader (fpic_load, fpic_load_profile, fpic_load_radial).  Four modes:

  ulps   the kernel's normals and sines against 50-digit values (tests/load_exact.py) over the 10^5 particles of its scene: an
         fp64 box loaded with vth = 1 (the velocities ARE the normals) and with vamp = 1 (the velocities ARE the sines).
         Prints the largest deviation in float64 ulps per column; tests/test_gpu_load.py takes four times the largest as
         the kernel's bound.
  time   a box of --grid^3 nodes with --particles particles, per precision: (a) load() of the whole population, (b) the
         setRange uploads of the same population from a host block that already exists, (c) a plain fill of six arrays of
         that size (the write stream's floor), and the two-pass form on a rank of a two-rank decomposition that keeps half
         of what it generates.  HIP events on the handle's stream, one warm-up, the median of --calls repetitions.
  profile  the same box and request, per precision and in one run: fpic_load (row (a) of `time`), the request with one
         1025-node density table, with three, and with three density tables, three thermal tables and a shear table
         (fpic_load_profile), and the setRange uploads (b) that are the floor of each.  Prints median, min, max and the
         ratios to (a).
  radial   the same box and request, per precision and in one run: fpic_load, fpic_load_profile with three density tables,
         and fpic_load_radial for a sphere with a 1025-node density, the same with thermal and radial-flow tables, and a
         cylinder with all five tables.  Prints median, min, max and the ratios to fpic_load.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fusion-sim_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def box_spec(grid, n, L):
    return dict(radius=L, length_y=L, height=L, nr=grid, ny=grid, nz=grid, dt=1e-11, nparticles=0, count=n, particle_mass=9.109e-31,
                particle_charge=-1.602e-19, geometry="cart3d", solver="none", macro_weight=1.0)


def ulps(args):
    import numpy as np
    import fusionpic as fp
    import load_exact as exact
    n, L = exact.ULP_PARTICLES, 1.6e-3
    req = exact.ulp_scene((L, L, L))
    hi, lo = exact.exact_normals_and_sines(req, np.arange(n))
    sim = fp.makeCylindricalParticlePusher(box_spec(16, n, L), precision="fp64")
    common = dict(seed=req["seed_lo"] | req["seed_hi"] << 32, stream=req["stream"], mode=[int(m) for m in req["m"]], xphase=req["xphase"], vphase=req["vphase"])
    sim.load(vth=1.0, **common)
    normals = sim.getParticles()["velocity"]
    sim.load(vamp=1.0, **common)
    sines = sim.getParticles()["velocity"]
    assert np.array_equal(sines[:, 0], sines[:, 1]) and np.array_equal(sines[:, 0], sines[:, 2])
    d = exact.ulps(np.concatenate([normals, sines[:, :1]], axis=1), hi, lo)
    out = dict(particles=n, normals=[float(x) for x in d.max(axis=0)[:3]], sine=float(d[:, 3].max()), largest=float(d.max()))
    print(json.dumps(out))
    sim.destroy()


def timed(torch, stream, calls, fn):
    """median milliseconds of fn() between two events on `stream`, after one warm-up"""
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


def time_(args):
    import numpy as np
    import torch
    import fusionpic as fp
    n, grid = args.particles, args.grid
    L = grid * 3e-4
    request = dict(drift=(0.0, 0.0, 0.01), vth=1e-3, mode=(1, 0, 0), xamp=(1e-3 * L, 0, 0), vamp=(1e-5, 0, 0))
    stream = torch.cuda.Stream()
    out = {"particles": n, "grid": grid, "calls": args.calls}
    for precision in ("fp32", "fp64"):
        T, esize = (np.float32, 4) if precision == "fp32" else (np.float64, 8)
        sim = fp.makeCylindricalParticlePusher(box_spec(grid, n, L), precision=precision)
        sim.setStream(stream.cuda_stream)
        res = {}
        res["load"] = timed(torch, stream, args.calls, lambda: sim.load(**request))
        res["load_lattice_cold"] = timed(torch, stream, args.calls, lambda: sim.load(lattice=True))
        block = 1 << 23
        rng = np.random.default_rng(1)
        pos, vel = (rng.random((block, 3)) * L).astype(T), rng.normal(0, 1e-3, (block, 3)).astype(T)

        def upload():
            for first in range(0, n, block):
                m = min(block, n - first)
                sim.setRange(first, position=pos[:m], velocity=vel[:m])
        res["setRange"] = timed(torch, stream, max(1, args.calls // 3), upload)
        sim.destroy()
        del sim
        with torch.cuda.stream(stream):
            six = torch.empty(6 * n, dtype=torch.float32 if precision == "fp32" else torch.float64, device="cuda")
            res["fill"] = timed(torch, stream, args.calls, lambda: six.fill_(1.0))
            del six
        torch.cuda.empty_cache()
        # the two-pass form: rank 0 of two generates all n and keeps the lower half of the planes
        rank = fp.makeCylindricalParticlePusher(box_spec(grid, n // 2 + n // 16, L), precision=precision)
        rank.domainInit(0, 2, ghost_planes=2, migrate_every=4)
        rank.setStream(stream.cuda_stream)
        kept = []
        res["load_keep"] = timed(torch, stream, args.calls, lambda: kept.append(rank.load(count=n, **request)))
        res["kept"] = kept[-1]
        rank.destroy()
        del rank
        torch.cuda.empty_cache()
        res["bytes"] = 6 * n * esize
        res["load_over_fill"] = res["load"][0] / res["fill"][0]
        res["load_below_setRange"] = res["load"][0] < res["setRange"][0]
        out[precision] = res
        print(precision, json.dumps(res), flush=True)
    print(json.dumps(out))


def profile(args):
    import numpy as np
    import torch
    import fusionpic as fp
    n, grid = args.particles, args.grid
    L = grid * 3e-4
    request = dict(drift=(0.0, 0.0, 0.01), vth=1e-3, mode=(1, 0, 0), xamp=(1e-3 * L, 0, 0), vamp=(1e-5, 0, 0))
    x = np.linspace(0.0, 1.0, 1025)
    gauss, wavy, ramp = np.exp(-0.5 * ((x - 0.5) / 0.2) ** 2), 1.0 + 0.5 * np.cos(7 * x), 0.5 + x
    tables = {
        "load": {},
        "density_1": dict(density=(gauss, None, None)),
        "density_3": dict(density=(gauss, wavy, ramp)),
        "density_3_thermal_3_shear": dict(density=(gauss, wavy, ramp), thermal=(ramp, gauss + 0.5, wavy), shear=dict(axis=1, component=2, values=0.01 * np.sin(9 * x))),
    }
    stream = torch.cuda.Stream()
    out = {"particles": n, "grid": grid, "calls": args.calls}
    for precision in ("fp32", "fp64"):
        T = np.float32 if precision == "fp32" else np.float64
        sim = fp.makeCylindricalParticlePusher(box_spec(grid, n, L), precision=precision)
        sim.setStream(stream.cuda_stream)
        res = {}
        for name, tabs in tables.items():
            res[name] = timed(torch, stream, args.calls, lambda: sim.load(**request, **tabs))
        block = 1 << 23
        rng = np.random.default_rng(1)
        pos, vel = (rng.random((block, 3)) * L).astype(T), rng.normal(0, 1e-3, (block, 3)).astype(T)

        def upload():
            for first in range(0, n, block):
                m = min(block, n - first)
                sim.setRange(first, position=pos[:m], velocity=vel[:m])
        res["setRange"] = timed(torch, stream, 1, upload)
        sim.destroy()
        del sim
        torch.cuda.empty_cache()
        res["over_load"] = {name: res[name][0] / res["load"][0] for name in tables}
        res["below_setRange"] = {name: res[name][2] < res["setRange"][0] for name in tables}
        out[precision] = res
        print(precision, json.dumps(res), flush=True)
    print(json.dumps(out))


def radial(args):
    import numpy as np
    import torch
    import fusionpic as fp
    n, grid = args.particles, args.grid
    L = grid * 3e-4
    request = dict(drift=(0.0, 0.0, 0.01), vth=1e-3, mode=(1, 0, 0), xamp=(1e-3 * L, 0, 0), vamp=(1e-5, 0, 0))
    x = np.linspace(0.0, 1.0, 1025)
    gauss, wavy, ramp = np.exp(-0.5 * ((x - 0.5) / 0.2) ** 2), 1.0 + 0.5 * np.cos(7 * x), 0.5 + x
    ball = dict(geometry="sphere", center=(0.5 * L, 0.5 * L, 0.5 * L), r_max=0.4 * L)
    column = dict(ball, geometry="cylinder", axis=2)
    cases = {
        "load": {},
        "density_3": dict(density=(gauss, wavy, ramp)),
        "sphere_density": dict(radial=dict(ball, density=gauss)),
        "sphere_density_thermal_flow": dict(radial=dict(ball, density=gauss, thermal=ramp, flow_radial=-0.01 * x)),
        "cylinder_all_five": dict(radial=dict(column, density=gauss, thermal=ramp, flow_radial=-0.01 * x, flow_azimuthal=0.02 * x, flow_axial=0.01 * wavy)),
    }
    stream = torch.cuda.Stream()
    out = {"particles": n, "grid": grid, "calls": args.calls}
    for precision in ("fp32", "fp64"):
        sim = fp.makeCylindricalParticlePusher(box_spec(grid, n, L), precision=precision)
        sim.setStream(stream.cuda_stream)
        res = {}
        for name, extra in cases.items():
            res[name] = timed(torch, stream, args.calls, lambda: sim.load(**request, **extra))
        sim.destroy()
        del sim
        torch.cuda.empty_cache()
        res["over_load"] = {name: res[name][0] / res["load"][0] for name in cases}
        out[precision] = res
        print(precision, json.dumps(res), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ulps", "time", "profile", "radial"])
    ap.add_argument("--particles", type=int, default=500000000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    {"ulps": ulps, "time": time_, "profile": profile, "radial": radial}[a.mode](a)
