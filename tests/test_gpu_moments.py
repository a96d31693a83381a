"""Fluid moment grids of the CART3D box, reduced on the GPU (fpic_moments): every grid and `rejected` against
tests/moments_reference.py applied to a read-back of the same state, as exact integers — all ten moments of both species
of stepped boxes in both field modes and precisions, the charge grid rebuilt from the N grids bit for bit, awkward grid
shapes, the tiled pass against the flat one, particle order, particles that have left their tile's window, sub-masks and
sweeps, values that are rejected, the exact-sum identities, decomposed ranks (in-process group, slab-only and whole-grid
arrays; the communicator over the stand-in RCCL), the Node host, every refusal, that a call changes nothing, and fluid()
on a drifting Maxwellian.  A box that holds a non-finite velocity is never stepped."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import moments_reference as mr
from helpers import ROOT
from test_gpu_histogram import box_spec, em_dt, group_of, plain_box, two_species_box

pytestmark = pytest.mark.gpu

ME, QE, MP = 9.109e-31, -1.602e-19, 1.67e-27
C = 2.998e8
PRECISIONS = ["fp32", "fp64"]
DTYPE = {"fp32": np.float32, "fp64": np.float64}
HOT_STEPS = 7            # steps of the hot run of test_particles_outside_their_window (chosen on the GPU, see its docstring)


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def shape_of(sim):
    return (sim.nx, sim.ny, sim.nz)


def check(sim, which="order2", species=0, stored=None, scope="global"):
    """the library's grids of one handle against the reference over its read-back, exactly.  Returns the library's result."""
    p = stored if stored is not None else sim.getParticles(species=species)
    want, rej = mr.moments(p["position"], p["velocity"], shape_of(sim), which)
    got = sim.moments(which, species=species, scope=scope)
    assert sorted(got) == sorted(list(want) + ["rejected", "spilled"])
    assert got["rejected"] == rej, (which, got["rejected"], rej)
    for name, grid in want.items():
        assert got[name].dtype == np.int64 and got[name].shape == (sim.nz, sim.ny, sim.nx)
        assert np.array_equal(got[name], grid), (which, name, int(np.count_nonzero(got[name] != grid)))
    return got


def check_identities(got, velocity, live=None):
    """the two identities of the definition on a result, and the float64 bound on the first moments"""
    sums, rej = mr.particle_sums(velocity, mr.mask_of([k for k in got if k in mr.NAMES]), live)
    assert got["rejected"] == rej
    for name, want in sums.items():
        assert int(got[name].sum()) == want, name
    # |sum_nodes F_a / 2^32 - sum v_a| <= count * 2^-32: every t = floor(m 2^32) lies within 2^-32 below its m.  The sum of
    # the read-back's float64 values is formed exactly (rationals), so the bound is the derived one and nothing else.
    v = np.asarray(velocity).astype(np.float64)
    ok = ~mr.rejected(v) if live is None else live & ~mr.rejected(v)
    count = int(ok.sum())
    for a, name in enumerate(("FX", "FY", "FZ")):
        if name in got:
            exact = sum((Fraction(float(x)) for x in v[ok, a]), Fraction(0))
            assert abs(Fraction(int(got[name].sum()), 2 ** 32) - exact) <= Fraction(count, 2 ** 32), name


# ---- all ten moments of both species on stepped boxes; the charge grid from the N grids
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stepped_two_species_box(fp, precision, solver):
    sim, spec, _ = two_species_box(fp, precision, solver)
    sim.precalc()
    sim.step(5)
    if solver == "yee":
        sim.density()
    rho = sim.readField(fp.F3_RHO_FIXED).reshape(sim.nz, sim.ny, sim.nx)
    total = np.zeros_like(rho)
    for s, Z in ((0, 1), (1, -1)):        # the library's charge numbers: q_s / q_0 (electrons 1, ions -1)
        p = sim.getParticles(species=s)
        got = check(sim, "order2", species=s, stored=p)
        assert got["rejected"] == 0
        print(precision, solver, "species", s, "spilled", got["spilled"], "of", len(p["velocity"]))
        check_identities(got, p["velocity"])
        total += Z * got["N"]
    assert np.array_equal(total, rho)          # sum over the species of Z_s N_s is FPIC_F3_RHO_FIXED, bit for bit
    sim.destroy()


# ---- grid shapes: not powers of two, not multiples of a tile, smaller than a tile, 2 nodes on an axis
SHAPES = [((20, 18, 12), "poisson_fft"), ((24, 40, 9), "poisson_fft"), ((5, 6, 7), "poisson_fft"), ((2, 16, 3), "poisson_fft"), ((33, 2, 17), "poisson_fft"),
          ((17, 16, 2), "none"), ((20, 18, 12), "yee"), ((9, 24, 10), "yee"), ((5, 6, 7), "yee")]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape,solver", SHAPES)
def test_grid_shapes(fp, precision, shape, solver):
    sim, spec, _ = two_species_box(fp, precision, solver, shape=shape, n=6000, ni=2000, seed=sum(shape))
    flat = check(sim)                                          # as loaded: the flat pass
    assert flat["spilled"] == 6000
    if solver == "none":
        sim.sort()
    else:
        sim.precalc()
        sim.step(3)
        if solver == "yee":
            sim.density()
    rho = sim.readField(fp.F3_RHO_FIXED).reshape(sim.nz, sim.ny, sim.nx)
    a, b = check(sim, species=0), check(sim, species=1)
    assert a["spilled"] < 6000                                 # binned: the tiled pass
    if solver != "none":
        assert np.array_equal(a["N"] - b["N"], rho)            # charge numbers q_s / q_0: 1 and -1
    sim.destroy()


# ---- the tiled pass against the flat one, and the particle order
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_binned_equals_unbinned_and_order_does_not_matter(fp, precision, solver):
    shape, n = (32, 24, 20), 30000
    L = tuple(1e-3 * s for s in shape)
    rng = np.random.default_rng(17)
    pos, vel = rng.random((n, 3)) * L, rng.normal(0, 0.2, (n, 3))
    dt = em_dt(shape, L) if solver == "yee" else 5e-12
    flat = fp.makeCylindricalParticlePusher(box_spec(shape, L, n, dt, solver="none"), precision=precision)
    flat.set(position=pos, velocity=vel)
    a = check(flat)
    assert a["spilled"] == n and a["rejected"] == 0
    perm = rng.permutation(n)
    results = []
    for order, how in ((np.arange(n), "precalc"), (perm, "precalc"), (perm[::-1], "sort")):     # (precalc() deposits and solves; sort() bins)
        sim = fp.makeCylindricalParticlePusher(box_spec(shape, L, n, dt, solver=solver, macro_weight=1e3), precision=precision)
        sim.set(position=pos[order], velocity=vel[order])
        if how == "precalc":
            sim.precalc()
        sim.sort()
        got = sim.moments("order2")
        assert got["spilled"] == 0 and got["rejected"] == 0           # nobody has moved since the binning
        results.append(got)
        sim.destroy()
    for got in results:
        for name in mr.NAMES:
            assert got[name].tobytes() == a[name].tobytes(), name
    flat.destroy()


# ---- particles that have left their tile's window before a re-binning
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_particles_outside_their_window(fp, precision, solver):
    """A hot box stepped HOT_STEPS times: some particles have crossed their tile's faces since the last binning and add
    through global memory, the others through the window in LDS; the sums are exact all the same.  The speed (0.03 c
    thermal) and the step count are chosen so that 0 < spilled < count holds in both field modes and precisions (measured
    on an MI355X: the electrostatic box re-bins every fourth step and holds 344 .. 1455 of 20000 particles outside their
    windows in between, 1056 after seven steps; the full-EM box gains about 100 a step, 724 after seven); the fraction is
    printed."""
    sim, spec, _ = two_species_box(fp, precision, solver)
    sim.precalc()
    sim.step(HOT_STEPS)
    p = sim.getParticles()
    got = check(sim, "order2", stored=p)
    n = len(p["velocity"])
    print("%s %s: %d of %d particles outside their tile's window (%.2f %%)" % (precision, solver, got["spilled"], n, 100.0 * got["spilled"] / n))
    assert 0 < got["spilled"] < n
    check_identities(got, p["velocity"])
    sim.destroy()


# ---- sub-masks and sweeps
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sub_masks_equal_the_full_request(fp, precision, solver):
    sim, spec, _ = two_species_box(fp, precision, solver, n=12000, ni=3000)
    for state in ("flat", "tiled"):
        if state == "tiled":
            sim.precalc()
            sim.step(HOT_STEPS)
        full = sim.moments("order2")            # (more than one sweep of 17 x 17 x 9 windows)
        for which in ["n", "order1", ["N"], ["FX"], ["SYZ"], ["FX", "FY", "FZ"], ["SXX", "SYY", "SZZ"], ["N", "SXX", "SYY", "SZZ"],
                      ["SXY", "SXZ", "SYZ", "FZ", "N"], list(mr.NAMES[1:]), list(mr.NAMES)] + [[name] for name in mr.NAMES]:
            part = sim.moments(which)
            names = [k for k in part if k in mr.NAMES]
            assert sorted(names) == sorted(n_ for b, n_ in enumerate(mr.NAMES) if mr.mask_of(which) >> b & 1)
            assert (part["rejected"], part["spilled"]) == (full["rejected"], full["spilled"]), which
            for name in names:
                assert part[name].tobytes() == full[name].tobytes(), (state, which, name)
        check(sim, "order1")
    sim.destroy()


# ---- rejected particles: a box that is never stepped
@pytest.mark.parametrize("binned", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rejected_particles(fp, precision, binned):
    T = DTYPE[precision]
    n = 40000
    sim, L = plain_box(fp, precision, n, shape=(24, 20, 12))
    rng = np.random.default_rng(31)
    vel = rng.normal(0, 5.0, (n, 3)).astype(T)
    top = np.nextafter(T(128), T(0))
    vel[3::97, 0] = np.nan
    vel[5::89, 1] = np.inf
    vel[7::83, 2] = -np.inf
    vel[11::101, 0] = 128
    vel[13::103, 2] = -128
    vel[17::107, 1] = 1e30
    vel[19::109] = [top, -top, top]              # the largest value below the limit: accepted
    vel[23::113, 1] = -top
    sim.set(position=rng.random((n, 3)) * L, velocity=vel)
    if binned:
        sim.sort()
    p = sim.getParticles()
    assert p["velocity"].dtype == T and np.array_equal(p["velocity"], vel, equal_nan=True)
    got = check(sim, "order2", stored=p)
    want_rej = int(mr.rejected(vel.astype(np.float64)).sum())
    assert got["rejected"] == want_rej and 2000 < want_rej < 4000
    assert got["spilled"] == (0 if binned else n - want_rej)
    check_identities(got, vel)
    assert int(got["N"].sum()) == mr.ONE * (n - want_rej)
    only_n = check(sim, "n", stored=p)           # N alone: the same rule, the same grid
    assert only_n["rejected"] == want_rej and only_n["N"].tobytes() == got["N"].tobytes()
    sim.destroy()


# ---- decomposition: members of an in-process group against the reference and against one handle of the same scene
def union_reference(sims, shape, which="order2"):
    parts = [s.domainGet() for s in sims]
    pos = np.concatenate([p["position"] for p in parts])
    vel = np.concatenate([p["velocity"] for p in parts])
    return mr.moments(pos, vel, shape, which, dead_slots=True), pos, vel


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("world,dist,every,em,precision", [(2, 0, 1, False, "fp32"), (2, 1, 1, False, "fp64"), (4, 0, 2, False, "fp32"),
                                                           (4, 2, 2, False, "fp64"), (2, 0, 2, True, "fp32"), (4, 0, 2, True, "fp64")])
def test_decomposed_group(fp, monkeypatch, world, dist, every, em, precision, compact):
    import decomp_scene as ds
    if not compact:
        monkeypatch.setenv("FPIC_DOMAIN_COMPACT", "0")
    shape = (16, 16, 32) if world == 2 else (16, 16, 64)
    sc = ds.build(fp, dict(world=world, shape=shape, ghost=2, every=every, em=em, distributed_solve=dist, precision=precision,
                           n=20000, seed=world + dist))
    one = fp.makeCylindricalParticlePusher(sc["spec"], precision=precision)
    one.set(position=sc["pos"], velocity=sc["vel"])
    if em:
        one.set(edge_E=sc["E"], face_B=sc["B"])
    else:
        one.precalc()
    g = group_of(fp, sc)
    if not compact:
        monkeypatch.delenv("FPIC_DOMAIN_COMPACT")
    for frame in range(3):
        one.step(); g.step()
        got = g.moments("order2")
        (want, rej), pos, vel = union_reference(g.sims, shape)
        assert got["rejected"] == rej == 0
        for name in mr.NAMES:
            assert np.array_equal(got[name], want[name]), (frame, name)
        check_identities(got, vel, live=~(pos[:, 0] < 0))
        if dist < 2:       # (those runs are the one handle's bit for bit)
            h1 = one.moments("order2")
            for name in mr.NAMES:
                assert h1[name].tobytes() == got[name].tobytes(), (frame, name)
        sub = g.moments(["N", "FZ"])
        assert sub["N"].tobytes() == got["N"].tobytes() and sub["FZ"].tobytes() == got["FZ"].tobytes()
    # a member's LOCAL grids are zero on the planes it does not hold (slab-only arrays) and add up over the members
    local = [s.moments("n", scope="local") for s in g.sims]
    assert sum(int(l["N"].sum()) for l in local) == mr.ONE * sc["n"]
    if compact and world == 4:
        nzl = shape[2] // world
        for r, l in enumerate(local):
            far = (np.arange(shape[2]) - r * nzl - nzl // 2) % shape[2]
            far = (far > nzl // 2 + 8) & (far < shape[2] - nzl // 2 - 8)     # well beyond the slab and its halo
            assert far.any() and not l["N"][far].any()
    dead = sum(int((s.domainGet()["position"][:, 0] < 0).sum()) for s in g.sims)
    print("world", world, "dist", dist, "em", em, "compact", compact, "dead slots held at the end", dead)
    with pytest.raises(fp.FusionPicError, match="in-process group"):
        g.sims[0].moments("n", scope="global")
    assert sum(s.domainStats()["migrated"] for s in g.sims) > 0
    one.destroy()
    for s in g.sims:
        s.destroy()


# ---- the communicator: ranks as threads of one process over the stand-in RCCL (tests/fake_rccl)
COMM_DRIVER = r'''
import hashlib, json, os, sys, threading
sys.path.insert(0, os.path.join(sys.argv[1], "fusion-sim_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import fusionpic as fp
import decomp_scene as ds
import moments_reference as mr
import test_gpu_histogram as th
import test_gpu_moments as tm
sc = ds.build(fp, json.loads(sys.argv[2]))
requests = json.loads(sys.argv[3])
world = sc["world"]
uid = fp.commUniqueId()
out, err = [None] * world, [None] * world
def digest(m):
    return {k: (hashlib.sha256(v.tobytes()).hexdigest() if k in mr.NAMES else v) for k, v in m.items()}
def rank_main(r):
    try:
        s = fp.makeCylindricalParticlePusher(dict(sc["spec"], count=3 * sc["n"]), precision=sc["precision"])
        s.commInit(uid, r, world)
        s.domainInit(r, world, ghost_planes=sc["G"], migrate_every=sc["every"], distributed_solve=sc["dist_solve"])
        first = int(sc["counts"][:r].sum())
        s.domainSet(sc["pos"][first:first + sc["counts"][r]], sc["vel"][first:first + sc["counts"][r]], first_id=first)
        s.precalc()
        for _ in range(sc["frames"]):
            s.step()
        res = []
        for which in requests:
            g = s.moments(which, scope="global")
            l = s.moments(which, scope="local")
            res.append((digest(g), int(l["N"].sum()) if "N" in l else None))
        out[r] = (res, s.domainStats()["migrated"])
        s.destroy()
    except Exception as e:
        err[r] = repr(e)
threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
for t in threads: t.start()
for t in threads: t.join()
if any(err):
    print(json.dumps({"error": err})); sys.exit(0)
g = th.group_of(fp, sc)
for _ in range(sc["frames"]):
    g.step()
grp = []
for which in requests:
    m = g.moments(which)
    (want, rej), pos, vel = tm.union_reference(g.sims, sc["shape"], which)
    ok = m["rejected"] == rej and all(np.array_equal(m[k], want[k]) for k in want)
    grp.append((digest(m), bool(ok)))
print(json.dumps({"ranks": out, "group": grp}))
'''


@pytest.mark.parametrize("world,shape", [(2, (16, 16, 32)), (3, (12, 16, 18)), (2, (64, 64, 32))])
def test_communicator_global_equals_group_sums(fp, world, shape):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "fake_rccl")])
    env = dict(os.environ, FPIC_RCCL_LIBRARY=os.path.join(ROOT, "tests", "fake_rccl", "libfakerccl.so"))
    case = dict(world=world, shape=shape, ghost=2 if world == 2 else 1, every=2 if world == 2 else 1, em=False, distributed_solve=0,
                precision="fp32", n=20000, seed=8, frames=3)
    # (64 x 64 x 32 nodes: a grid is 2^17 words, the ten of them more than one chunk of the gather)
    requests = ["order2", "n", ["FX", "SYZ"]]
    raw = subprocess.check_output([sys.executable, "-c", COMM_DRIVER, ROOT, json.dumps(case), json.dumps(requests)], env=env, timeout=900)
    res = json.loads(raw.decode().strip().splitlines()[-1])
    assert "error" not in res, res
    ranks = res["ranks"]
    assert sum(r[1] for r in ranks) > 0                                   # particles migrated
    for i, (want, ok) in enumerate(res["group"]):
        assert ok, requests[i]                                            # the group's sum is the reference's
        for r in range(world):
            got = ranks[r][0][i][0]
            assert sorted(got) == sorted(want)
            for k in want:
                assert got[k] == want[k], (requests[i], r, k)             # every rank: the group's sums and counters, bit for bit
        if ranks[0][0][i][1] is not None:
            assert sum(ranks[r][0][i][1] for r in range(world)) == mr.ONE * case["n"]   # the LOCAL grids count every particle once


def test_moments_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    rng = np.random.default_rng(2)
    n, shape, L = 4000, (16, 12, 10), (0.016, 0.012, 0.010)
    spec = box_spec(shape, L, n, 5e-12, macro_weight=1e15 * np.prod(L) / n)
    # (float32 values: both hosts hand the library the same numbers)
    pos, vel = (rng.random((n, 3)) * L).astype(np.float32), rng.normal(0, 2e-3, (n, 3)).astype(np.float32)
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, p=pos.astype(np.float64).tolist(), v=vel.astype(np.float64).tolist())))
    script = r"""
const fs = require('fs');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.set({position: inp.p, velocity: inp.v});
const loaded = sim.moments({which: 'order2'});
sim.precalc();
sim.step(3);
const a = sim.moments({species: 0, which: 'order2'});
const b = sim.moments({which: ['FX', 'N']}, 'local');
const c = sim.moments({which: 'n'});
const errors = [];
for (const bad of [{which: 'order3'}, {which: ['N', 'Q']}, {which: []}, {which: 'n', species: 3}, {which: 5}, 7, null]) {
  try { sim.moments(bad); errors.push(null); } catch (e) { errors.push(String(e.message)); }
}
const str = (m) => { const o = {}; for (const k of Object.keys(m)) o[k] = (m[k] instanceof BigInt64Array) ? Array.from(m[k], String) : m[k]; return o; };
const back = sim.getParticles();
console.log(JSON.stringify({loaded: str(loaded), a: str(a), b: str(b), c: str(c), big: a.SXY instanceof BigInt64Array, errors: errors,
  position: Array.from(back.position), velocity: Array.from(back.velocity)}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    # the Node host's grids are the reference's over the Node host's own read-back, whichever request they came from ...
    back_p, back_v = np.array(out["position"], dtype=np.float32).reshape(n, 3), np.array(out["velocity"], dtype=np.float32).reshape(n, 3)
    want, rej = mr.moments(back_p, back_v, shape, "order2")
    assert out["big"] and rej == out["a"]["rejected"] == 0 and out["a"]["spilled"] < n and out["loaded"]["spilled"] == n
    assert sorted(out["a"]) == sorted(list(mr.NAMES) + ["rejected", "spilled"]) and sorted(out["b"]) == ["FX", "N", "rejected", "spilled"] and sorted(out["c"]) == ["N", "rejected", "spilled"]
    for res in (out["a"], out["b"], out["c"]):
        for k, v in res.items():
            if k in mr.NAMES:
                assert [int(x) for x in v] == want[k].ravel().tolist(), k
            else:
                assert v == out["a"][k], k
    # ... and the Python host's of the same upload (the entry point and element type of the Node host's set()), bit for bit
    sim = fp.makeCylindricalParticlePusher(spec)
    sim.setRange(0, position=pos.astype(np.float64), velocity=vel.astype(np.float64))
    full = check(sim, "order2")
    assert sorted(out["loaded"]) == sorted(full)
    for k, v in out["loaded"].items():
        assert ([int(x) for x in v] == full[k].ravel().tolist()) if k in mr.NAMES else (v == full[k]), k
    assert all(e is not None and " <- " in e for e in out["errors"]), out["errors"]
    sim.destroy()


# ---- refusals
def test_refusals_name_the_property(fp):
    sim, spec, _ = two_species_box(fp, "fp32", "poisson_fft", shape=(16, 16, 16), n=2000, ni=500)
    lib = sim._lib

    def raw(**kw):
        """a request written straight into the structure"""
        s = fp.MomentsSpec()
        s.species, s.mask = kw.get("species", 0), kw.get("mask", 1)
        for k, v in enumerate(kw.get("reserved", (0, 0, 0, 0))):
            s.reserved[k] = v
        out, info = (ctypes.c_int64 * (10 * 16 ** 3))(), fp.MomentsInfo()
        sim._check(lib.fpic_moments(sim._h, ctypes.byref(s), kw.get("scope", 0), out, ctypes.byref(info)))
        return sum(out[:16 ** 3])

    assert raw() == 2000 * mr.ONE and raw(species=1) == 500 * mr.ONE and raw(mask=0x3FF, scope=1) == 2000 * mr.ONE
    for kw, prop in ((dict(species=2), ".species"), (dict(species=-1), ".species"), (dict(mask=0), ".mask"), (dict(mask=1 << 10), ".mask"),
                     (dict(mask=0x7FF), ".mask"), (dict(mask=0x80000001), ".mask"), (dict(reserved=(0, 1, 0, 0)), ".reserved"),
                     (dict(reserved=(0, 0, 0, np.nan)), ".reserved"), (dict(scope=2), ".scope"), (dict(scope=-1), ".scope")):
        with pytest.raises(fp.FusionPicError) as e:
            raw(**kw)
        assert prop + " <- " in str(e.value), (kw, str(e.value))
    for kw, prop in ((dict(which="order3"), ".which"), (dict(which=["N", "FW"]), ".which"), (dict(which=[]), ".mask"), (dict(which="n", species=5), ".species")):
        with pytest.raises(fp.FusionPicError) as e:
            sim.moments(**kw)
        assert prop + " <- " in str(e.value), (kw, str(e.value))
    s, info = fp.MomentsSpec(), fp.MomentsInfo()
    s.mask = 1
    out = (ctypes.c_int64 * 16 ** 3)()
    for args in ((None, 0, out, ctypes.byref(info)), (ctypes.byref(s), 0, None, ctypes.byref(info)), (ctypes.byref(s), 0, out, None)):
        assert lib.fpic_moments(sim._h, *args) != 0
        assert b"Non-optional property is undefined" in lib.fpic_last_error(sim._h)
    sim.destroy()


def test_an_rz_handle_is_refused(fp):
    from helpers import make_spec
    sim = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    s, info = fp.MomentsSpec(), fp.MomentsInfo()
    s.mask = 1
    out = (ctypes.c_int64 * 4096)()
    assert sim._lib.fpic_moments(sim._h, ctypes.byref(s), 0, out, ctypes.byref(info)) != 0
    assert b"needs a CART3D handle" in sim._lib.fpic_last_error(sim._h)
    sim.destroy()


def test_needs_no_precalc(fp):
    sim, spec, _ = two_species_box(fp, "fp64", "poisson_fft", shape=(16, 16, 16), n=5000, ni=100)
    check(sim, "order1")
    check(sim, "order2", species=1)
    sim.destroy()


# ---- the call changes nothing
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_call_changes_nothing(fp, precision, solver):
    fields = [fp.F3_RHO_FIXED, fp.F3_E] + ([fp.F3_EDGE_E, fp.F3_FACE_B, fp.F3_J_FIXED] if solver == "yee" else [fp.F3_PHI])
    sim, spec, _ = two_species_box(fp, precision, solver, shape=(16, 16, 16), n=8000, ni=4000, seed=5)
    twin, _, _ = two_species_box(fp, precision, solver, shape=(16, 16, 16), n=8000, ni=4000, seed=5)
    sim.precalc(); twin.precalc()
    sim.step(5); twin.step(5)
    before = [sim.getParticles(species=s) for s in range(2)]
    before_f = [sim.readField(w).tobytes() for w in fields]
    row = sim._energy_row("global").tobytes()
    a = sim.moments("order2")
    b = sim.moments("order2", species=1)
    a2 = sim.moments("order2")
    assert all(a[k].tobytes() == a2[k].tobytes() for k in mr.NAMES) and (a["rejected"], a["spilled"]) == (a2["rejected"], a2["spilled"])
    loc = sim.moments("order2", scope="local")
    assert all(a[k].tobytes() == loc[k].tobytes() for k in mr.NAMES)
    after = [sim.getParticles(species=s) for s in range(2)]
    for s in range(2):
        for k in ("position", "velocity"):
            assert before[s][k].tobytes() == after[s][k].tobytes(), (s, k)
    assert [sim.readField(w).tobytes() for w in fields] == before_f
    assert sim._energy_row("global").tobytes() == row
    # ... and a run with calls interleaved equals a run without, long enough for a re-binning to be decided on the way
    for _ in range(12):
        sim.step(1); twin.step(1)
        sim.moments("order2"); sim.moments("n", species=1)
    for s in range(2):
        p, q = sim.getParticles(species=s), twin.getParticles(species=s)
        assert p["position"].tobytes() == q["position"].tobytes() and p["velocity"].tobytes() == q["velocity"].tobytes()
    assert [sim.readField(w).tobytes() for w in fields] == [twin.readField(w).tobytes() for w in fields]
    sim.destroy(); twin.destroy()


# ---- fluid(): a uniform drifting Maxwellian
@pytest.mark.parametrize("precision", PRECISIONS)
def test_fluid_of_a_drifting_maxwellian(fp, precision):
    """Box averages of fluid() against the loaded drift and temperature within the sampling error of the test's own sizes:
    the mean of N = particles-per-node * nodes samples of a component has the standard deviation sigma / sqrt(N), their
    variance estimate the relative one sqrt(2 / (3 N)) (three components pooled); K = 5 such deviations are allowed."""
    K = 5.0
    shape, ppn = (16, 16, 16), 64
    nodes = shape[0] * shape[1] * shape[2]
    n = ppn * nodes
    L = tuple(1e-3 * s for s in shape)
    W = 2.5e5
    sim = fp.makeCylindricalParticlePusher(box_spec(shape, L, n, 1e-12, solver="none", macro_weight=W), precision=precision)
    rng = np.random.default_rng(77)
    u0, sigma = np.array([0.01, -0.02, 0.005]), 0.01
    sim.set(position=rng.random((n, 3)) * L, velocity=u0 + rng.normal(0, sigma, (n, 3)))
    sim.sort()
    f = sim.fluid()
    dv = np.prod(L) / nodes
    err = K / np.sqrt(ppn * nodes)
    assert f["n"].shape == (16, 16, 16) and f["u"].shape == (3, 16, 16, 16) and f["P"].shape == (3, 3, 16, 16, 16)
    assert abs(f["n"].mean() - W * ppn / dv) <= 1e-12 * W * ppn / dv             # every particle is counted: exact but for rounding
    u_box = f["flux"].sum(axis=(1, 2, 3)) / f["n"].sum()
    print(precision, "u_box / c", u_box / C, "loaded", u0, "allowed", err * sigma)
    assert np.all(np.abs(u_box / C - u0) <= err * sigma)
    T0 = ME * (sigma * C) ** 2 / 1.602176634e-19                                  # eV
    n_box = f["n"].mean()
    P_box = np.array([f["Pi"][a, a].mean() - ME * n_box * u_box[a] ** 2 for a in range(3)])
    T_box = P_box.sum() / (3 * n_box) / 1.602176634e-19
    print(precision, "T_box", T_box, "loaded", T0, "allowed relative", err * np.sqrt(2.0 / 3.0))
    assert abs(T_box / T0 - 1) <= err * np.sqrt(2.0 / 3.0)
    # per node: the definitions hold as identities of the returned arrays
    assert np.allclose(f["P"][0, 1], f["Pi"][0, 1] - ME * f["n"] * f["u"][0] * f["u"][1], rtol=1e-12, atol=0)
    assert np.allclose(f["T"], (f["P"][0, 0] + f["P"][1, 1] + f["P"][2, 2]) / (3 * f["n"]) / 1.602176634e-19, rtol=1e-12, atol=0)
    assert np.allclose(f["u"] * f["n"], f["flux"], rtol=1e-12, atol=0)
    sim.destroy()
