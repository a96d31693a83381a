"""GPU tests of the particle sources (fpic_reserve, fpic_population, fpic_inject*) against the numpy rule of
tests/inject_reference.py (checked on the CPU by tests/test_inject_reference.py) and against twins: a species that was
injected into equals the species a loader would have made, a box that gained particles equals a fresh box given the grown
population, a registered source equals the same applications made by hand.  The exact parts — ids, counts, the 128-bit
tallies, VOLUME positions without a displacement — are compared bit for bit; the rounded parts within the loader's bound
(tests/test_gpu_load.py: velocity_bound, position_bound, built on KERNEL_ULPS_MEASURED), which the flux kind carries through
its own few operations without a new measured constant.

fpic_energy has no fixed-point words in its row, so "what the species gained" is held against the exact tally of the rows
select() returns after the call minus that of the rows before it, as Python integers.

Met on an MI355X (fp64, 2003 particles per scene): largest |dv| / bound 0.207 (volume) and 0.244 (flux), volume |dp| / bound
0.499, flux normal position |dp| / bound 0.249; fp32: every stored velocity bit-equal to the rounded reference."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import histogram_reference as hr
import inject_reference as ir
import inject_scenes as sc
import load_reference as lr
import moments_reference as mr
import remove_reference as rr
from helpers import ROOT
from test_gpu_histogram import DTYPE, ME, MP, PRECISIONS, QE, box_spec, em_dt
from test_gpu_load import KERNEL_ULPS_MEASURED, ULPS, position_bound, velocity_bound
from test_gpu_remove import bits, refused, rows, same_boxes, same_rows, twin_of, unit_box

pytestmark = pytest.mark.gpu

W = 2.5e5
assert KERNEL_ULPS_MEASURED > 0


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def box(fp, precision, n, solver="poisson_fft", ni=0, load=True):
    """the scenes' box; its species loaded by the loader (stream 40 + species), none stepped"""
    spec = box_spec(sc.SHAPE, sc.L, n, em_dt(sc.SHAPE, sc.L) if solver == "yee" else sc.DT, solver=solver, macro_weight=W)
    sim = fp.makeCylindricalParticlePusher(spec, precision=precision)
    if ni:
        assert sim.addSpecies(MP, -QE, ni) == 1
    if load:
        for k in range(2 if ni else 1):
            sim.load(species=k, seed=99, stream=40 + k, vth=0.02 / (1 + 9 * k))
    return sim, spec


def source_of(scene):
    """the keywords inject() takes for a scene"""
    return {k: v for k, v in scene.items() if k not in ("n", "capacity")}


def reference_of(scene, dt, k=0, L=sc.L):
    req = ir.request(L, dt, kind=scene["kind"], **{key: scene[key] for key in ("axis", "side", "plane") if key in scene}, **sc.load_request(scene))
    return req, ir.sequence(scene["first"], scene["count"], k=k, epoch=scene.get("epoch", 0))


def same_result(got, want):
    for key in ("applications", "injected", "energy_fixed", "momentum_fixed"):
        assert got[key] == want[key], (key, got[key], want[key])
    if "energy" in want:
        for g, w in zip([got["energy"], got["charge"]] + got["momentum"], [want["energy"], want["charge"]] + want["momentum"]):
            assert g == w, (got, want)


def gained(before, after):
    """the exact tally of the rows after minus that of the rows before"""
    a, b = ir.tally_fast(after[2]), ir.tally_fast(before[2])
    return [x - y for x, y in zip(a, b)]


# ---- (a) the twin: an injected range is the range a loader writes into a larger species
@pytest.mark.parametrize("precision", PRECISIONS)
def test_twin_of_a_loaded_species(fp, precision):
    for kw in sc.VOLUME:
        a, _ = box(fp, precision, sc.N, load=False)
        b, _ = box(fp, precision, sc.N + sc.M, load=False)
        assert a.load(first=0, count=sc.N, **kw) == sc.N
        assert a.reserve(0, sc.N + sc.M) == sc.N + sc.M
        got = a.inject("volume", first=sc.N, count=sc.M, **kw)
        assert got["injected"] == sc.M and got["applications"] == 1
        assert b.load(first=0, count=sc.N, **kw) == sc.N and b.load(first=sc.N, count=sc.M, **kw) == sc.M
        assert a.population() == dict(n=sc.N + sc.M, capacity=sc.N + sc.M, id_span=sc.N + sc.M)
        pa, pb = a.getParticles(), b.getParticles()
        assert bits(pa["position"], pb["position"]) and bits(pa["velocity"], pb["velocity"]) and len(pa["position"]) == sc.N + sc.M
        ra, rb = rows(a), rows(b)
        assert same_rows(ra, rb) and bits(ra[0], np.arange(sc.N + sc.M, dtype=np.uint32))
        assert bits(a.getCells(), b.getCells())
        a.destroy()
        b.destroy()


# ---- (b), (d) both kinds against the numpy reference; the tallies exactly
def flux_bounds(req, j):
    """|v - v_ref| per component and |p_axis - ref| of a flux source: the loader's bound (ULPS ulps of each deviate, one rounding
    per operation on either side) on the three deviates n0, n1, s, and the normal velocity's carried through (dt c / L) f_t
    with the three roundings of the position's own operations"""
    r1, c, s, r3, _ = lr.normal_parts(req, j)
    dev = np.empty((len(j), 3))
    dev[:, req["t1"]], dev[:, req["t2"]], dev[:, req["axis"]] = r1 * c, r1 * s, r3
    th = req["vth"] * dev
    bv = ULPS * req["vth"] * np.spacing(np.abs(dev)) + 4 * np.spacing(np.maximum(np.abs(req["drift"] + th), np.abs(th)))
    p, v = ir.states(req, j)
    ft = lr.fractions(req, j)[:, req["axis"]]
    e = np.abs(p[:, req["axis"]] - req["plane_f"])
    bp = bv[:, req["axis"]] * req["step_f"] * ft + 3 * np.spacing(np.maximum(np.maximum(e, np.abs(p[:, req["axis"]])), abs(req["plane_f"])))
    return bv, bp


@pytest.mark.parametrize("scene", sc.SCENES, ids=lambda s: "%s-%d" % (s["kind"], s["stream"]))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_reference(fp, precision, scene):
    T = DTYPE[precision]
    sim, spec = box(fp, precision, scene["n"])
    n, m = scene["n"], scene["count"]
    assert sim.reserve(0, scene["capacity"]) == scene["capacity"]
    before = rows(sim)
    got = sim.inject(**source_of(scene))
    after = rows(sim)
    req, j = reference_of(scene, spec["dt"])
    want = ir.application(req, j, T, mass=ME, charge=QE, weight=W)
    assert sim.population() == dict(n=n + m, capacity=scene["capacity"], id_span=n + m)
    assert same_rows(tuple(x[:n] for x in after), before)                      # nobody else was touched
    assert bits(after[0], np.arange(n + m, dtype=np.uint32))
    pos, vel = after[1][n:], after[2][n:]
    want_p, want_v = ir.stored(req, j, T)
    exact = [a for a in range(3) if not (scene["kind"] == "flux" and a == scene["axis"])] if not np.any(req["xamp_f"]) else []
    for a in exact:     # integers, one rounded multiply, one rounded add: no tolerance
        assert bits(pos[:, a], want_p[:, a]), (a, int((pos[:, a] != want_p[:, a]).sum()))
    assert np.all(pos >= 0) and np.all(pos < 1)
    p64, v64 = ir.states(req, j)
    if scene["kind"] == "flux":
        bv, bp = flux_bounds(req, j)
        ax = scene["axis"]
        assert np.all(vel[:, ax] * scene["side"] > 0)
        wrapped = lr.wrap01(p64.copy())[:, ax]
        dpn = np.abs(pos[:, ax].astype(np.float64) - wrapped)
        dpn = np.minimum(dpn, 1.0 - dpn)                                         # (a plane on the box's face: the wrap's two sides)
    else:
        bv, bp = velocity_bound(req, j), None
    if precision == "fp64":
        dv = np.abs(vel - v64)
        print("%s fp64: largest |dv| / bound %.3f" % (scene["kind"], (dv / bv).max()))
        assert np.all(dv <= bv)
        if np.any(req["xamp_f"]):
            dp = np.abs(pos - lr.wrap01(p64.copy()))
            print("volume fp64: largest |dp| / bound %.3f" % (dp / position_bound(req, j)).max())
            assert np.all(dp <= position_bound(req, j))
        if scene["kind"] == "flux":
            print("flux fp64: largest normal |dp| / bound %.3f" % (dpn / bp).max())
            assert np.all(dpn <= bp)
        # the reference's own velocities differ from the kernel's in the last places: the tally is held against the rows
        assert [got["energy_fixed"]] + got["momentum_fixed"] == ir.tally_fast(vel)
    else:
        one = np.spacing(np.abs(want_v)).astype(np.float64)
        assert np.all(np.abs(vel.astype(np.float64) - want_v.astype(np.float64)) <= one)
        print("%s fp32: share of velocities not bit-equal %.2e" % (scene["kind"], (vel != want_v).mean()))
        assert (vel != want_v).mean() <= 1e-4          # (tests/test_gpu_load.py's share; at 2003 particles: none)
        dp = np.abs(pos.astype(np.float64) - want_p.astype(np.float64))
        assert np.all(np.minimum(dp, 1.0 - dp) <= np.spacing(np.maximum(want_p, T(2.0 ** -20))).astype(np.float64))
        if bits(vel, want_v):
            same_result(got, want)
    # (d) what the species gained: the rows after minus the rows before, as integers; the charge
    assert [got["energy_fixed"]] + got["momentum_fixed"] == gained(before, after)
    assert got["injected"] == m and got["charge"] == (float(m) * QE) * W == want["charge"]
    assert got["energy"] == 0.5 * ME * W * ir.C * ir.C * rr.fixed_to_double(got["energy_fixed"])
    assert sim.count() == n + m
    sim.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_species_on_one_stream_add_no_charge(fp, precision):
    sim, _ = box(fp, precision, sc.N, ni=sc.N)
    for k in range(2):
        sim.reserve(k, sc.N + sc.M)
    sim.precalc()
    rho = sim.readField(fp.F3_RHO_FIXED)
    assert np.any(rho != 0)
    kw = dict(kind="flux", axis=2, side=1, plane=0.3 * sc.L[2], seed=8, stream=3, vth=0.05, first=100, count=sc.M)
    for k in range(2):
        sim.inject(species=k, **kw)
    sim.precalc()
    assert bits(sim.readField(fp.F3_RHO_FIXED), rho)
    a, b = rows(sim, 0), rows(sim, 1)
    assert bits(a[1][sc.N:], b[1][sc.N:]) and bits(a[2][sc.N:], b[2][sc.N:])
    sim.destroy()


# ---- (c) counts that straddle a lane's vector, a workgroup's turn and the grid's turn
@pytest.mark.parametrize("precision", PRECISIONS)
def test_boundary_counts(fp, precision):
    """The slots at and past n + count (the padding up to n_pad) cannot be read through any call: no reader goes past n, and a
    later injection writes them before they become visible.  What can be seen is held: the old rows keep every bit, exactly
    n + count rows exist with the ids 0 .. n + count - 1, the far end of the range is the rule's, and — two applications
    against one: a second application lands on what the first left past its end — the species equals the single-shot twin."""
    kw = dict(seed=21, stream=6, vth=(0.03, 0.02, 0.01), drift=(0.0, 0.01, 0.0))
    for count in sc.boundary_counts():
        sim, spec = box(fp, precision, sc.N)
        before = rows(sim)
        sim.reserve(0, sc.N + count)
        got = sim.inject("volume", first=5, count=count, **kw)
        after = rows(sim)
        assert sim.population()["n"] == sc.N + count == len(after[0])
        assert bits(after[0], np.arange(sc.N + count, dtype=np.uint32))
        assert same_rows(tuple(x[:sc.N] for x in after), before)
        assert got["injected"] == count and [got["energy_fixed"]] + got["momentum_fixed"] == gained(before, after)
        if count <= sc.CHUNK + 1:
            req = ir.request(sc.L, spec["dt"], **kw)
            want_p, _ = ir.stored(req, ir.sequence(5, count), DTYPE[precision])
            assert bits(after[1][sc.N:], want_p)
        else:                                   # the far end of a long range: its last particles are the rule's
            req = ir.request(sc.L, spec["dt"], **kw)
            tail = ir.sequence(5, count)[-9:]
            assert bits(after[1][-9:], ir.stored(req, tail, DTYPE[precision])[0])
        if count <= sc.CHUNK + 1:               # in two applications of count and 7, against one of count + 7
            sim.reserve(0, sc.N + count + 7)
            sim.inject("volume", first=5 + count, count=7, **kw)
            one, _ = box(fp, precision, sc.N)
            one.reserve(0, sc.N + count + 7)
            one.inject("volume", first=5, count=count + 7, **kw)
            assert same_rows(rows(sim), rows(one))
            one.destroy()
        sim.destroy()


# ---- (e) a box that gained particles is the fresh box of the grown population
def grow(sim, solver):
    """a flux source and a volume source into both species on one stream each (a neutral pair: full EM needs it)"""
    for k in range(2):
        n = sim.population(k)["n"]
        sim.reserve(k, n + 1500)
    out = []
    for k in range(2):
        out.append(sim.inject("flux", species=k, axis=0, side=1, plane=0.25, seed=31, stream=2, vth=0.03, first=0, count=700))
        out.append(sim.inject("volume", species=k, lo=(0.2, 0.2, 0.2), hi=(0.8, 0.7, 0.9), seed=32, stream=3, vth=0.01, drift=(0.0, 0.0, 0.02), first=50, count=800))
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fresh_twin_electrostatic(fp, precision):
    sim, spec = unit_box(fp, precision, "poisson_fft", 4000, ni=1500, weight=2e9)
    sim.precalc()
    sim.substeps(5)
    got = grow(sim, "poisson_fft")
    assert all(g["injected"] in (700, 800) for g in got)
    assert sim.population(0)["n"] == 5500 and sim.population(1)["n"] == 3000
    twin = twin_of(fp, sim, spec, precision)
    twin.precalc()
    same_boxes(fp, sim, twin)
    for _ in range(5):
        sim.substeps(1)
        twin.substeps(1)
        same_boxes(fp, sim, twin)
    sim.destroy()
    twin.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_em_neutral_pair_against_a_twin(fp, precision):
    """the fields stay; the grown box steps as a box that was given the grown population and the same lattice fields"""
    sim, spec = unit_box(fp, precision, "yee", 4000, ni=1500, weight=2e9)
    sim.precalc()
    sim.substeps(4)
    which = (fp.F3_EDGE_E, fp.F3_FACE_B, fp.F3_E)
    fields = [sim.readField(w) for w in which]
    grow(sim, "yee")
    assert all(bits(sim.readField(w), f) for w, f in zip(which, fields))
    twin = twin_of(fp, sim, spec, precision)
    shape = (spec["nz"], spec["ny"], spec["nr"], 4)
    for key, f in (("edge_E", fields[0]), ("face_B", fields[1])):
        twin.set(**{key: np.ascontiguousarray(f.reshape(shape)[..., :3].transpose(2, 1, 0, 3))})
    assert all(bits(twin.readField(w), f) for w, f in zip(which[:2], fields[:2]))
    for _ in range(5):
        sim.substeps(1)
        twin.substeps(1)
        for k in range(2):
            assert same_rows(rows(sim, k), rows(twin, k), ids=False)
        assert all(bits(sim.readField(w), twin.readField(w)) for w in which[:2])
    sim.destroy()
    twin.destroy()


# ---- (f) the registered form
FLUX_ON = dict(kind="flux", axis=0, side=1, plane=0.5, seed=41, stream=1, vth=0.03, first=10, count=300)
VOLUME_ON = dict(kind="volume", species=1, lo=(0.1, 0.1, 0.1), hi=(0.9, 0.9, 0.9), seed=42, stream=2, vth=0.004, first=0, count=200, epoch=2)


@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_registered_equals_manual(fp, precision, solver):
    a, spec = unit_box(fp, precision, solver, 4000, ni=1000, weight=2e9)
    b, _ = unit_box(fp, precision, solver, 4000, ni=1000, weight=2e9)
    for s in (a, b):
        s.reserve(0, 4000 + 7 * 300)
        s.reserve(1, 1000 + 2 * 200)
        s.precalc()
    assert a.injectEvery(1, **FLUX_ON) == 0
    assert a.injectEvery(3, **VOLUME_ON) == 1
    a.substeps(7)
    parts = [[], []]
    for step in range(1, 8):
        b.substeps(1)
        parts[0].append(b.inject(**dict(FLUX_ON, first=10 + (step - 1) * 300)))
        if step % 3 == 0:
            parts[1].append(b.inject(**dict(VOLUME_ON, epoch=0, first=(2 + step // 3 - 1) * 200)))
    for index in range(2):
        got, want = a.injectStats(index), ir.add_results(parts[index])
        for key in want:
            assert got[key] == want[key], (index, key)
        assert got == a.injectStats(index, "local")
    assert a.injectStats(0)["applications"] == 7 and a.injectStats(1)["injected"] == 400
    assert a.population(0)["n"] == 4000 + 2100 and a.population(1)["n"] == 1400
    for s in range(2):
        assert same_rows(rows(a, s), rows(b, s))
    assert bits(a.readField(fp.F3_E), b.readField(fp.F3_E))
    assert len(a.getParticles()["position"]) == 6100          # the getter's count is the library's
    a.clearInjections()
    refused(fp, lambda: a.injectStats(0), -1, ".index")
    a.substeps(3)
    assert a.population(0)["n"] == 6100
    for s in (a, b):
        s.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_order_in_the_hook(fp, precision):
    """a sink that covers a source's window, registered beside it, leaves that sub-step's fresh particles alive; an energy row
    recorded on that sub-step counts them"""
    sim, spec = unit_box(fp, precision, "poisson_fft", 3000, weight=2e9)
    sim.reserve(0, 3000 + 2 * 500)
    sim.precalc()
    window = dict(lo=(0.4, 0.4, 0.4), hi=(0.6, 0.6, 0.6))
    source = sim.injectEvery(2, kind="volume", seed=51, stream=4, vth=0.001, first=0, count=500, **window)
    sink = sim.removeEvery(2, where={"x": (0.35, 0.65), "y": (0.35, 0.65), "z": (0.35, 0.65)})
    sim.recordEnergy(2)
    sim.substeps(2)
    gone = sim.removeStats(sink)["removed"]
    assert sim.injectStats(source)["injected"] == 500
    n = sim.population()
    assert n["n"] == 3000 - gone + 500 and n["id_span"] == 3000 + 500
    ids, pos, _ = rows(sim)
    assert np.array_equal(ids[-500:], np.arange(3000, 3500, dtype=np.uint32))
    assert np.all((pos[-500:] >= 0.4) & (pos[-500:] < 0.6))                    # alive inside the sink's window
    inside = np.all((pos[:-500] >= 0.35) & (pos[:-500] < 0.65), axis=1)
    assert not inside.any()
    row, _ = sim.energyHistory()
    assert int(row["count"][-1][0]) == n["n"]
    sim.substeps(2)        # the sink now takes the first application's particles (they have barely moved), the source refills
    assert sim.injectStats(source)["injected"] == 1000 and sim.removeStats(sink)["removed"] >= gone + 400
    assert sim.population()["id_span"] == 4000
    sim.destroy()


# ---- (g) a thinned species
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_thinned_species(fp, precision, tmp_path):
    sim, spec = unit_box(fp, precision, "poisson_fft", 3000, weight=2e9)
    sim.precalc()
    sim.substeps(3)
    removed = sim.remove(where={"x": (0.2, 0.6)})["removed"]
    assert 0 < removed < 3000
    assert sim.population() == dict(n=3000 - removed, capacity=3000, id_span=3000)
    held = rows(sim)
    refused(fp, lambda: sim.inject("volume", count=removed + 1, vth=0.01), -1, "fpic_reserve")     # the slots
    got = sim.inject("volume", count=removed, seed=61, stream=1, vth=0.01, first=9)                 # fills the capacity exactly
    assert got["injected"] == removed
    assert sim.population() == dict(n=3000, capacity=3000, id_span=3000 + removed)
    after = rows(sim)
    new = after[0] >= 3000
    assert bits(after[0][new], np.arange(3000, 3000 + removed, dtype=np.uint32)) and same_rows(tuple(x[~new] for x in after), held)
    refused(fp, sim.getParticles, -5, "fpic_renumber")                                              # still thinned
    assert sim.injectEvery(1000, count=1, vth=0.01) == 0
    refused(fp, sim.renumber, -5, "registered")                                                     # as for every registered operator
    sim.clearInjections()
    assert sim.renumber() == 3000
    again = rows(sim)
    assert bits(again[0], np.arange(3000, dtype=np.uint32)) and bits(again[1], after[1]) and bits(again[2], after[2])
    assert bits(sim.getParticles()["position"], after[1])
    assert sim.population()["id_span"] == 3000
    sim.substeps(2)
    sim.destroy()


# ---- (h) reserve()
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_reserve_preserves_a_stepped_box(fp, precision, solver):
    a, spec = unit_box(fp, precision, solver, 4000, ni=1500, weight=2e9)
    b, _ = unit_box(fp, precision, solver, 4000, ni=1500, weight=2e9)
    for s in (a, b):
        s.precalc()
        s.substeps(9)        # (past a re-binning: the slots are permuted, a census is pending)
    which = (fp.F3_E, fp.F3_RHO_FIXED) + ((fp.F3_EDGE_E, fp.F3_FACE_B) if solver == "yee" else ())
    before = [rows(a, k) for k in range(2)], [a.readField(w) for w in which], a.energy()
    assert a.reserve(0, 100) == 4000 and a.reserve(0, 4000) == 4000              # too small: a no-op
    assert a.reserve(0, 4001) == 4001 and a.reserve(0, 9000) == 9000             # growing twice, across a stride
    assert a.reserve(1, 1501) == 1501 and a.reserve(1, 1500) == 1501
    assert a.population(0) == dict(n=4000, capacity=9000, id_span=4000) and a.population(1)["capacity"] == 1501
    assert all(same_rows(rows(a, k), before[0][k]) for k in range(2))
    assert all(bits(a.readField(w), f) for w, f in zip(which, before[1]))
    assert {k: np.asarray(v).tobytes() for k, v in a.energy().items()} == {k: np.asarray(v).tobytes() for k, v in before[2].items()}
    pa, pb = a.getParticles(), b.getParticles()
    assert bits(pa["position"], pb["position"]) and bits(pa["velocity"], pb["velocity"])
    for _ in range(10):
        a.substeps(1)
        b.substeps(1)
        assert all(same_rows(rows(a, k), rows(b, k)) for k in range(2))
        assert all(bits(a.readField(w), b.readField(w)) for w in which)
    refused(fp, lambda: a.reserve(0, (1 << 32) - 4096 - 1), -1, ".capacity")
    refused(fp, lambda: a.reserve(5, 10), -1, "species")
    assert a.population(0)["capacity"] == 9000
    for s in (a, b):
        s.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_reserve_under_registered_cell_operators(fp, precision):
    """the cell index of collidePairEvery / fusionYieldEvery / fusionSpectrumEvery is sized from the species' stride when they
    are registered and the hook never grows it: a reserve() across a stride AFTER the registration regrows it (the next due
    sub-step used to fail with "found species 1 larger than at its registration"), and the run equals the one that reserved first"""
    fusion = dict(sigma=np.linspace(1e-28, 4e-28, 16), g_lo=0.0, g_hi=0.5, tau=1e-9, seed=5, stream=2)
    sims = [unit_box(fp, precision, "poisson_fft", 1500, ni=900, weight=2e9)[0] for _ in range(2)]
    a, b = sims
    for k in range(2):
        b.reserve(k, 2100)
    for s in sims:
        s.precalc()
        assert s.collidePairEvery(1, 0, 1, log_lambda=10.0, tau=1e-9, seed=3) == 0 and s.fusionYieldEvery(1, 1, **fusion) == 0
        assert s.fusionSpectrumEvery(2, 0, 1, axis="cm", bins=8, lo=0.0, hi=400 * fp.KEV, **fusion) == 0
        s.substeps(1)
    for k in range(2):
        assert a.reserve(k, 2100) == 2100            # 1500 and 900 pad to 2048 and 1024: both strides grow
    for s in sims:
        for k in range(2):
            s.inject("volume", species=k, seed=32, stream=3, vth=0.01, first=50, count=600)
        s.substeps(2)
    for k in range(2):
        assert same_rows(rows(a, k), rows(b, k)) and a.population(k) == dict(n=(2100, 1500)[k], capacity=2100, id_span=(2100, 1500)[k])
    assert a.pairStats(0) == b.pairStats(0) and a.pairStats(0)["applications"] == 3 and a.fusionStats(0)["pairs"] == b.fusionStats(0)["pairs"]
    assert a.fusionSpectrumRead(0)["pairs"] == b.fusionSpectrumRead(0)["pairs"]
    for s in sims:
        s.destroy()


# ---- (i) capacity and id refusals change nothing
def test_refusals_change_nothing(fp):
    sim, spec = unit_box(fp, "fp32", "poisson_fft", 1000, weight=2e9)
    sim.precalc()
    sim.substeps(2)
    before = rows(sim), sim.readField(fp.F3_E), sim.population(), sim.stats()["sort_passes"]
    kw = dict(seed=1, vth=0.01)
    calls = [
        (lambda: sim.inject("volume", count=1, **kw), -1, ("fpic_reserve",)),                                 # no room
        (lambda: sim.inject("volume", count=1, first=(1 << 32) - 1, **kw), -1, (".first",)),                  # the loader's 32-bit rule
        (lambda: sim.inject("volume", count=1 << 32, **kw), -1, (".first",)),
        (lambda: sim.inject("volume", count=5, epoch=1 << 31, first=0, **kw), -5, ("2^32",)),                 # the sequence numbers
        (lambda: sim.inject("flux", count=1, axis=0, side=0, **kw), -1, (".side",)),
        (lambda: sim.inject("flux", count=1, axis=0, side=1, plane=1.5, **kw), -1, (".plane",)),
        (lambda: sim.inject("flux", count=1, axis=1, side=1, drift=(0, 0.1, 0), **kw), -1, (".drift",)),
        (lambda: sim.inject("flux", count=1, axis=1, side=1, paired=True, **kw), -1, ("PAIRED",)),
        (lambda: sim.inject("flux", count=1, axis=1, side=1, mode=(1, 0, 0), **kw), -1, (".mode",)),
        (lambda: sim.inject("volume", count=1, axis=1, **kw), -1, (".axis",)),
        (lambda: sim.inject("volume", count=1, species=3, **kw), -1, (".species",)),
        (lambda: sim.injectEvery(0, count=1, **kw), -1, (".every",)),
        (lambda: sim.injectStats(0), -1, (".index",)),
    ]
    for call, code, words in calls:
        refused(fp, call, code, *words)
    sim.reserve(0, 1010)
    after_reserve = rows(sim)
    refused(fp, lambda: sim.inject("volume", count=11, **kw), -1, "fpic_reserve")
    assert sim.inject("volume", count=0, **kw)["injected"] == 0                                               # nothing to do: nothing happens
    assert same_rows(rows(sim), after_reserve) and same_rows(after_reserve, before[0]) and sim.population()["n"] == 1000
    assert bits(sim.readField(fp.F3_E), before[1])
    # a registered source that stops fitting fails the step with a state error; what it did before stays
    assert sim.injectEvery(1, count=6, **kw) == 0
    sim.substeps(1)
    assert sim.population()["n"] == 1006
    refused(fp, lambda: sim.substeps(1), -5, "fpic_reserve")
    assert sim.population()["n"] == 1006 and sim.injectStats(0)["applications"] == 1 and sim.injectStats(0)["injected"] == 6
    sim.clearInjections()
    for k in range(fp.INJECT_MAX_OPS):
        assert sim.injectEvery(1000, count=1, **kw) == k
    refused(fp, lambda: sim.injectEvery(1000, count=1, **kw), -1, "FPIC_INJECT_MAX_OPS")
    sim.destroy()
    from helpers import make_spec
    rz = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    for call in (lambda: rz.inject(count=1), lambda: rz.injectEvery(1, count=1), lambda: rz.injectStats(0), rz.clearInjections, lambda: rz.reserve(0, 10), rz.population):
        refused(fp, call, -5, "CART3D")
    rz.destroy()


# ---- (j) every operator and diagnostic on a grown species
@pytest.mark.parametrize("precision", PRECISIONS)
def test_operators_and_diagnostics_on_a_grown_species(fp, precision):
    """two boxes at the same sub-step hold the same population, one because its species grew (reserve + inject), one because
    it was made that large and loaded: the per-particle and the cell operators (collide in its elastic and relax kinds,
    collideGas, force, collidePair, fusionYield, fusionSpectrum), which act by id and stored state, do the same to both; the diagnostics of the grown box against their references; sort, the series, a sink after the source"""
    sizes, more = (sc.N, 1500), (sc.M, 300)
    a, _ = box(fp, precision, sizes[0], ni=sizes[1], load=False)
    b, _ = box(fp, precision, sizes[0] + more[0], ni=sizes[1] + more[1], load=False)
    for k in range(2):
        kw = dict(species=k, seed=71, stream=k, vth=0.02 / (1 + 9 * k), drift=(0.0, 0.0, 0.01))
        assert a.load(first=0, count=sizes[k], **kw) == sizes[k]
        a.reserve(k, sizes[k] + more[k])
        assert a.inject("volume", first=sizes[k], count=more[k], **kw)["injected"] == more[k]
        assert b.load(first=0, count=sizes[k] + more[k], **kw) == sizes[k] + more[k]
    for s in (a, b):
        s.addB(0.0, 0.02, 0.05)
        s.precalc()
    same_boxes(fp, a, b)
    sigma = np.full(16, 3e-19)
    before = rows(a)
    tallies = []
    fusion = dict(sigma=np.linspace(1e-28, 4e-28, 16), g_lo=0.0, g_hi=0.5, tau=1e-9, seed=5, stream=2, epoch=1)
    for s in (a, b):
        s.collide("elastic", nu_tau=0.8, vth=0.02, mass_ratio=2.0, seed=7, epoch=3)
        s.collide("relax", nu_tau=0.1, vth=0.01, seed=8)
        s.collideGas("exchange", density=2e19, tau=1e-9, sigma=sigma, g_lo=0.0, g_hi=0.5, vth=0.01, seed=9)
        s.force(waves=[dict(amp=5e4, mode=(1, 0, 2), nu=0.25)])
        pairs = s.collidePair(0, 1, log_lambda=10.0, tau=1e-9, seed=3)
        assert pairs["pairs"] > 0
        # the tallies over the cell index, which is sized from the species' arrays: unlike and like pairs, the yield and its spectrum
        got = [s.fusionYield(0, 1, **fusion), s.fusionYield(0, **fusion), s.fusionSpectrum(0, 1, axis="cm", bins=16, lo=0.0, hi=400 * fp.KEV, **fusion),
               s.fusionSpectrum(1, axis="cm", bins=8, lo=0.0, hi=4000 * fp.KEV, **fusion)]
        assert all(g["pairs"] > 0 and g["reactions_exact"] > 0 for g in got)
        tallies.append([{k: np.asarray(v).tolist() for k, v in g.items()} for g in got])
    assert tallies[0] == tallies[1]
    same_boxes(fp, a, b)
    ra = rows(a)
    assert not bits(ra[2][sizes[0]:], before[2][sizes[0]:])          # (the operators reached the new particles)
    a.sort()
    assert same_rows(rows(a), ra)
    got = a.histogram("vx", 32, (-0.1, 0.1))
    counts, outside = hr.histogram(ra[1], ra[2], ["vx"], [32], [(-0.1, 0.1)])
    assert np.array_equal(got["counts"], counts) and got["outside"] == outside
    m = a.moments("order1")
    want, _ = mr.moments(ra[1], ra[2], sc.SHAPE, "order1")
    assert all(np.array_equal(m[key], want[key]) for key in ("N", "FX", "FY", "FZ"))
    last = sizes[0] + more[0] - 1
    tr = a.series(tracers=[0, last])["tracers"]
    assert np.array_equal(tr[1][3:6], ra[2][last].astype(np.float64)) and np.array_equal(tr[0][3:6], ra[2][0].astype(np.float64))
    ma, mb = a.modes([(1, 0, 0), (0, 2, 1)]), b.modes([(1, 0, 0), (0, 2, 1)])
    assert all(np.asarray(ma[k]).tobytes() == np.asarray(mb[k]).tobytes() for k in ma)
    for _ in range(3):
        for s in (a, b):
            s.substeps(3)                         # (past the re-binning of the eighth sub-step)
        same_boxes(fp, a, b)
    ra = rows(a)
    assert a.remove(where={"x": (0.0, 0.1)})["removed"] == int((ra[1][:, 0] < 0.1).sum()) > 0      # a sink after a source
    a.substeps(2)
    assert a.population()["n"] == a.count()
    a.destroy()
    b.destroy()


# ---- (k) checkpoint round trip of a grown species
@pytest.mark.parametrize("precision", PRECISIONS)
def test_checkpoint_of_a_grown_species(fp, precision, tmp_path):
    sim, spec = unit_box(fp, precision, "poisson_fft", 4000, ni=1500, weight=2e9)
    sim.precalc()
    sim.substeps(3)
    grow(sim, "poisson_fft")
    path = str(tmp_path / "grown.ckpt")
    sim.saveCheckpoint(path)
    sim.substeps(4)
    want = [rows(sim, k) for k in range(2)], sim.readField(fp.F3_E)
    fresh, _ = unit_box(fp, precision, "poisson_fft", 4000, ni=1500, weight=2e9)
    refused(fp, lambda: fresh.loadCheckpoint(path), -1, "fpic_reserve")            # the species lacks the capacity
    for k in range(2):
        fresh.reserve(k, sim.population(k)["n"] + 10)
    fresh.loadCheckpoint(path)
    assert fresh.population(0) == dict(n=5500, capacity=5510, id_span=5500) and fresh.population(1)["n"] == 3000
    fresh.substeps(4)
    assert all(same_rows(rows(fresh, k), want[0][k]) for k in range(2)) and bits(fresh.readField(fp.F3_E), want[1])
    sim.loadCheckpoint(path)                                                        # and into the handle that wrote it
    sim.substeps(4)
    assert all(same_rows(rows(sim, k), want[0][k]) for k in range(2))
    sim.destroy()
    fresh.destroy()


# ---- (l) a decomposition
def test_a_decomposition_is_refused(fp):
    sims = [unit_box(fp, "fp32", "poisson_fft", 100, b=False)[0] for _ in range(2)]
    for r, s in enumerate(sims):
        s.domainInit(r, 2, ghost_planes=1)
    group = fp.BoxGroup(sims)
    for owner in sims + [group]:
        for call in (lambda: owner.inject(count=1), lambda: owner.injectEvery(1, count=1), lambda: owner.injectStats(0), owner.clearInjections,
                     lambda: owner.reserve(0, 200)):
            refused(fp, call, -5, "undecomposed")
    assert sims[0].population() == dict(n=0, capacity=100, id_span=0)              # a rank's own numbers
    for s in sims:
        s.destroy()


# ---- (m) the Node host
def test_inject_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    n = 4000
    spec = box_spec((8, 8, 8), (1.0, 1.0, 1.0), n, 1e-9, solver="poisson_fft", macro_weight=2e9)
    population = dict(seed=123456789, stream=3, drift=[0.0, 0.01, 0.0], vth=0.05)
    now = dict(kind="flux", axis=2, side=-1, plane=0.75, seed=5, stream=1, vth=[0.01, 0.02, 0.03], first=3, count=500)
    on = dict(kind="volume", lo=[0.1, 0.1, 0.1], hi=[0.9, 0.5, 0.9], seed=6, stream=2, vth=0.02, first=0, count=250, epoch=1)
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, population=population, now=now, on=on)))
    script = r"""
const fs = require('fs');
const crypto = require('crypto');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.load(inp.population);
const reserved = sim.reserve(0, 5000);
sim.precalc();
const plain = (r) => ({applications: r.applications, injected: r.injected, energy_fixed: r.energyFixed.toString(),
  momentum_fixed: r.momentumFixed.map((x) => x.toString()), energy: r.energy, momentum: Array.from(r.momentum), charge: r.charge});
const first = plain(sim.inject(inp.now));
const index = sim.injectEvery(2, inp.on);
sim.step(2);
const stats = plain(sim.injectStats(index));
const local = plain(sim.injectStats(index, 'local'));
const got = sim.getParticles();          // (no population() first: the getter learns the count a registered source has changed)
const cells = sim.getCells();
const pop = sim.population(0);
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const errors = [];
const tries = [() => sim.inject(7), () => sim.inject({kind: 'beam', count: 1}), () => sim.inject({count: 1}), () => sim.inject({kind: 'flux', count: 1, axis: 0, side: 0}),
  () => sim.inject({species: 3, count: 0}), () => sim.injectEvery(0, {count: 1}), () => sim.injectEvery(0.5, {count: 1}), () => sim.injectStats(4),
  () => sim.injectStats(0.5), () => sim.reserve(0, 4294967295), () => sim.reserve(9, 10), () => sim.population(9),
  () => sim.getParticles({position: new Float32Array(3 * 4000), velocity: new Float32Array(3 * 4000)}), () => sim.getCells(new Int32Array(4000))];
for (const t of tries) { try { t(); errors.push(null); } catch (err) { errors.push(String(err.message)); } }
sim.clearInjections();
let cleared = null;
try { sim.injectStats(0); } catch (err) { cleared = String(err.message); }
const rank = empic.makeCylindricalParticlePusher(inp.spec);
rank.domainInit(0, 1);
const rankPop = rank.population(0);        // a rank's own numbers; its capacity stays what domainGet sizes its arrays by
const held = rank.domainGet(0);
rank.destroy();
console.log(JSON.stringify({cells: cells.length, rankPop: rankPop, held: held.n, heldRoom: held.position.buffer.byteLength / 12, reserved: reserved, first: first, index: index, stats: stats, local: local, pop: pop, position: sha(got.position), velocity: sha(got.velocity),
  rows: got.position.length / 3, errors: errors, cleared: cleared}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    sim = fp.makeCylindricalParticlePusher(spec)
    sim.load(**population)
    assert sim.reserve(0, 5000) == out["reserved"] == 5000
    sim.precalc()
    plain = lambda r: dict(r, energy_fixed=str(r["energy_fixed"]), momentum_fixed=[str(x) for x in r["momentum_fixed"]])
    lists = lambda w: {k: tuple(v) if isinstance(v, list) else v for k, v in w.items()}
    first = sim.inject(**lists(now))
    assert first["injected"] == 500 and out["first"] == plain(first)
    assert sim.injectEvery(2, **lists(on)) == out["index"] == 0
    sim.step(2)
    stats = sim.injectStats(0)
    assert stats["applications"] == 2 and stats["injected"] == 500 and out["stats"] == plain(stats) == out["local"]
    assert out["pop"] == sim.population() == dict(n=5000, capacity=5000, id_span=5000) and out["rows"] == 5000
    got = sim.getParticles()
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert (out["position"], out["velocity"]) == (sha(got["position"]), sha(got["velocity"]))
    assert all(e is not None for e in out["errors"]), out["errors"]
    assert "fpic_reserve" in out["errors"][2] and "5000" in out["errors"][-1] and "15000" in out["errors"][-2]      # the stale sizes are refused
    assert out["cells"] == 5000 and out["rankPop"] == dict(n=0, capacity=4000, id_span=0) and out["held"] == 0 and out["heldRoom"] == 4000
    assert out["cleared"] is not None and ".index" in out["cleared"]
    sim.destroy()
