"""The prescribed external forces (fpic_force*) on the GPU against the numpy restatement of their rule
(tests/force_reference.py, proved on the CPU by tests/test_force_reference.py, where the scenes used here are defined and
shown to reach every path): the exact part bit for bit, the rounded part within a bound, the exact tallies, the registered
form against a manual loop, the equivalence with a field in the push, a decomposition that must hold the same particles as
one handle, the refusals, and the JavaScript host.

The bound of the rounded part is built as in tests/test_gpu_collide.py, with its constant: ULPS ulps on the device's and the
reference's cospi, carried through amp, the sum over the waves and sc; every other operation of the rule is one rounding,
counted once on either side (half an ulp each: one spacing); the cast to the handle's precision is one more such operation.
The window, the tapers, theta and arg are the same IEEE operations on either side and carry no error.  Met on an MI355X:
see DESIGN.md 4.22 for the largest distance observed."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import force_reference as ref
from helpers import ROOT
from test_force_reference import (DT, ENVELOPE, ENVELOPE_EPOCH, ENVELOPE_SUBSTEPS, FOUR_WAVES, L, ME, N_SMALL, ONE_PLAIN, SHAPE, SPECIES, TAPER_DYADIC,
                                  TAPER_SMOOTH, WINDOW, scene)
from test_gpu_collide import ULPS
from test_gpu_histogram import PRECISIONS, em_dt

pytestmark = pytest.mark.gpu

DTYPE = {"fp32": np.float32, "fp64": np.float64}
W = 2.5e5


def launch_shape():
    import re
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_force_kernels.hpp")).read()
    get = lambda name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    return get("kForceBlocks"), get("kForceThreads")


BLOCKS, THREADS = launch_shape()
N_BIG = BLOCKS * THREADS * 4 + 2049            # just above one full trip of the grid-stride loop: a second trip and a ragged tail
assert N_BIG == 2099201 and N_BIG % 4 == 1


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def spec_of(n, solver="none", dt=DT, shape=SHAPE, lengths=L, **kw):
    s = dict(radius=lengths[0], length_y=lengths[1], height=lengths[2], nr=shape[0], ny=shape[1], nz=shape[2], dt=dt, nparticles=0, count=n,
             particle_mass=SPECIES[0]["mass"], particle_charge=SPECIES[0]["charge"], geometry="cart3d", solver=solver, macro_weight=W)
    s.update(kw)
    return s


def filled(fp, precision, n, counts=(None, 1000), seed=1, **kw):
    """a box with the two species, species 0 holding scene(n) and species 1 scene(counts[1], seed + 1)"""
    sim = fp.makeCylindricalParticlePusher(spec_of(n, **kw), precision=precision)
    assert sim.addSpecies(SPECIES[1]["mass"], SPECIES[1]["charge"], counts[1]) == 1
    for species, m in ((0, n), (1, counts[1])):
        frac, vel = scene(m, seed + species)
        sim.set(position=frac * np.array(L), velocity=vel, species=species)
    return sim


def accel(waves):
    """the same waves with amplitudes for kind 'accel' (m/s^2: kq = dt / c is 1.7e-20, so 1e17 m/s^2 move v by 1e-3 c a sub-step)"""
    return [dict(w, amp=tuple(float(x) * 1e11 for x in w["amp"])) for w in waves]


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def request_of(species, waves, **kw):
    sp = SPECIES[species]
    return ref.request(L, DT, sp["charge"], sp["mass"], waves, **kw)


def check_tallies(got, before, after, inside, mass, applications=1):
    t = ref.tallies(before, after, inside)
    assert got["applications"] == applications and got["kicked"] == t["kicked"]
    assert got["work_fixed"] == t["work_fixed"] and got["impulse_fixed"] == t["impulse_fixed"], (got, t)
    d = ref.derived(t, mass, W)
    assert got["work"] == d["work"] and got["impulse"] == d["impulse"], (got, d)
    return t


# ---- 1. the exact part (and 3. the tallies): no cosine but cospi(0) = 1
EXACT = {
    "whole box": dict(),
    "window": dict(WINDOW),
    "window and dyadic tapers": dict(WINDOW, taper=TAPER_DYADIC),
    "one taper on the whole box": dict(taper=(None, TAPER_DYADIC[1], None)),
}


def exact_case(fp, precision, n, species, sort, names, kind="field"):
    counts = (None, n if species == 1 else 1000)
    sim = filled(fp, precision, n if species == 0 else 1000, counts=counts)
    if sort:
        sim.sort()
    waves = ONE_PLAIN if kind == "field" else accel(ONE_PLAIN)
    for name in names:
        kw = EXACT[name]
        req = request_of(species, waves, kind=ref.FIELD if kind == "field" else ref.ACCEL, **kw)
        before = sim.getParticles(species=species)
        got = sim.force(waves=waves, species=species, kind=kind, **kw)
        after = sim.getParticles(species=species)
        want, k = ref.stored(req, 0, before["position"], before["velocity"])
        assert bits(after["velocity"], want), (name, n, precision, species, sort)
        assert bits(after["position"], before["position"])
        ins = k["inside"]
        assert bits(after["velocity"][~ins], before["velocity"][~ins]) and got["kicked"] == int(ins.sum())
        assert ins.all() == ("window" not in name) and (after["velocity"][ins] != before["velocity"][ins]).any()
        check_tallies(got, before["velocity"], after["velocity"], ins, SPECIES[species]["mass"])
        other = 1 - species
        assert sim.force(waves=ONE_PLAIN, species=other, envelope=dict(start=1))["applications"] == 0       # (not active at count 0)
    sim.destroy()


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("species", [0, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_part_and_tallies(fp, precision, species, sort):
    exact_case(fp, precision, N_SMALL, species, sort, sorted(EXACT), kind="field" if species == 0 else "accel")
    if species == 0:
        exact_case(fp, precision, N_SMALL, 1, sort, ["window and dyadic tapers"], kind="field")     # the other charge and mass


@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_part_beyond_one_trip_of_the_grid(fp, precision):
    exact_case(fp, precision, N_BIG, 0, precision == "fp64", ["whole box", "window and dyadic tapers"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_term_outside_the_fixed_point_range_makes_its_double_nan(fp, precision):
    n = 257
    sim = filled(fp, precision, n)
    vel = scene(n)[1].copy()
    vel[5] = (200.0, 0.0, 0.0)                                              # |v|^2 = 40000 >= 2^15: the work's term is outside, vx itself inside
    vel[9] = (0.0, -40000.0, 0.0)                                           # vy itself outside (and |v|^2)
    sim.set(velocity=vel)
    before = sim.getParticles()
    got = sim.force(waves=ONE_PLAIN)
    after = sim.getParticles()
    want, k = ref.stored(request_of(0, ONE_PLAIN), 0, before["position"], before["velocity"])
    assert bits(after["velocity"], want) and got["kicked"] == n and got["applications"] == 1
    everybody = np.ones(n, dtype=bool)
    but = lambda *who: np.isin(np.arange(n), who, invert=True)
    tally = lambda mask: ref.tallies(before["velocity"], after["velocity"], mask)
    # a term outside the range adds nothing to its sum and makes the sum's double NaN; the other sums are untouched
    assert np.isnan(got["work"]) and got["work_fixed"] == tally(but(5, 9))["work_fixed"]
    assert np.isnan(got["impulse"][1]) and got["impulse_fixed"][1] == tally(but(9))["impulse_fixed"][1]
    whole = tally(everybody)
    d = ref.derived(whole, ME, W)
    for a in (0, 2):
        assert got["impulse_fixed"][a] == whole["impulse_fixed"][a] and got["impulse"][a] == d["impulse"][a]
    sim.destroy()


# ---- 2. the rounded part
def spacing(x):
    return np.spacing(np.maximum(np.abs(x), np.finfo(np.float64).tiny))


def value_bound(req, k, v, dtype):
    """|v' - v'_ref| allowed per component: ULPS ulps on every cospi, carried through amp, the sum and sc, plus one rounding
    per operation on either side (one spacing), plus the cast to the handle's precision"""
    c = k["c"]
    e = e_err = None
    for w, wave in enumerate(req["waves"]):
        amp = wave["amp"][None, :]
        t = amp * c[:, w:w + 1]
        t_err = np.abs(amp) * (ULPS * spacing(c[:, w:w + 1])) + spacing(t)
        if e is None:
            e, e_err = t, t_err
        else:
            s = e + t
            e_err = e_err + t_err + spacing(np.maximum.reduce([np.abs(e), np.abs(t), np.abs(s)]))
            e = s
    sc = k["sc"][:, None]
    d = sc * e
    d_err = np.abs(sc) * e_err + spacing(d)
    out = v + d
    err = d_err + spacing(np.maximum.reduce([np.abs(v), np.abs(d), np.abs(out)]))
    if dtype == np.float32:
        err = err + np.spacing(np.abs(out.astype(np.float32))).astype(np.float64)
    return err


ROUNDED = {
    "four waves, window, tapers": (FOUR_WAVES, dict(WINDOW, taper=TAPER_SMOOTH, epoch=1234567)),
    "one wave, whole box": (FOUR_WAVES[3:], dict(epoch=77)),
    "four waves, one taper": (FOUR_WAVES, dict(taper=(None, TAPER_SMOOTH[1], None), epoch=(1 << 40) + 5)),
}


def rounded_case(fp, precision, n, sort, names):
    T = DTYPE[precision]
    sim = filled(fp, precision, n)
    if sort:
        sim.sort()
    for name in names:
        waves, kw = ROUNDED[name]
        req = request_of(0, waves, **kw)
        before = sim.getParticles()
        got = sim.force(waves=waves, **kw)
        after = sim.getParticles()
        want, k = ref.stored(req, 0, before["position"], before["velocity"])
        ins = k["inside"]
        assert got["kicked"] == int(ins.sum()) and bits(after["position"], before["position"]) and bits(after["velocity"][~ins], before["velocity"][~ins])
        dv = np.abs(after["velocity"].astype(np.float64) - want.astype(np.float64))[ins]
        bound = value_bound(req, k, before["velocity"].astype(np.float64), T)[ins]
        print("%s %s n=%d: largest |dv| / bound %.3f, share bit-equal %.4f" % (precision, name, n, (dv / bound).max(), (dv == 0).mean()))
        assert np.all(dv <= bound), (name, precision, n)
        assert np.abs(k["d"][ins]).max() > 1e-4
        check_tallies(got, before["velocity"], after["velocity"], ins, ME)
    sim.destroy()


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rounded_part_within_the_bound(fp, precision, sort):
    rounded_case(fp, precision, N_SMALL, sort, sorted(ROUNDED))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rounded_part_beyond_one_trip_of_the_grid(fp, precision):
    rounded_case(fp, precision, N_BIG, precision == "fp32", ["four waves, window, tapers"])


# ---- 4. the registered form equals the manual loop
@pytest.mark.parametrize("solver", ["none", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_registered_equals_manual(fp, precision, solver):
    n = N_SMALL
    dt = em_dt(SHAPE, L) if solver == "yee" else DT
    ops = [dict(waves=ONE_PLAIN, species=0, envelope=ENVELOPE, epoch=ENVELOPE_EPOCH),
           dict(waves=FOUR_WAVES, species=0, taper=TAPER_SMOOTH, **WINDOW),
           dict(waves=accel(FOUR_WAVES[:2]), species=1, kind="accel", lo=(0.0, L[1] / 4, 0.0), hi=(L[0], 3 * L[1] / 4, L[2]))]
    a, b, c = (filled(fp, precision, n, solver=solver, dt=dt) for _ in range(3))
    for s in (a, b, c):
        s.precalc()
    assert [a.forceOn(**op) for op in ops] == [0, 1, 2]
    a.recordEnergy(1, 64)
    a.substeps(ENVELOPE_SUBSTEPS)
    rows, dropped = a.energyHistory()
    assert dropped == 0 and list(rows["substep"]) == list(range(1, ENVELOPE_SUBSTEPS + 1))
    sums = [dict(ref.ZERO, applications=0) for _ in ops]
    for k in range(1, ENVELOPE_SUBSTEPS + 1):
        b.substeps(1)
        c.substeps(1)
        pre = b.energy()["kinetic"][0]
        for op, total in zip(ops, sums):
            held = b.getParticles(species=op["species"]) if not 3 <= k <= 11 and op is ops[0] else None
            got = b.force(**op)
            if op is ops[0]:
                assert got["applications"] == (1 if 3 <= k <= 11 else 0), k
            if held is not None:                                              # an inactive sub-step: no application, no bit changed
                now = b.getParticles(species=op["species"])
                assert got == dict(applications=0, kicked=0, work_fixed=0, impulse_fixed=[0, 0, 0], work=0.0, impulse=[0.0, 0.0, 0.0])
                assert bits(now["velocity"], held["velocity"]) and bits(now["position"], held["position"])
            total["applications"] += got["applications"]
            total.update(ref.add_tallies(total, got))
        for op in (ops[1], ops[0], ops[2]):                                   # the third twin: the first two requests in the other order
            c.force(**op)
        post = b.energy()["kinetic"][0]
        # the row recorded after sub-step k holds the kinetic energy after the kicks of that sub-step (the same exact sum),
        # and that is not the energy before them
        assert rows["kinetic"][k - 1][0] == post and abs(post - pre) > 1e-9 * pre, k
    for species in (0, 1):
        pa, pb = a.getParticles(species=species), b.getParticles(species=species)
        assert bits(pa["velocity"], pb["velocity"]) and bits(pa["position"], pb["position"]), species
    pc = c.getParticles()
    assert not bits(a.getParticles()["velocity"], pc["velocity"])             # registration order is the order of application
    assert np.abs(a.getParticles()["velocity"].astype(np.float64) - pc["velocity"].astype(np.float64)).max() < 1e-5
    for i, (op, total) in enumerate(zip(ops, sums)):
        got = a.forceStats(i)
        d = ref.derived(total, SPECIES[op["species"]]["mass"], W)
        assert got == dict(total, work=d["work"], impulse=d["impulse"]), (i, got, total)
        assert a.forceStats(i, "local") == got
    assert [s["applications"] for s in sums] == [9, ENVELOPE_SUBSTEPS, ENVELOPE_SUBSTEPS] and sums[0]["kicked"] == 9 * n
    # cleared: the handle runs on like one that never registered
    a.clearForces()
    with pytest.raises(fp.FusionPicError, match=r"\.index <- "):
        a.forceStats(0)
    a.substeps(2)
    b.substeps(2)
    pa, pb = a.getParticles(), b.getParticles()
    assert bits(pa["velocity"], pb["velocity"]) and bits(pa["position"], pb["position"])
    # a new registration starts from zero
    assert a.forceOn(waves=ONE_PLAIN) == 0
    a.substeps(1)
    got = a.forceStats(0)
    assert got["applications"] == 1 and got["kicked"] == n and got["work_fixed"] != 0
    for s in (a, b, c):
        s.destroy()


# ---- 5. equivalence with a field in the push
def test_a_registered_uniform_field_equals_the_field_in_the_push(fp):
    """FPIC_SOLVER_NONE, no B, fp64, N = 8 sub-steps.  Handle A is pushed in an uploaded uniform E0; handle B has no field,
    is kicked once and then runs with the same field registered: its kick after sub-step j is the two half-kicks of A's
    sub-step j + 1, so the positions agree and v_B less one kick K = kq E0 agrees with v_A.

    The bound, per component, with u = 2^-53 (u |x| < spacing(x)) and V = max |v0| + (N + 1) |K|, the largest |v| of the run.
    A, per sub-step: the gather is eight fused multiply-adds of weights that add up to exactly 1 (8 half-ulps of E0: 8 u
    relative), hc = ((q dt) / (2 m)) / c is three roundings, hc Ex one: 12 u of the half-kick on either half, 12 u |K| per
    sub-step; the two additions to v round by half a spacing(V) each.  B, per kick: kq = (q dt) / (m c) three roundings,
    d = scale e one (4 u |K|), the addition half a spacing(V); N + 1 kicks, the test's subtraction of K one more rounding and
    K itself counted once more.  Together |v_B - K - v_A| <= (16 N + 8) spacing(|K|) + (3 N / 2 + 1) spacing(V).
    Positions: x' = wrap01(fma(dx, v', x)) rounds by at most 2^-53 in the fma and 2^-53 in the wrap on either side, and the
    velocities differ by at most the bound above: |x_B - x_A| <= N (2 2^-52 + dx bound_v), taken around the periodic box."""
    n, N = N_SMALL, 8
    E0 = np.array([3.0e5, -1.0e5, 2.0e5])
    frac, vel = scene(n)
    a = fp.makeCylindricalParticlePusher(spec_of(n), precision="fp64")
    b = fp.makeCylindricalParticlePusher(spec_of(n), precision="fp64")
    for s, field in ((a, E0), (b, np.zeros(3))):
        s.set(position=frac * np.array(L), velocity=vel, E=np.broadcast_to(field, SHAPE + (3,)).copy())
        s.precalc()
    wave = [dict(amp=tuple(E0))]
    assert b.force(waves=wave)["kicked"] == n and b.forceOn(waves=wave) == 0
    a.substeps(N)
    b.substeps(N)
    pa, pb = a.getParticles(), b.getParticles()
    K = np.float64(request_of(0, wave)["kq"]) * E0
    V = np.abs(vel).max(axis=0) + (N + 1) * np.abs(K)
    bound_v = (16 * N + 8) * spacing(np.abs(K)) + (1.5 * N + 1) * spacing(V)
    dv = np.abs((pb["velocity"] - K[None, :]) - pa["velocity"])
    dx = DT * ref.C / np.array(L)
    bound_x = N * (2 * 2.0 ** -52 + dx * bound_v)
    d = np.abs(pb["position"] - pa["position"])
    d = np.minimum(d, 1.0 - d)
    print("equivalence: largest |dv| / bound %.3f, |dx| / bound %.3f; the run moved v by %.3g" % ((dv / bound_v).max(), (d / bound_x).max(), np.abs(N * K).max()))
    assert np.all(dv <= bound_v[None, :]) and np.all(d <= bound_x[None, :])
    assert np.abs(pa["velocity"] - vel).max() > 1e-3                         # (the field did move the particles)
    assert b.forceStats(0)["applications"] == N
    a.destroy()
    b.destroy()


# ---- 6. a decomposition holds the same particles
DSHAPE = (8, 8, 24)                                                          # (three slabs of a full-EM box need 2 (G + 2) <= nz / 3 planes)
DL = (2.0 ** -7, 2.0 ** -7, 3 * 2.0 ** -7)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_decomposition_holds_the_same_particles(fp, precision, solver, world):
    n = 20011
    dt = em_dt(DSHAPE, DL) if solver == "yee" else DT
    population = dict(seed=0xABCDEF, stream=6, drift=(0.0, 0.0, 0.1), vth=0.03)
    op = dict(waves=FOUR_WAVES[:2], lo=(DL[0] / 4, 0.0, DL[2] / 8), hi=(3 * DL[0] / 4, DL[1], 7 * DL[2] / 8), taper=TAPER_SMOOTH,
              envelope=dict(start=2, stop=7, values=[0.5, 1.0, 0.25]))
    make = lambda: fp.makeCylindricalParticlePusher(spec_of(n, solver=solver, dt=dt, shape=DSHAPE, lengths=DL, macro_weight=1e3), precision=precision)
    one = make()
    assert one.load(**population) == n
    sims = []
    for r in range(world):
        s = make()
        s.domainInit(r, world, ghost_planes=2, migrate_every=2, distributed_solve=0)
        sims.append(s)
    g = fp.BoxGroup(sims)
    assert sum(g.load(count=n, **population)) == n
    one.precalc()
    g.precalc()
    first = (one.force(**dict(op, envelope=None)), g.force(**dict(op, envelope=None)))
    assert first[0] == first[1] and 0 < first[0]["kicked"] < n
    assert one.forceOn(**op) == g.forceOn(**op) == 0
    one.step(4)
    g.step(4)
    stats = [m.domainStats() for m in g.sims]
    assert sum(s["migrated"] for s in stats) > 0 and sum(s["lost"] for s in stats) == 0
    want = one.getParticles()
    parts = [m.domainGet() for m in g.sims]
    ids = np.concatenate([p["ids"] for p in parts])
    order = np.argsort(ids, kind="stable")
    assert np.array_equal(ids[order], np.arange(n))
    for key in ("position", "velocity"):
        assert bits(np.concatenate([p[key] for p in parts])[order], want[key]), key
    whole, summed = one.forceStats(0), g.forceStats(0)
    assert whole == summed and whole["applications"] == 6 and 0 < whole["kicked"] < 6 * n, (whole, summed)
    assert len({m.forceStats(0, "local")["kicked"] for m in g.sims}) > 1
    g.clearForces()
    one.destroy()
    for m in g.sims:
        m.destroy()


# ---- 7. refusals; the next valid call succeeds
def test_refusals(fp):
    from helpers import make_spec
    rz = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    for call in (lambda: rz.force(waves=ONE_PLAIN), lambda: rz.forceOn(waves=ONE_PLAIN), lambda: rz.forceStats(0), rz.clearForces):
        with pytest.raises(fp.FusionPicError, match="needs a CART3D handle") as e:
            call()
        assert e.value.code == -5
    rz.destroy()
    sim = filled(fp, "fp32", 1000)
    nan, inf = float("nan"), float("inf")
    w = lambda **kw: [dict(dict(amp=1.0), **kw)]
    table = [1.0, 2.0]
    cases = [
        (dict(waves=w(), kind=2), ".kind <- must be 0 (field) or 1 (accel)"), (dict(waves=w(), kind=-1), ".kind <- must be 0"),
        (dict(waves=w(), species=2), ".species <- no such species"), (dict(waves=w(), species=-1), ".species <- no such species"),
        (dict(waves=[]), ".nwaves <- must be 1 .. FPIC_FORCE_MAX_WAVES (4)"), (dict(waves=w() * 5), ".nwaves <- must be 1 .. FPIC_FORCE_MAX_WAVES (4)"),
        (dict(waves=w(amp=(0, nan, 0))), ".amp <- must be finite"), (dict(waves=w(amp=inf)), ".amp <- must be finite"), (dict(waves=w() + w(amp=-inf)), ".amp <- must be finite"),
        (dict(waves=w(nu=nan)), ".nu <- must be finite"), (dict(waves=w(frequency=inf)), ".nu <- must be finite"), (dict(waves=w(phase=inf)), ".phase <- must be finite"),
        (dict(waves=w(), lo=(0, nan, 0)), ".lo, .hi <- must be finite"), (dict(waves=w(), hi=inf), ".lo, .hi <- must be finite"),
        (dict(waves=w(), lo=(-1e-9, 0, 0)), ".lo, .hi <- the window must lie within 0 <= lo < hi <= L"),
        (dict(waves=w(), hi=(L[0], L[1], L[2] * 1.001)), ".lo, .hi <- the window must lie within"), (dict(waves=w(), lo=L[0] / 2, hi=L[0] / 2), ".lo, .hi <- the window must lie within"),
        (dict(waves=w(), lo=L[0] / 2, hi=L[0] / 4), ".lo, .hi <- the window must lie within"),
        (dict(waves=w(mode=(0, 32769, 0))), ".mode <- components must lie within +-2^15"), (dict(waves=w(mode=(-32769, 0, 0))), ".mode <- components must lie within +-2^15"),
        (dict(waves=w(), taper=(None, [1.0], None)), ".taper_n <- a table has 2 .. FPIC_FORCE_TABLE_MAX nodes"), (dict(waves=w(), taper=(np.ones(1026), None, None)), ".taper_n <- a table has 2 .."),
        (dict(waves=w(), envelope=dict(start=0, stop=9, values=[1.0])), ".envelope_n <- a table has 2 .."), (dict(waves=w(), envelope=dict(start=0, stop=9, values=np.ones(1026))), ".envelope_n <- a table has 2 .."),
        (dict(waves=w(), taper=(None, None, [1.0, nan])), ".taper <- the nodes must be finite"), (dict(waves=w(), envelope=dict(start=0, stop=9, values=[inf, 1.0])), ".envelope <- the nodes must be finite"),
        (dict(waves=w(), envelope=dict(start=5, stop=4)), ".start <- must not lie after stop"),
        (dict(waves=w(), envelope=dict(start=4, stop=4, values=table)), ".stop <- an envelope table needs start < stop < FPIC_FORCE_FOREVER"),
        (dict(waves=w(), envelope=dict(start=4, values=table)), ".stop <- an envelope table needs start < stop < FPIC_FORCE_FOREVER"),
    ]
    before = [sim.getParticles(species=s) for s in (0, 1)]
    for kw, message in cases:
        for call in (lambda: sim.force(**kw), lambda: sim.forceOn(**kw)):
            with pytest.raises(fp.FusionPicError) as e:
                call()
            assert message in str(e.value) and e.value.code == -1, (kw, str(e.value))
    lib = sim._lib
    good = lambda: fp._force_spec(DT, list(L), waves=w())[0]
    assert lib.fpic_force(sim._h, None, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_force_register(sim._h, None, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_force_stats(sim._h, 0, 0, None) == -1 and b".out <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    for poke in (lambda s: s.reserved.__setitem__(2, 1.0), lambda s: setattr(s, "reserved_i32", 1), lambda s: setattr(s.wave[2], "reserved", 1)):
        s = good()
        poke(s)
        for rc in (lib.fpic_force(sim._h, s, None), lib.fpic_force_register(sim._h, s, None)):
            assert rc == -1 and b".reserved <- must be zero" in lib.fpic_last_error(sim._h)
    for counts in ((2, 0, 0, 0), (0, 0, 0, 2)):                              # a null table with a node count
        s = good()
        s.taper_n[0], s.envelope_n, s.stop = counts[0], counts[3], 9
        assert lib.fpic_force(sim._h, s, None) == -1 and b"null but its node count is not zero" in lib.fpic_last_error(sim._h)
    for index in (0, -1):
        with pytest.raises(fp.FusionPicError, match=r"\.index <- no such registered request"):
            sim.forceStats(index)
    for s in (0, 1):
        now = sim.getParticles(species=s)
        assert bits(now["velocity"], before[s]["velocity"]) and bits(now["position"], before[s]["position"])   # nothing refused has touched a particle
    assert [sim.forceOn(waves=w(amp=1e6 * k), species=k % 2) for k in range(fp.FORCE_MAX_OPS)] == list(range(fp.FORCE_MAX_OPS))
    with pytest.raises(fp.FusionPicError, match=r"\.spec <- FPIC_FORCE_MAX_OPS \(8\) requests are registered already"):
        sim.forceOn(waves=w())
    with pytest.raises(fp.FusionPicError, match=r"\.index <- no such registered request"):
        sim.forceStats(fp.FORCE_MAX_OPS)
    with pytest.raises(fp.FusionPicError, match=r"\.scope <- "):
        sim._check(lib.fpic_force_stats(sim._h, 0, 7, fp.ForceResult()))
    sim.precalc()
    sim.step(1)
    assert sim.forceStats(0)["applications"] == 2 and sim.forceStats(0)["kicked"] == 2000 and sim.forceStats(0)["work_fixed"] == 0   # (amp 0: kicked, stored, no work)
    assert sim.forceStats(7)["kicked"] == 2000 and sim.forceStats(7)["work_fixed"] != 0
    sim.clearForces()
    assert lib.fpic_force(sim._h, good(), None) == 0                           # `out` is optional
    assert sim.force(waves=w())["kicked"] == 1000 and sim.forceOn(waves=w()) == 0
    sim.destroy()


# ---- 8. the JavaScript host
def test_force_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    n = 4000
    spec = spec_of(n)
    population = dict(seed=123456789, stream=3, drift=[0.0, 0.01, 0.0], vth=0.02)
    tapers = [None, [0.5, 1.5], list(np.linspace(0.0, 1.0, 9) ** 2)]
    now = dict(waves=[dict(amp=[1.5e6, 0.0, -0.7e6], mode=[1, 0, -2], nu=0.013, phase=0.1), dict(amp=2.0e5, frequency=3.0e9)], kind="field",
               lo=[L[0] / 4, 0.0, 0.0], hi=[3 * L[0] / 4, L[1], L[2]], taper=tapers, epoch=5)
    on = dict(waves=[dict(amp=[0.0, 1.0e15, 0.0], mode=[0, 0, 3], nu=0.25)], kind="accel", envelope=dict(start=2, stop=4, values=[1.0, 0.5, 2.0]))
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, population=population, now=now, on=on)))
    script = r"""
const fs = require('fs');
const crypto = require('crypto');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.load(inp.population);
sim.precalc();
const plain = (r) => ({applications: r.applications, kicked: r.kicked, work_fixed: r.workFixed.toString(), impulse_fixed: r.impulseFixed.map((x) => x.toString()),
  work: r.work, impulse: Array.from(r.impulse)});
const first = plain(sim.force(inp.now));
const index = sim.forceOn(inp.on);
sim.step(2);
const stats = plain(sim.forceStats(index));
const local = plain(sim.forceStats(index, 'local'));
const r = sim.select({});
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const errors = [];
const one = {waves: [{amp: 1}]};
const tries = [() => sim.force({waves: [{amp: 1}], kind: 'gravity'}), () => sim.force({}), () => sim.force(7), () => sim.force({waves: []}),
  () => sim.force({waves: [{amp: [1, 2]}]}), () => sim.force({waves: [{amp: 1, nu: 1, frequency: 1}]}), () => sim.force({waves: [{amp: 1}], species: 3}),
  () => sim.force({waves: [{amp: 1}], epoch: -1}), () => sim.force({waves: [{amp: 1}], taper: [null, [1], null]}), () => sim.force({waves: [{amp: 1, mode: [1, 2]}]}),
  () => sim.force({waves: [{amp: 1}], envelope: {start: 5, stop: 4}}), () => sim.forceOn({waves: [{amp: 1}], lo: 1}), () => sim.forceStats(4), () => sim.forceStats(0.5)];
for (const t of tries) { try { t(); errors.push(null); } catch (err) { errors.push(String(err.message)); } }
sim.clearForces();
let cleared = null;
try { sim.forceStats(0); } catch (err) { cleared = String(err.message); }
console.log(JSON.stringify({first: first, index: index, stats: stats, local: local, ids: sha(r.ids), position: sha(r.position), velocity: sha(r.velocity), errors: errors, cleared: cleared}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    sim = fp.makeCylindricalParticlePusher(spec)
    sim.load(**population)
    sim.precalc()
    text = lambda r: dict(r, work_fixed=str(r["work_fixed"]), impulse_fixed=[str(x) for x in r["impulse_fixed"]])
    first = text(sim.force(**now))
    index = sim.forceOn(**on)
    sim.step(2)
    stats = text(sim.forceStats(index))
    want = sim.select()
    sim.destroy()
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    assert out["first"] == first and 0 < first["kicked"] < n and first["work_fixed"] != "0"
    assert out["index"] == index == 0 and out["stats"] == stats == out["local"] and stats["applications"] == 3 and stats["kicked"] == 3 * n
    assert (out["ids"], out["position"], out["velocity"]) == (sha(want["ids"]), sha(want["position"]), sha(want["velocity"]))
    assert all(err is not None and " <- " in err for err in out["errors"]), out["errors"]
    assert out["cleared"] is not None and ".index <- " in out["cleared"]
