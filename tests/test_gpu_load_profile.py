"""The profiled load (fpic_load_profile) on the GPU against the numpy restatement of its rule (tests/load_profile_reference.py,
proved on the CPU by tests/test_load_profile_reference.py and held to the header by tests/test_load_profile_host.py): the
exact parts bit for bit — positions without a displacement, velocities with vth = 0 and a shear table —, the rounded parts
within the bound tests/test_gpu_load.py uses for them (ULPS ulps of each normal and sine, carried through vth_eff and the
amplitudes; vth_eff and drift_eff are themselves exact parts), ranges and flags, a species whose order has changed, the
identity without tables, a decomposition whose ranks hold very different shares, neutrality, the histogram of a loaded
profile, the refusals, and the JavaScript host.

Met on an MI355X at 100003 particles with three density tables, three thermal tables and a shear table: largest |dv| / bound
0.388, |dp| / bound 0.499 (fp64); fp32: no stored value that is not bit-equal to the rounded reference."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import load_profile_reference as pref
import load_reference as ref
from helpers import ROOT
from test_gpu_histogram import DTYPE, MP, PRECISIONS, QE, box_spec, em_dt
from test_gpu_load import L, SHAPE, SUB, ULPS, bits

pytestmark = pytest.mark.gpu


def gaussian(nodes, sigma=0.2):
    x = np.linspace(0.0, 1.0, nodes)
    return np.exp(-0.5 * ((x - 0.5) / sigma) ** 2)


G1025 = gaussian(1025)
HOLES_MID_END = [1, 1, 0, 0, 0, 2, 0]
HOLES_ENDS = [0, 0, 1, 3, 0, 0]
WAVY = 1.0 + 0.5 * np.cos(np.linspace(0, 7, 1025))
SHEAR = dict(axis=1, component=2, values=[-0.02, 0.03, 0.01, -0.05])


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def box(fp, precision, n, solver="poisson_fft", shape=SHAPE, lengths=L):
    dt = em_dt(shape, lengths) if solver == "yee" else 5e-12
    spec = box_spec(shape, lengths, n, dt, solver=solver, macro_weight=1e15 * np.prod(lengths) / n)
    return fp.makeCylindricalParticlePusher(spec, precision=precision)


# ---- 1. the exact parts: no tolerance
EXACT = [   # (solver, density, thermal, shear, sub-box)
    ("poisson_fft", ([0.0, 1.0], None, None), None, dict(axis=0, component=0, values=[0.01, -0.01]), SUB),
    ("yee", (None, [2.0, 0.5, 3.0], G1025), (None, [1.0, 2.0], None), SHEAR, SUB),
    ("none", (HOLES_ENDS, HOLES_MID_END, G1025), ([0.5, 0.0, 4.0], WAVY, [2.0, 1.0]), dict(axis=2, component=1, values=np.sin(np.linspace(0, 9, 1025)) * 0.1), SUB),
    ("none", (None, None, [1e-300, 1, 1e-300]), None, None, {}),
]


@pytest.mark.parametrize("case", range(len(EXACT)))
@pytest.mark.parametrize("lattice", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_parts_bit_for_bit(fp, precision, lattice, case):
    T = DTYPE[precision]
    solver, density, thermal, shear, sub = EXACT[case]
    kw = dict(seed=0xC0FFEE0123456789, stream=5, lattice=lattice, drift=(0.0, 0.001, -0.002), vth=0, density=density, thermal=thermal, shear=shear, **sub)
    req = pref.request(L, **kw)
    for n in (1, 3, 257, 40009):
        i = np.arange(n)
        sim = box(fp, precision, n, solver)
        assert sim.load(**kw) == n
        got = sim.getParticles()
        sim.destroy()
        want_p, want_v = pref.stored_positions(req, i, T), pref.stored_velocities(req, i, T)
        assert bits(got["position"], want_p), (n, int((got["position"] != want_p).any(axis=1).sum()))
        assert bits(got["velocity"], want_v), (n, int((got["velocity"] != want_v).any(axis=1).sum()))
        assert np.all(want_p >= T(0)) and np.all(want_p < T(1))
    _, j = pref.fractions(req, i)
    for a in range(3):
        if density[a] is not None:
            d = np.asarray(density[a], dtype=np.float64)
            assert np.all((d[:-1] + d[1:])[j[:, a]] > 0)                       # no particle in an interval without mass
    if shear is not None:
        assert np.unique(want_v[:, shear["component"]]).size > 1000          # (the shear is there)


# ---- 2. the rounded parts
def velocity_bound(req, i):
    """test_gpu_load.velocity_bound with vth_eff and drift_eff (exact parts, identical on both sides) for vth and drift"""
    n = ref.normals(req, i)
    _, theta, f = pref.base(req, i)
    s = ref.sinpi(2.0 * (theta + req["vphase"]))[:, None]
    vth, drift = pref.vth_eff(req, f), pref.drift_eff(req, f)
    th, wv = vth * n, req["vamp"] * s
    scale = np.maximum(np.maximum(np.abs(drift + th), np.abs(th)), np.maximum(np.abs(wv), np.abs(drift + th + wv)))
    return ULPS * (vth * np.spacing(np.abs(n)) + np.abs(req["vamp"]) * np.spacing(np.abs(s))) + 4 * np.spacing(scale)


def position_bound(req, i):
    p, theta, _ = pref.base(req, i)
    s = ref.sinpi(2.0 * (theta + req["xphase"]))[:, None]
    return ULPS * np.abs(req["xamp_f"]) * np.spacing(np.abs(s)) + 2 * np.spacing(np.maximum(np.abs(p), np.abs(req["xamp_f"] * s)))


ROUNDED = dict(seed=77, stream=2, drift=(0.01, 0.0, -0.02), vth=(0.05, 0.02, 0.1), mode=(2, 1, -3), xamp=(2e-5, 0.0, -1e-5), xphase=0.125,
               vamp=(1e-3, 2e-3, 0.0), vphase=0.3, density=(G1025, [2.0, 0.5, 3.0], HOLES_ENDS), thermal=([1.0, 2.0], WAVY, [0.5, 0.25, 4.0]), shear=SHEAR, **SUB)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rounded_parts_within_the_bound(fp, precision):
    T = DTYPE[precision]
    n = 100003
    i = np.arange(n)
    req = pref.request(L, **ROUNDED)
    sim = box(fp, precision, n)
    assert sim.load(**ROUNDED) == n
    got = sim.getParticles()
    sim.destroy()
    want_p, want_v = pref.stored_positions(req, i, np.float64), pref.velocities(req, i)
    assert np.all(want_p[:, (0, 2)] > 0.05) and np.all(want_p[:, (0, 2)] < 0.95)      # (the displaced components do not wrap in this scene)
    if precision == "fp64":
        dv, dp = np.abs(got["velocity"] - want_v), np.abs(got["position"] - want_p)
        print("fp64: largest |dv| / bound %.3f, |dp| / bound %.3f" % ((dv / velocity_bound(req, i)).max(), (dp / position_bound(req, i)).max()))
        assert np.all(dv <= velocity_bound(req, i))
        assert np.all(dp <= position_bound(req, i))
        assert bits(got["position"][:, 1], want_p[:, 1])                               # (y is not displaced: an exact part)
    else:
        for name, g, w in (("velocity", got["velocity"], want_v.astype(T)), ("position", got["position"], pref.stored_positions(req, i, T))):
            off = g != w
            print("fp32 %s: share not bit-equal %.2e" % (name, off.mean()))
            assert np.all(np.abs(g.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)).astype(np.float64)), name
            assert off.mean() <= 1e-4, name


# ---- 3. ranges and flags
PROFILE = dict(density=(HOLES_ENDS, None, G1025), thermal=(None, [1.0, 2.0], None), shear=SHEAR)


def close_v(got, req, i, T):
    want = pref.velocities(req, i)
    return np.all(np.abs(got.astype(np.float64) - want) <= velocity_bound(req, i) + np.spacing(np.abs(want).astype(T)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ranges_and_flags(fp, precision):
    T = DTYPE[precision]
    n = 4099
    rng = np.random.default_rng(8)
    sim = box(fp, precision, n)
    sim.set(position=rng.random((n, 3)) * L, velocity=rng.normal(0, 0.01, (n, 3)))
    before = sim.getParticles()
    kw = dict(seed=4, stream=9, vth=0.03, drift=(0.0, 0.01, 0.0), **SUB, **PROFILE)
    req = pref.request(L, **kw)
    assert sim.load(first=3, count=1026, **kw) == 1026 and sim.load(first=2049, **kw) == n - 2049      # first no multiple of 4; tails of 1 and 2 slots
    got = sim.getParticles()
    loaded = np.zeros(n, dtype=bool)
    loaded[3:3 + 1026] = True
    loaded[2049:] = True
    i = np.arange(n)[loaded]
    assert bits(got["position"][loaded], pref.stored_positions(req, i, T)) and close_v(got["velocity"][loaded], req, i, T)
    for k in ("position", "velocity"):
        assert bits(got[k][~loaded], before[k][~loaded]), k                       # every other particle keeps its bits
        assert np.all((got[k][loaded] != before[k][loaded]).any(axis=1)), k
    # one array only; the other keeps its bits everywhere.  The velocity alone still reads the tables at the position the
    # request would give
    other = dict(kw, seed=5)
    oreq = pref.request(L, **other)
    sim.load(first=1, count=7, position=False, **other)
    now = sim.getParticles()
    assert bits(now["position"], got["position"]) and close_v(now["velocity"][1:8], oreq, np.arange(1, 8), T)
    assert np.all(now["velocity"][1:8] != got["velocity"][1:8]) and bits(now["velocity"][8:], got["velocity"][8:]) and bits(now["velocity"][:1], got["velocity"][:1])
    cold = dict(other, vth=0)
    sim.load(first=1, count=7, position=False, **cold)
    assert bits(sim.getParticles()["velocity"][1:8], pref.stored_velocities(pref.request(L, **cold), np.arange(1, 8), T))
    now = sim.getParticles()
    sim.load(first=4090, velocity=False, **other)
    last = sim.getParticles()
    assert bits(last["velocity"], now["velocity"]) and bits(last["position"][4090:], pref.stored_positions(oreq, np.arange(4090, n), T))
    assert bits(last["position"][:4090], now["position"][:4090])
    # pairs on a density profile: exact negatives with zero drift
    sim.load(seed=6, vth=(0.05, 0.02, 0.1), paired=True, density=PROFILE["density"])
    v = sim.getParticles()["velocity"]
    assert np.all(v[0:n - 1:2] + v[1:n:2] == 0) and np.all(v[0:n - 1:2] != 0)
    sim.destroy()


# ---- 4. after the order has changed
@pytest.mark.parametrize("precision", PRECISIONS)
def test_after_a_rebinning_has_permuted_the_slots(fp, precision, monkeypatch):
    monkeypatch.setenv("FPIC_TWO_LEVEL_MIN", "1")
    T = DTYPE[precision]
    n = 20011
    rng = np.random.default_rng(12)
    sim = box(fp, precision, n)
    sim.set(position=rng.random((n, 3)) * L, velocity=rng.normal(0, 0.02, (n, 3)))
    sim.precalc()
    sim.substeps(9)
    sim.sort()
    stepped = sim.getParticles()
    kw = dict(seed=21, stream=1, vth=0.02, lattice=True, **PROFILE)
    req = pref.request(L, **kw)
    first, count = 1001, 9002
    assert sim.load(first=first, count=count, **kw) == count
    got = sim.getParticles()
    inside = np.zeros(n, dtype=bool)
    inside[first:first + count] = True
    i = np.arange(n)[inside]
    assert bits(got["position"][inside], pref.stored_positions(req, i, T)) and close_v(got["velocity"][inside], req, i, T)
    for k in ("position", "velocity"):
        assert bits(got[k][~inside], stepped[k][~inside]), k
    sim.precalc()          # (the loaded state runs on)
    sim.step()
    sim.destroy()


# ---- 5. without a table the call is fpic_load, bit for bit
@pytest.mark.parametrize("precision", PRECISIONS)
def test_without_tables_it_is_the_plain_load(fp, precision):
    n = 40009
    kw = dict(seed=77, stream=2, drift=(0.01, 0.0, -0.02), vth=(0.05, 0.02, 0.1), mode=(2, 1, -3), xamp=(2e-5, 0.0, -1e-5), xphase=0.125, vamp=(1e-3, 2e-3, 0.0),
              vphase=0.3, paired=True, **SUB)
    sim = box(fp, precision, n)
    assert sim.load(**kw) == n
    plain = sim.getParticles()

    def same():
        now = sim.getParticles()
        return bits(now["position"], plain["position"]) and bits(now["velocity"], plain["velocity"])

    sim.load(seed=1)
    assert not same()
    assert sim.load(density=[None] * 3, **kw) == n and same()
    sim.load(seed=1)
    assert sim.load(density=[None] * 3, thermal=(None, None, None), **kw) == n and same()
    for profile in (ctypes.byref(fp.LoadProfile()), None):                       # all zero; a null pointer
        sim.load(seed=1)
        loaded = ctypes.c_uint64()
        assert sim._lib.fpic_load_profile(sim._h, ctypes.byref(fp._load_spec(L, **kw)), profile, ctypes.byref(loaded)) == 0 and loaded.value == n and same()
    sim.destroy()


# ---- 6. a decomposition gets the same particles, however unevenly the profile shares them out
def members(fp, world, precision, capacity, shape, lengths):
    sims = []
    for r in range(world):
        s = box(fp, precision, capacity[r] if isinstance(capacity, (list, tuple)) else capacity, shape=shape, lengths=lengths)
        s.domainInit(r, world, ghost_planes=2, migrate_every=2, distributed_solve=0)
        sims.append(s)
    return sims


# world 2: the upper half of z is massless, rank 1 keeps nothing; world 3 (12 planes): the middle third is
WORLDS = {2: (SHAPE, L, [1.0, 2.0, 0.0, 0.0, 0.0], 1), 3: ((16, 16, 12), (0.016, 0.016, 0.012), [1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 3.0], 1)}


def group_request(world):
    return dict(seed=0xABCDEF, stream=6, drift=(0.0, 0.0, 0.01), vth=0.03, mode=(1, 0, 1), xamp=(0.07 * L[0], 0.0, 0.0), xphase=0.25,
                density=(G1025, None, WORLDS[world][2]), thermal=(None, None, [1.0, 2.0]), shear=SHEAR)


@pytest.mark.parametrize("world,precision", [(2, "fp32"), (3, "fp64")])
def test_a_decomposition_holds_the_same_particles(fp, world, precision):
    T = DTYPE[precision]
    shape, lengths, _, empty = WORLDS[world]
    request = group_request(world)
    n, nzl = 40009, shape[2] // world
    one = box(fp, precision, n, shape=shape, lengths=lengths)
    assert one.load(**request) == n
    want = one.getParticles()
    want_plane = ref.plane(want["position"][:, 2], shape[2])
    req, i = pref.request(lengths, **request), np.arange(n)
    assert bits(want["position"][:, 1:], pref.stored_positions(req, i, T)[:, 1:])      # (x is displaced: a rounded part)
    g = fp.BoxGroup(members(fp, world, precision, n, shape, lengths))
    counts = g.load(count=n, **request)
    parts = [m.domainGet() for m in g.sims]
    assert counts == [len(p["ids"]) for p in parts] and sum(counts) == n
    assert counts[empty] == 0 and min(c for r, c in enumerate(counts) if r != empty) > 1000 and len(set(counts)) == world
    for r, p in enumerate(parts):
        assert np.all(np.diff(p["ids"].astype(np.int64)) > 0)                                        # ascending: the slot order is the id order
        assert np.array_equal(np.sort(np.flatnonzero(want_plane // nzl == r)), p["ids"])                 # exactly the particles of its planes
        assert bits(p["position"], want["position"][p["ids"]]) and bits(p["velocity"], want["velocity"][p["ids"]])
    # two ranges appended equal the single range
    h = fp.BoxGroup(members(fp, world, precision, n, shape, lengths))
    cut = 7777
    a, b = h.load(count=cut, **request), h.load(first=cut, count=n - cut, append=True, **request)
    assert [x + y for x, y in zip(a, b)] == counts
    for m, p in zip(h.sims, parts):
        q = m.domainGet()
        assert np.array_equal(q["ids"], p["ids"]) and bits(q["position"], p["position"]) and bits(q["velocity"], p["velocity"])
        m.destroy()
    one.destroy()
    for m in g.sims:
        m.destroy()


def test_a_member_one_short_of_capacity_changes_nothing(fp):
    n, world = 40009, 2
    shape, lengths, _, _ = WORLDS[world]
    request = group_request(world)
    g = fp.BoxGroup(members(fp, world, "fp32", n, shape, lengths))
    counts = g.load(count=n, **request)
    for m in g.sims:
        m.destroy()
    assert counts == [n, 0]
    tight = fp.BoxGroup(members(fp, world, "fp32", [n - 1, 16], shape, lengths))
    small = tight.sims[0].load(count=500, **request)
    held = tight.sims[0].domainGet()
    assert small == len(held["ids"]) == 500
    with pytest.raises(fp.FusionPicError) as e:
        tight.sims[0].load(count=n, **request)
    assert e.value.code == -1 and str(n) in str(e.value) and str(n - 1) in str(e.value) and ".count <- " in str(e.value)
    with pytest.raises(fp.FusionPicError) as e:
        tight.sims[0].load(first=500, count=n - 500, append=True, **request)
    assert e.value.code == -1
    now = tight.sims[0].domainGet()
    assert np.array_equal(now["ids"], held["ids"]) and bits(now["position"], held["position"]) and bits(now["velocity"], held["velocity"])
    assert tight.sims[0].load(count=n - 1, **request) == n - 1 and tight.sims[1].load(count=n, **request) == 0      # exactly full; the empty rank
    for m in tight.sims:
        m.destroy()


# ---- 7. one seed and stream, opposite charges, a density profile: the box is exactly neutral
@pytest.mark.parametrize("precision", PRECISIONS)
def test_same_stream_opposite_charge_is_neutral(fp, precision):
    n = 40009
    sim = box(fp, precision, n)
    ions = sim.addSpecies(MP, -QE, n)
    kw = dict(seed=31, vth=0.01, mode=(1, 0, 0), xamp=(1e-4, 0, 0), density=(G1025, HOLES_ENDS, [0.0, 1.0]), thermal=([1.0, 2.0], None, None))
    sim.load(stream=3, **kw)
    sim.load(species=ions, stream=3, **dict(kw, thermal=None, vth=1e-4))
    sim.precalc()
    rho = sim.readField(fp.F3_RHO_FIXED)
    assert rho.dtype == np.int64 and rho.size == 16 ** 3 and not rho.any()
    e, p = sim.getParticles(), sim.getParticles(species=ions)
    assert bits(e["position"], p["position"])
    sim.load(species=ions, stream=4, **kw)
    sim.precalc()
    assert sim.readField(fp.F3_RHO_FIXED).any()
    sim.destroy()


# ---- 8. the histogram of a loaded profile is the reference's interval counts
@pytest.mark.parametrize("lattice", [False, True])
def test_histogram_equals_the_interval_counts(fp, lattice):
    n, K = 100003, 1024
    kw = dict(seed=0xFEED, stream=1, lattice=lattice, density=(G1025, None, None))
    sim = box(fp, "fp64", n)
    assert sim.load(**kw) == n
    h = sim.histogram("x", K, (0.0, 1.0))
    sim.destroy()
    _, j = pref.fractions(pref.request(L, **kw), np.arange(n))
    want = np.bincount(j[:, 0], minlength=K)
    assert h["outside"] == 0 and np.array_equal(h["counts"].astype(np.int64), want)
    expect = n * np.diff(pref.cumulative(G1025)) / pref.cumulative(G1025)[-1]
    assert (np.abs(want - expect).max() <= 12.25) == lattice                      # (a quiet start, or not: tests/test_load_profile_reference.py)


# ---- 9. refusals; the next valid call succeeds
def test_refusals(fp):
    from helpers import make_spec
    rz = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    with pytest.raises(fp.FusionPicError, match="needs a CART3D handle") as e:
        rz.load(vth=0.01, density=([1.0, 2.0], None, None))
    assert e.value.code == -5
    rz.destroy()
    sim = box(fp, "fp32", 1000)
    sim.load(seed=9, vth=0.01)
    before = sim.getParticles()
    ok2 = [1.0, 2.0]
    for kw, prop in ((dict(density=([1.0], None, None)), ".density_n"), (dict(density=(None, np.ones(1026), None)), ".density_n"), (dict(thermal=(None, None, [1.0])), ".thermal_n"),
                     (dict(thermal=(np.ones(1026), None, None)), ".thermal_n"), (dict(shear=dict(axis=0, component=0, values=[0.1])), ".shear_n"),
                     (dict(shear=dict(axis=0, component=0, values=np.zeros(1026))), ".shear_n"),
                     (dict(density=(None, [1.0, float("nan")], None)), ".density"), (dict(density=(None, [1.0, float("inf")], None)), ".density"),
                     (dict(density=([1.0, -1e-9, 1.0], None, None)), ".density"), (dict(density=(None, None, [0.0, 0.0, 0.0])), ".density"),
                     (dict(thermal=([1.0, float("nan")], None, None)), ".thermal"), (dict(thermal=(None, [-1.0, 1.0], None)), ".thermal"),
                     (dict(shear=dict(axis=0, component=0, values=[0.0, float("inf")])), ".shear"),
                     (dict(shear=dict(axis=3, component=0, values=ok2)), ".shear_axis"), (dict(shear=dict(axis=-1, component=0, values=ok2)), ".shear_axis"),
                     (dict(shear=dict(axis=0, component=3, values=ok2)), ".shear_component"), (dict(shear=dict(axis=0, component=-1, values=ok2)), ".shear_component"),
                     (dict(density=(ok2, None, None), vth=-0.1), ".vth"), (dict(density=(ok2, None, None), first=1001), ".first")):
        with pytest.raises(fp.FusionPicError) as e:
            sim.load(**kw)
        assert prop + " <- " in str(e.value) and e.value.code == -1, (kw, str(e.value))
    table = (ctypes.c_double * 2)(1.0, 2.0)

    def direct(change):
        p = fp.LoadProfile()
        change(p)
        return sim._lib.fpic_load_profile(sim._h, ctypes.byref(fp._load_spec(L, vth=0.01)), ctypes.byref(p), None), sim._lib.fpic_last_error(sim._h)

    def reserved(p):
        p.reserved[1] = 1

    def null_density(p):
        p.density_n[0] = 2

    def null_thermal(p):
        p.thermal_n[2] = 2

    def null_shear(p):
        p.shear_n = 2

    for change, prop in ((reserved, b".reserved <- "), (null_density, b".density <- "), (null_thermal, b".thermal <- "), (null_shear, b".shear <- ")):
        rc, why = direct(change)
        assert rc == -1 and prop in why, (prop, why)
    assert sim._lib.fpic_load_profile(sim._h, None, None, None) == -1 and b"Non-optional property is undefined" in sim._lib.fpic_last_error(sim._h)
    now = sim.getParticles()
    assert bits(now["position"], before["position"]) and bits(now["velocity"], before["velocity"])      # a refused call changes nothing

    def good(p):
        p.density_n[0], p.density[0] = 2, ctypes.cast(table, ctypes.POINTER(ctypes.c_double))

    assert direct(good)[0] == 0                                                   # `loaded` is optional
    assert sim.load(vth=0.01, density=(ok2, None, None)) == 1000 and sim.load(first=1000, density=(ok2, None, None)) == 0
    sim.destroy()


# ---- 10. the JavaScript host
def test_load_profile_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    n = 4000
    spec = box_spec(SHAPE, L, n, 5e-12, macro_weight=1e15 * np.prod(L) / n)
    request = dict(seed=123456789, stream=3, lo=list(SUB["lo"]), hi=list(SUB["hi"]), drift=[0.0, 0.01, 0.0], vth=0.02, mode=[1, 0, 2], xamp=[1e-5, 0.0, 0.0],
                   xphase=0.25, vamp=1e-3, vphase=0.5, density=[G1025.tolist(), None, [0.0, 0.0, 1.0, 3.0, 0.0, 0.0]], thermal=[None, [1.0, 2.0], None],
                   shear=dict(axis=1, component=2, values=[-0.02, 0.03, 0.01, -0.05]))
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, request=request)))
    script = r"""
const fs = require('fs');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
const loaded = sim.load(inp.request);
const typed = sim.load(Object.assign({}, inp.request, {first: 10, count: 21, seed: 5, lattice: true, thermal: null, density: [null, new Float64Array([1, 0, 2]), null]}));
const hex = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('hex');
const r = sim.select({every: [40, 7]});
const errors = [];
for (const bad of [{density: [[1], null, null]}, {density: [null, null]}, {density: [[1, 'a'], null, null]}, {density: 5}, {thermal: [null, [1, -1], null]}, {thermal: [[1, 2], [1, 2]]},
                   {shear: {axis: 3, component: 0, values: [1, 2]}}, {shear: {axis: 0, component: 0.5, values: [1, 2]}}, {shear: {axis: 0, component: 0}}, {shear: [1, 2]},
                   {density: [[0, 0], null, null]}, {density: [[1, NaN], null, null]}, {density: [[1, 2], null, null], vth: -1}]) {
  try { sim.load(bad); errors.push(null); } catch (err) { errors.push(String(err.message)); }
}
console.log(JSON.stringify({loaded: loaded, typed: typed, ids: Array.from(r.ids), position: hex(r.position), velocity: hex(r.velocity), errors: errors}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    sim = fp.makeCylindricalParticlePusher(spec)
    assert sim.load(**request) == n == out["loaded"]
    assert sim.load(**dict(request, first=10, count=21, seed=5, lattice=True, thermal=None, density=[None, [1.0, 0.0, 2.0], None])) == 21 == out["typed"]
    want = sim.select(every=(40, 7))
    assert len(want["ids"]) == 100 and out["ids"] == want["ids"].tolist()
    assert out["position"] == want["position"].tobytes().hex() and out["velocity"] == want["velocity"].tobytes().hex()
    assert all(err is not None and " <- " in err for err in out["errors"]), out["errors"]
    sim.destroy()
