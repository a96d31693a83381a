"""The radial load (fpic_load_radial) on the GPU against the numpy restatement of its rule (tests/load_radial_reference.py,
proved on the CPU by tests/test_load_radial_reference.py and held to the header by tests/test_load_radial_host.py): the
exact parts bit for bit — the sphere's z and v_z, the cylinder's axial coordinate and axial velocity with vth = 0, every
coordinate where the angle's word is 0 —, the rounded parts within the bound tests/test_gpu_load.py uses (ULPS ulps of each
normal, cospi and sinpi, carried through rho r_max / L, vth_eff, the flow values and the phase), ranges and flags, a species
whose order has changed, neutrality, a decomposition one of whose ranks holds nothing, the wrap, the interval counts, the
refusals, and the JavaScript host.

Met on an MI355X at 100003 particles (fp64): a sphere with its three tables largest |dv| / bound 0.171, |dp| / bound 0.430; a
column with all five 0.165 and 0.420; fp32: no stored value that is not bit-equal to the rounded reference."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import load_profile_reference as pref
import load_radial_reference as rref
import load_reference as ref
from helpers import ROOT
from test_gpu_histogram import DTYPE, MP, PRECISIONS, QE, box_spec, em_dt
from test_gpu_load import L, SHAPE, ULPS, bits

pytestmark = pytest.mark.gpu

X65 = np.linspace(0.0, 1.0, 65)
G65 = np.exp(-0.5 * ((X65 - 0.5) / 0.15) ** 2)
G1025 = np.exp(-0.5 * ((np.linspace(0.0, 1.0, 1025) - 0.5) / 0.2) ** 2)
CORE_AND_SHELL = np.where(X65 < 0.3, 0.2, 0.0) + np.where((X65 >= 0.6) & (X65 <= 0.85), 1.0, 0.0)
HOLES_MID_END = [1, 1, 0, 0, 0, 2, 0]
HOLES_ENDS = [0, 0, 1, 3, 0, 0]
WAVY = 1.0 + 0.5 * np.cos(np.linspace(0, 7, 1025))
IMPLOSION = [0.0, -0.01, -0.03, -0.02]
MID = tuple(0.5 * l for l in L)
SIZES = (1, 3, 257, 40009)


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def box(fp, precision, n, solver="poisson_fft", shape=SHAPE, lengths=L):
    dt = em_dt(shape, lengths) if solver == "yee" else 5e-12
    spec = box_spec(shape, lengths, n, dt, solver=solver, macro_weight=1e15 * np.prod(lengths) / n)
    return fp.makeCylindricalParticlePusher(spec, precision=precision)


def sphere(center=MID, r_max=0.004, **tables):
    return dict(geometry="sphere", center=center, r_max=r_max, **tables)


def column(axis, center=MID, r_max=0.004, **tables):
    return dict(geometry="cylinder", axis=axis, center=center, r_max=r_max, **tables)


def reference(radial, lengths=L, **kw):
    return rref.request(lengths, **radial, **kw)


def exact_axis(radial):
    return 2 if radial["geometry"] == "sphere" else radial["axis"]


# ---- the bound of the rounded parts
def direction_error(req, pt):
    """what ULPS ulps of cospi and sinpi, and the one rounded product q cs (q sn) on either side, make of dir[n][3]"""
    f = pt["f"]
    e = np.zeros(f.shape)
    if req["geometry"] == "sphere":
        cs, sn = ref.cospi(2.0 * f[:, 2]), ref.sinpi(2.0 * f[:, 2])
        e[:, 0] = pt["q"] * ULPS * np.spacing(np.abs(cs)) + np.spacing(np.abs(pt["dir"][:, 0]))
        e[:, 1] = pt["q"] * ULPS * np.spacing(np.abs(sn)) + np.spacing(np.abs(pt["dir"][:, 1]))
    else:
        a = req["axis"]
        e[:, (a + 1) % 3] = ULPS * np.spacing(np.abs(pt["dir"][:, (a + 1) % 3]))
        e[:, (a + 2) % 3] = ULPS * np.spacing(np.abs(pt["dir"][:, (a + 2) % 3]))
    return e


def base_errors(req, i):
    """(|dp| allowed of the undisplaced position, |d theta| that follows from it, p, theta, parts)"""
    p, theta, pt = rref.base(req, i)
    off = (pt["rho"][:, None] * req["rl"]) * pt["dir"]
    dp = (pt["rho"][:, None] * req["rl"]) * direction_error(req, pt) + 2 * np.spacing(np.maximum(np.abs(p), np.abs(off)))    # the product and the sum, on either side
    if req["geometry"] == "cylinder":
        dp[:, req["axis"]] = 0.0                                                                                             # the plain rule's coordinate: exact
    dtheta = (np.abs(req["m"]) * dp).sum(axis=1) + 3 * np.spacing(np.abs(req["m"] * p).sum(axis=1))
    return dp, dtheta, p, theta, pt


def position_bound(req, i):
    dp, dtheta, p, theta, _ = base_errors(req, i)
    s = ref.sinpi(2.0 * (theta + req["xphase"]))[:, None]
    ds = ULPS * np.spacing(np.abs(s)) + 2 * np.pi * dtheta[:, None]
    return dp + np.abs(req["xamp_f"]) * ds + 2 * np.spacing(np.maximum(np.abs(p), np.abs(req["xamp_f"] * s)))


def velocity_bound(req, i):
    """test_gpu_load.velocity_bound with vth_eff for vth, the flows' share of the direction's error, the phase's share of the
    position's, and one rounding per operation of the sum (at most eight, on either side)"""
    n = ref.normals(req, i)
    _, dtheta, _, theta, pt = base_errors(req, i)
    de = direction_error(req, pt)
    look = lambda key: np.zeros(len(n)) if req[key] is None else np.abs(pref.lookup(req[key], pt["rho"])[0])
    u_r, u_t, u_a = look("flow_radial"), look("flow_azimuthal"), look("flow_axial")
    vth = np.broadcast_to(req["vth"], n.shape) * (1.0 if req["thermal"] is None else pref.lookup(req["thermal"], pt["rho"])[0][:, None])
    flow = u_r[:, None] * de
    if req["geometry"] == "cylinder":
        b, c = (req["axis"] + 1) % 3, (req["axis"] + 2) % 3
        flow[:, b] += u_t * de[:, c]
        flow[:, c] += u_t * de[:, b]
    s = ref.sinpi(2.0 * (theta + req["vphase"]))[:, None]
    ds = ULPS * np.spacing(np.abs(s)) + 2 * np.pi * dtheta[:, None]
    scale = np.abs(req["drift"]) + (u_r + u_t + u_a)[:, None] + np.abs(vth * n) + np.abs(req["vamp"] * s)
    return flow + ULPS * vth * np.spacing(np.abs(n)) + np.abs(req["vamp"]) * ds + 8 * np.spacing(scale)


def close_v(got, req, i, T):
    want = rref.velocities(req, i)
    return np.all(np.abs(got.astype(np.float64) - want) <= velocity_bound(req, i) + np.spacing(np.abs(want).astype(T)))


def close_p(got, req, i, T):
    """within the bound and one rounding to T - of the position as it is cast, and of 1 where it wraps (u - floor(u) is
    rounded at that size) -, the distance taken round the box: a value a last bit below 0 is stored a last bit below 1"""
    raw = rref.positions(req, i)
    d = np.abs(got.astype(np.float64) - ref.wrap01(raw.copy()))
    cast = np.spacing(np.maximum(np.abs(raw), np.where((raw < 0) | (raw >= 1), 1.0, 0.0)).astype(T)).astype(np.float64)
    return np.all(np.minimum(d, 1 - d) <= position_bound(req, i) + cast)


# ---- 1. the exact parts: no tolerance
EXACT = [   # (solver, the body, lo, hi of the request)
    ("poisson_fft", sphere(density=CORE_AND_SHELL, thermal=[1.0, 2.0], flow_radial=IMPLOSION), None, None),
    ("yee", sphere(center=(0.005, 0.011, 0.0045), r_max=0.0035, density=G1025, flow_radial=np.sin(np.linspace(0, 9, 1025)) * 0.1), None, None),
    ("none", sphere(r_max=0.008), None, None),
    ("yee", column(0, density=HOLES_ENDS, thermal=WAVY, flow_radial=IMPLOSION, flow_azimuthal=[0.0, 0.02], flow_axial=[0.03, 0.0, -0.03]), (0.002, 0, 0), (0.014, L[1], L[2])),
    ("none", column(1, center=(0.009, 0.0, 0.0035), r_max=0.003, density=HOLES_MID_END, flow_axial=G1025 * 0.2), None, None),
    ("poisson_fft", column(2, r_max=0.008, density=[1e-300, 1, 1e-300], flow_azimuthal=WAVY * 0.01, flow_axial=[0.0, 0.0, 0.04]), (0, 0, 0.004), (L[0], L[1], 0.012)),
]


@pytest.mark.parametrize("case", range(len(EXACT)))
@pytest.mark.parametrize("lattice", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_parts_bit_for_bit(fp, precision, lattice, case):
    T = DTYPE[precision]
    solver, radial, lo, hi = EXACT[case]
    kw = dict(seed=0xC0FFEE0123456789, stream=5, lattice=lattice, drift=(0.0, 0.001, -0.002), vth=0, lo=lo, hi=hi)
    req = reference(radial, **kw)
    a = exact_axis(radial)
    for n in SIZES:
        i = np.arange(n)
        sim = box(fp, precision, n, solver)
        assert sim.load(radial=radial, **kw) == n
        got = sim.getParticles()
        sim.destroy()
        want_p, want_v = rref.stored_positions(req, i, T), rref.stored_velocities(req, i, T)
        assert bits(got["position"][:, a], want_p[:, a]), (n, int((got["position"][:, a] != want_p[:, a]).sum()))
        assert bits(got["velocity"][:, a], want_v[:, a]), (n, int((got["velocity"][:, a] != want_v[:, a]).sum()))
        assert close_p(got["position"], req, i, T) and close_v(got["velocity"], req, i, T)
        assert np.all(got["position"] >= T(0)) and np.all(got["position"] < T(1))
    assert np.unique(want_p[:, a]).size > 30000 and (radial.get("flow_radial") is None and radial.get("flow_axial") is None or np.unique(want_v[:, a]).size > 1000)


# ---- 2. the rounded parts
ROUNDED = dict(seed=77, stream=2, drift=(0.01, 0.0, -0.02), vth=(0.05, 0.02, 0.1), mode=(2, 1, -3), xamp=(2e-5, 0.0, -1e-5), xphase=0.125, vamp=(1e-3, 2e-3, 0.0), vphase=0.3)
BODIES = {   # (the body, the sub-box of the request)
    "sphere": (sphere(r_max=0.006, density=G1025, thermal=WAVY, flow_radial=IMPLOSION), {}),
    "column": (column(1, r_max=0.006, density=CORE_AND_SHELL, thermal=[1.0, 2.0], flow_radial=IMPLOSION, flow_azimuthal=[0.0, 0.05], flow_axial=G65 * 0.1),
               dict(lo=(0.0, 0.002, 0.0), hi=(L[0], 0.014, L[2]))),
}


@pytest.mark.parametrize("name", sorted(BODIES))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rounded_parts_within_the_bound(fp, precision, name):
    """Met on an MI355X at 100003 particles (fp64), largest |dv| / bound, |dp| / bound: sphere 0.171, 0.430; column 0.165,
    0.420.  fp32: every stored value bit-equal to the rounded reference."""
    T = DTYPE[precision]
    n = 100003
    i = np.arange(n)
    radial, sub = BODIES[name]
    req = reference(radial, **ROUNDED, **sub)
    sim = box(fp, precision, n)
    assert sim.load(radial=radial, **ROUNDED, **sub) == n
    got = sim.getParticles()
    sim.destroy()
    want_p, want_v = rref.stored_positions(req, i, np.float64), rref.velocities(req, i)
    assert np.all(want_p > 0.05) and np.all(want_p < 0.95)                              # (nothing wraps in this scene)
    if precision == "fp64":
        dv, dp = np.abs(got["velocity"] - want_v), np.abs(got["position"] - want_p)
        print("%s fp64: largest |dv| / bound %.3f, |dp| / bound %.3f" % (name, (dv / velocity_bound(req, i)).max(), (dp / position_bound(req, i)).max()))
        assert np.all(dv <= velocity_bound(req, i))
        assert np.all(dp <= position_bound(req, i))
    else:
        for what, g, w in (("velocity", got["velocity"], want_v.astype(T)), ("position", got["position"], rref.stored_positions(req, i, T))):
            off = g != w
            print("%s fp32 %s: share not bit-equal %.2e" % (name, what, off.mean()))
            assert np.all(np.abs(g.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)).astype(np.float64)), what
            assert off.mean() <= 1e-4, what


# ---- 3. ranges and flags
BODY = sphere(center=(0.007, 0.008, 0.009), r_max=0.005, density=CORE_AND_SHELL, thermal=[1.0, 2.0], flow_radial=IMPLOSION)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ranges_and_flags(fp, precision):
    T = DTYPE[precision]
    n = 4099
    rng = np.random.default_rng(8)
    sim = box(fp, precision, n)
    sim.set(position=rng.random((n, 3)) * L, velocity=rng.normal(0, 0.01, (n, 3)))
    before = sim.getParticles()
    kw = dict(seed=4, stream=9, vth=0.03, drift=(0.0, 0.01, 0.0))
    req = reference(BODY, **kw)
    assert sim.load(first=3, count=1026, radial=BODY, **kw) == 1026 and sim.load(first=2049, radial=BODY, **kw) == n - 2049      # first no multiple of 4; tails of 1 and 2 slots
    got = sim.getParticles()
    loaded = np.zeros(n, dtype=bool)
    loaded[3:3 + 1026] = True
    loaded[2049:] = True
    i = np.arange(n)[loaded]
    assert bits(got["position"][loaded][:, 2], rref.stored_positions(req, i, T)[:, 2]) and close_p(got["position"][loaded], req, i, T) and close_v(got["velocity"][loaded], req, i, T)
    for k in ("position", "velocity"):
        assert bits(got[k][~loaded], before[k][~loaded]), k                       # every other particle keeps its bits
        assert np.all((got[k][loaded] != before[k][loaded]).any(axis=1)), k
    # one array only; the other keeps its bits everywhere.  The velocity alone still reads the tables at the radius the
    # request would give
    other = dict(kw, seed=5)
    oreq = reference(BODY, **other)
    sim.load(first=1, count=7, position=False, radial=BODY, **other)
    now = sim.getParticles()
    assert bits(now["position"], got["position"]) and close_v(now["velocity"][1:8], oreq, np.arange(1, 8), T)
    assert np.all(now["velocity"][1:8] != got["velocity"][1:8]) and bits(now["velocity"][8:], got["velocity"][8:]) and bits(now["velocity"][:1], got["velocity"][:1])
    cold = dict(other, vth=0)
    sim.load(first=1, count=7, position=False, radial=BODY, **cold)
    assert bits(sim.getParticles()["velocity"][1:8, 2], rref.stored_velocities(reference(BODY, **cold), np.arange(1, 8), T)[:, 2])
    now = sim.getParticles()
    sim.load(first=4090, velocity=False, radial=BODY, **other)
    last = sim.getParticles()
    assert bits(last["velocity"], now["velocity"]) and bits(last["position"][4090:, 2], rref.stored_positions(oreq, np.arange(4090, n), T)[:, 2])
    assert close_p(last["position"][4090:], oreq, np.arange(4090, n), T) and bits(last["position"][:4090], now["position"][:4090])
    # pairs in a body without thermal and flow tables (those are read at each particle's own radius): exact negatives with zero drift
    sim.load(seed=6, vth=(0.05, 0.02, 0.1), paired=True, radial=sphere(density=CORE_AND_SHELL))
    v = sim.getParticles()["velocity"]
    assert np.all(v[0:n - 1:2] + v[1:n:2] == 0) and np.all(v[0:n - 1:2] != 0)
    sim.destroy()


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
    body = column(2, r_max=0.005, density=G65, thermal=[1.0, 2.0], flow_azimuthal=[0.0, 0.02])
    kw = dict(seed=21, stream=1, vth=0.02, lattice=True)
    req = reference(body, **kw)
    first, count = 1001, 9002
    assert sim.load(first=first, count=count, radial=body, **kw) == count
    got = sim.getParticles()
    inside = np.zeros(n, dtype=bool)
    inside[first:first + count] = True
    i = np.arange(n)[inside]
    assert bits(got["position"][inside][:, 2], rref.stored_positions(req, i, T)[:, 2]) and close_p(got["position"][inside], req, i, T) and close_v(got["velocity"][inside], req, i, T)
    for k in ("position", "velocity"):
        assert bits(got[k][~inside], stepped[k][~inside]), k
    sim.precalc()          # (the loaded state runs on)
    sim.step()
    sim.destroy()


# ---- 4. one seed and stream, opposite charges: the box is exactly neutral
@pytest.mark.parametrize("precision", PRECISIONS)
def test_same_stream_opposite_charge_is_neutral(fp, precision):
    n = 40009
    sim = box(fp, precision, n)
    ions = sim.addSpecies(MP, -QE, n)
    body = sphere(center=(0.002, 0.008, 0.015), r_max=0.005, density=CORE_AND_SHELL, thermal=[1.0, 2.0], flow_radial=IMPLOSION)       # (across two faces)
    kw = dict(seed=31, vth=0.01, mode=(1, 0, 0), xamp=(1e-4, 0, 0))
    sim.load(stream=3, radial=body, **kw)
    sim.load(species=ions, stream=3, radial=dict(body, thermal=None, flow_radial=None), **dict(kw, vth=1e-4))
    sim.precalc()
    rho = sim.readField(fp.F3_RHO_FIXED)
    assert rho.dtype == np.int64 and rho.size == 16 ** 3 and not rho.any()
    e, p = sim.getParticles(), sim.getParticles(species=ions)
    assert bits(e["position"], p["position"])
    sim.load(species=ions, stream=4, radial=body, **kw)
    sim.precalc()
    assert sim.readField(fp.F3_RHO_FIXED).any()
    sim.destroy()


# ---- 5. a decomposition gets the same particles; an off-centre sphere leaves one rank most of the body and one none
def members(fp, world, precision, capacity, shape, lengths):
    sims = []
    for r in range(world):
        s = box(fp, precision, capacity, shape=shape, lengths=lengths)
        s.domainInit(r, world, ghost_planes=2, migrate_every=2, distributed_solve=0)
        sims.append(s)
    return sims


# (shape, lengths, the sphere, the rank that holds nothing): world 2 - the ball lies in the lower half of z; world 3 (12
# planes, 4 per rank) - it spans z in [0.3, 6.1] mm of 12: most of it in rank 0, the rest in rank 1
WORLDS = {2: (SHAPE, L, sphere(center=(0.006, 0.009, 0.0042), r_max=0.0035, density=CORE_AND_SHELL, thermal=[1.0, 2.0], flow_radial=IMPLOSION), 1),
          3: ((16, 16, 12), (0.016, 0.016, 0.012), sphere(center=(0.006, 0.009, 0.0032), r_max=0.0029, density=G65, thermal=[1.0, 2.0], flow_radial=IMPLOSION), 2)}
GROUP = dict(seed=0xABCDEF, stream=6, drift=(0.0, 0.0, 0.01), vth=0.03, mode=(1, 1, 0), xamp=(0.05 * L[0], 0.0, 0.0), xphase=0.25)


def zero_word_index(req, axis):
    """the particle index whose lattice word on `axis` is 0: i mult + shift = 0 (mod 2^32), mult odd"""
    return (-req["shift"][axis] * pow(ref.MULT[axis], -1, 1 << 32)) % (1 << 32)


@pytest.mark.parametrize("world,precision", [(2, "fp32"), (3, "fp64")])
def test_a_decomposition_holds_the_same_particles(fp, world, precision):
    T = DTYPE[precision]
    shape, lengths, body, empty = WORLDS[world]
    n, nzl = 40009, shape[2] // world
    one = box(fp, precision, n, shape=shape, lengths=lengths)
    assert one.load(radial=body, **GROUP) == n
    want = one.getParticles()
    want_plane = ref.plane(want["position"][:, 2], shape[2])
    req, i = reference(body, lengths, **GROUP), np.arange(n)
    assert bits(want["position"][:, 2], rref.stored_positions(req, i, T)[:, 2]) and close_p(want["position"], req, i, T)
    g = fp.BoxGroup(members(fp, world, precision, n, shape, lengths))
    counts = g.load(count=n, radial=body, **GROUP)
    parts = [m.domainGet() for m in g.sims]
    assert counts == [len(p["ids"]) for p in parts] and sum(counts) == n
    assert counts[empty] == 0 and counts[0] > n // 2 and len(set(counts)) == world
    for r, p in enumerate(parts):
        assert np.all(np.diff(p["ids"].astype(np.int64)) > 0)                                        # ascending: the slot order is the id order
        assert np.array_equal(np.sort(np.flatnonzero(want_plane // nzl == r)), p["ids"])                 # exactly the particles of its planes
        assert bits(p["position"], want["position"][p["ids"]]) and bits(p["velocity"], want["velocity"][p["ids"]])
    # two ranges appended equal the single range
    cut = 7777
    a, b = g.load(count=cut, radial=body, **GROUP), g.load(first=cut, count=n - cut, append=True, radial=body, **GROUP)
    assert [x + y for x, y in zip(a, b)] == counts
    for m, p in zip(g.sims, parts):
        q = m.domainGet()
        assert np.array_equal(q["ids"], p["ids"]) and bits(q["position"], p["position"]) and bits(q["velocity"], p["velocity"])
    # where the angle's word is 0 its cosine and sine are exact, and so is every coordinate: a lattice load of the index
    # whose z word is 0 (a rank takes any 32-bit id) and of its two neighbours
    cold = dict(GROUP, lattice=True, vth=0, xamp=0)
    creq = reference(body, lengths, **cold)
    i0 = zero_word_index(creq, 2)
    first = min(max(i0 - 1, 0), (1 << 32) - 4)
    ids = np.arange(first, first + 3, dtype=np.uint64)
    assert ref.fractions(creq, ids)[int(i0 - first), 2] == 0
    assert sum(g.load(first=int(first), count=3, radial=body, **cold)) == 3
    held = [m.domainGet() for m in g.sims]
    got_ids = np.concatenate([h["ids"] for h in held]).astype(np.uint64)
    got_p, got_v = np.concatenate([h["position"] for h in held]), np.concatenate([h["velocity"] for h in held])
    order = np.argsort(got_ids)
    assert np.array_equal(got_ids[order], ids)
    k = int(i0 - first)
    assert bits(got_p[order][k], rref.stored_positions(creq, ids, T)[k]) and bits(got_v[order][k], rref.stored_velocities(creq, ids, T)[k])
    assert close_p(got_p[order], creq, ids, T)
    one.destroy()
    for m in g.sims:
        m.destroy()


# ---- 6. a body across the periodic boundary wraps
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_body_across_the_boundary_wraps(fp, precision):
    T = DTYPE[precision]
    n = 40009
    i = np.arange(n)
    sim = box(fp, precision, n)
    for radial in (sphere(center=(0.0, L[1], 0.0155), r_max=0.006, density=G65), column(0, center=(0.0, 0.0005, L[2]), r_max=0.006, flow_azimuthal=[0.0, 0.01])):
        kw = dict(seed=15, stream=2, vth=0.01, mode=(0, 1, 0), xamp=(0.0, 1e-4, 0.0))
        assert sim.load(radial=radial, **kw) == n
        p = sim.getParticles()["position"]
        assert p.dtype == T and np.all(p >= 0) and np.all(p < 1)
        for a in (1, 2):
            assert (p[:, a] < 0.3).sum() > 5000 and (p[:, a] > 0.7).sum() > 5000 and not ((p[:, a] > 0.45) & (p[:, a] < 0.55)).any()     # on both sides of the face
        req = reference(radial, **kw)
        a = exact_axis(radial)
        assert bits(p[:, a], rref.stored_positions(req, i, T)[:, a])                      # (y alone is displaced here)
        assert close_p(p, req, i, T)
    sim.destroy()


# ---- 7. the interval counts of a loaded body are the reference's
@pytest.mark.parametrize("lattice", [False, True])
@pytest.mark.parametrize("name", ["sphere", "column"])
def test_interval_counts_equal_the_references(fp, lattice, name):
    n, K = 40009, 64
    radial = sphere(center=(0.007, 0.008, 0.009), r_max=0.006, density=CORE_AND_SHELL) if name == "sphere" else column(1, center=(0.007, 0.008, 0.009), r_max=0.006, density=CORE_AND_SHELL)
    kw = dict(seed=0xFEED, stream=1, lattice=lattice)
    sim = box(fp, "fp64", n)
    assert sim.load(radial=radial, **kw) == n
    p = sim.getParticles()["position"]
    sim.destroy()
    req = reference(radial, **kw)
    x = (p - req["c_f"]) / req["rl"]
    if name == "column":
        x[:, 1] = 0.0
    rho = np.sqrt((x * x).sum(axis=1))
    pt = rref.parts(req, np.arange(n))
    assert np.abs(rho - pt["rho"]).max() <= 1e-13                                       # (a dozen roundings of 1.1e-16 of values of 1/2, over r_max / L = 3/8)
    got, want = np.bincount(np.minimum((rho * K).astype(np.int64), K - 1), minlength=K), np.bincount(pt["j"], minlength=K)
    assert np.array_equal(got, want) and not want[(CORE_AND_SHELL[:-1] + CORE_AND_SHELL[1:]) == 0].any()


# ---- 8. refusals; the next valid call succeeds
def test_refusals(fp):
    from helpers import make_spec
    rz = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    with pytest.raises(fp.FusionPicError, match="needs a CART3D handle") as e:
        rz.load(vth=0.01, radial=sphere())
    assert e.value.code == -5
    rz.destroy()
    sim = box(fp, "fp32", 1000)
    sim.load(seed=9, vth=0.01)
    before = sim.getParticles()
    ok2, nan, inf = [1.0, 2.0], float("nan"), float("inf")
    for radial, prop in ((dict(sphere(), geometry=0), ".geometry"), (dict(sphere(), geometry=3), ".geometry"), (column(3), ".axis"), (column(-1), ".axis"), (dict(sphere(), axis=1), ".axis"),
                         (sphere(r_max=0.0), ".r_max"), (sphere(r_max=-0.001), ".r_max"), (sphere(r_max=inf), ".r_max"), (sphere(r_max=nan), ".r_max"),
                         (sphere(r_max=0.0081), ".r_max"), (column(2, r_max=0.0081), ".r_max"),
                         (sphere(center=(-1e-9, 0.008, 0.008)), ".center"), (sphere(center=(0.008, 0.0161, 0.008)), ".center"), (column(2, center=(0.008, 0.008, nan)), ".center"),
                         (sphere(density=[1.0]), ".density_n"), (sphere(density=np.ones(1026)), ".density_n"), (sphere(thermal=[1.0]), ".thermal_n"), (sphere(thermal=np.ones(1026)), ".thermal_n"),
                         (sphere(flow_radial=[0.1]), ".radial_n"), (column(0, flow_azimuthal=np.zeros(1026)), ".azimuthal_n"), (column(0, flow_axial=[0.1]), ".axial_n"),
                         (sphere(density=[1.0, nan]), ".density"), (sphere(density=[1.0, inf]), ".density"), (sphere(density=[1.0, -1e-9, 1.0]), ".density"),
                         (sphere(density=[0.0, 0.0, 0.0]), ".density"), (column(1, density=[0.0, 0.0]), ".density"),
                         (sphere(thermal=[1.0, nan]), ".thermal"), (sphere(thermal=[-1.0, 1.0]), ".thermal"), (sphere(flow_radial=[0.0, inf]), ".radial"),
                         (column(0, flow_azimuthal=[nan, 0.0]), ".azimuthal"), (column(0, flow_axial=[0.0, -inf]), ".axial"),
                         (sphere(flow_azimuthal=ok2), ".azimuthal_n"), (sphere(flow_axial=ok2), ".azimuthal_n")):
        with pytest.raises(fp.FusionPicError) as e:
            sim.load(radial=radial, vth=0.01)
        assert prop + " <- " in str(e.value) and e.value.code == -1, (radial, str(e.value))
    for kw, prop in ((dict(vth=-0.1), ".vth"), (dict(first=1001), ".first")):           # what fpic_load refuses
        with pytest.raises(fp.FusionPicError) as e:
            sim.load(radial=sphere(), **kw)
        assert prop + " <- " in str(e.value) and e.value.code == -1
    assert sim.load(radial=column(2, r_max=0.008), lo=(0, 0, 0.004), hi=(L[0], L[1], 0.005)) == 1000     # (the column's own axis does not bound r_max)
    sim.load(seed=9, vth=0.01)
    for clash in (dict(density=(ok2, None, None)), dict(thermal=(None, ok2, None)), dict(shear=dict(axis=0, component=0, values=ok2))):
        with pytest.raises(ValueError):
            sim.load(radial=sphere(), **clash)
    table = (ctypes.c_double * 2)(1.0, 2.0)

    def direct(change):
        p = fp._load_radial(sphere())
        change(p)
        return sim._lib.fpic_load_radial(sim._h, ctypes.byref(fp._load_spec(L, vth=0.01)), ctypes.byref(p), None), sim._lib.fpic_last_error(sim._h)

    def reserved(k):
        def change(p):
            p.reserved[k] = 1
        return change

    def null_table(name):
        def change(p):
            setattr(p, name + "_n", 2)
            if name in ("azimuthal", "axial"):
                p.geometry = fp.LOAD_CYLINDER
        return change

    for change, prop in [(reserved(k), b".reserved <- ") for k in range(3)] + [(null_table(t), b"." + t.encode() + b" <- the table is null") for t in ("density", "thermal", "radial", "azimuthal", "axial")]:
        rc, why = direct(change)
        assert rc == -1 and prop in why, (prop, why)
    assert sim._lib.fpic_load_radial(sim._h, None, None, None) == -1 and b"Non-optional property is undefined" in sim._lib.fpic_last_error(sim._h)
    assert sim._lib.fpic_load_radial(sim._h, ctypes.byref(fp._load_spec(L)), None, None) == -1 and b".radial <- " in sim._lib.fpic_last_error(sim._h)
    now = sim.getParticles()
    assert bits(now["position"], before["position"]) and bits(now["velocity"], before["velocity"])      # a refused call changes nothing

    def good(p):
        p.density_n, p.density = 2, ctypes.cast(table, ctypes.POINTER(ctypes.c_double))

    assert direct(good)[0] == 0                                                   # `loaded` is optional
    assert sim.load(vth=0.01, radial=sphere(density=ok2)) == 1000 and sim.load(first=1000, radial=sphere(density=ok2)) == 0
    sim.destroy()


# ---- 9. the JavaScript host
def test_load_radial_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    n = 4000
    spec = box_spec(SHAPE, L, n, 5e-12, macro_weight=1e15 * np.prod(L) / n)
    common = dict(seed=123456789, stream=3, drift=[0.0, 0.01, 0.0], vth=0.02, mode=[1, 0, 2], xamp=[1e-5, 0.0, 0.0], xphase=0.25, vamp=1e-3, vphase=0.5)
    ball = dict(common, radial=dict(geometry="sphere", center=[0.007, 0.008, 0.009], r_max=0.005, density=G1025.tolist(), thermal=[1.0, 2.0], flow_radial=IMPLOSION))
    pinch = dict(common, seed=5, lattice=True, first=10, count=2021, lo=[0.0, 0.002, 0.0], hi=[0.016, 0.014, 0.016],
                 radial=dict(geometry="cylinder", axis=1, center=[0.007, 0.0, 0.009], r_max=0.004, density=[1.0, 0.0, 2.0], flow_azimuthal=[0.0, 0.02], flow_axial=[0.03, 0.01]))
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, ball=ball, pinch=pinch)))
    script = r"""
const fs = require('fs');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
const loaded = sim.load(inp.ball);
inp.pinch.radial.density = new Float64Array(inp.pinch.radial.density);
const typed = sim.load(inp.pinch);
const hex = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('hex');
const r = sim.select({every: [40, 7]});
const errors = [];
const ok = {geometry: 'sphere', center: [0.008, 0.008, 0.008], r_max: 0.004};
for (const bad of [{radial: 5}, {radial: [1, 2]}, {radial: Object.assign({}, ok, {geometry: 'ball'})}, {radial: Object.assign({}, ok, {center: [1, 2]})}, {radial: Object.assign({}, ok, {r_max: 'x'})},
                   {radial: Object.assign({}, ok, {axis: 0.5})}, {radial: Object.assign({}, ok, {density: [1, 'a']})}, {radial: Object.assign({}, ok, {density: [1]})},
                   {radial: Object.assign({}, ok, {r_max: 1})}, {radial: Object.assign({}, ok, {flow_axial: [1, 2]})}, {radial: ok, density: [[1, 2], null, null]},
                   {radial: ok, shear: {axis: 0, component: 0, values: [1, 2]}}, {radial: ok, vth: -1}]) {
  try { sim.load(bad); errors.push(null); } catch (err) { errors.push(String(err.message)); }
}
console.log(JSON.stringify({loaded: loaded, typed: typed, ids: Array.from(r.ids), position: hex(r.position), velocity: hex(r.velocity), errors: errors}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    sim = fp.makeCylindricalParticlePusher(spec)
    assert sim.load(**ball) == n == out["loaded"]
    assert sim.load(**pinch) == 2021 == out["typed"]
    want = sim.select(every=(40, 7))
    assert len(want["ids"]) == 100 and out["ids"] == want["ids"].tolist()
    assert out["position"] == want["position"].tobytes().hex() and out["velocity"] == want["velocity"].tobytes().hex()
    assert all(err is not None and " <- " in err for err in out["errors"]), out["errors"]
    sim.destroy()
