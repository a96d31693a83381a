"""The energy and momentum diagnostics of the 3-D box (fpic_energy_now) against the exact reference of
tests/energy_reference.py, on the paths that tests/test_gpu_energy.py leaves unrun: species counts on either side of every
boundary of the particle pass's loop (derived from its launch grid, read from the kernel header), up to the 16 species a
row holds, velocities where a fixed-point conversion goes wrong, non-finite velocities, field sums in which every thread
adds many nodes, and decomposed ranks that hold dead slots.  Particle entries (count, kinetic, momentum, speed_max) are
bit-identical to the reference applied to the stored velocities; field sums lie within the rounding bound of their
summation depth.  A box that holds a non-finite velocity is never stepped."""
import math
import os
import re

import numpy as np
import pytest

import energy_reference as er
from helpers import ROOT

pytestmark = pytest.mark.gpu

ME, QE, MP = 9.109e-31, -1.602e-19, 1.67e-27
W = 2.5e5
PRECISIONS = ["fp32", "fp64"]
DTYPE = {"fp32": np.float32, "fp64": np.float64}
LANES = {"fp32": 4, "fp64": 2}          # particles per 16-byte vector of the particle pass


def launch_grid():
    """kDiagBlocks, kDiagThreads and kDiagFieldBlocks of the kernels, so that a new launch grid moves the counts with it"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_diag_kernels.hpp")).read()
    get = lambda name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    return get("kDiagBlocks"), get("kDiagThreads"), get("kDiagFieldBlocks")


BLOCKS, THREADS, FIELD_BLOCKS = launch_grid()
SWEEP = BLOCKS * THREADS                # vectors one pass of the grid covers; the two-vector loop runs beyond it


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def make_box(fp, precision, n0, shape=(8, 8, 8), solver="none"):
    L = tuple(1e-3 * s for s in shape)
    dt = 0.5 / (er.C * math.sqrt(sum((shape[a] / L[a]) ** 2 for a in range(3)))) if solver == "yee" else 1e-12
    spec = dict(radius=L[0], length_y=L[1], height=L[2], nr=shape[0], ny=shape[1], nz=shape[2], dt=dt, nparticles=0, count=n0,
                particle_mass=ME, particle_charge=QE, geometry="cart3d", solver=solver, macro_weight=W)
    return fp.makeCylindricalParticlePusher(spec, precision=precision), spec


def cell_volume(spec):
    return (spec["radius"] / spec["nr"]) * (spec["length_y"] / spec["ny"]) * (spec["height"] / spec["nz"])


def bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def check_species(row, s, v, mass, weight=W):
    """entry s of a raw fpic_energy row against the reference applied to the stored velocities v, bit for bit"""
    want = er.species_row(v, mass, weight)
    assert int(row["count"][s]) == want["count"], s
    assert bits(row["kinetic"][s]) == bits(want["kinetic"]), (s, row["kinetic"][s], want["kinetic"])
    assert bits(row["momentum"][s]) == bits(want["momentum"]), (s, row["momentum"][s], want["momentum"])
    assert bits(row["speed_max"][s]) == bits(want["speed_max"]), (s, row["speed_max"][s], want["speed_max"])


def check_unused_slots(row):
    ns = int(row["nspecies"])
    for key in ("count", "kinetic", "momentum", "speed_max"):
        assert not np.any(row[key][ns:]), key
    assert not np.any(row["reserved"])


def thermal(rng, n, sigma, T):
    """normal velocities with one row in 5 scaled down by 1e-9: terms over many scales, small negative ones included"""
    v = rng.standard_normal((n, 3)) * sigma
    v[::5] *= 1e-9
    return v.astype(T)


# ---- (a) the particle pass's loop: counts on either side of every boundary, up to 16 species in one box
def loop_counts(lanes):
    S = SWEEP
    return [1, lanes - 1, lanes + 1, S * lanes - 1, S * lanes, S * lanes + 1, 2 * S * lanes - 1, 2 * S * lanes + 1, 3 * S * lanes + lanes - 1]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loop_boundaries_of_the_particle_pass(fp, precision):
    T, lanes = DTYPE[precision], LANES[precision]
    rng = np.random.default_rng(21)
    counts = loop_counts(lanes)
    sim, _ = make_box(fp, precision, counts[0])
    with pytest.raises(fp.FusionPicError, match=r"\.count <- must be at least 1"):
        sim.addSpecies(MP, -QE, 0)                   # an empty species is refused (count 0 has no row to test)
    masses = [ME]
    for n in counts[1:]:
        masses.append(MP * len(masses))
        assert sim.addSpecies(masses[-1], -QE, n) == len(masses) - 1
    while len(masses) < fp.ENERGY_SPECIES:           # the rest of the 16: small odd counts
        counts.append(2 * len(masses) + 1)
        masses.append(ME * len(masses))
        assert sim.addSpecies(masses[-1], -QE, counts[-1]) == len(masses) - 1
    for s, n in enumerate(counts):
        sim.set(velocity=thermal(rng, n, 0.03, T), species=s)
    row = sim._energy_row("global")
    assert int(row["nspecies"]) == fp.ENERGY_SPECIES
    for s, n in enumerate(counts):
        v = sim.getParticles(species=s)["velocity"]
        assert len(v) == n
        check_species(row, s, v, masses[s])
        del v
    nv = -(-max(counts) // lanes)
    print("%s: largest species %d particles = %d vectors = %.2f sweeps of %d vectors (%d x %d threads); %d species in one row"
          % (precision, max(counts), nv, nv / SWEEP, SWEEP, BLOCKS, THREADS, len(counts)))
    assert nv > 3 * SWEEP
    sim.destroy()


def test_seventeenth_species_is_refused(fp):
    sim, _ = make_box(fp, "fp32", 3)
    for _ in range(fp.ENERGY_SPECIES - 1):
        sim.addSpecies(MP, -QE, 5)
    assert int(sim._energy_row("global")["nspecies"]) == fp.ENERGY_SPECIES
    sim.addSpecies(MP, -QE, 5)
    with pytest.raises(fp.FusionPicError, match="report at most 16 species"):
        sim.energy()
    with pytest.raises(fp.FusionPicError, match="report at most 16 species"):
        sim.recordEnergy(1)
    sim.destroy()


# ---- (b) velocity content where a conversion to fixed point goes wrong
def neighbours(x, T):
    x = T(x)
    return [x, np.nextafter(x, T(0)), np.nextafter(x, T(np.inf))]


def as_rows(rng, values, T):
    """a list of component values -> [m][3] rows: every value once per column, the columns shuffled independently"""
    vals = np.array(values, dtype=T)
    return np.stack([rng.permutation(vals) for _ in range(3)], axis=1)


def content_species(rng, T):
    """(name, mass, velocities) of one species of each kind"""
    out = [("thermal electrons", ME, (rng.standard_normal((100003, 3)) * 0.03).astype(T)),
           ("slow ions", MP, (rng.standard_normal((100001, 3)) * 1e-5).astype(T))]
    # a cold beam: every component just below -1e-20 c, where 2^64 + x rounded to a multiple of 2^11 units was wrong by 1.6 %
    out.append(("cold beam", 2 * MP, (-1e-20 * (1 + 1e-3 * rng.random((50001, 3)))).astype(T)))
    # the edges of the old conversion and of the exponent range
    edges = []
    for p in (-16, -17, -28, -29, -57, -58):
        for x in neighbours(2.0 ** p, T):
            edges += [x, -x, T(3) * x, -T(3) * x]
    out.append(("edges", 3 * MP, as_rows(rng, edges * 5, T)))
    # tiny components, whose sum stays below 2^53 units so that one unit shows in the row: 2^-70 and its neighbours, zeros
    # of both signs, subnormals of the storage type, exact multiples of 2^-80
    sub = np.nextafter(T(0), T(1))
    tiny = [T(0), -T(0), sub, -sub, T(7) * sub, -T(7) * sub, np.finfo(T).tiny / T(2), -np.finfo(T).tiny / T(2)]
    for x in neighbours(2.0 ** -70, T):
        tiny += [x, -x]
    tiny += list((rng.integers(-2 ** 20, 2 ** 20, 200) * 2.0 ** -80).astype(T))
    tiny += list((-rng.random(200) * 2.0 ** -66).astype(T))
    out.append(("tiny", 4 * MP, as_rows(rng, tiny * 3, T)))
    # speeds up to 100 c, inside the bound |v|^2 < 2^15
    d = rng.standard_normal((20001, 3))
    out.append(("fast", 5 * MP, (d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0, 100, (20001, 1))).astype(T)))
    # +- pairs of exact multiples of 2^-80 (every double above 2^-28 and every float above 2^-57 is one): the momentum is
    # exactly zero in fixed point, which no float sum promises
    u = (rng.standard_normal((30000, 3)) * 0.03).astype(T)
    u[np.abs(u) < 2.0 ** -20] = 0
    k = (rng.integers(-2 ** 20, 2 ** 20, (1000, 3)) * 2.0 ** -80).astype(T)
    half = np.concatenate([u, k])
    out.append(("pairs", 6 * MP, rng.permutation(np.concatenate([half, -half]))))
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
def test_velocity_content(fp, precision):
    T = DTYPE[precision]
    rng = np.random.default_rng(5)
    species = content_species(rng, T)
    sim, _ = make_box(fp, precision, len(species[0][2]))
    for s, (_, mass, v) in enumerate(species):
        if s:
            assert sim.addSpecies(mass, -QE if mass != ME else QE, len(v)) == s
        sim.set(velocity=v, species=s)
    row = sim._energy_row("global")
    assert int(row["nspecies"]) == len(species)
    check_unused_slots(row)
    for s, (name, mass, v) in enumerate(species):
        stored = sim.getParticles(species=s)["velocity"]
        if name == "tiny":
            sub = (stored != 0) & (np.abs(stored) < np.finfo(T).tiny)
            flushed = er.species_row(np.where(sub, T(0), stored), mass, W)
            print("%s: %d subnormal components sent, %d stored; the pass converts them %s" % (
                precision, int(np.sum((v != 0) & (np.abs(v) < np.finfo(T).tiny))), int(sub.sum()),
                "as flushed to zero" if bits(row["momentum"][s]) == bits(flushed["momentum"]) and sub.any() else "exactly"))
        if name == "slow ions":
            assert np.mean(np.abs(stored.astype(np.float64)) < 2.0 ** -17) > 0.3
        check_species(row, s, stored, mass)
        if name == "pairs":
            assert not np.any(row["momentum"][s]) and row["kinetic"][s] > 0
    sim.destroy()


# ---- (c) non-finite velocities: the species reports a non-finite value, the others are untouched
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("bad", ["nan", "+inf", "-inf"])
def test_non_finite_velocity(fp, precision, bad):
    T = DTYPE[precision]
    rng = np.random.default_rng(17)
    n = 40961
    sim, _ = make_box(fp, precision, n)
    masses = [ME, MP, 2 * MP]
    assert sim.addSpecies(MP, -QE, n + 2) == 1 and sim.addSpecies(2 * MP, -QE, n + 5) == 2
    vs = [thermal(rng, n, 0.03, T), thermal(rng, n + 2, 0.03, T), thermal(rng, n + 5, 1e-5, T)]
    comp = {"nan": 0, "+inf": 1, "-inf": 2}[bad]
    vs[1][n // 3, comp] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[bad]
    for s, v in enumerate(vs):
        sim.set(velocity=v, species=s)
    row = sim._energy_row("global")
    stored = [sim.getParticles(species=s)["velocity"] for s in range(3)]
    assert int(row["count"][1]) == n + 2
    got = (row["kinetic"][1], row["momentum"][1][comp], row["speed_max"][1])
    assert not np.isfinite(got[0]) and not np.isfinite(got[2]) and not np.isfinite(got[1]), got
    if bad == "nan":
        assert np.isnan(row["speed_max"][1])
    else:
        assert row["speed_max"][1] == np.inf
    for s in (0, 2):                # nothing leaks into the other species
        check_species(row, s, stored[s], masses[s])
    pm = MP * W * er.C
    for a in range(3):              # the finite components are summed as ever
        if a != comp:
            assert bits(row["momentum"][1][a]) == bits(pm * er.from_fix(er.fix_sum(stored[1][:, a].astype(np.float64)))), a
    sim.destroy()


# ---- (d) field sums where every thread adds several nodes
def field_tolerance(nodes):
    """(relative bound, nodes per thread) of a field sum over `nodes` nodes.  Every summand is >= 0, so a sum in which each
    term passes through at most D rounded additions is within D u / (1 - D u) of the exact sum, u = 2^-53.  Here D is:
    2 for the node's |E|^2 = (ex^2 + ey^2) + ez^2 (the squares are rounded as the reference rounds them); k = the nodes one
    thread adds (ceil(nodes / (kDiagFieldBlocks kDiagThreads))); 6 levels of the wave's butterfly (64 lanes); the waves of a
    workgroup added one after the other (kDiagThreads / 64 - 1); in the combining workgroup, ceil(kDiagFieldBlocks /
    kDiagThreads) partials per thread and again 6 + kDiagThreads / 64 - 1.  Three more roundings: the kernel's product with
    0.5 eps0 dV, and the reference's correctly rounded fsum and its own product."""
    k = -(-nodes // (FIELD_BLOCKS * THREADS))
    waves = THREADS // 64
    depth = 2 + k + 6 + (waves - 1) + -(-FIELD_BLOCKS // THREADS) + 6 + (waves - 1) + 3
    u = 2.0 ** -53
    return depth * u / (1 - depth * u), k


def spiky_field(rng, shape, scale):
    """normal values with a few spikes up and down, so that the terms span many orders of magnitude"""
    f = rng.standard_normal(shape + (3,)) * scale
    flat = f.reshape(-1, 3)
    idx = rng.choice(len(flat), 64, replace=False)
    flat[idx[:32]] *= 1e5
    flat[idx[32:]] *= 1e-7
    return f


def within(got, want, tol, what):
    err = abs(got - want) / want
    assert err <= tol, (what, got, want, err, tol)
    return err


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", [(64, 64, 64), (96, 80, 72), (256, 256, 256)])
def test_field_e_sum_electrostatic(fp, precision, shape):
    rng = np.random.default_rng(shape[0] + shape[2])
    sim, spec = make_box(fp, precision, 1, shape=shape)
    sim.set(E=spiky_field(rng, shape, 1e3))
    row = sim._energy_row("global")
    E = sim.readField(fp.F3_E)[:, :3]                # the stored values
    tol, k = field_tolerance(E.shape[0])
    err = within(float(row["field_e"]), er.field_e(E, cell_volume(spec)), tol, "field_e")
    print("%s %s: %d nodes, %d per thread, error %.2e of a bound %.2e" % (precision, shape, E.shape[0], k, err, tol))
    assert row["field_b"] == 0 and row["field_b_external"] == 0
    sim.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", [(64, 64, 64), (96, 80, 72)])
def test_field_sums_full_em(fp, precision, shape):
    rng = np.random.default_rng(shape[1])
    n = 2000
    sim, spec = make_box(fp, precision, n, shape=shape, solver="yee")
    L = (spec["radius"], spec["length_y"], spec["height"])
    sim.set(position=rng.random((n, 3)) * L, velocity=rng.normal(0, 0.05, (n, 3)))
    sim.set(edge_E=spiky_field(rng, shape, 1e4), face_B=spiky_field(rng, shape, 0.05))
    row = sim._energy_row("global")
    E, B = sim.readField(fp.F3_EDGE_E)[:, :3], sim.readField(fp.F3_FACE_B)[:, :3]
    tol, k = field_tolerance(E.shape[0])
    dv = cell_volume(spec)
    ee = within(float(row["field_e"]), er.field_e(E, dv), tol, "field_e")
    eb = within(float(row["field_b"]), er.field_b(B, dv), tol, "field_b")
    print("%s %s full EM: %d per thread, errors %.2e %.2e of a bound %.2e" % (precision, shape, k, ee, eb, tol))
    sim.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_open_chain_row_equals_closed_row(fp, precision):
    """after one sub-step the chained lattice step leaves B at the half time; the row forms B of the integer time in
    registers, and must equal the row after F3_FACE_B has stored it — on a grid where the field loop runs"""
    shape = (64, 64, 48)
    rng = np.random.default_rng(48)
    n = 20000
    sim, spec = make_box(fp, precision, n, shape=shape, solver="yee")
    L = (spec["radius"], spec["length_y"], spec["height"])
    sim.set(position=rng.random((n, 3)) * L, velocity=rng.normal(0, 0.05, (n, 3)))
    sim.set(edge_E=rng.normal(0, 1e4, shape + (3,)), face_B=rng.normal(0, 0.05, shape + (3,)))
    sim.substeps(1)
    open_row = sim._energy_row("global")
    B = sim.readField(fp.F3_FACE_B)[:, :3]            # (closes the chain)
    closed = sim._energy_row("global")
    for key in ("field_e", "field_b", "kinetic", "momentum", "speed_max", "count"):
        assert np.asarray(open_row[key]).tobytes() == np.asarray(closed[key]).tobytes(), key
    tol, k = field_tolerance(B.shape[0])
    assert k >= 2
    within(float(closed["field_b"]), er.field_b(B, cell_volume(spec)), tol, "field_b")
    sim.destroy()


# ---- (e) decomposed ranks: their own particles, dead slots among them, and their own planes
def test_decomposed_ranks(fp):
    import decomp_scene as ds
    n, world = 5000000, 2
    sc = ds.build(fp, dict(world=world, shape=(16, 16, 32), ghost=2, every=1, em=False, distributed_solve=0, precision="fp32", n=n, seed=31))
    sims = []
    for r in range(world):
        s = fp.makeCylindricalParticlePusher(dict(sc["spec"], count=n), precision="fp32")
        s.domainInit(r, world, ghost_planes=sc["G"], migrate_every=sc["every"])
        first = int(sc["counts"][:r].sum())
        s.domainSet(sc["pos"][first:first + sc["counts"][r]], sc["vel"][first:first + sc["counts"][r]], first_id=first)
        sims.append(s)
    g = fp.BoxGroup(sims)
    g.precalc()
    for _ in range(3):
        g.step()
        if sum(s.domainStats()["migrated"] for s in sims) > 0:
            break
    assert sum(s.domainStats()["migrated"] for s in sims) > 0
    nzl = sc["shape"][2] // world
    dv = cell_volume(sc["spec"])
    held = []
    for r, s in enumerate(sims):
        row = s._energy_row("local")
        got = s.domainGet()
        held.append(len(got["ids"]))
        assert int(row["nspecies"]) == 1
        check_species(row, 0, got["velocity"], ME, sc["spec"]["macro_weight"])
        E = s.readField(fp.F3_E).reshape(sc["shape"][2], -1, 4)[r * nzl:(r + 1) * nzl, :, :3]
        tol, _ = field_tolerance(E.shape[0] * E.shape[1])
        within(float(row["field_e"]), er.field_e(E, dv), tol, "field_e of rank %d" % r)
    print("decomposed: ranks hold %s particles (a sweep covers %d)" % (held, SWEEP * LANES["fp32"]))
    assert max(held) > SWEEP * LANES["fp32"] and sum(held) == n
    for s in sims:
        s.destroy()
