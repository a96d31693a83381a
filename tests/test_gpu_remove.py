"""GPU tests of the absorbing particle sinks (fpic_remove*, fpic_renumber) against the numpy rule of
tests/remove_reference.py.  Everything is exact: counts, the 128-bit tallies word for word, the doubles, the survivors bit for
bit.  A species is read through select() — ascending id, the stored values — before and after a call; the reference works on
those rows.  The scenes and their conditions are tests/remove_scenes.py (checked on the CPU by tests/test_remove_reference.py).
"""
import math

import numpy as np
import pytest

import histogram_reference as hr
import moments_reference as mr
import remove_reference as rr
import remove_scenes as rs
from test_gpu_histogram import DTYPE, ME, MP, PRECISIONS, QE, box_spec, em_dt, plain_box, two_species_box

pytestmark = pytest.mark.gpu

W = 2.5e5


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rows(sim, species=0):
    r = sim.select(species=species)
    return r["ids"], r["position"], r["velocity"]


def same_rows(a, b, ids=True):
    return (not ids or bits(a[0], b[0])) and bits(a[1], b[1]) and bits(a[2], b[2])


def same_result(got, want):
    for key in ("applications", "scanned", "removed", "energy_fixed", "momentum_fixed"):
        assert got[key] == want[key], (key, got[key], want[key])
    if "energy" in want:
        for g, w in zip([got["energy"], got["charge"]] + got["momentum"], [want["energy"], want["charge"]] + want["momentum"]):
            assert g == w or (math.isnan(g) and math.isnan(w)), (got, want)


def unit_box(fp, precision, solver, n, ni=0, shape=(8, 8, 8), seed=5, dt=1e-9, weight=1e3, b=True):
    """a box of unit edges (stored fractions = metres: select()'s rows upload without rounding), thermal electrons and ions"""
    L = (1.0, 1.0, 1.0)
    spec = box_spec(shape, L, n, em_dt(shape, L) if solver == "yee" else dt, solver=solver, macro_weight=weight)
    sim = fp.makeCylindricalParticlePusher(spec, precision=precision)
    pos, vel = rs.population(n, seed)
    sim.set(position=pos, velocity=vel)
    if ni:
        assert sim.addSpecies(MP, -QE, ni) == 1
        pi, vi = rs.population(ni, seed + 1)
        sim.set(position=pi, velocity=vi * 0.1, species=1)
    if b:
        sim.addB(0.0, 0.02, 0.05)
    return sim, spec


def remove_and_check(sim, spec, species=0, mass=ME, charge=QE, **req):
    """one remove() against the reference: the result and the survivors; returns the result"""
    before = rows(sim, species)
    survivors, want = rr.remove(*before, mass=mass, charge=charge, weight=spec["macro_weight"], **req)
    got = sim.remove(species=species, **req)
    same_result(got, want)
    assert same_rows(rows(sim, species), survivors), req
    assert sim.count(species=species) == len(survivors[0])
    return got


# ---- 1. against the reference: every request of the scenes, as loaded and after sub-steps that permuted the slots
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_requests_on_a_species_as_loaded(fp, precision, solver):
    for req in rs.REQUESTS:
        sim, spec = unit_box(fp, precision, solver, rs.N)
        got = remove_and_check(sim, spec, **req)
        assert 0 < got["removed"] < rs.N, req
        sim.destroy()


@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_requests_after_substeps(fp, precision, solver):
    for req in rs.REQUESTS[::3]:
        sim, spec = unit_box(fp, precision, solver, rs.N, ni=2000)
        sim.precalc()
        sim.substeps(10)
        got = remove_and_check(sim, spec, **req)
        assert 0 < got["removed"] < rs.N, req
        ions = remove_and_check(sim, spec, species=1, mass=MP, charge=-QE, where={"z": (0.2, 0.6)})
        assert 0 < ions["removed"] < 2000
        sim.substeps(2)     # the thinned box steps on
        assert sim.count() == rs.N - got["removed"]
        sim.destroy()


def test_values_outside_the_fixed_point_range(fp):
    """a removed particle whose |v|^2 reaches 2^15 (or is not finite) adds nothing and makes the double NaN"""
    for precision in PRECISIONS:
        sim, L = plain_box(fp, precision, 64)
        pos, vel = rs.population(64, 2)
        pos[:, 0] *= 0.5
        pos[[5, 9], 0] = 0.75
        vel[5] = (200.0, 0.0, 0.0)          # |v|^2 = 40000 >= 2^15, vx in range
        vel[9] = (np.inf, 0.0, 0.0)         # (an infinite value lies in no interval: the window is on x)
        sim.set(position=pos * L, velocity=vel)
        spec = dict(macro_weight=W)
        got = remove_and_check(sim, spec, where={"x": (0.6, None)})
        assert got["removed"] == 2 and math.isnan(got["energy"]) and math.isnan(got["momentum"][0]) and got["momentum"][1] == 0.0
        sim.destroy()


# ---- 2. loop and chunk boundaries
def boundary_case(fp, precision, n, light=False):
    sim, L = plain_box(fp, precision, n)
    rng = np.random.default_rng(n % 1000)
    dt = DTYPE[precision] if light else np.float64
    pos, vel = rng.random((n, 3), dtype=np.float32).astype(dt), (rng.random((n, 3), dtype=np.float32).astype(dt) - dt(0.5)) * dt(0.1)
    slots = rs.planted(n, precision)
    vel[slots, 0] = 1.0
    sim.set(position=pos * np.asarray(L, dtype=dt), velocity=vel)
    return sim, slots


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loop_and_chunk_boundaries(fp, precision):
    for n in rs.boundary_counts(precision):
        sim, slots = boundary_case(fp, precision, n)
        got = remove_and_check(sim, dict(macro_weight=W), where={"vx": (0.5, None)})
        assert got["removed"] == len(slots) and got["scanned"] == n
        after = rows(sim)
        assert bits(after[0], np.setdiff1d(np.arange(n, dtype=np.uint32), slots.astype(np.uint32)))
        sim.destroy()


@pytest.mark.parametrize("side", [-1, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_grid_stride(fp, precision, side):
    """n = one turn of the grid -+ 1 slot: too many rows for one select(), so a sample of the ids is compared"""
    n = rs.GRID_STRIDE + side
    sim, slots = boundary_case(fp, precision, n, light=True)
    sample = dict(every=(65537, 3))
    before = sim.select(**sample)
    got = sim.remove(where={"vx": (0.5, None)})
    assert got["removed"] == len(slots) and got["scanned"] == n
    assert got["momentum_fixed"][0] == len(slots) << 80
    assert sim.count() == n - len(slots) and sim.count(where={"vx": (0.5, None)}) == 0
    after = sim.select(**sample)
    keep = ~np.isin(before["ids"], slots)
    assert bits(after["ids"], before["ids"][keep]) and bits(after["position"], before["position"][keep]) and bits(after["velocity"], before["velocity"][keep])
    tail = sim.select(where={"x": (None, None)}, every=(n // 5, (n - 2) % (n // 5)))      # the id of the last survivor's class
    assert (n - 2) in tail["ids"] or (n - 2) in slots
    sim.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_everything_nothing_and_twice(fp, precision):
    sim, spec = unit_box(fp, precision, "poisson_fft", rs.N)
    sim.precalc()
    first = remove_and_check(sim, spec, where={"x": (0.0, 0.5)})
    second = remove_and_check(sim, spec, where={"vx": (0.0, None)}, every=(2, 1))      # from an already thinned species
    assert 0 < second["removed"] < rs.N - first["removed"]
    for req in rs.NONE:
        assert remove_and_check(sim, spec, **req)["removed"] == 0
    left = sim.count()
    gone = remove_and_check(sim, spec, **rs.ALL)
    assert gone["removed"] == left and sim.count() == 0
    assert sim.remove()["scanned"] == 0
    sim.substeps(2)      # an empty species steps
    assert sim.renumber() == 0
    sim.destroy()


# ---- 3. removing nothing is a no-op
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_removing_nothing_changes_nothing(fp, precision, solver):
    sims = [unit_box(fp, precision, solver, 3000, ni=1000)[0] for _ in range(2)]
    for s in sims:
        s.precalc()
        s.substeps(3)
    a, b = sims
    before = [rows(a, k) for k in range(2)], a.readField(fp.F3_E), a.energy(), a.stats()["sort_passes"]
    for req in rs.NONE:
        for k in range(2):
            got = a.remove(species=k, **req)
            assert got["removed"] == 0 and got["scanned"] == (3000, 1000)[k] and got["energy_fixed"] == 0
    assert all(same_rows(rows(a, k), before[0][k]) for k in range(2)) and bits(a.readField(fp.F3_E), before[1])
    assert {k: np.asarray(v).tobytes() for k, v in a.energy().items()} == {k: np.asarray(v).tobytes() for k, v in before[2].items()}
    assert a.stats()["sort_passes"] == before[3]
    assert bits(a.getParticles()["position"], b.getParticles()["position"])      # not thinned
    for s in sims:
        s.substeps(6)
    assert a.stats()["sort_passes"] == b.stats()["sort_passes"]
    assert all(same_rows(rows(a, k), rows(b, k)) for k in range(2)) and bits(a.readField(fp.F3_E), b.readField(fp.F3_E))
    for s in sims:
        s.destroy()


# ---- 4. fresh twin, electrostatic
def twin_of(fp, sim, spec, precision):
    """a new box whose species hold exactly the survivors select() returns, in ascending id"""
    held = [rows(sim, k) for k in range(2)]
    t = fp.makeCylindricalParticlePusher(dict(spec, count=len(held[0][0])), precision=precision)
    assert t.addSpecies(MP, -QE, len(held[1][0])) == 1
    for k in range(2):
        t.set(position=held[k][1], velocity=held[k][2], species=k)
    t.addB(0.0, 0.02, 0.05)
    for k in range(2):      # the round trip through the upload is exact in a unit box
        assert same_rows(rows(t, k), held[k], ids=False)
    return t


def same_boxes(fp, a, b):
    for k in range(2):
        assert same_rows(rows(a, k), rows(b, k), ids=False)
        ma, mb = a.moments(species=k), b.moments(species=k)
        assert all(bits(ma[key], mb[key]) for key in ma)
    assert bits(a.readField(fp.F3_E), b.readField(fp.F3_E)) and bits(a.readField(fp.F3_RHO_FIXED), b.readField(fp.F3_RHO_FIXED))
    ea, eb = a.energy(), b.energy()
    assert all(np.asarray(ea[key]).tobytes() == np.asarray(eb[key]).tobytes() for key in ea if key != "substep")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fresh_twin_electrostatic(fp, precision):
    sim, spec = unit_box(fp, precision, "poisson_fft", 4000, ni=1500, weight=2e9)
    sim.precalc()
    sim.substeps(5)
    for k, (mass, charge) in enumerate([(ME, QE), (MP, -QE)]):
        slab = remove_and_check(sim, spec, species=k, mass=mass, charge=charge, where={"x": (0.3, 0.55)})
        tail = remove_and_check(sim, spec, species=k, mass=mass, charge=charge, where={"v2": ((0.05, 0.005)[k] ** 2, None)})
        assert slab["removed"] > 0 and tail["removed"] > 0
    twin = twin_of(fp, sim, spec, precision)
    twin.precalc()
    same_boxes(fp, sim, twin)
    for _ in range(12):      # (past the re-binning of the eighth sub-step)
        sim.substeps(1)
        twin.substeps(1)
        same_boxes(fp, sim, twin)
    sim.destroy()
    twin.destroy()


# ---- 5. full EM: the fields stay, the survivors are pushed as in an untouched copy
@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_em_keeps_the_fields(fp, precision):
    a, spec = unit_box(fp, precision, "yee", 4000, weight=2e9)
    b, _ = unit_box(fp, precision, "yee", 4000, weight=2e9)
    for s in (a, b):
        s.precalc()
        s.substeps(4)
    fields = [a.readField(w) for w in (fp.F3_EDGE_E, fp.F3_FACE_B, fp.F3_E)]
    got = remove_and_check(a, spec, where={"x": (0.2, 0.7)}, every=(2, 0))
    assert 0 < got["removed"] < 4000
    assert all(bits(a.readField(w), f) for w, f in zip((fp.F3_EDGE_E, fp.F3_FACE_B, fp.F3_E), fields))
    a.substeps(1)
    b.substeps(1)
    ra, rb = rows(a), rows(b)
    keep = np.isin(rb[0], ra[0])
    assert bits(ra[0], rb[0][keep]) and bits(ra[1], rb[1][keep]) and bits(ra[2], rb[2][keep])
    a.destroy()
    b.destroy()


# ---- 6. the registered form
EDGE = dict(where={"x": (0.1, 0.9), "z": (0.1, 0.9)}, outside=True)


@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_registered_equals_manual(fp, precision, solver):
    k, m = 3, 12
    a, spec = unit_box(fp, precision, solver, 4000, ni=1000, weight=2e9)
    b, _ = unit_box(fp, precision, solver, 4000, ni=1000, weight=2e9)
    for s in (a, b):
        s.precalc()
    assert a.removeEvery(k, **EDGE) == 0
    assert a.removeEvery(2 * k, species=1, where={"vz": (0.0, None)}) == 1
    a.substeps(m)
    parts = [[], []]
    for step in range(1, m // k + 1):
        b.substeps(k)
        parts[0].append(b.remove(**EDGE))
        if step % 2 == 0:
            parts[1].append(b.remove(species=1, where={"vz": (0.0, None)}))
    for index in range(2):
        got, want = a.removeStats(index), rr.add_results(parts[index])
        same_result(got, want)
        assert got["removed"] > 0
    assert parts[0][0]["removed"] > 0 and parts[0][-1]["removed"] > 0      # the edge layer keeps absorbing
    for s in range(2):
        assert same_rows(rows(a, s), rows(b, s))
    assert bits(a.readField(fp.F3_E), b.readField(fp.F3_E))
    a.clearRemovals()
    with pytest.raises(fp.FusionPicError):
        a.removeStats(0)
    n = a.count()
    a.substeps(k)
    assert a.count() == n
    for s in (a, b):
        s.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_order_in_the_hook(fp, precision):
    """a fusion tally of the same sub-step sees the unthinned species, an energy row recorded on it the thinned one; two
    sinks run in registration order: a particle both name is the first one's"""
    import test_gpu_fusion as tf
    sims = [tf.like_box(fp, precision) for _ in range(2)]
    a, b = sims
    n = a.count()
    for s in sims:
        s.fusionYieldEvery(2, 0, **tf.table_kw(), **tf.SEEDS)
        s.recordEnergy(2)
    first = a.removeEvery(2, where={"x": (None, 0.5)})
    second = a.removeEvery(2, where={"y": (None, 0.5)})
    for s in sims:
        s.substeps(2)
    fa, fb = a.fusionStats(0), b.fusionStats(0)
    assert fa["pairs"] > 0 and {k: fa[k] for k in tf.COUNTS} == {k: fb[k] for k in tf.COUNTS}
    one, two = a.removeStats(first), a.removeStats(second)
    before = rows(b)
    in_x, in_y = before[1][:, 0] < 0.5, before[1][:, 1] < 0.5
    assert one["removed"] == int(in_x.sum()) > 0 and two["removed"] == int((in_y & ~in_x).sum()) > 0
    assert two["scanned"] == n - one["removed"]
    row, _ = a.energyHistory()
    assert int(row["count"][0][0]) == n - one["removed"] - two["removed"] == a.count()
    for s in sims:
        s.destroy()


# ---- 7. the other operators on a thinned species
@pytest.mark.parametrize("precision", PRECISIONS)
def test_per_particle_operators_on_a_thinned_species(fp, precision):
    """collide, collideGas and force act per particle by id and stored state: the survivors of a thinned box receive what the
    same particles of an untouched copy receive; histogram, moments and sort against their references"""
    a, spec = unit_box(fp, precision, "poisson_fft", rs.N)
    b, _ = unit_box(fp, precision, "poisson_fft", rs.N)
    for s in (a, b):
        s.precalc()
        s.substeps(3)
    remove_and_check(a, spec, where={"y": (0.2, 0.7)}, every=(3, 2))
    sigma = np.full(16, 3e-19)
    for s in (a, b):
        s.collide("elastic", nu_tau=0.8, vth=0.02, mass_ratio=2.0, seed=7, epoch=3)
        s.collideGas("exchange", density=2e19, tau=1e-9, sigma=sigma, g_lo=0.0, g_hi=0.5, vth=0.01, seed=9)
        s.force(waves=[dict(amp=5e4, mode=(1, 0, 2), nu=0.25)])
    ra, rb = rows(a), rows(b)
    keep = np.isin(rb[0], ra[0])
    assert not bits(rb[2], rows(unit_box(fp, precision, "poisson_fft", rs.N)[0])[2])      # (the operators did something)
    assert bits(ra[0], rb[0][keep]) and bits(ra[1], rb[1][keep]) and bits(ra[2], rb[2][keep])
    a.sort()
    assert same_rows(rows(a), ra)
    got = a.histogram("vx", 32, (-0.1, 0.1))
    counts, outside = hr.histogram(ra[1], ra[2], ["vx"], [32], [(-0.1, 0.1)])
    assert np.array_equal(got["counts"], counts) and got["outside"] == outside
    m = a.moments("order1")
    want, _ = mr.moments(ra[1], ra[2], (8, 8, 8), "order1")
    assert all(np.array_equal(m[key], want[key]) for key in ("N", "FX", "FY", "FZ"))
    a.substeps(9)
    assert a.count() == len(ra[0])
    a.destroy()
    b.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_series_on_a_thinned_species(fp, precision):
    sim, L = plain_box(fp, precision, 500)
    pos, vel = rs.population(500, 4)
    sim.set(position=pos * L, velocity=vel)
    sim.remove(where={"x": (None, 0.5)})
    ids, p, v = rows(sim)
    alive, dead = int(ids[-1]), int(np.setdiff1d(np.arange(500), ids)[0])
    assert alive >= len(ids)      # a surviving tracer whose id is not below the new count
    got = sim.series(tracers=[alive, dead])["tracers"]
    assert np.all(got[1] == 0)
    assert np.array_equal(got[0][3:6], v[-1].astype(np.float64)) and np.any(got[0][:3] != 0)
    with pytest.raises(fp.FusionPicError):
        sim.series(tracers=[500])
    sim.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pair_and_fusion_on_a_thinned_species(fp, precision):
    """the cell operators over the survivors with their ids, against their own references"""
    import fusion_reference as fr
    import fusion_scene as fscene
    import pair_reference as pr
    import pair_scene as pscene
    import test_gpu_fusion as tf
    import test_gpu_pair as tp
    sim = tf.like_box(fp, precision)
    s = fscene.like_scene()
    sim.remove(every=(3, 1))
    ids = rows(sim)[0].astype(np.int64)
    assert 0 < len(ids) < len(s["pos"])
    got = sim.fusionYield(0, tau=fscene.TAU, grid=True, **tf.table_kw(), **tf.SEEDS)
    out = fr.apply(tf.request(True), fscene.NCELLS, fscene.cell_index(s["pos"][ids]), ids, s["vel"][ids])
    assert out["pairs"] > 0
    tf.check(got, out)
    sim.destroy()
    sim = tp.like_box(fp, precision)
    s = pscene.like_scene()
    sim.remove(every=(4, 2), outside=False)
    ids, _, before = rows(sim)
    idx = ids.astype(np.int64)
    got = sim.collidePair(0, log_lambda=pscene.LOG_LAMBDA, tau=pscene.TAU, **tp.SEEDS)
    out = pr.apply(tp.request(True, s["W"]), pscene.cell_index(s["pos"][idx]), idx, s["vel"][idx].astype(DTYPE[precision]))
    assert got == tp.counts_of(out) and got["pairs"] > 0
    after = rows(sim)[2]
    assert np.array_equal((after != before).any(axis=1), (out["va"] != before).any(axis=1))
    sim.destroy()


# ---- 8. renumber()
@pytest.mark.parametrize("precision", PRECISIONS)
def test_renumber(fp, precision, tmp_path):
    sim, spec = unit_box(fp, precision, "poisson_fft", 4000, ni=1500, weight=2e9)
    assert sim.renumber() == 4000 and bits(rows(sim)[0], np.arange(4000, dtype=np.uint32))      # a no-op on an unthinned species
    sim.precalc()
    sim.substeps(5)
    for k in range(2):
        sim.remove(species=k, where={"x": (0.3, 0.55)})
    held = [rows(sim, k) for k in range(2)]
    twin = twin_of(fp, sim, spec, precision)
    twin.precalc()
    for k in range(2):
        n = sim.renumber(species=k)
        assert n == len(held[k][0]) == sim.count(species=k)
        after = rows(sim, k)
        assert bits(after[0], np.arange(n, dtype=np.uint32)) and bits(after[0], np.sort(rr.renumber(held[k][0])))
        assert bits(after[1], held[k][1]) and bits(after[2], held[k][2])      # ascending old id, values untouched
        got = sim.getParticles(species=k)
        assert bits(got["position"], held[k][1]) and bits(got["velocity"], held[k][2])
        assert sim.renumber(species=k) == n
    assert bits(sim.readField(fp.F3_E), twin.readField(fp.F3_E))
    sim.set(position=held[1][1], velocity=held[1][2], species=1)      # the caller-order upload works again
    sim.precalc()
    path = str(tmp_path / "thinned.ckpt")
    sim.saveCheckpoint(path)
    sim.substeps(3)
    twin.substeps(3)
    same_boxes(fp, sim, twin)
    sim.loadCheckpoint(path)
    sim.substeps(3)
    same_boxes(fp, sim, twin)
    sim.destroy()
    twin.destroy()


# ---- 9. refusals
def refused(fp, call, code, *words):
    with pytest.raises(fp.FusionPicError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_caller_order_calls_are_refused_on_a_thinned_species(fp, tmp_path):
    sim, spec = unit_box(fp, "fp32", "poisson_fft", 1000, ni=200)
    sim.remove(where={"x": (None, 0.25)})
    pos, vel = rs.population(1000, 1)
    calls = [sim.getParticles, sim.getCells, lambda: sim.getRange(0, 10), lambda: sim.getRange(0, 10, cells=True) and None,
             lambda: sim.set(position=pos), lambda: sim.setRange(0, position=pos[:10], velocity=vel[:10]), lambda: sim.load(vth=0.01),
             lambda: sim.load(vth=0.01, density=([1.0, 2.0], None, None)), lambda: sim.saveCheckpoint(str(tmp_path / "no.ckpt")),
             lambda: sim.domainInit(0, 1)]
    for call in calls:
        refused(fp, call, -5, "fpic_select", "fpic_renumber")
    assert sim.getParticles(species=1)["position"].shape == (200, 3)      # the other species is not thinned
    sim.recordSeries(1, tracers=[0])
    refused(fp, sim.renumber, -5, "series")
    sim.recordSeries(0)
    sim.removeEvery(1, where={"x": (None, 0.3)})
    refused(fp, sim.renumber, -5, "registered")
    sim.clearRemovals()
    sim.collideEvery(1, "relax", nu_tau=0.1, vth=0.01)
    refused(fp, sim.renumber, -5, "registered")
    sim.clearCollisions()
    assert sim.renumber() == sim.count()
    sim.destroy()


def test_bad_requests_and_other_handles_are_refused(fp):
    sim, _ = unit_box(fp, "fp32", "none", 100)
    bad = [lambda: sim.remove(where={"x": (0.5, 0.5)}), lambda: sim.remove(where={"x": (float("nan"), 1)}), lambda: sim.remove(species=3),
           lambda: sim.remove(every=(3, 3)), lambda: sim.removeEvery(0), lambda: sim.removeStats(0), lambda: sim.removeStats(-1)]
    for call in bad:
        refused(fp, call, -1)
    for call in (lambda: sim.remove(where={"w": (0, 1)}), lambda: sim.remove(outside=1), lambda: sim.remove(every=(1,)), lambda: sim.removeEvery(True)):
        refused(fp, call, -1)
    s = fp.RemoveSpec()
    out = fp.RemoveResult()
    for field, value in (("flags", 2), ("reserved_u", 1)):
        setattr(s, field, value)
        assert sim._lib.fpic_remove(sim._h, s, out) == -1
        setattr(s, field, 0)
    s.reserved[2] = 1.0
    assert sim._lib.fpic_remove(sim._h, s, out) == -1 and sim._lib.fpic_remove(sim._h, None, out) == -1
    for k in range(fp.REMOVE_MAX_OPS):
        assert sim.removeEvery(1, where={"vx": (5.0, None)}) == k
    refused(fp, lambda: sim.removeEvery(1), -1, "FPIC_REMOVE_MAX_OPS")
    assert sim.count() == 100
    sim.destroy()
    rz = fp.makeCylindricalParticlePusher(dict(radius=1.0, height=2.0, nr=16, nz=16, dt=1e-9, nparticles=4, particle_mass=ME, particle_charge=QE))
    for call in (rz.remove, lambda: rz.removeEvery(1), lambda: rz.removeStats(0), rz.clearRemovals, rz.renumber):
        refused(fp, call, -5)
    rz.destroy()


def test_a_decomposition_is_refused(fp):
    sims = [unit_box(fp, "fp32", "poisson_fft", 100, b=False)[0] for _ in range(2)]
    for r, s in enumerate(sims):
        s.domainInit(r, 2, ghost_planes=1)
    group = fp.BoxGroup(sims)
    for owner in sims + [group]:
        for call in (owner.remove, lambda: owner.removeEvery(1), lambda: owner.removeStats(0), owner.clearRemovals, owner.renumber):
            refused(fp, call, -5, "undecomposed")
    for s in sims:
        s.destroy()


# ---- 10. the Node host
def test_remove_through_the_javascript_host(fp, tmp_path):
    import hashlib
    import json
    import os
    import shutil
    import subprocess
    from helpers import ROOT
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    n = 4000
    spec = box_spec((8, 8, 8), (1.0, 1.0, 1.0), n, 1e-9, solver="poisson_fft", macro_weight=2e9)
    population = dict(seed=123456789, stream=3, drift=[0.0, 0.01, 0.0], vth=0.05)
    now = dict(where={"x": [0.25, 0.5], "v2": [None, 0.01]}, every=[3, 1])
    on = dict(where={"x": [0.1, 0.9], "z": [0.1, 0.9]}, outside=True)
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, population=population, now=now, on=on)))
    script = r"""
const fs = require('fs');
const crypto = require('crypto');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.load(inp.population);
sim.precalc();
const plain = (r) => ({applications: r.applications, scanned: r.scanned, removed: r.removed, energy_fixed: r.energyFixed.toString(),
  momentum_fixed: r.momentumFixed.map((x) => x.toString()), energy: r.energy, momentum: Array.from(r.momentum), charge: r.charge});
const first = plain(sim.remove(inp.now));
const index = sim.removeEvery(2, inp.on);
sim.step(2);
const stats = plain(sim.removeStats(index));
const local = plain(sim.removeStats(index, 'local'));
const r = sim.select({});
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const errors = [];
const tries = [() => sim.remove(7), () => sim.remove({where: {w: [0, 1]}}), () => sim.remove({where: {x: [0.5, 0.5]}}), () => sim.remove({species: 3}),
  () => sim.remove({every: [3, 3]}), () => sim.remove({outside: 1}), () => sim.removeEvery(0, {}), () => sim.removeEvery(0.5, {}), () => sim.removeStats(4),
  () => sim.removeStats(0.5), () => sim.getParticles(), () => sim.renumber()];
for (const t of tries) { try { t(); errors.push(null); } catch (err) { errors.push(String(err.message)); } }
sim.clearRemovals();
let cleared = null;
try { sim.removeStats(0); } catch (err) { cleared = String(err.message); }
const count = sim.renumber();
const got = sim.getParticles();
console.log(JSON.stringify({first: first, index: index, stats: stats, local: local, ids: sha(r.ids), position: sha(r.position), velocity: sha(r.velocity), errors: errors,
  cleared: cleared, count: count, renumbered: sha(got.position)}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    sim = fp.makeCylindricalParticlePusher(spec)
    sim.load(**population)
    sim.precalc()
    plain = lambda r: dict(r, energy_fixed=str(r["energy_fixed"]), momentum_fixed=[str(x) for x in r["momentum_fixed"]])
    tup = lambda w: {k: tuple(v) for k, v in w.items()}
    first = sim.remove(where=tup(now["where"]), every=tuple(now["every"]))
    assert 0 < first["removed"] < n and out["first"] == plain(first)
    assert sim.removeEvery(2, where=tup(on["where"]), outside=True) == out["index"] == 0
    sim.step(2)
    stats = sim.removeStats(0)
    assert stats["applications"] == 2 and stats["removed"] > 0 and out["stats"] == plain(stats) == out["local"]
    r = sim.select()
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert (out["ids"], out["position"], out["velocity"]) == (sha(r["ids"]), sha(r["position"]), sha(r["velocity"]))
    assert all(e is not None for e in out["errors"]), out["errors"]
    assert "fpic_renumber" in out["errors"][-2] and "registered" in out["errors"][-1]      # a thinned species; a registration
    assert out["cleared"] is not None and ".index" in out["cleared"]
    sim.clearRemovals()
    assert sim.renumber() == out["count"] == len(r["ids"])
    assert out["renumbered"] == sha(sim.getParticles()["position"])
    sim.destroy()
