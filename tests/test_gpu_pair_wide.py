"""fpic_pair and fpic_fusion on the GPU off the 16^3 box: the scenes of tests/pair_wide_scene.py (37 x 33 x 29 cells; held on
the CPU by tests/test_pair_wide_reference.py) against the same numpy references as tests/test_gpu_pair.py and
tests/test_gpu_fusion.py, whose helpers are used here.  What these scenes reach and the 16^3 box does not: the scan's carry
over three turns and its ragged tail; a workgroup's second chunk and the clipped last chunk of the pairing pass and of the
tally; runs cut by the total of two species, a cell that fills the LDS alone, an overfull cell in the middle of a chunk;
partial tiles on every axis, electrostatic and full EM; a grid whose three edges differ, where a slip in the linearisation
aliases cells (the tally's per-cell grid shows it); the second trip of the index passes (big_like); and, in fresh child
processes under FPIC_PAIR_FORMS, the plain count, the plain fill and ranking by counting for long segments.

The bounds are those of tests/test_gpu_pair.py (ULPS, FP32_SHARE; the tally has no tolerance) with the amplification of
chains and triples measured on these scenes: WIDE_AMPLIFICATION = 4 x 0.218 = 0.88 (tests/test_pair_wide_reference.py).
Every scene runs in two slot orders, as uploaded (slot = id, nearly every particle outside "the turn's tile") and after
precalc(); sort() (binned), and the two must agree bit for bit; sort() moves nothing, so one reference serves both.

Met on an MI355X (fp64, largest |dv| / bound, single-stage / chains and triples): wide_like 0.44 / 0.30; wide_unlike 0.43 /
0.20 (electrons), 0.47 / 0.23 (protons).  fp32: no stored value that is not bit-equal to the reference, on either wide scene,
under full EM, or among the 43471 particles of big_like's sampled cells; big_like's |dP| and |dE| stay below 4e-6 of the
bound (whose reduction term grows with the square of the count).  Under the 16^3 scenes' amplification of 0.16 the chains
and triples of wide_like would have stood at 1.6 of the bound: the amplification has to be the one measured on the scene."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_reference as fref
import pair_reference as ref
import pair_wide_scene as wide
import test_gpu_fusion as tf
from helpers import ROOT
from test_gpu_histogram import PRECISIONS, em_dt
from test_gpu_pair import DTYPE, bits, box, check_values, counts_of, request
from test_pair_wide_reference import WIDE_AMPLIFICATION

pytestmark = pytest.mark.gpu

C = ref.C
FORMS = (0, 3, 5)              # with the default 7: count, fill and sort each in both of their forms
CHILD_TIMEOUT = 600


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def scene_of(name):
    return {"like": wide.wide_like, "unlike": wide.wide_unlike, "big": wide.big_like}[name]()


def species_of(name):
    """[(positions, velocities)] per species"""
    s = scene_of(name)
    return [(s["pos_a"], s["vel_a"]), (s["pos_b"], s["vel_b"])] if name == "unlike" else [(s["pos"], s["vel"])]


def handle(fp, make, name, precision, binned, **kw):
    """the scene in a handle of tests/test_gpu_pair.py's box (electrons, protons) or tests/test_gpu_fusion.py's (deuterons,
    tritons), in the caller's order or binned"""
    sp = species_of(name)
    sim = make(fp, precision, len(sp[0][0]), ions=len(sp[1][0]) if len(sp) > 1 else 0, **wide.BOX_KW, **kw)
    for k, (pos, vel) in enumerate(sp):
        sim.set(position=pos, velocity=vel, species=k)
    if binned:
        sim.precalc()
        sim.sort()
    # before anything else: the deposit's cell is floor(position), as every reference below assumes
    for k, (pos, _) in enumerate(sp):
        assert np.array_equal(sim.getCells(species=k), wide.cell_index(pos)), (name, precision, binned, k)
    return sim


def pair_handle(fp, name, precision, binned, **kw):
    return handle(fp, box, name, precision, binned, W=scene_of(name)["W"], **kw)


def fusion_handle(fp, name, precision, binned, **kw):
    return handle(fp, tf.box, name, precision, binned, **kw)


def pair_kw():
    return dict(log_lambda=wide.LOG_LAMBDA, tau=wide.TAU, **wide.SEEDS)


def fusion_kw():
    return dict(tau=tf.scene.TAU, grid=True, **tf.table_kw(), **tf.SEEDS)


_want = {}


def pair_wanted(name, precision):
    """the pair reference on a wide scene, once per (scene, precision); the schedule once per scene"""
    if (name, precision) not in _want:
        sp = species_of(name)
        req = request(name == "like", scene_of(name)["W"], **wide.SEEDS)
        args = [x for pos, vel in sp for x in (wide.cell_index(pos), np.arange(len(pos)))]
        if ("plan", name) not in _want:
            _want["plan", name] = ref.schedule(req, *args)
        vel = [v.astype(DTYPE[precision]) for _, v in sp]
        out = ref.apply(req, args[0], args[1], vel[0], *((args[2], args[3], vel[1]) if len(sp) > 1 else ()), plan=_want["plan", name])
        assert 0 < out["strong"] < out["pairs"] and out["overfull_cells"] == 1
        _want[name, precision] = out
    return _want[name, precision]


def fusion_wanted(name):
    """the tally's reference on a wide scene, once (the velocities are float32 values: one result for both precisions)"""
    if ("fusion", name) not in _want:
        sp = species_of(name)
        args = [x for pos, vel in sp for x in (wide.cell_index(pos), np.arange(len(pos)), vel)]
        out = fref.apply(tf.request(name == "like"), wide.NCELLS, *args)
        assert out["pairs"] > 1000 and out["below"] > 100 and out["above"] > 100 and out["overfull_cells"] == 1
        assert np.count_nonzero(out["grid"]) > 5000 and out["grid"][0] > 0 and out["grid"][-1] > 0
        out["grid"].setflags(write=False)
        _want["fusion", name] = out
    return _want["fusion", name]


def check_tally(got, out):
    """every count and every word of the grid (tests/test_gpu_fusion.py's check, on this grid)"""
    grid = got["grid"]
    assert grid.dtype == np.int64 and grid.shape == wide.SHAPE[::-1]
    assert {k: got[k] for k in tf.COUNTS} == tf.counts_of(out), ({k: got[k] for k in tf.COUNTS}, tf.counts_of(out))
    assert got["reactions"] == float(out["reactions_exact"]) * 2.0 ** out["unit_exponent"]
    wrong = np.flatnonzero(grid.ravel() != out["grid"])
    assert len(wrong) == 0, "%d cells differ, the first at %s" % (len(wrong), wrong[:8])
    assert int(grid.sum()) == out["reactions_exact"]


def overfull_of(name):
    return (wide.LIKE_RUN_AT + 4, 2049) if name == "like" else (wide.UNLIKE_RUN_AT + 1, 4097)


def run_pair(fp, name, precision, binned, **kw):
    """collidePair on a fresh handle: (counts, before, after) with the species' read-backs"""
    sim = pair_handle(fp, name, precision, binned, **kw)
    species = len(species_of(name))
    before = tf.state(sim, species)
    got = sim.collidePair(0, 1 if species > 1 else None, **pair_kw())
    after = tf.state(sim, species)
    sim.destroy()
    return got, before, after


def check_pair(name, precision, got, before, after):
    out = pair_wanted(name, precision)
    cell, particles = overfull_of(name)
    print("%s %s: %s" % (name, precision, got))
    assert got == counts_of(out) and (got["overfull_cells"], got["overfull_particles"]) == (1, particles)
    for k, (side, (pos, vel)) in enumerate(zip("ab", species_of(name))):
        assert bits(after[k]["position"], before[k]["position"])
        assert bits(before[k]["velocity"], vel.astype(DTYPE[precision]))
        check_values(precision, after[k]["velocity"], before[k]["velocity"], out, side, WIDE_AMPLIFICATION)
        inside = wide.cell_index(pos) == cell
        assert inside.sum() in (2048, 2049) and bits(after[k]["velocity"][inside], before[k]["velocity"][inside])


# ---- a. fpic_pair on the wide scenes
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["like", "unlike"])
def test_pair_on_the_wide_scenes(fp, name, precision):
    plain = run_pair(fp, name, precision, False)
    check_pair(name, precision, *plain)
    binned = run_pair(fp, name, precision, True)
    assert binned[0] == plain[0]
    for k in range(len(plain[2])):
        assert bits(binned[2][k]["velocity"], plain[2][k]["velocity"]) and bits(binned[2][k]["position"], plain[2][k]["position"]), (name, precision, k)


# ---- b. fpic_fusion on the same scenes
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["like", "unlike"])
def test_fusion_on_the_wide_scenes(fp, name, precision):
    out = fusion_wanted(name)
    species = len(species_of(name))
    for binned in (False, True):
        sim = fusion_handle(fp, name, precision, binned)
        before = tf.state(sim, species)
        got = sim.fusionYield(0, 1 if species > 1 else None, **fusion_kw())
        assert tf.same_state(before, tf.state(sim, species))
        sim.destroy()
        print("%s %s %s: %s" % (name, precision, "binned" if binned else "as uploaded", {k: got[k] for k in tf.COUNTS}))
        check_tally(got, out)


# ---- c. full EM: tiles of 8 x 8 x 8 cells, 5 x 5 x 4 of them, partial on every axis
def test_the_full_em_tiling(fp):
    dt = em_dt(wide.SHAPE, wide.L)
    check_pair("unlike", "fp32", *run_pair(fp, "unlike", "fp32", True, dt=dt, solver="yee"))
    sim = fusion_handle(fp, "unlike", "fp32", True, dt=dt, solver="yee")
    before = tf.state(sim, 2)
    got = sim.fusionYield(0, 1, **fusion_kw())
    assert tf.same_state(before, tf.state(sim, 2))
    sim.destroy()
    check_tally(got, fusion_wanted("unlike"))


# ---- d. the second trip of the index passes
def run_big(fp, binned):
    """the tally, then the collisions, of big_like on a fresh fp32 handle (the tally changes nothing)"""
    s = wide.big_like()
    sim = pair_handle(fp, "big", "fp32", binned)
    before = sim.getParticles()
    e0 = sim.energy()
    tally = sim.fusionYield(0, **fusion_kw())
    assert tf.same_state([before], [sim.getParticles()])
    got = sim.collidePair(0, **pair_kw())
    e1 = sim.energy()
    after = sim.getParticles()
    sim.destroy()
    assert bits(before["velocity"], s["vel"]) and bits(after["position"], before["position"])
    return dict(tally=tally, pair=got, before=before, after=after, e0=e0, e1=e1)


def test_the_second_trip_of_the_index_passes(fp):
    s = wide.big_like()
    n = wide.N_BIG
    plain, binned = run_big(fp, False), run_big(fp, True)
    pairs, cells = wide.like_pairs(np.bincount(s["cell"], minlength=wide.NCELLS))
    assert cells == wide.NCELLS
    for run in (plain, binned):
        got, tally = run["pair"], run["tally"]
        assert got == dict(applications=1, pairs=pairs, strong=got["strong"], cells=cells, overfull_cells=0, overfull_particles=0) and 0 < got["strong"] < pairs
        assert tally["pairs"] + tally["below"] + tally["above"] == pairs and (tally["cells"], tally["overfull_cells"], tally["overfull_particles"]) == (cells, 0, 0)
        assert tally["grid"].shape == wide.SHAPE[::-1] and int(tally["grid"].sum()) == tally["reactions_exact"] and (tally["grid"] > 0).all()
    # everything is the same in the two orders
    assert plain["pair"] == binned["pair"] and bits(plain["after"]["velocity"], binned["after"]["velocity"])
    grid = plain["tally"].pop("grid")
    assert bits(grid, binned["tally"].pop("grid")) and plain["tally"] == binned["tally"]
    # the references on the particles of every 97th cell, with their real ids
    ids = np.flatnonzero(s["cell"] % wide.BIG_EVERY == 0)
    out = ref.apply(request(True, s["W"], **wide.SEEDS), s["cell"][ids], ids, s["vel"][ids])
    assert 0 < out["strong"] < out["pairs"]
    check_values("fp32", plain["after"]["velocity"][ids], plain["before"]["velocity"][ids], out, "a", WIDE_AMPLIFICATION)
    want = fref.apply(tf.request(True, W=s["W"]), wide.NCELLS, s["cell"][ids], ids, s["vel"][ids])
    mine = np.arange(0, wide.NCELLS, wide.BIG_EVERY)
    assert np.array_equal(grid.ravel()[mine], want["grid"][mine]) and int(want["grid"].sum()) == int(want["grid"][mine].sum()) > 0
    assert (plain["tally"]["unit_exponent"], want["cells"]) == (want["unit_exponent"], len(mine))
    # momentum and kinetic energy: the bound of test_gpu_pair.test_momentum_and_energy_are_conserved (its docstring)
    eps = float(np.finfo(np.float32).eps)
    vmax = 1.5 * float(np.abs(plain["after"]["velocity"]).max())
    mv, mvv = wide.ME * vmax, wide.ME * vmax ** 2
    p_bound = pairs * 9 * eps * mv * s["W"] * C + n * 2.0 ** -53 * n * mv * s["W"] * C
    e_bound = pairs * 27 * eps * mvv * s["W"] * C * C + n * 2.0 ** -53 * n * mvv * s["W"] * C * C
    dp = np.abs(plain["e1"]["momentum"].sum(axis=0) - plain["e0"]["momentum"].sum(axis=0))
    de = abs(plain["e1"]["kinetic"].sum() - plain["e0"]["kinetic"].sum())
    print("big_like: |dP| / bound %s, |dE| / bound %.3g" % (dp / p_bound, de / e_bound))
    assert np.all(dp <= p_bound) and de <= e_bound
    assert (plain["after"]["velocity"] != plain["before"]["velocity"]).any(axis=1).mean() > 0.99


# ---- e. the other forms of the passes
def digests(fp):
    """what (a), (b) and (d) compute, as counts and sha256 digests: {case: {tally, grid, pair, velocity}}, every case on a
    fresh handle of tests/test_gpu_pair.py's box (the tally first: it changes nothing)"""
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = {}
    cases = [(name, precision, binned) for name in ("like", "unlike") for precision in PRECISIONS for binned in (False, True)]
    for name, precision, binned in cases + [("big", "fp32", False), ("big", "fp32", True)]:
        species = len(species_of(name))
        sim = pair_handle(fp, name, precision, binned)
        tally = sim.fusionYield(0, 1 if species > 1 else None, **fusion_kw())
        pair = sim.collidePair(0, 1 if species > 1 else None, **pair_kw())
        after = tf.state(sim, species)
        sim.destroy()
        grid = tally.pop("grid")
        assert tally["pairs"] > 0 and pair["pairs"] > 0
        out["%s %s %s" % (name, precision, "binned" if binned else "as uploaded")] = dict(
            tally={k: int(tally[k]) for k in tf.COUNTS}, grid=sha(grid), pair={k: int(v) for k, v in pair.items()}, velocity=[sha(a["velocity"]) for a in after])
    return out


def test_the_other_forms_of_the_passes(fp):
    """FPIC_PAIR_FORMS is read once per process, so each value gets a fresh child (tests/pair_forms_child.py), one after
    another; a child that fails or runs out of time fails the test there and no further child is started.  Neither the order
    inside a segment (count, fill) nor the sort used may show in any digest."""
    assert "FPIC_PAIR_FORMS" not in os.environ, "the in-process run must be the default form"
    mine = digests(fp)
    assert len(mine) == 10
    for name in ("like", "unlike", "big"):            # (and the orders agree, as in (a), (b) and (d))
        for precision in PRECISIONS if name != "big" else ["fp32"]:
            assert mine["%s %s binned" % (name, precision)] == mine["%s %s as uploaded" % (name, precision)]
    child = os.path.join(ROOT, "tests", "pair_forms_child.py")
    for forms in FORMS:
        done = subprocess.run([sys.executable, child], env=dict(os.environ, FPIC_PAIR_FORMS=str(forms)), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              timeout=CHILD_TIMEOUT)
        assert done.returncode == 0, "FPIC_PAIR_FORMS=%d: exit status %d\n%s" % (forms, done.returncode, done.stderr.decode()[-2000:])
        got = json.loads(done.stdout.decode().strip().splitlines()[-1])
        assert got["forms"] == str(forms)
        for case in mine:
            assert got["digests"][case] == mine[case], (forms, case)
