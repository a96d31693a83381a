"""The fusion yield tally (fpic_fusion*) on the GPU against the numpy restatement of its rule (tests/fusion_reference.py, held
to the header bit for bit on the CPU by tests/test_fusion_host.py) on the scenes of tests/fusion_scene.py.  The tally is
integers of double arithmetic whose every operation is rounded once, so there is no tolerance anywhere: every count and every
word of the int64 grid equal the reference, in fp32 and fp64, electrostatic and full EM; no byte of a particle changes; the
result does not depend on the slots; the registered form accumulates what a manual loop of calls adds up, sees the velocities
a pair operator of the same sub-step has written, and drains with fusionGrid(reset=True); an all-zero table launches
nothing; the refusals; the JavaScript host."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import fusion_reference as ref
import fusion_scene as scene
import pair_scene
from helpers import ROOT
from test_gpu_histogram import PRECISIONS, box_spec, em_dt

pytestmark = pytest.mark.gpu

DTYPE = {"fp32": np.float32, "fp64": np.float64}
SEEDS = dict(seed=0xD07F00D123456789, stream=6, epoch=4)
MD, MT, QP = 3.3435837724e-27, 5.0073567446e-27, 1.602176634e-19
COUNTS = ("applications", "pairs", "below", "above", "cells", "overfull_cells", "overfull_particles", "yield_hi", "yield_lo", "unit_exponent", "reactions_exact")


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def box(fp, precision, n, W=scene.W, dt=5e-12, solver="none", ions=0, **kw):
    spec = box_spec(scene.SHAPE, scene.L, n, dt, solver=solver, macro_weight=W, particle_mass=MD, particle_charge=QP, **kw)
    sim = fp.makeCylindricalParticlePusher(spec, precision=precision)
    if ions:
        assert sim.addSpecies(MT, QP, ions) == 1
    return sim


def like_box(fp, precision, **kw):
    s = scene.like_scene()
    sim = box(fp, precision, len(s["pos"]), **kw)
    sim.set(position=s["pos"], velocity=s["vel"])
    return sim


def unlike_box(fp, precision, **kw):
    s = scene.unlike_scene()
    sim = box(fp, precision, len(s["pos_a"]), ions=len(s["pos_b"]), **kw)
    sim.set(position=s["pos_a"], velocity=s["vel_a"])
    sim.set(position=s["pos_b"], velocity=s["vel_b"], species=1)
    return sim


def table_kw(g_lo=scene.G_LO):
    S, lo, hi = scene.table(g_lo)
    return dict(sigma=S, g_lo=lo, g_hi=hi)


def request(like, g_lo=scene.G_LO, tau=scene.TAU, W=scene.W, **seeds):
    S, lo, hi = scene.table(g_lo)
    return ref.request(S, lo, hi, tau, W, scene.DV, like=like, **dict(SEEDS, **seeds))


_want = {}


def wanted(like, g_lo=scene.G_LO):
    """the reference's result on the scene, computed once (the velocities are float32 values: one result for both precisions)"""
    key = (like, g_lo)
    if key not in _want:
        if like:
            s = scene.like_scene()
            out = ref.apply(request(True, g_lo), scene.NCELLS, scene.cell_index(s["pos"]), np.arange(len(s["pos"])), s["vel"])
        else:
            s = scene.unlike_scene()
            out = ref.apply(request(False, g_lo), scene.NCELLS, scene.cell_index(s["pos_a"]), np.arange(len(s["pos_a"])), s["vel_a"],
                            scene.cell_index(s["pos_b"]), np.arange(len(s["pos_b"])), s["vel_b"])
        out["grid"].setflags(write=False)
        _want[key] = out
    return _want[key]


def counts_of(out, applications=1):
    return dict(applications=applications, **{k: int(out[k]) for k in COUNTS[1:]})


def check(got, out, applications=1):
    """every count and every word of the grid"""
    grid = got.pop("grid")
    assert grid.dtype == np.int64 and grid.shape == scene.SHAPE[::-1]
    assert {k: got[k] for k in COUNTS} == counts_of(out, applications), (got, counts_of(out, applications))
    assert got["reactions"] == float(out["reactions_exact"]) * 2.0 ** out["unit_exponent"]
    assert np.array_equal(grid.ravel(), out["grid"])
    assert int(grid.sum()) == out["reactions_exact"]


def state(sim, species):
    return [sim.getParticles(species=k) for k in range(species)]


def same_state(before, after):
    return all(sorted(a) == sorted(b) and all(bits(np.asarray(a[key]), np.asarray(b[key])) for key in a) for a, b in zip(before, after))


# ---- 1. every count and every word of the grid; no byte of a particle changes
def test_the_reference_is_not_trivial():
    like, unlike, zero = wanted(True), wanted(False), wanted(True, 0.0)
    for out in (like, unlike):
        assert out["pairs"] > 100 and out["below"] > 10 and out["above"] > 10 and out["reactions_exact"] > 2 ** 40 and out["overfull_cells"] == 0
        assert np.count_nonzero(out["grid"]) >= 8
    assert like["cells"] == sum(1 for n in scene.LIKE_COUNTS if n >= 2) and unlike["cells"] == sum(1 for a, b in scene.UNLIKE_COUNTS if min(a, b) > 0)
    assert like["pairs"] + like["below"] + like["above"] == sum(n // 2 + (2 if n % 2 and n > 1 else 0) for n in scene.LIKE_COUNTS)
    assert unlike["pairs"] + unlike["below"] + unlike["above"] == sum(max(a, b) for a, b in scene.UNLIKE_COUNTS if min(a, b) > 0)
    assert like["weights"] == sum(n * n / 2.0 for n in scene.LIKE_COUNTS if n >= 2) and unlike["weights"] == sum(a * b for a, b in scene.UNLIKE_COUNTS)
    # the chosen pairs: one at rest (below this table; inside the table from 0, yielding 0) and one on the node 32
    nodes = scene.G_LO + np.arange(scene.N) / 4096.0
    assert (like["g"] == 0).sum() == 1 and like["what"][like["g"] == 0][0] == 1
    at = np.flatnonzero(like["g"] == scene.NODE_G)
    assert len(at) == 1 and nodes[32] == scene.NODE_G and like["what"][at[0]] == 0
    rest = np.flatnonzero(zero["g"] == 0)
    assert len(rest) == 1 and zero["what"][rest[0]] == 0 and zero["q"][rest[0]] == 0 and zero["below"] == 0 and zero["pairs"] == like["pairs"] + like["below"]


@pytest.mark.parametrize("solver", ["none", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_count_and_every_cell(fp, precision, solver):
    dt = em_dt(scene.SHAPE, scene.L) if solver == "yee" else 5e-12
    sim = like_box(fp, precision, dt=dt, solver=solver)
    before = state(sim, 1)
    got = sim.fusionYield(0, tau=scene.TAU, grid=True, **table_kw(), **SEEDS)
    from_zero = sim.fusionYield(0, None, tau=scene.TAU, grid=True, **table_kw(0.0), **SEEDS)
    assert same_state(before, state(sim, 1))
    sim.destroy()
    print("like species %s %s: %s" % (precision, solver, {k: got[k] for k in COUNTS}))
    check(got, wanted(True))
    check(from_zero, wanted(True, 0.0))
    sim = unlike_box(fp, precision, dt=dt, solver=solver)
    before = state(sim, 2)
    got = sim.fusionYield(0, 1, tau=scene.TAU, grid=True, **table_kw(), **SEEDS)
    without_grid = sim.fusionYield(0, 1, tau=scene.TAU, **table_kw(), **SEEDS)
    # the species exchanged: a tie now goes to the tritons, so only the classification-free counts must agree
    swapped = sim.fusionYield(1, 0, tau=scene.TAU, **table_kw(), **SEEDS)
    assert same_state(before, state(sim, 2))
    sim.destroy()
    print("unlike species %s %s: %s" % (precision, solver, {k: got[k] for k in COUNTS}))
    assert "grid" not in without_grid and without_grid == {k: v for k, v in got.items() if k != "grid"}
    check(got, wanted(False))
    assert swapped["cells"] == got["cells"] and swapped["pairs"] + swapped["below"] + swapped["above"] == got["pairs"] + got["below"] + got["above"]


# ---- 2. full and overfull cells
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_full_cell_is_tallied_and_an_overfull_one_is_skipped(fp, precision):
    cap = fp.PAIR_CELL_MAX
    assert cap == ref.CELL_MAX == 2048
    cells = [(8, 8, 7), (9, 8, 7), (7, 8, 7), (15, 15, 15)]
    na, nb = [cap + 1, cap, 10, 7], [3, cap, cap + 1, 7]
    pa, va = pair_scene.populate(na, 41, 0.01, cells)
    pb, vb = pair_scene.populate(nb, 42, 0.008, cells)
    sim = box(fp, precision, len(pa), ions=len(pb))
    sim.set(position=pa, velocity=va)
    sim.set(position=pb, velocity=vb, species=1)
    before = state(sim, 2)
    got = [sim.fusionYield(0, tau=scene.TAU, grid=True, **table_kw(), **SEEDS), sim.fusionYield(1, tau=scene.TAU, grid=True, **table_kw(), **SEEDS),
           sim.fusionYield(0, 1, tau=scene.TAU, grid=True, **table_kw(), **SEEDS)]
    assert same_state(before, state(sim, 2))
    sim.destroy()
    ca, cb, ia, ib = scene.cell_index(pa), scene.cell_index(pb), np.arange(len(pa)), np.arange(len(pb))
    want = [ref.apply(request(True), scene.NCELLS, ca, ia, va), ref.apply(request(True), scene.NCELLS, cb, ib, vb), ref.apply(request(False), scene.NCELLS, ca, ia, va, cb, ib, vb)]
    assert [(w["overfull_cells"], w["overfull_particles"], w["cells"]) for w in want] == [(1, cap + 1, 3), (1, cap + 1, 3), (2, 2 * cap + 15, 2)]
    full = scene.cell_index(np.array([[9.5, 8.5, 7.5]]))[0]
    assert all(w["grid"][full] > 0 for w in want) and want[2]["weights"] == cap * cap + 49
    for g, w in zip(got, want):
        check(g, w)
        assert int(max(w["grid"])) < 2 ** 51


# ---- 3. independence of the slots
@pytest.mark.parametrize("precision", PRECISIONS)
def test_slot_independence(fp, precision):
    kw = dict(tau=scene.TAU, grid=True, **table_kw(), **SEEDS)
    # a: sorted into tiles, then pushed with no field at a time step at which a thermal particle crosses half a cell per
    # sub-step: particles leave their cells and tiles and sit in the slots of tiles they have left
    a = unlike_box(fp, precision, dt=2e-7)
    a.precalc()
    sorted_now = a.fusionYield(0, 1, **kw)             # (before the sort: the caller's order)
    a.sort()
    after_sort = a.fusionYield(0, 1, **kw)
    a.substeps(3)
    start = state(a, 2)
    s = scene.unlike_scene()
    metres = [p["position"] * DTYPE[precision](scene.L[0]) for p in start]          # (read back as fractions of the box; times 16: exact)
    moved = scene.cell_index(metres[0].astype(np.float64)) != scene.cell_index(s["pos_a"])
    tile = lambda pos: (np.floor(np.asarray(pos, dtype=np.float64)).astype(np.int64) >> 3)
    assert moved.mean() > 0.3 and (tile(metres[0]) != tile(s["pos_a"])).any(axis=1).sum() > 10
    got_a = [a.fusionYield(0, 1, **kw), a.fusionYield(0, **dict(kw, epoch=9)), a.fusionYield(1, **dict(kw, epoch=10))]
    a.destroy()
    check(sorted_now, wanted(False))
    check(after_sort, wanted(False))
    # b: the same particles uploaded in the caller's order (slot = id) into a fresh handle
    b = box(fp, precision, len(s["pos_a"]), ions=len(s["pos_b"]), dt=2e-7)
    for k in range(2):
        b.set(position=metres[k], velocity=start[k]["velocity"], species=k)
    got_b = [b.fusionYield(0, 1, **kw), b.fusionYield(0, **dict(kw, epoch=9)), b.fusionYield(1, **dict(kw, epoch=10))]
    other = b.fusionYield(0, 1, **dict(kw, epoch=77))
    b.destroy()
    for x, y in zip(got_a, got_b):
        assert np.array_equal(x.pop("grid"), y.pop("grid")) and x == y and x["pairs"] > 0 and x["reactions_exact"] > 0
    # and the reference on that state; another epoch is another pairing
    cells = [scene.cell_index(m.astype(np.float64)) for m in metres]
    want = ref.apply(request(False), scene.NCELLS, cells[0], np.arange(len(cells[0])), start[0]["velocity"], cells[1], np.arange(len(cells[1])), start[1]["velocity"])
    assert got_b[0] == counts_of(want) | dict(reactions=got_b[0]["reactions"])
    assert other["reactions_exact"] != got_b[0]["reactions_exact"]


# ---- 4. the registered form equals the manual loop; the drain
@pytest.mark.parametrize("solver", ["none", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_registered_equals_manual(fp, precision, solver):
    dt = em_dt(scene.SHAPE, scene.L) if solver == "yee" else 5e-12
    a, b = (unlike_box(fp, precision, dt=dt, solver=solver) for _ in range(2))
    for s in (a, b):
        s.precalc()
    ops = [(1, (0, 1), dict(table_kw(), seed=61, stream=1)), (2, (0, None), dict(table_kw(0.0), seed=62, stream=2, epoch=100)), (3, (1, 1), dict(table_kw(), seed=63))]
    assert [a.fusionYieldEvery(every, *sp, **kw) for every, sp, kw in ops] == [0, 1, 2]
    zero = a.fusionStats(2)
    assert zero["applications"] == 0 and zero["reactions_exact"] == 0 and not a.fusionGrid(2).any()
    a.substeps(4)
    sums = [dict(grid=np.zeros(scene.SHAPE[::-1], dtype=np.int64), **{k: 0 for k in COUNTS}) for _ in ops]
    for k in range(1, 5):
        b.substeps(1)
        for (every, sp, kw), total in zip(ops, sums):
            if k % every == 0:
                got = b.fusionYield(*sp, tau=every * dt, grid=True, **dict(kw, epoch=k + kw.get("epoch", 0)))
                for key in COUNTS + ("grid",):
                    total[key] = got[key] if key == "unit_exponent" else total[key] + got[key]
    assert same_state(state(a, 2), state(b, 2))
    for i, total in enumerate(sums):
        stats, grid = a.fusionStats(i), a.fusionGrid(i)
        total["yield_hi"], total["yield_lo"] = total["reactions_exact"] >> 32, total["reactions_exact"] & 0xFFFFFFFF
        assert {k: stats[k] for k in COUNTS} == {k: total[k] for k in COUNTS}, (i, stats, total)
        assert np.array_equal(grid, total["grid"]) and int(grid.sum()) == stats["reactions_exact"]
        assert a.fusionStats(i, "local") == stats
    assert [a.fusionStats(i)["applications"] for i in range(3)] == [4, 2, 1] and all(a.fusionStats(i)["pairs"] > 0 and a.fusionStats(i)["reactions_exact"] > 0 for i in range(3))
    # the drain: the copy first, then zero — grid, totals and applications; the other operators keep theirs
    kept = a.fusionGrid(1)
    drained = a.fusionGrid(0, reset=True)
    assert np.array_equal(drained, sums[0]["grid"]) and not a.fusionGrid(0).any()
    after = a.fusionStats(0)
    assert all(after[k] == 0 for k in COUNTS if k != "unit_exponent") and after["unit_exponent"] == sums[0]["unit_exponent"]
    assert np.array_equal(a.fusionGrid(1), kept)
    a.substeps(1)
    b.substeps(1)
    again = b.fusionYield(0, 1, tau=dt, grid=True, **dict(ops[0][2], epoch=5))
    assert np.array_equal(a.fusionGrid(0), again["grid"]) and a.fusionStats(0)["reactions_exact"] == again["reactions_exact"] and a.fusionStats(0)["applications"] == 1
    # clearFusion drops them all; a new registration starts from zero
    a.clearFusion()
    with pytest.raises(fp.FusionPicError, match=r"\.index <- "):
        a.fusionStats(0)
    assert a.fusionYieldEvery(1, 0, **table_kw()) == 0
    assert a.fusionStats(0)["applications"] == 0 and not a.fusionGrid(0).any()
    a.substeps(1)
    assert a.fusionStats(0)["applications"] == 1 and a.fusionStats(0)["pairs"] > 0
    a.destroy()
    b.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_tally_sees_the_collided_velocities(fp, precision):
    """registered beside a pair operator on the same species and the same sub-step: the pair operator runs first"""
    W = pair_scene.weight(7, 0.01, ma=MD, qa=QP, mb=MT, qb=QP)
    a, b, c = (unlike_box(fp, precision, W=W) for _ in range(3))
    for s in (a, b, c):
        s.precalc()
    fusion = dict(table_kw(), seed=71)
    assert a.fusionYieldEvery(1, 0, 1, **fusion) == 0              # (registered first: it still runs behind the pair operator)
    assert a.collidePairEvery(1, 0, 1, log_lambda=10.0, seed=72) == 0
    assert c.fusionYieldEvery(1, 0, 1, **fusion) == 0
    a.substeps(2)
    c.substeps(2)
    total = np.zeros(scene.SHAPE[::-1], dtype=np.int64)
    for k in (1, 2):
        b.substeps(1)
        assert b.collidePair(0, 1, log_lambda=10.0, seed=72, epoch=k)["pairs"] > 0
        total += b.fusionYield(0, 1, grid=True, **dict(fusion, epoch=k))["grid"]
    assert same_state(state(a, 2), state(b, 2))
    with_collisions, without = a.fusionGrid(0), c.fusionGrid(0)
    for s in (a, b, c):
        s.destroy()
    assert total.any() and np.array_equal(with_collisions, total) and not np.array_equal(without, total)


# ---- 5. an all-zero table
def test_an_all_zero_table_launches_nothing(fp):
    sim = unlike_box(fp, "fp32")
    got = sim.fusionYield(0, 1, sigma=np.zeros(5), g_lo=0.0, g_hi=0.05, grid=True)
    assert not got.pop("grid").any() and got.pop("applications") == 1 and got.pop("reactions") == 0.0 and all(v == 0 for v in got.values()), got
    assert sim.fusionYieldEvery(1, 0, 1, sigma=np.zeros(2), g_lo=0.0, g_hi=0.05) == 0
    sim.precalc()
    sim.substeps(2)
    stats = sim.fusionStats(0)
    assert stats.pop("applications") == 2 and all(v == 0 for v in stats.values()) and not sim.fusionGrid(0).any()
    # the next table with something in it works
    assert sim.fusionYield(0, 1, tau=scene.TAU, **table_kw(), **SEEDS)["reactions_exact"] == wanted(False)["reactions_exact"]
    sim.destroy()


# ---- 6. refusals; the next valid call succeeds
def test_refusals(fp):
    from helpers import make_spec
    good = table_kw()
    rz = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    for call in (lambda: rz.fusionYield(0, **good), lambda: rz.fusionYieldEvery(1, 0, **good), lambda: rz.fusionStats(0), lambda: rz.fusionGrid(0), rz.clearFusion):
        with pytest.raises(fp.FusionPicError, match="needs a CART3D handle") as e:
            call()
        assert e.value.code == -5
    rz.destroy()
    sim = like_box(fp, "fp32")
    nan, inf = float("nan"), float("inf")
    S = np.array(good["sigma"])
    spoiled = lambda k, v: np.concatenate([S[:k], [v], S[k + 1:]])
    cases = [
        (dict(a=1), ".species_a <- no such species"), (dict(a=-1), ".species_a <- no such species"), (dict(b=1), ".species_b <- no such species"),
        (dict(b=-2), ".species_b <- no such species"), (dict(tau=nan), ".tau <- must not be NaN"), (dict(tau=0.0), ".tau <- must be positive and finite"),
        (dict(tau=-1e-9), ".tau <- must be positive and finite"), (dict(tau=inf), ".tau <- must be positive and finite"),
        (dict(sigma=[1e-28]), ".n <- must be 2 .. FPIC_FUSION_TABLE_MAX (4096)"), (dict(sigma=np.zeros(4097)), ".n <- must be 2 .. FPIC_FUSION_TABLE_MAX (4096)"),
        (dict(g_lo=-1e-9), ".g_lo <- must be finite and not negative"), (dict(g_lo=nan), ".g_lo <- must be finite and not negative"),
        (dict(g_lo=inf), ".g_lo <- must be finite and not negative"), (dict(g_hi=good["g_lo"]), ".g_hi <- must be finite and above g_lo"),
        (dict(g_hi=0.001), ".g_hi <- must be finite and above g_lo"), (dict(g_hi=inf), ".g_hi <- must be finite and above g_lo"), (dict(g_hi=nan), ".g_hi <- must be finite and above g_lo"),
        (dict(sigma=spoiled(0, -1e-40)), ".sigma <- every entry must be finite and not negative"), (dict(sigma=spoiled(96, inf)), ".sigma <- every entry must be finite and not negative"),
        (dict(sigma=spoiled(50, nan)), ".sigma <- every entry must be finite and not negative"), (dict(sigma=S / S.max() * 1e300), ".sigma <- the yield bound"),
    ]
    before = state(sim, 1)
    for kw, message in cases:
        kw = dict(good, **kw)
        for call in (lambda: sim.fusionYield(**kw), lambda: sim.fusionYieldEvery(1, **kw)):
            with pytest.raises(fp.FusionPicError) as e:
                call()
            assert message in str(e.value) and e.value.code == -1, (kw, str(e.value))
    lib = sim._lib
    for field, value in (("reserved_i", 1), ("reserved", None)):
        s = fp._fusion_spec(5e-12, **good)
        if value is None:
            s.reserved[2] = 1.0
        else:
            s.reserved_i = value
        assert lib.fpic_fusion(sim._h, s, None, None) == -1 and b".reserved <- must be zero" in lib.fpic_last_error(sim._h)
        assert lib.fpic_fusion_register(sim._h, s, 1, None) == -1 and b".reserved <- must be zero" in lib.fpic_last_error(sim._h)
    s = fp._fusion_spec(5e-12, **good)
    s.sigma = None
    assert lib.fpic_fusion(sim._h, s, None, None) == -1 and b".sigma <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_fusion(sim._h, None, None, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_fusion_register(sim._h, None, 1, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_fusion_stats(sim._h, 0, 0, None) == -1 and b".out <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    for every in (0, -1):
        with pytest.raises(fp.FusionPicError, match=r"\.every <- must be at least 1"):
            sim.fusionYieldEvery(every, tau=scene.TAU, **good)
    for index in (0, -1):
        for call in (lambda: sim.fusionStats(index), lambda: sim.fusionGrid(index), lambda: sim.fusionGrid(index, reset=True)):
            with pytest.raises(fp.FusionPicError, match=r"\.index <- no such registered operator"):
                call()
    assert same_state(before, state(sim, 1))
    assert [sim.fusionYieldEvery(1000 + k, **good) for k in range(fp.FUSION_MAX_OPS)] == list(range(fp.FUSION_MAX_OPS))
    with pytest.raises(fp.FusionPicError, match=r"\.spec <- FPIC_FUSION_MAX_OPS \(4\) operators are registered already"):
        sim.fusionYieldEvery(1, **good)
    with pytest.raises(fp.FusionPicError, match=r"\.index <- no such registered operator"):
        sim.fusionStats(fp.FUSION_MAX_OPS)
    with pytest.raises(fp.FusionPicError, match=r"\.scope <- "):
        sim._check(lib.fpic_fusion_stats(sim._h, 0, 7, fp.FusionResult()))
    assert lib.fpic_fusion_grid(sim._h, 0, None, 0) == -1 and b".grid <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_fusion_grid(sim._h, 0, None, 1) == 0                                 # a reset alone
    sim.clearFusion()
    assert lib.fpic_fusion(sim._h, fp._fusion_spec(5e-12, tau=scene.TAU, **good, **SEEDS), None, None) == 0     # `out` and `grid` are optional
    got = sim.fusionYield(0, tau=scene.TAU, grid=True, **good, **SEEDS)
    check(got, wanted(True))
    sim.destroy()


def test_a_decomposition_is_refused(fp):
    """as fpic_pair: all five calls say so, on a member and on the group"""
    good = table_kw()
    sims = []
    for r in range(2):
        s = box(fp, "fp32", 1000)
        s.domainInit(r, 2, ghost_planes=2, migrate_every=2, distributed_solve=0)
        sims.append(s)
    g = fp.BoxGroup(sims)
    for owner in (sims[0], g):
        for call in (lambda: owner.fusionYield(0, **good), lambda: owner.fusionYieldEvery(1, 0, **good), lambda: owner.fusionStats(0), lambda: owner.fusionGrid(0), owner.clearFusion):
            with pytest.raises(fp.FusionPicError, match="cannot pair a cell alone") as e:
                call()
            assert e.value.code == -5 and "needs an undecomposed handle" in str(e.value)
    for s in sims:
        s.destroy()


# ---- 7. the JavaScript host
def test_fusion_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    n = 4000
    spec = box_spec(scene.SHAPE, scene.L, n, 5e-12, solver="none", macro_weight=scene.W, particle_mass=MD, particle_charge=QP)
    population = dict(seed=123456789, stream=3, drift=[0.0, 0.01, 0.0], vth=0.01)
    S, g_lo, g_hi = scene.table()
    now = dict(a=0, sigma=S.tolist(), gLo=g_lo, gHi=g_hi, tau=1e-9, seed=99, stream=4, epoch=7)
    every = dict(sigma=S.tolist(), gLo=g_lo, gHi=g_hi, seed=5)
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, population=population, now=now, every=every)))
    script = r"""
const fs = require('fs');
const crypto = require('crypto');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.load(inp.population);
sim.precalc();
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const plain = (r) => { const o = {}; for (const k of Object.keys(r)) o[k] = k === 'grid' ? sha(r[k]) : (typeof r[k] === 'bigint' ? r[k].toString() : r[k]); return o; };
const first = plain(sim.fusionYield(Object.assign({grid: true}, inp.now)));
const bare = plain(sim.fusionYield(inp.now));
const index = sim.fusionYieldEvery(2, inp.every);
sim.step(2);
const stats = plain(sim.fusionStats(index));
const local = plain(sim.fusionStats(index, 'local'));
const grid = sim.fusionGrid(index);
const drained = sim.fusionGrid(index, true);
const after = plain(sim.fusionStats(index));
const errors = [];
const ok = inp.now;
const tries = [() => sim.fusionYield({}), () => sim.fusionYield(7), () => sim.fusionYield(Object.assign({}, ok, {sigma: 'x'})), () => sim.fusionYield(Object.assign({}, ok, {sigma: [1e-28]})),
  () => sim.fusionYield(Object.assign({}, ok, {a: 3})), () => sim.fusionYield(Object.assign({}, ok, {b: 1})), () => sim.fusionYield(Object.assign({}, ok, {seed: -1})),
  () => sim.fusionYield(Object.assign({}, ok, {tau: 0})), () => sim.fusionYield(Object.assign({}, ok, {gHi: 0})), () => sim.fusionYield(Object.assign({}, ok, {gLo: 'x'})),
  () => sim.fusionYield(Object.assign({}, ok, {sigma: [1e-28, -1e-28]})), () => sim.fusionYieldEvery(0, ok), () => sim.fusionYieldEvery(1.5, ok), () => sim.fusionStats(4),
  () => sim.fusionGrid(4), () => sim.fusionGrid(0.5)];
for (const t of tries) { try { t(); errors.push(null); } catch (err) { errors.push(String(err.message)); } }
sim.clearFusion();
let cleared = null;
try { sim.fusionStats(0); } catch (err) { cleared = String(err.message); }
console.log(JSON.stringify({first: first, bare: bare, index: index, stats: stats, local: local, grid: sha(grid), gridType: grid.constructor.name, gridLength: grid.length,
  drained: sha(drained), after: after, errors: errors, cleared: cleared}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    import hashlib
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    sim = fp.makeCylindricalParticlePusher(spec)
    sim.load(**population)
    sim.precalc()
    first = sim.fusionYield(0, sigma=S, g_lo=g_lo, g_hi=g_hi, tau=1e-9, seed=99, stream=4, epoch=7, grid=True)
    index = sim.fusionYieldEvery(2, sigma=S, g_lo=g_lo, g_hi=g_hi, seed=5)
    sim.step(2)
    stats, grid = sim.fusionStats(index), sim.fusionGrid(index)
    sim.destroy()
    names = {"overfull_cells": "overfullCells", "overfull_particles": "overfullParticles", "yield_hi": "yieldHi", "yield_lo": "yieldLo", "unit_exponent": "unitExponent",
             "reactions_exact": "reactionsExact"}
    camel = lambda d: {names.get(k, k): (str(v) if k == "reactions_exact" else sha(v) if k == "grid" else v) for k, v in d.items()}
    assert out["first"] == camel(first) and first["pairs"] > 0 and first["reactions_exact"] > 0
    assert out["bare"] == {k: v for k, v in camel(first).items() if k != "grid"}
    assert out["index"] == index == 0 and out["stats"] == camel(stats) == out["local"] and stats["applications"] == 2 and stats["reactions_exact"] > 0
    assert (out["grid"], out["gridType"], out["gridLength"]) == (sha(grid), "BigInt64Array", scene.NCELLS) and out["drained"] == out["grid"]
    assert out["after"]["applications"] == 0 and out["after"]["reactionsExact"] == "0" and out["after"]["pairs"] == 0
    assert all(err is not None and " <- " in err for err in out["errors"]), out["errors"]
    assert out["cleared"] is not None and ".index <- " in out["cleared"]
