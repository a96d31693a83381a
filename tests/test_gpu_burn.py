"""The fusion burn (fpic_burn*) on the GPU against the numpy restatement of its rule (tests/burn_reference.py, proved on the
CPU by tests/test_burn_reference.py and held to the header's core bit for bit by tests/test_burn_host.py) on the scenes of
tests/burn_scenes.py.  The rule has no transcendental — every operation is one of + - x / sqrt in double, rounded once — so
there is NO TOLERANCE anywhere: every count, every fixed-point word, the survivors of both reactants, and the ids, positions and
stored velocities of the products equal the reference rounded to the handle's precision bit for bit, in fp32 and fp64, with the
electrostatic and the full-EM solver, at three taus (few events, many blocked, saturated).  Further: the independence of slots
and binning; the sums against the energy diagnostics; the registered form against a manual loop; a tally beside a burner; no
event and a fit refusal change nothing; an untracked product, like species, an empty product species; the refusals and a
BoxGroup."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import burn_reference as ref
import burn_scenes as sc
import ionize_reference as iref
import remove_reference as rref
from helpers import ROOT
from test_gpu_histogram import PRECISIONS, box_spec, em_dt
from test_gpu_remove import bits, refused, rows, same_rows

pytestmark = pytest.mark.gpu

DTYPE = {"fp32": np.float32, "fp64": np.float64}
COUNTS = ("pairs", "below", "above", "cells", "overfull_cells", "overfull_particles", "accepted", "blocked", "saturated", "burnt")
SOLVERS = ["poisson_fft", "yee"]


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


class Box:
    """a scene in a handle: species a (0), b (1 or None), the products p3, p4 behind them — an alpha (2 e) and a proton, one
    particle each, with room for `room` more"""

    def __init__(self, fp, precision, name, solver="none", room=0, dt=5e-12):
        p = sc.particles(name)
        self.shape, self.L, self.like, self.precision = p["shape"], p["L"], p["like"], precision
        dt = em_dt(self.shape, self.L) if solver == "yee" else dt
        spec = box_spec(self.shape, self.L, len(p["a"][0]), dt, solver=solver, macro_weight=sc.W, particle_mass=sc.MD, particle_charge=sc.QP)
        self.sim = sim = fp.makeCylindricalParticlePusher(spec, precision=precision)
        sim.set(position=p["a"][0], velocity=p["a"][1])
        self.a, self.b = 0, None
        if not self.like:
            self.b = sim.addSpecies(sc.MT, sc.QP, len(p["b"][0]))
            sim.set(position=p["b"][0], velocity=p["b"][1], species=self.b)
        self.p3 = sim.addSpecies(sc.MA, 2 * sc.QP, 1)
        self.p4 = sim.addSpecies(sc.MP, sc.QP, 1)
        centre = np.array([self.L]) * 0.5
        for k, v in ((self.p3, 0.004), (self.p4, -0.003)):
            sim.set(position=centre, velocity=np.array([[v, 0.0, v]]), species=k)
            if room:
                sim.reserve(k, 1 + room)
        self.species = [k for k in (self.a, self.b, self.p3, self.p4) if k is not None]
        self.table = sc.table()
        self.mass = {self.a: sc.MD, self.b: sc.MT, self.p3: sc.MA, self.p4: sc.MP}
        self.charge = {self.a: sc.QP, self.b: sc.QP, self.p3: 2 * sc.QP, self.p4: sc.QP}

    def held(self):
        return {k: (rows(self.sim, k), self.sim.population(k)) for k in self.species}

    def side(self, held, k):
        (ids, pos, vel), _ = held[k]
        return dict(cell=sc.cells_of(pos, self.shape), ids=ids, pos=pos, vel=vel)

    def burn(self, tau, tracked=True, **kw):
        return self.sim.burn(self.a, self.b, products=(self.p3, self.p4 if tracked else None), tau=tau, q_value=sc.Q_DT, other_mass=0.0 if tracked else sc.MN,
                             **self.table, **dict(sc.SEEDS, **kw))

    def request(self, tau, tracked=True, **kw):
        dv = float(np.prod(np.array(self.L) / np.array(self.shape)))
        t = self.table
        return ref.request(t["sigma"], t["g_lo"], t["g_hi"], tau, sc.W, dv, sc.MD, sc.MD if self.like else sc.MT, sc.MA, sc.MP if tracked else sc.MN, q_value=sc.Q_DT,
                           like=self.like, **dict(sc.SEEDS, **kw))


def same_group(got, want, count, mass, charge, weight=sc.W):
    """a group of the result against the exact sums of the reference's rows, and the doubles derived from them"""
    assert got["energy_fixed"] == want["energy_fixed"] and got["momentum_fixed"] == want["momentum_fixed"], (got, want)
    d = iref.derived(want, count, mass, charge, weight)
    assert got["energy"] == d["energy"] and got["momentum"] == d["momentum"] and got["charge"] == d["charge"], (got, d)


def check_against(sim, app, species, before, got, mass, charge, weight=sc.W, other=(sc.MN, 0.0)):
    """one application `got` of a handle against the reference's `app` of the state `before` ({k: (rows, population)}, read
    before it): everything bit for bit.  species = (a, b or None: a with itself, p3, p4 or None: the fourth particle leaves the
    box and has other = (mass, charge)); mass, charge: per species"""
    a, b, p3, p4 = species
    T = before[a][0][2].dtype
    assert ref.conditions_hold(app)
    assert {k: got[k] for k in COUNTS} == {k: app[k] for k in COUNTS}, ({k: got[k] for k in COUNTS}, {k: app[k] for k in COUNTS})
    assert got["applications"] == 1 and got["accepted"] == got["burnt"] + got["blocked"]
    m = app["m"]
    # the survivors: every bit, their ids, their order
    for k, keep in ((a, app["keep_a"]), (b, app["keep_b"])):
        if k is None:
            continue
        was = before[k][0]
        assert same_rows(rows(sim, k), tuple(x[keep] for x in was)), k
        now = sim.population(k)
        assert now["n"] == int(keep.sum()) and now["id_span"] == before[k][1]["id_span"]
    # the products: behind the old rows, ids from the id span on in the order of the species_a reactants' ids
    for k, name in ((p3, "product_a"), (p4, "product_b")):
        if k is None:
            continue
        was, pop = before[k]
        held = rows(sim, k)
        new = app[name]
        assert new["velocity"].dtype == T and len(held[0]) == pop["n"] + m
        assert same_rows(tuple(x[:pop["n"]] for x in held), was), name
        assert bits(held[0][pop["n"]:], (pop["id_span"] + np.arange(m)).astype(np.uint32)), name
        assert bits(held[1][pop["n"]:], new["position"]), name
        assert bits(held[2][pop["n"]:], new["velocity"]), (name, int((held[2][pop["n"]:] != new["velocity"]).sum()))
        now = sim.population(k)
        assert now["n"] == pop["n"] + m and now["id_span"] == pop["id_span"] + m
    same_group(got["reactant_a"], app["lost_a"], app["lost_a"]["count"], mass[a], charge[a], weight)
    same_group(got["reactant_b"], app["lost_b"], app["lost_b"]["count"], mass[a if b is None else b], charge[a if b is None else b], weight)
    same_group(got["product_a"], app["gain_a"], m, mass[p3], charge[p3], weight)
    same_group(got["product_b"], app["gain_b"], m, other[0] if p4 is None else mass[p4], other[1] if p4 is None else charge[p4], weight)


def check_application(box, before, got, tau, tracked=True, **kw):
    """one application `got` to the state `before` (Box.held()): everything bit for bit.  Returns the reference's application"""
    A, B = box.side(before, box.a), None if box.like else box.side(before, box.b)
    (_, pop3), (_, pop4) = before[box.p3], before[box.p4]
    app = ref.application(box.request(tau, tracked, **kw), A, B, pop3["n"], pop3["id_span"], pop4["n"], pop4["id_span"], tracked_b=tracked)
    check_against(box.sim, app, (box.a, box.b, box.p3, box.p4 if tracked else None), before, got, box.mass, box.charge)
    if not tracked:      # the species that was not named keeps every row
        assert same_rows(rows(box.sim, box.p4), before[box.p4][0]) and box.sim.population(box.p4) == before[box.p4][1]
    return app


# ---- 1. against the reference: every scene, three taus, both precisions, both solvers
@pytest.mark.parametrize("name", sc.SCENES)
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_reference(fp, precision, solver, name):
    for k, which in enumerate(("rare", "many", "saturated")):
        box = Box(fp, precision, name, solver=solver, room=8000)
        if k == 1:
            box.sim.sort()
        before = box.held()
        tracked = k != 0                                                      # (the rare case: the fourth particle leaves the box)
        got = box.burn(sc.TAUS[which], tracked)
        app = check_application(box, before, got, sc.TAUS[which], tracked)
        print("%s %s %s %s: %s" % (name, precision, solver, which, {c: got[c] for c in COUNTS}))
        if which == "rare":
            assert app["m"] > 0 or name not in ("full", "full_like")
        if which == "many":
            assert app["blocked"] > 0
        if which == "saturated":
            assert app["saturated"] > 0 and app["blocked"] > 0
        if name == "wide":
            assert app["cells"] == sum(1 for a, b in sc.WIDE_COUNTS.values() if min(a, b) > 0) and (which != "saturated" or app["m"] > 10)
        if name == "full":
            assert app["overfull_cells"] == 2 and app["overfull_particles"] == sc.PAIR_CELL_MAX + 1 + 3 + 10 + sc.PAIR_CELL_MAX + 1
        if name == "full_like":
            assert app["overfull_cells"] == 1 and app["overfull_particles"] == sc.PAIR_CELL_MAX + 1 and app["cells"] == 4
        box.sim.destroy()


# ---- 2. the slots and the binning do not matter; applications follow each other
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_after_substeps_that_move_particles_and_a_second_application(fp, precision, solver):
    """sub-steps re-bin the particles (the slots are permuted, ids are no longer the slots) and, at the electrostatic box's
    large dt (a thermal particle flies a third of a cell per sub-step), carry them across cells and tiles; a second application
    acts on thinned reactants and grown products.  The fields of this dense box heat the particles, so the table is flat
    and takes every relative speed: what is checked is the state the applications meet, not the physics"""
    box = Box(fp, precision, "unlike", solver=solver, room=4000, dt=1e-7)
    box.table = dict(sigma=np.full(8, 3e-28), g_lo=0.0, g_hi=1000.0)
    sim = box.sim
    start = box.held()
    sim.precalc()
    sim.substeps(9)
    if solver == "poisson_fft":
        moved = box.held()
        assert (sc.cells_of(moved[0][0][1], box.shape) != sc.cells_of(start[0][0][1], box.shape)).mean() > 0.2
    events = []
    for k, tau in enumerate((sc.TAUS["saturated"] / 1000, sc.TAUS["saturated"] / 30, sc.TAUS["saturated"])):
        before = box.held()
        got = box.burn(tau, epoch=20 + k)
        app = check_application(box, before, got, tau, epoch=20 + k)
        events.append(app["m"])
        sim.substeps(2)
    print("events of the three applications:", events)
    assert events[0] > 0 and sum(events[1:]) > 0
    sim.destroy()


# ---- 3. the sums against the energy diagnostics
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_sums_are_what_the_energy_diagnostics_lose_and_gain(fp, precision):
    """energy() is the exact fixed-point sum over a species' rows times the species' scale (tests/test_gpu_energy_exact.py); the
    sum over the rows after minus the sum before is, species by species, the result's words"""
    box = Box(fp, precision, "unlike", solver="poisson_fft", room=4000)
    sim = box.sim
    sim.precalc()
    total = lambda held: {k: iref.gain(held[k][0][2]) for k in box.species}

    def against_energy(sums):
        e = sim.energy()
        for k in box.species:
            ke = 0.5 * box.mass[k] * sc.W * rref.C * rref.C
            assert e["kinetic"][k] == ke * rref.fixed_to_double(sums[k]["energy_fixed"]), k

    before = box.held()
    s0 = total(before)
    against_energy(s0)
    got = box.burn(sc.TAUS["many"])
    s1 = total(box.held())
    against_energy(s1)
    assert got["burnt"] > 0
    for k, name, sign in ((box.a, "reactant_a", -1), (box.b, "reactant_b", -1), (box.p3, "product_a", 1), (box.p4, "product_b", 1)):
        assert s1[k]["energy_fixed"] - s0[k]["energy_fixed"] == sign * got[name]["energy_fixed"], name
        assert [x - y for x, y in zip(s1[k]["momentum_fixed"], s0[k]["momentum_fixed"])] == [sign * x for x in got[name]["momentum_fixed"]], name
    sim.substeps(2)                                                            # the burnt box steps on
    sim.destroy()


# ---- 4. the registered form
def add_groups(parts, name):
    return dict(energy_fixed=sum(p[name]["energy_fixed"] for p in parts), momentum_fixed=[sum(p[name]["momentum_fixed"][a] for p in parts) for a in range(3)])


@pytest.mark.parametrize("solver", SOLVERS)
def test_the_registered_form_equals_a_manual_loop(fp, solver):
    a, b = Box(fp, "fp32", "unlike", solver=solver, room=4000), Box(fp, "fp32", "unlike", solver=solver, room=4000)
    for box in (a, b):
        box.sim.precalc()
    kw = dict(products=(a.p3, a.p4), tau=sc.TAUS["many"], q_value=sc.Q_DT, **sc.table(), **sc.SEEDS)
    index = a.sim.burnEvery(2, 0, 1, **kw)
    assert index == 0
    parts = []
    for s in range(1, 7):
        a.sim.substeps(1)
        b.sim.substeps(1)
        if s % 2 == 0:
            parts.append(b.sim.burn(0, 1, **dict(kw, epoch=sc.SEEDS["epoch"] + s)))
        for k in a.species:
            assert same_rows(rows(a.sim, k), rows(b.sim, k)), (s, k)
    stats = a.sim.burnStats(index)
    assert stats["applications"] == 3 and sum(p["burnt"] for p in parts) > 0
    for c in COUNTS:
        assert stats[c] == sum(p[c] for p in parts), c
    for name in ("reactant_a", "reactant_b", "product_a", "product_b"):
        want = add_groups(parts, name)
        assert stats[name]["energy_fixed"] == want["energy_fixed"] and stats[name]["momentum_fixed"] == want["momentum_fixed"], name
    refused(fp, lambda: a.sim.renumber(0), -5, "registered")
    a.sim.clearBurn()
    refused(fp, lambda: a.sim.burnStats(0), -1, "no such registered burner")
    for box in (a, b):
        box.sim.destroy()


def test_a_tally_beside_a_burner_sees_the_unburnt_plasma(fp):
    a, b = Box(fp, "fp64", "unlike", room=4000), Box(fp, "fp64", "unlike", room=4000)
    tally = dict(tau=1e-9, **sc.table(), seed=77, stream=1, epoch=2)
    t = a.sim.fusionYieldEvery(1, 0, 1, **tally)
    a.sim.burnEvery(1, 0, 1, products=(a.p3, a.p4), tau=sc.TAUS["saturated"], q_value=sc.Q_DT, **sc.table(), **sc.SEEDS)
    t2 = b.sim.fusionYieldEvery(1, 0, 1, **tally)
    a.sim.substeps(1)
    b.sim.substeps(1)
    got, want = a.sim.fusionStats(t), b.sim.fusionStats(t2)
    assert got == want and got["pairs"] > 0
    assert a.sim.burnStats(0)["burnt"] > 0 and a.sim.population(0)["n"] < b.sim.population(0)["n"]
    for box in (a, b):
        box.sim.destroy()


# ---- 5. nothing happens: no event, a refusal
def test_no_event_changes_nothing(fp):
    box = Box(fp, "fp32", "unlike", solver="poisson_fft", room=10)
    sim = box.sim
    sim.precalc()
    sim.substeps(2)
    before = box.held()
    e, rho = sim.readField(fp.F3_E), sim.readField(fp.F3_RHO_FIXED)
    got = box.burn(1e-30)                                                       # P far below 2^-33: no word accepts
    assert got["burnt"] == 0 and got["accepted"] == 0 and got["pairs"] > 0
    zero = sim.burn(0, 1, products=(box.p3, box.p4), tau=1.0, sigma=np.zeros(4), g_lo=0.0, g_hi=1.0)
    assert zero["pairs"] == 0 and zero["cells"] == 0                            # max sigma = 0: nothing is launched
    after = box.held()
    assert all(same_rows(after[k][0], before[k][0]) and after[k][1] == before[k][1] for k in box.species)
    assert bits(sim.readField(fp.F3_E), e) and bits(sim.readField(fp.F3_RHO_FIXED), rho)
    assert sim.getParticles(species=0)["position"].shape[0] == before[0][1]["n"]      # not thinned: the caller-order calls serve
    sim.substeps(1)
    sim.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_refusal_for_room_changes_nothing_and_reserve_mends_it(fp, precision):
    _, app = sc.reference("unlike", "many", DTYPE[precision], tracked_b=True)
    m = app["m"]
    assert m > 1
    box = Box(fp, precision, "unlike", solver="poisson_fft", room=m)
    sim = box.sim
    short = sim.addSpecies(sc.MP, sc.QP, 1)                                     # a second proton species, one short of the room
    sim.reserve(short, m)
    sim.precalc()
    kw = dict(tau=sc.TAUS["many"], q_value=sc.Q_DT, **sc.table(), **sc.SEEDS)
    before = box.held()
    before_short = rows(sim, short), sim.population(short)
    e = sim.readField(fp.F3_E)
    refused(fp, lambda: sim.burn(0, 1, products=(box.p3, short), **kw), -1, ".product_b", "fpic_reserve", "nothing was changed")
    after = box.held()
    assert all(same_rows(after[k][0], before[k][0]) and after[k][1] == before[k][1] for k in box.species)
    assert same_rows(rows(sim, short), before_short[0]) and sim.population(short) == before_short[1] and bits(sim.readField(fp.F3_E), e)
    assert sim.getParticles(species=0)["position"].shape[0] == before[0][1]["n"]      # no thinned mark
    sim.reserve(short, m + 1)
    got = sim.burn(0, 1, products=(box.p3, short), **kw)
    assert got["burnt"] == m and sim.population(short)["n"] == m + 1 and sim.population(box.p3)["n"] == m + 1
    sim.destroy()


GROUPS = ("reactant_a", "reactant_b", "product_a", "product_b")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_registered_application_that_does_not_fit_fails_the_step_and_changes_nothing(fp, precision):
    """a burner registered for every sub-step whose fourth product has no room at all (capacity 1, one particle): the step
    returns FPIC_ERR_STATE, and the box is, bit for bit, the twin's that stepped without a burner — every row of every
    species, the fields, no thinned mark — and the burner's totals are zeros, every count and every fixed-point word.  After
    reserve() the next sub-step applies it"""
    boxes = [Box(fp, precision, "unlike", solver="poisson_fft", room=4000) for _ in range(2)]
    shorts = [b.sim.addSpecies(sc.MP, sc.QP, 1) for b in boxes]                 # (capacity 1, full)
    assert shorts[0] == shorts[1]
    short = shorts[0]
    (a, b) = boxes
    for x in boxes:
        x.sim.set(position=np.array([x.L]) * 0.25, velocity=np.array([[0.001, 0.0, 0.0]]), species=short)
        x.sim.precalc()
    kw = dict(tau=sc.TAUS["many"], q_value=sc.Q_DT, **sc.table(), **sc.SEEDS)
    index = a.sim.burnEvery(1, 0, 1, products=(a.p3, short), **kw)
    refused(fp, lambda: a.sim.substeps(1), -5, ".product_b", "fpic_reserve", "nothing was changed")
    b.sim.substeps(1)
    for k in a.species + [short]:
        assert same_rows(rows(a.sim, k), rows(b.sim, k)) and a.sim.population(k) == b.sim.population(k), k
    for which in (fp.F3_E, fp.F3_RHO_FIXED):
        assert bits(a.sim.readField(which), b.sim.readField(which))
    assert a.sim.getParticles(species=0)["position"].shape[0] == a.sim.population(0)["n"]      # no thinned mark
    stats = a.sim.burnStats(index)
    assert stats["applications"] == 0 and all(stats[c] == 0 for c in COUNTS)
    assert all(stats[g]["energy_fixed"] == 0 and stats[g]["momentum_fixed"] == [0, 0, 0] and stats[g]["charge"] == 0.0 for g in GROUPS)
    # with room the next sub-step applies it: the twin makes the same application by hand
    a.sim.reserve(short, 4001)
    b.sim.reserve(short, 4001)
    a.sim.substeps(1)
    b.sim.substeps(1)
    got = b.sim.burn(0, 1, products=(b.p3, short), **dict(kw, epoch=sc.SEEDS["epoch"] + 2))
    stats = a.sim.burnStats(index)
    assert got["burnt"] > 0 and stats["applications"] == 1 and all(stats[c] == got[c] for c in COUNTS)
    assert all(stats[g]["energy_fixed"] == got[g]["energy_fixed"] and stats[g]["momentum_fixed"] == got[g]["momentum_fixed"] for g in GROUPS)
    for k in a.species + [short]:
        assert same_rows(rows(a.sim, k), rows(b.sim, k)), k
    for x in boxes:
        x.sim.destroy()


def test_a_product_species_that_starts_empty(fp):
    box = Box(fp, "fp64", "like", room=2000)
    sim = box.sim
    for k in (box.p3, box.p4):
        assert sim.remove(species=k)["removed"] == 1 and sim.population(k)["n"] == 0
    before = box.held()
    got = box.burn(sc.TAUS["many"])
    app = check_application(box, before, got, sc.TAUS["many"])
    now = sim.population(box.p3)
    assert app["m"] > 0 and now["n"] == app["m"] and now["id_span"] == 1 + app["m"]
    sim.destroy()


# ---- 6. the refusals
def test_the_refusals(fp):
    box = Box(fp, "fp32", "unlike", room=10)
    sim = box.sim
    good = dict(products=(box.p3, box.p4), tau=1.0, q_value=sc.Q_DT, **sc.table())
    bad = [(dict(products=(9, box.p4)), ".product_a"), (dict(products=(box.p3, 9)), ".product_b"), (dict(products=(box.p3, -2)), ".product_b"),
           (dict(products=(0, box.p4)), ".product_a"), (dict(products=(box.p3, 1)), ".product_b"), (dict(products=(box.p3, box.p3)), ".product_b"),
           (dict(other_mass=1e-27), ".other_mass"), (dict(products=(box.p3, None)), ".other_mass"), (dict(products=(box.p3, None), other_mass=float("inf")), ".other_mass"),
           (dict(q_value=float("nan")), ".q_value"), (dict(tau=0.0), ".tau"), (dict(g_hi=0.0), ".g_hi"), (dict(sigma=-sc.table()["sigma"]), ".sigma")]
    for change, word in bad:
        refused(fp, lambda: sim.burn(0, 1, **dict(good, **change)), -1, word)
    refused(fp, lambda: sim.burn(7, 1, **good), -1, ".species_a")
    refused(fp, lambda: sim.burnEvery(0, 0, 1, **good), -1, ".every")
    for k in range(fp.BURN_MAX_OPS):
        assert sim.burnEvery(3, 0, 1, **good) == k
    refused(fp, lambda: sim.burnEvery(3, 0, 1, **good), -1, "FPIC_BURN_MAX_OPS")
    refused(fp, lambda: sim.burnStats(fp.BURN_MAX_OPS), -1, ".index")
    sim.clearBurn()
    assert sim.burnEvery(3, 0, 1, **good) == 0
    sim.destroy()
    rz = fp.makeCylindricalParticlePusher(dict(radius=1.0, height=2.0, nr=16, nz=16, dt=1e-9, nparticles=4, particle_mass=1e-27, particle_charge=1e-19))
    for call in (lambda: rz.burn(0, 1, **good), lambda: rz.burnEvery(1, 0, 1, **good), lambda: rz.burnStats(0), rz.clearBurn):
        refused(fp, call, -5)
    rz.destroy()


def test_a_box_group_refuses_by_name(fp):
    group = object.__new__(fp.BoxGroup)                                         # (the refusals read no member)
    for name, call in (("burn", lambda: group.burn(0, 1)), ("burnEvery", lambda: group.burnEvery(1, 0, 1)), ("burnStats", lambda: group.burnStats(0)),
                       ("clearBurn", group.clearBurn)):
        refused(fp, call, -5, name, "undecomposed")


# ---- 7. the JavaScript host
def test_burn_through_the_javascript_host(fp, tmp_path):
    """the same box through Node: the result of a call, the totals of a registered burner and the rows of every species equal
    the Python wrapper's"""
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    p = sc.particles("unlike")
    box = Box(fp, "fp64", "unlike", solver="poisson_fft", room=4000)
    spec = box_spec(box.shape, box.L, len(p["a"][0]), 5e-12, solver="poisson_fft", macro_weight=sc.W, particle_mass=sc.MD, particle_charge=sc.QP)
    t = sc.table()
    request = dict(a=0, b=1, products=[2, 3], sigma=t["sigma"].tolist(), gLo=t["g_lo"], gHi=t["g_hi"], tau=sc.TAUS["many"], qValue=sc.Q_DT, seed=0xB0510123456, stream=3, epoch=9)
    centre = (np.array([box.L]) * 0.5).tolist()
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, precision="fp64", request=request, room=4000, species=[
        dict(position=np.asarray(p["a"][0]).tolist(), velocity=np.asarray(p["a"][1], dtype=np.float64).tolist()),
        dict(mass=sc.MT, charge=sc.QP, position=np.asarray(p["b"][0]).tolist(), velocity=np.asarray(p["b"][1], dtype=np.float64).tolist()),
        dict(mass=sc.MA, charge=2 * sc.QP, position=centre, velocity=[[0.004, 0.0, 0.004]]),
        dict(mass=sc.MP, charge=sc.QP, position=centre, velocity=[[-0.003, 0.0, -0.003]])])))
    script = r"""
const fs = require('fs');
const crypto = require('crypto');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(Object.assign({}, inp.spec, {precision: inp.precision}));
inp.species.forEach((s, k) => {
  if (k) sim.addSpecies(s.mass, s.charge, s.position.length);
  sim.set({position: s.position, velocity: s.velocity}, k);
  if (k >= 2) sim.reserve(k, 1 + inp.room);
});
sim.precalc();
const group = (g) => ({energy_fixed: g.energyFixed.toString(), momentum_fixed: g.momentumFixed.map((x) => x.toString()), energy: g.energy, momentum: Array.from(g.momentum), charge: g.charge});
const plain = (r) => ({applications: r.applications, pairs: r.pairs, below: r.below, above: r.above, cells: r.cells, overfull_cells: r.overfullCells,
  overfull_particles: r.overfullParticles, accepted: r.accepted, blocked: r.blocked, saturated: r.saturated, burnt: r.burnt,
  reactant_a: group(r.reactantA), reactant_b: group(r.reactantB), product_a: group(r.productA), product_b: group(r.productB)});
const first = plain(sim.burn(inp.request));
const index = sim.burnEvery(2, Object.assign({}, inp.request, {products: [2, null], otherMass: 1.67492749804e-27}));
sim.step(2);
const stats = plain(sim.burnStats(index));
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const rows = [0, 1, 2, 3].map((k) => { const r = sim.select({species: k}); return [sha(r.ids), sha(r.position), sha(r.velocity)]; });
const counts = [0, 1, 2, 3].map((k) => sim.population(k).n);
const errors = [];
const ok = inp.request;
const tries = [() => sim.burn({}), () => sim.burn(7), () => sim.burn(Object.assign({}, ok, {products: [2]})), () => sim.burn(Object.assign({}, ok, {products: [0, 3]})),
  () => sim.burn(Object.assign({}, ok, {products: [2.5, 3]})), () => sim.burn(Object.assign({}, ok, {qValue: 'x'})), () => sim.burn(Object.assign({}, ok, {otherMass: 1e-27})),
  () => sim.burnEvery(0, ok), () => sim.burnEvery(1.5, ok), () => sim.burnStats(4), () => sim.burnStats(0.5)];
for (const t of tries) { try { t(); errors.push(null); } catch (err) { errors.push(String(err.message)); } }
sim.clearBurn();
let cleared = null;
try { sim.burnStats(0); } catch (err) { cleared = String(err.message); }
console.log(JSON.stringify({first: first, index: index, stats: stats, rows: rows, counts: counts, errors: errors, cleared: cleared}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    # the same through the Python wrapper
    sim = box.sim
    sim.precalc()
    kw = dict(sigma=t["sigma"], g_lo=t["g_lo"], g_hi=t["g_hi"], tau=sc.TAUS["many"], q_value=sc.Q_DT, seed=request["seed"], stream=3, epoch=9)
    first = sim.burn(0, 1, products=(2, 3), **kw)
    index = sim.burnEvery(2, 0, 1, products=(2, None), other_mass=sc.MN, **kw)
    sim.step(2)
    stats = sim.burnStats(index)
    plain = lambda r: {k: ({"energy_fixed": str(v["energy_fixed"]), "momentum_fixed": [str(x) for x in v["momentum_fixed"]], "energy": v["energy"], "momentum": v["momentum"],
                            "charge": v["charge"]} if isinstance(v, dict) else v) for k, v in r.items()}
    assert first["burnt"] > 0 and stats["applications"] == 2 and out["index"] == index == 0
    assert out["first"] == plain(first), (out["first"], plain(first))
    assert out["stats"] == plain(stats), (out["stats"], plain(stats))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert out["rows"] == [[sha(x) for x in rows(sim, k)] for k in range(4)] and out["counts"] == [sim.population(k)["n"] for k in range(4)]
    words = [".sigma", ".request", ".products", ".product_a", ".productA", ".qValue", ".other_mass", ".every", ".every", ".index", ".index"]
    assert len(out["errors"]) == len(words) and all(e is not None and w in e for e, w in zip(out["errors"], words)), out["errors"]
    assert out["cleared"] is not None and "no such registered burner" in out["cleared"]
    sim.destroy()
