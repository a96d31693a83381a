"""Generation 2 of the random call sequences on the CART3D box: the six newest operator families — force() / forceOn(),
collideGas() / collideGasEvery(), fusionYield() / fusionYieldEvery() / fusionGrid(), fusionSpectrum() / fusionSpectrumEvery() /
fusionSpectrumRead(), load(density=, thermal=, shear=) and load(radial=) — under the relations of tests/test_gpu_sequences.py,
whose helpers this module uses.  tests/sequence_model.py (generation 2) turns a seed into the scene and the steps;
tests/test_sequence_model.py proves on the CPU that the committed SEEDS2 reach the states meant here and that no committed request
is vacuous.  Everything below is equality bit for bit or of exact integers: no tolerance anywhere.

Relation 1, a fresh twin per step, as in generation 1: B is filled from A.saveCheckpoint(), both get the operation, and the
particles by id, the fields and the returned values agree — the returned dictionaries whole, their integers (work_fixed,
impulse_fixed, energy_fixed, momentum_fixed, the counts) as integers and their derived floats as bits (exact()).
The time of a one-shot force() is the HANDLE'S OWN count of sub-steps plus the request's epoch (at = diag.substep + epoch in
fes_force.inc.hpp), where collide, collideGas, collidePair and the fusion calls take an absolute epoch.  A checkpoint carries
no sub-step count, and loadCheckpoint does not rewind the count of the handle it loads into (fes_checkpoint.inc.hpp never
touches diag.substep): so the test's own count t of A's sub-steps IS A's count whatever was loaded in between, the fresh twin's
count is 0, and the twin's force() carries epoch + t.  The control: on one seed a second twin gets epoch + t + 1, and it differs.
With operators registered on A, B gets the manual loop in the hook's full order (diag_after_substep): substeps(1), the forces
in registration order (a one-shot force adds B's own running count j, so the request carries epoch + t - j), collide,
collideGas, collidePair, fusionYield, fusionSpectrum, then the recorder rows; at the end A's forceStats, gasStats, fusionStats,
fusionGrid and fusionSpectrumRead are the integer sums of what B returned along the way, and C's.
Relation 2: C gets the state-changing operations and nothing else, and A equals it at the midpoint and at the end: now also
fusionYield, fusionSpectrum and the five stats reads write no particle.  fusionYield (the counts and every cell of the grid)
and fusionSpectrum (every bin, under, over, and their sum) on A are held to tests/fusion_reference.py and
tests/fusion_spectrum_reference.py on A.getParticles() and A.getCells() read just before; a stats read in mid-run equals the
sums B has returned so far.
The named sequence of the resets: fusionGrid(reset=True) and fusionSpectrumRead(reset=True) directly after a substeps, after a
one-shot operation and after a loadCheckpoint; the pieces A read, added as Python integers, and A's last read equal what B
returned and what C, which never resets, reads at the end; no piece is all zero.
Relation 3: the six decompositions of generation 1 under sequences with one-shot forces and windowed collisions of both kinds,
a full reload from a density profile and one from a radial body, forceOn and collideGasEvery registered beside collideEvery,
and both fusion calls refused once on the group and on a rank with nothing changed; forceStats and gasStats of the group are
one handle's.  The kicks stay below the background's thermal speed (asserted on the CPU): lost == 0, migrated > 0.
The resume: all six families registered, their periods dividing the cut, a force envelope across it.

Wall times on an MI355X, one run of the module on its own (18.5 s in all):
    relations 1 + 2, 12 seeds     13.4 s together: 0.7 to 1.0 s each, 2.3 s and 2.5 s for the first electrostatic and the first
                                  full-EM seed of the process (the transform library and the code objects are loaded there)
    the resets                    0.5 s
    relation 3, 6 cases           2.1 s together: 0.04 to 0.10 s each, 1.35 s and 0.43 s for the first two full-EM groups
    the resume, both solvers      0.2 s together
A negative control of the whole construction, run once by hand and not kept: with the windowed background operator drawing its
random words by slot instead of by id (a different counter value, never an address; whether a single-operation test sees it
was not tried: those of tests/test_gpu_gas.py that sort() first compare with the id-keyed reference and should) 9 of the
12 seeds fail: five at their first gas_exchange / gas_elastic step on a species a fused re-binning push has permuted (the
returned counts differ from the twin's), four at the first substeps at which the registered collideGasEvery is due (particles
differ from the manual loop's).  The three seeds that pass (9, 38, 149) have no operators registered and drew no gas step.  The
resets, all six group cases (at their first or second frame: collideGasEvery on ranks whose slots are not the ids) and both
resumes fail with it too."""
import struct
import time

import numpy as np
import pytest

import decomp_scene
import sequence_model as model
import test_gpu_sequences as g1

pytestmark = pytest.mark.gpu

COUNTS = ("applications", "pairs", "below", "above", "cells", "overfull_cells", "overfull_particles", "yield_hi", "yield_lo", "unit_exponent", "reactions_exact")
FAMILIES = ("collide", "pair", "force0", "force1", "gas", "fusion", "spectrum")


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def exact(x):
    """a returned value with every float as its bits and every array as its bytes: equal means bit for bit"""
    if isinstance(x, dict):
        return {k: exact(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [exact(v) for v in x]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, float):
        return struct.pack("<d", x)
    return x


def ints_of(d):
    """the exact integers of a returned dictionary as Python integers (an int64 grid as a flat list); the two words of a
    yield are left out (reactions_exact is their value)"""
    out = {}
    for k, v in d.items():
        if k in ("yield_hi", "yield_lo") or isinstance(v, bool):
            continue
        if isinstance(v, int):
            out[k] = v
        elif isinstance(v, list) and all(isinstance(x, int) for x in v):
            out[k] = list(v)
        elif isinstance(v, np.ndarray) and v.dtype == np.int64:
            out[k] = [int(x) for x in v.ravel()]
    return out


def add_ints(total, got):
    for k, v in ints_of(got).items():
        if k == "unit_exponent":
            total[k] = v
        elif isinstance(v, list):
            total[k] = [x + y for x, y in zip(total.get(k, [0] * len(v)), v)]
        else:
            total[k] = total.get(k, 0) + v


def plus(piece, have):
    total = {k: (list(v) if isinstance(v, list) else v) for k, v in piece.items()}
    add_ints(total, have)
    return total


def equal_sums(have, total):
    """every integer of `have` is the sum kept in `total` (nothing summed yet: zero)"""
    return all((k == "unit_exponent" and k not in total) or v == total.get(k, [0] * len(v) if isinstance(v, list) else 0) for k, v in have.items())


# ---------------------------------------------------------------------------------------------- the operations
def register2(sim, sc, shift=0):
    """all six families of a generation-2 scene; shift: the sub-steps a resumed run has behind it"""
    g1.register(sim, sc, shift)
    for i, kw in enumerate(sc["force_on"]):
        assert sim.forceOn(**dict(kw, epoch=kw["epoch"] + shift)) == i
    ge, fe, se = sc["gas_every"], sc["fusion_every"], sc["spectrum_every"]
    assert sim.collideGasEvery(ge["every"], ge["kind"], **dict(ge["kw"], epoch=ge["kw"]["epoch"] + shift)) == 0
    assert sim.fusionYieldEvery(fe["every"], fe["a"], fe["b"], **dict(fe["kw"], epoch=fe["kw"]["epoch"] + shift)) == 0
    assert sim.fusionSpectrumEvery(se["every"], se["a"], se["b"], **dict(se["kw"], epoch=se["kw"]["epoch"] + shift)) == 0


def apply2(sim, sc, st, files, shift=0):
    """one state-changing operation of generation 2 on a handle; what it returned.  shift: what a one-shot force adds to its
    epoch (the sub-steps the handle it is compared with has behind it and this one has not)"""
    kind = st["kind"]
    if kind.startswith("force_"):
        out = sim.force(**dict(st["kw"], epoch=st["kw"]["epoch"] + shift))
    elif kind.startswith("gas_"):
        out = sim.collideGas(st["what"], **st["kw"])
    elif kind in ("load_profile", "load_radial"):
        tables = dict(radial=st["radial"]) if kind == "load_radial" else dict(density=st["density"], thermal=st["thermal"], shear=st["shear"])
        out = sim.load(species=st["species"], first=st["first"], count=st["count"], seed=st["seed"], stream=st["stream"], lo=st["lo"], hi=st["hi"], drift=st["drift"],
                       vth=st["vth"], lattice=st["lattice"], position=st["what"] != "velocity", velocity=st["what"] != "position", **tables)
    else:
        return g1.apply(sim, sc, st, files)
    if st["precalc"]:
        sim.precalc()
    return out


def manual_substeps2(fp, b, sc, k, t, sums, due):
    """the manual equivalent of substeps(k) on a handle with the scene's operators registered, in the hook's order, from the
    test's own count t of A's sub-steps; the integers go to sums, the rows of the sub-steps where a recorder is due to `due`"""
    ce, pe, ge, fe, se, rec = sc["collide_every"], sc["pair_every"], sc["gas_every"], sc["fusion_every"], sc["spectrum_every"], sc["recorders"]
    for j in range(1, k + 1):
        b.substeps(1)
        t += 1
        for i, kw in enumerate(sc["force_on"]):      # (B has j sub-steps of its own behind it: at = j + epoch + t - j)
            add_ints(sums["force%d" % i], b.force(**dict(kw, epoch=kw["epoch"] + t - j)))
        if t % ce["every"] == 0:
            add_ints(sums["collide"], b.collide(ce["kind"], species=ce["species"], **dict(ce["kw"], epoch=t + ce["kw"]["epoch"])))
        if t % ge["every"] == 0:
            add_ints(sums["gas"], b.collideGas(ge["kind"], **dict(ge["kw"], epoch=t + ge["kw"]["epoch"])))
        if t % pe["every"] == 0:
            add_ints(sums["pair"], b.collidePair(pe["a"], pe["b"], **dict(pe["kw"], epoch=t + pe["kw"]["epoch"])))
        if t % fe["every"] == 0:
            add_ints(sums["fusion"], b.fusionYield(fe["a"], fe["b"], grid=True, **dict(fe["kw"], epoch=t + fe["kw"]["epoch"])))
        if t % se["every"] == 0:
            add_ints(sums["spectrum"], b.fusionSpectrum(se["a"], se["b"], **dict(se["kw"], epoch=t + se["kw"]["epoch"])))
        if t % rec["energy"]["every"] == 0:
            row = np.zeros(1, dtype=fp.ENERGY_DTYPE)
            row[0] = b._energy_row("global")
            row["substep"] = 0
            due["energy"].append((t, row.tobytes()))
        if t % rec["series"]["every"] == 0:
            s = rec["series"]
            got = b.series(points=s["points"], tracers=np.array(s["tracers"]), species=s["species"])
            due["series"].append((t, got["points"].tobytes() + got["tracers"].tobytes()))
        if t % rec["modes"]["every"] == 0:
            m = rec["modes"]
            due["modes"].append((t, b._modes_rows(m["modes"], m["fields"], "global")[0].tobytes()))
    return t


def stats_of(sim, pieces=None):
    """the integers of every registered family of a handle (plus the pieces a reset has taken away)"""
    out = dict(collide=ints_of(sim.collisionStats(0)), pair=ints_of(sim.pairStats(0)), force0=ints_of(sim.forceStats(0)), force1=ints_of(sim.forceStats(1)),
               gas=ints_of(sim.gasStats(0)), fusion=ints_of(dict(sim.fusionStats(0), grid=sim.fusionGrid(0))), spectrum=ints_of(sim.fusionSpectrumRead(0)))
    for key in pieces or {}:
        out[key] = plus(pieces[key], out[key])
    return out


def reset(a, pieces, where):
    """both reads with reset on A: the piece is kept, it is not all zero, and behind the copy everything is zero"""
    fusion = ints_of(dict(a.fusionStats(0), grid=a.fusionGrid(0, reset=True)))
    spectrum = ints_of(a.fusionSpectrumRead(0, reset=True))
    assert fusion["applications"] > 0 and fusion["pairs"] > 0 and fusion["reactions_exact"] == sum(fusion["grid"]) > 0, where
    assert spectrum["applications"] > 0 and spectrum["pairs"] > 0 and sum(spectrum["bins"]) + spectrum["under"] + spectrum["over"] == spectrum["reactions_exact"] > 0, where
    add_ints(pieces["fusion"], fusion)
    add_ints(pieces["spectrum"], spectrum)
    for zero in (ints_of(dict(a.fusionStats(0), grid=a.fusionGrid(0))), ints_of(a.fusionSpectrumRead(0))):
        assert all(not any(v) if isinstance(v, list) else v == 0 for k, v in zero.items() if k != "unit_exponent"), (where, "not zero behind the copy")


# ---------------------------------------------------------------------------------------------- the reads
def state_of(sim, sc, which):
    """what the references take: the stored fractions and velocities by id and the deposit's cells, read now"""
    out = [None] * len(sc["counts"])
    for sp in which:
        p = sim.getParticles(species=sp)
        out[sp] = dict(frac=p["position"], vel=p["velocity"], cell=sim.getCells(species=sp).astype(np.int64), ids=np.arange(sc["counts"][sp]))
    return out


def read2(fp, a, sc, r, files, tmp_path, rho_current, sums, pieces):
    kind = r["kind"]
    if kind in ("fusionYield", "fusionSpectrum"):
        state = state_of(a, sc, {r["a"]} | ({r["b"]} if r["b"] is not None else set()))
        if kind == "fusionYield":
            got = a.fusionYield(r["a"], r["b"], grid=True, **r["kw"])
            want = model.fusion_want(sc, state, r["a"], r["b"], r["kw"])[1]
            grid = got.pop("grid")
            assert grid.dtype == np.int64 and grid.shape == tuple(sc["shape"])[::-1]
            assert np.array_equal(grid.ravel(), want["grid"]) and int(grid.sum()) == want["reactions_exact"], (kind, int(grid.sum()), want["reactions_exact"])
        else:
            got = a.fusionSpectrum(r["a"], r["b"], **r["kw"])
            want = model.spectrum_want(sc, state, r["a"], r["b"], r["kw"])
            assert (got["bins"], got["under"], got["over"]) == (want["bins"], want["under"], want["over"]), (got["bins"], want["bins"], got["under"], want["under"])
            assert sum(got["bins"]) + got["under"] + got["over"] == got["reactions_exact"] and np.array_equal(got["edges"], want["edges"])
        assert {k: got[k] for k in COUNTS} == dict(applications=1, **{k: int(want[k]) for k in COUNTS[1:]}), (kind, {k: got[k] for k in COUNTS}, {k: int(want[k]) for k in COUNTS[1:]})
        assert got["pairs"] > 0 and got["reactions_exact"] > 0, (kind, got["pairs"])
    elif kind == "forceStats":
        assert all(equal_sums(ints_of(a.forceStats(i)), sums["force%d" % i]) for i in range(2))
    elif kind == "gasStats":
        assert equal_sums(ints_of(a.gasStats(0)), sums["gas"])
    elif kind == "fusionStats":
        assert equal_sums(plus({k: v for k, v in pieces["fusion"].items() if k != "grid"}, ints_of(a.fusionStats(0))), sums["fusion"])
    elif kind == "fusionGrid":
        assert equal_sums(plus({k: v for k, v in pieces["fusion"].items() if k == "grid"}, ints_of(dict(grid=a.fusionGrid(0)))), sums["fusion"])
    elif kind == "fusionSpectrumRead":
        assert equal_sums(plus(pieces["spectrum"], ints_of(a.fusionSpectrumRead(0))), sums["spectrum"])
    else:
        g1.read(fp, a, sc, r, files, tmp_path, rho_current)


# ---------------------------------------------------------------------------------------------- relations 1 and 2
def run_sequence2(fp, sc, steps, tmp_path, monkeypatch, control=None):
    """control: the index of the force step at which a second twin gets epoch + t + 1 and must differ"""
    if sc["staged"]:
        monkeypatch.setenv("FPIC_TWO_LEVEL_MIN", "1")
    a, c = g1.build(fp, sc), g1.build(fp, sc)
    for sim in (a, c):
        g1.start(sim, sc)
        if sc["registered"]:
            register2(sim, sc)
    if sc["registered"]:
        rec = sc["recorders"]
        a.recordEnergy(rec["energy"]["every"], rec["energy"]["capacity"])
        a.recordSeries(rec["series"]["every"], rec["series"]["capacity"], points=rec["series"]["points"], tracers=np.array(rec["series"]["tracers"]),
                       species=rec["series"]["species"])
        a.recordModes(rec["modes"]["every"], rec["modes"]["capacity"], rec["modes"]["modes"], rec["modes"]["fields"])
    sums, pieces, due = {k: {} for k in FAMILIES}, dict(fusion={}, spectrum={}), dict(energy=[], series=[], modes=[])
    files, t, controlled = [], 0, 0
    passes0 = a.stats()["sort_passes"]
    rho_current = True
    before_p, before_f = g1.particles_of(a, sc), g1.fields_of(fp, a, sc)
    for index, st in enumerate(steps):
        kind = st["kind"]
        where = "seed %d step %d %s" % (sc["seed"], index, kind)
        b = g1.twin_of(fp, sc, a, tmp_path / "twin.ckpt")
        wrong = g1.twin_of(fp, sc, a, tmp_path / "twin.ckpt") if control == index else None
        passes = a.stats()["sort_passes"]
        got_a = apply2(a, sc, st, files)
        apply2(c, sc, st, files)
        if kind == "substeps" and sc["registered"]:
            t = manual_substeps2(fp, b, sc, st["k"], t, sums, due)
            got_b = None
        else:
            got_b = apply2(b, sc, st, files, shift=t)      # (the twin is fresh: its own count is 0, A's is t)
            t += st.get("k", 0)
        assert exact(got_a) == exact(got_b), (where, got_a, got_b)
        pa, pb = g1.particles_of(a, sc), g1.particles_of(b, sc)
        for sp, (x, y) in enumerate(zip(pa, pb)):
            assert g1.bits(x["position"], y["position"]), (where, "position of species", sp, int((x["position"] != y["position"]).any(axis=1).sum()))
            assert g1.bits(x["velocity"], y["velocity"]), (where, "velocity of species", sp, int((x["velocity"] != y["velocity"]).any(axis=1).sum()))
        if wrong is not None:      # the control: the same request one sub-step later is another kick
            got_w = apply2(wrong, sc, st, files, shift=t + 1)
            assert got_w["kicked"] == got_a["kicked"] > 0 and got_w["work_fixed"] != got_a["work_fixed"], (where, got_w, got_a)
            assert not g1.same_particles(pa, g1.particles_of(wrong, sc)), (where, "epoch + t + 1 gave the same particles")
            wrong.destroy()
            controlled += 1
        face_b = model.compares_face_b(index)
        fa, fb = g1.fields_of(fp, a, sc, face_b=face_b), g1.fields_of(fp, b, sc, face_b=face_b)
        fresh = g1.deposits(sc, st) | ({"rho"} if sc["solver"] == "yee" else set())
        for name in fa:
            if name in ("rho", "J") and name not in fresh:
                assert fa[name] == before_f[name], (where, name, "written by an operation that deposits nothing")
            else:
                assert fa[name] == fb[name], (where, name)
        b.destroy()
        # the operation did something: A's bytes moved, or it returned a positive count
        moved = not g1.same_particles(pa, before_p) or any(fa[name] != before_f[name] for name in fa if name in before_f)
        if kind.startswith("force_"):
            assert st["t"] == t, (where, st["t"], t)
            if st["active"]:
                assert got_a["applications"] == 1 and got_a["kicked"] > 0 and not g1.same_particles(pa, before_p), (where, got_a)
            else:
                assert got_a["applications"] == 0 and got_a["kicked"] == 0 and got_a["work_fixed"] == 0 and g1.same_particles(pa, before_p), (where, got_a)
        elif kind.startswith("gas_"):
            assert got_a["applications"] == 1 and 0 < got_a["collided"] <= got_a["candidates"] and not g1.same_particles(pa, before_p), (where, got_a)
        elif kind in ("load_profile", "load_radial"):
            assert got_a == st["count"] and not g1.same_particles(pa, before_p), (where, got_a)
        else:
            counted = bool(got_a) and (got_a if isinstance(got_a, int) else max(got_a.get("collided", 0), got_a.get("pairs", 0))) > 0
            assert moved or counted or (kind == "sort" and a.stats()["sort_passes"] > passes), where
            if kind.startswith("collide_") or kind.startswith("pair_"):
                assert counted and moved, (where, got_a)
        before_p, before_f = pa, fa
        if g1.deposits(sc, st) & {"rho"}:
            rho_current = True
        elif (kind in model.POSITION_KINDS2 and st["what"] != "velocity") or kind == "loadCheckpoint" or sc["solver"] == "yee":
            rho_current = False
        for r in st["reads"]:
            read2(fp, a, sc, r, files, tmp_path, rho_current and sc["solver"] != "yee", sums, pieces)
        if st.get("reset"):
            reset(a, pieces, where)
        if index == len(steps) // 2:      # the midpoint: C's lattice step stays open (no density(), no B of the integer time)
            assert g1.same_particles(g1.particles_of(a, sc), g1.particles_of(c, sc)), (where, "A and C")
            fa, fc = g1.fields_of(fp, a, sc, density=False, face_b=False), g1.fields_of(fp, c, sc, density=False, face_b=False)
            assert all(fa[name] == fc[name] for name in fa if not (name == "rho" and sc["solver"] == "yee")), (where, "fields of A and C")
    # the end: A, read and saved and copied (and drained) all the way, is C, which was not
    assert g1.same_particles(g1.particles_of(a, sc), g1.particles_of(c, sc)), (sc["seed"], "A and C at the end")
    fa, fc = g1.fields_of(fp, a, sc), g1.fields_of(fp, c, sc)
    assert all(fa[name] == fc[name] for name in fa), (sc["seed"], "fields of A and C at the end")
    assert a.stats()["sort_passes"] > passes0 and controlled == (control is not None)
    if sc["registered"]:
        have, theirs = stats_of(a, pieces), stats_of(c)
        for key in FAMILIES:
            assert equal_sums(have[key], sums[key]) and have[key] == theirs[key], (sc["seed"], key, {k: v for k, v in have[key].items() if k != "grid"}, {k: v for k, v in sums[key].items() if k != "grid"})
        if not pieces["fusion"]:      # (nothing was drained: the whole dictionaries, derived floats as bits)
            for call in ("forceStats", "gasStats", "fusionStats", "fusionSpectrumRead", "fusionGrid"):
                assert exact(getattr(a, call)(0)) == exact(getattr(c, call)(0)), (sc["seed"], call)
            assert exact(a.forceStats(1)) == exact(c.forceStats(1))
        lo, hi = sc["force_window"]
        assert sums["force0"]["applications"] == hi - lo + 1 and sums["force1"]["applications"] == t, (sums["force0"]["applications"], sums["force1"]["applications"], t)
        assert sums["collide"]["collided"] > 0 and sums["pair"]["pairs"] > 0 and sums["force0"]["kicked"] > 0 and sums["force1"]["kicked"] > 0
        assert sums["gas"]["collided"] > 0 and sums["fusion"]["reactions_exact"] == sum(sums["fusion"]["grid"]) > 0 and sum(sums["spectrum"]["bins"]) > 0
        assert all(sums[key]["applications"] == t // sc[key + "_every"]["every"] >= 3 for key in ("collide", "pair", "gas", "fusion", "spectrum"))
        rec = sc["recorders"]
        erows, edropped = a.energyHistory()
        hist, sdropped = a.seriesHistory()
        msub, mout, _, mdropped = a._modes_history_rows("global")
        erows = erows.copy()
        labels = dict(energy=[int(x) for x in erows["substep"]], series=hist["substep"].tolist(), modes=msub.tolist())
        erows["substep"] = 0
        rows = dict(energy=[erows[i:i + 1].tobytes() for i in range(len(erows))],
                    series=[hist["points"][i].tobytes() + hist["tracers"][i].tobytes() for i in range(len(hist["substep"]))],
                    modes=[mout[i].tobytes() for i in range(len(msub))])
        for name, dropped in (("energy", edropped), ("series", sdropped), ("modes", mdropped)):
            cap = rec[name]["capacity"]
            assert dropped == len(due[name]) - cap > 0, (name, dropped, len(due[name]))
            assert labels[name] == [tt for tt, _ in due[name][-cap:]], (name, labels[name])
            assert rows[name] == [row for _, row in due[name][-cap:]], (sc["seed"], name)      # (the rows see the kicked, gas-collided state)
            assert len(set(rows[name])) == cap
    a.destroy()
    c.destroy()
    return pieces


@pytest.mark.parametrize("seed", model.SEEDS2)
def test_generation_2_any_state_against_a_fresh_twin_and_reading_changes_nothing(fp, tmp_path, monkeypatch, seed):
    t0 = time.perf_counter()
    control_seed, control_index = model.epoch_control()
    run_sequence2(fp, model.scene2(seed), model.sequence2(seed), tmp_path, monkeypatch, control=control_index if seed == control_seed else None)
    print("generation 2 seed %d: %.2f s" % (seed, time.perf_counter() - t0))


def test_the_resets_zero_behind_the_copy(fp, tmp_path, monkeypatch):
    """the named sequence `resets` under relations 1 and 2: what A drained in three pieces and holds at the end adds up to
    what the manual loop returned and to what C, which never resets, reads (run_sequence2's last comparison)"""
    t0 = time.perf_counter()
    sc, steps = model.NAMED2["resets"]()
    pieces = run_sequence2(fp, sc, steps, tmp_path, monkeypatch)
    assert pieces["fusion"]["applications"] == pieces["spectrum"]["applications"] == model.substeps_of(steps[:[i for i, st in enumerate(steps) if st.get("reset")][-1]])
    print("named resets: %.2f s" % (time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------- relation 3: the decomposition
@pytest.mark.parametrize("index", range(len(model.GROUP_CASES)))
def test_a_decomposition_under_the_generation_2_sequence(fp, monkeypatch, index):
    t0 = time.perf_counter()
    case, steps = model.group_case2(index), model.group_sequence2(index)
    if case["staged"]:
        monkeypatch.setenv("FPIC_TWO_LEVEL_MIN", "1")
    sc = decomp_scene.build(fp, case)
    n, world = sc["n"], sc["world"]
    one = fp.makeCylindricalParticlePusher(sc["spec"], precision=sc["precision"])
    one.set(position=sc["pos"], velocity=sc["vel"])
    ranks = []
    for r in range(world):
        s = fp.makeCylindricalParticlePusher(dict(sc["spec"], count=3 * n), precision=sc["precision"])
        s.domainInit(r, world, ghost_planes=sc["G"], migrate_every=sc["every"], distributed_solve=sc["dist_solve"])
        first = int(sc["counts"][:r].sum())
        s.domainSet(sc["pos"][first:first + sc["counts"][r]], sc["vel"][first:first + sc["counts"][r]], first_id=first)
        ranks.append(s)
    group = fp.BoxGroup(ranks)
    if sc["em"]:
        for s in ranks + [one]:
            s.addB(0.0, 0.0, 0.01)
    one.precalc()
    group.precalc()
    ce, fo, ge = case["collide_every"], case["force_on"], case["gas_every"]
    assert one.collideEvery(ce["every"], ce["kind"], **ce["kw"]) == group.collideEvery(ce["every"], ce["kind"], **ce["kw"]) == 0
    assert one.forceOn(**fo) == group.forceOn(**fo) == 0
    assert one.collideGasEvery(ge["every"], ge["kind"], **ge["kw"]) == group.collideGasEvery(ge["every"], ge["kind"], **ge["kw"]) == 0
    tally = dict(sigma=model.fusion_table(), g_lo=model.FUSION_G[0], g_hi=model.FUSION_G[1])
    spectrum = dict(tally, axis="cm", bins=7, lo=0.0, hi=1e-15)
    refused = 0
    before = g1.gathered(ranks)
    for i, st in enumerate(steps):
        where = "case %d step %d %s" % (index, i, st["kind"])
        kind = st["kind"]
        if kind == "step":
            one.step()
            group.step()
        elif kind.startswith("force_"):
            x, y = one.force(**st["kw"]), group.force(**st["kw"])
            assert exact(x) == exact(y) and x["applications"] == 1 and x["kicked"] > 0, (where, x, y)
        elif kind.startswith("gas_"):
            x, y = one.collideGas(st["what"], **st["kw"]), group.collideGas(st["what"], **st["kw"])
            assert exact(x) == exact(y) and x["collided"] > 0, (where, x, y)
        elif kind.startswith("reload_"):
            assert one.load(**st["population"]) == n == sum(group.load(**st["population"])), where
            one.precalc()
            group.precalc()
        elif kind == "fusion_refused":
            held = g1.gathered(ranks)
            for owner in (group, ranks[0]):
                for call in (lambda: owner.fusionYield(0, **tally), lambda: owner.fusionYieldEvery(1, 0, **tally),
                             lambda: owner.fusionSpectrum(0, **spectrum), lambda: owner.fusionSpectrumEvery(1, 0, **spectrum)):
                    with pytest.raises(fp.FusionPicError, match="cannot pair a cell alone") as e:
                        call()
                    assert e.value.code == -5 and "needs an undecomposed handle" in str(e.value)
            assert all(g1.bits(x, y) for x, y in zip(held, g1.gathered(ranks))), where
            refused += 1
        else:
            raise AssertionError(kind)
        ids, pos, vel = g1.gathered(ranks)
        want = one.getParticles()
        assert np.array_equal(ids, np.arange(n)), where
        assert g1.bits(pos, want["position"]), (where, int((pos != want["position"]).any(axis=1).sum()))
        assert g1.bits(vel, want["velocity"]), (where, int((vel != want["velocity"]).any(axis=1).sum()))
        assert one.collisionStats(0) == group.collisionStats(0), where
        assert exact(one.forceStats(0)) == exact(group.forceStats(0)) and exact(one.gasStats(0)) == exact(group.gasStats(0)), (where, one.forceStats(0), group.forceStats(0))
        # the operation did something (a vacuous equality cannot pass): every operation but the refusal moves velocities
        assert g1.bits(vel, before[2]) == (kind == "fusion_refused") and (kind != "step" and not kind.startswith("reload_") or not g1.bits(pos, before[1])), where
        before = (ids, pos, vel)
        for r in st["reads"]:
            g1.group_read(one, group, r)
    stats = [s.domainStats() for s in ranks]
    assert refused == 1 and sum(s["migrated"] for s in stats) > 0 and sum(s["lost"] for s in stats) == 0
    assert one.collisionStats(0)["collided"] > 0 and one.forceStats(0)["kicked"] > 0 and one.gasStats(0)["collided"] > 0
    assert 0 < one.forceStats(0)["applications"] == 8 and one.gasStats(0)["applications"] > 0
    for s in ranks + [one]:
        s.destroy()
    print("generation 2 group case %d: %.2f s" % (index, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------- the resume
@pytest.mark.parametrize("solver,precision", model.RESUME)
def test_a_run_with_all_six_families_registered_resumes_bit_for_bit(fp, tmp_path, solver, precision):
    """N sub-steps with all six families registered (the periods divide the cut t, a force envelope lies across it); the same
    run cut after t sub-steps, saved, loaded into a fresh handle on which everything is registered with epoch + t, and run for
    N - t: the same particles and fields, and every tally of the two parts adds up to the whole run's as exact integers."""
    t0 = time.perf_counter()
    sc = model.resume_scene2(solver, precision)
    t, n = model.RESUME_T, model.RESUME_N
    whole, first, rest = g1.build(fp, sc), g1.build(fp, sc), g1.build(fp, sc)
    for sim in (whole, first):
        g1.start(sim, sc)
        register2(sim, sc)
    whole.substeps(n)
    first.substeps(t)
    first.saveCheckpoint(tmp_path / "cut.ckpt")
    rest.loadCheckpoint(tmp_path / "cut.ckpt")
    register2(rest, sc, shift=t)
    rest.substeps(n - t)
    assert g1.same_particles(g1.particles_of(whole, sc), g1.particles_of(rest, sc))
    fw, fr = g1.fields_of(fp, whole, sc), g1.fields_of(fp, rest, sc)
    assert all(fw[name] == fr[name] for name in fw), [name for name in fw if fw[name] != fr[name]]
    assert not g1.same_particles(g1.particles_of(first, sc), g1.particles_of(rest, sc))
    # (the comparison has teeth: the same resumption with the epochs off by one sub-step is another run)
    wrong = g1.build(fp, sc)
    wrong.loadCheckpoint(tmp_path / "cut.ckpt")
    register2(wrong, sc, shift=t + 1)
    wrong.substeps(n - t)
    assert not g1.same_particles(g1.particles_of(whole, sc), g1.particles_of(wrong, sc))
    wrong.destroy()
    parts, total = [stats_of(first), stats_of(rest)], stats_of(whole)
    for key in FAMILIES:
        assert plus(parts[0][key], parts[1][key]) == total[key], (key, {k: v for k, v in total[key].items() if k != "grid"})
    lo, hi = sc["force_window"]
    assert (parts[0]["force0"]["applications"], parts[1]["force0"]["applications"], total["force1"]["applications"]) == (t - lo + 1, hi - t, n)
    every = model.RESUME2_EVERY
    assert all(total[key]["applications"] == n // every[key] for key in every)
    for part in parts + [total]:
        assert part["force0"]["kicked"] > 0 and part["force1"]["kicked"] > 0 and part["gas"]["collided"] > 0 and part["collide"]["collided"] > 0 and part["pair"]["pairs"] > 0
        assert part["fusion"]["reactions_exact"] == sum(part["fusion"]["grid"]) > 0 and sum(part["spectrum"]["bins"]) > 0
    for sim in (whole, first, rest):
        sim.destroy()
    print("generation 2 resume %s %s: %.2f s" % (solver, precision, time.perf_counter() - t0))
