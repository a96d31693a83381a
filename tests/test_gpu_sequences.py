"""Random call sequences on the CART3D box (tests/sequence_model.py turns a seed into a scene and a list of operations; tests/
test_sequence_model.py proves on the CPU that the committed seeds reach the states meant here).  Everything below is equality
bit for bit: no tolerance anywhere.

The chain of trust.  The reference tests of the suite (tests/*_reference.py and their GPU tests) prove every operation on a
handle in the PLAIN state — a fresh handle, slot = id, nothing binned, no census, no re-binning pending, the lattice step
closed.  Relation 1 adds "whatever state the handle is in": before every state-changing operation of a sequence a twin B in
the plain state is filled from A.saveCheckpoint() (raw state in the caller's order: the copy is exact), both get the
operation, and every particle by id, the fields and the returned counts must agree.  With operators registered on A, B gets
the manual loop of test_registered_equals_manual (substeps(1), the background operator with epoch = t + spec.epoch, the pair
operator), and the rows B shows at the sub-steps where A's recorders are due are A's three histories at the end.
Relation 2: a handle C gets the state-changing operations and nothing else; A, which is read, saved and copied all the time,
equals it at the midpoint and at the end — the reading calls (and saveCheckpoint's closing of an open lattice step) change
nothing.  The reads that return exact integers are held to the numpy references over A.getParticles() read just before.
Relation 3: a BoxGroup of 2 and of 3 in-process ranks against one handle under one sequence.
The resume: a run with registered operators, cut at a common multiple of their periods, continues bit for bit.

What a checkpoint does not carry is compared accordingly: the integer charge grid (and, full EM, the current grid) of the twin
is the deposit of its own last sub-step or precalc(), so after an operation that deposits nothing those grids of A must be
what they were before it; under full EM density() on both handles comes first, as in
test_box_checkpoint_resume_is_bit_identical.

The group's list.  Nothing of the issue's list is refused on a group except the binary collisions, which stay refused
("... needs an undecomposed handle: between two migrations the particles of a cell can sit on two ranks (in the ghost planes),
so a rank cannot pair a cell alone"): asserted once inside every sequence, with nothing changed.  distributed_solve = 1 is
documented as bit-identical on power-of-two grids only, so those cases run on 16 x 8 x 16 and on two ranks; full EM needs
slabs of 8 planes for 2 ghost planes, so its cases have nz = 16 or 24.  group.energy() adds the ranks' rounded doubles: its
integer part (count) and speed_max are compared.

Wall times on an MI355X, one run of the module on its own (in the run of the whole suite, where the transform library and
the kernels are loaded already, the first family took 8.3 s):
    relations 1 + 2, 12 seeds     11.5 s together: 0.5 to 0.8 s each, 2.2 s for the first electrostatic and the first full-EM seed
                                  of the process (the transform library and the code objects are loaded there)
    the named sequence            0.6 s
    relation 3, 6 cases           1.9 s together: 0.02 to 0.07 s each, 1.3 s and 0.4 s for the first two full-EM groups
    the resume, both solvers      0.2 s together
A negative control of the whole construction, run once by hand and not kept: with the velocity upload writing by slot instead
of by id (in bounds, and invisible to every single-operation test, which uploads before the first binning), all 12 seeds fail
at their first set / setRange of velocities on a binned species."""
import time

import numpy as np
import pytest

import decomp_scene
import histogram_reference as hr
import moments_reference as mref
import select_reference as sref
import sequence_model as model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- handles of a scene
def build(fp, sc):
    sim = fp.makeCylindricalParticlePusher(sc["spec"], precision=sc["precision"], sort_interval=sc["sort_interval"])
    for sp in range(1, len(sc["counts"])):
        assert sim.addSpecies(sc["masses"][sp], sc["charges"][sp], sc["counts"][sp]) == sp
    return sim


def start(sim, sc):
    for sp, n in enumerate(sc["counts"]):
        pos, vel = model.particles(sc["seed"], 1000 + sp, n)
        sim.set(position=pos, velocity=vel, species=sp)
    if sc["solver"] == "none":
        sim.set(E=model.given_field(sc["seed"]))
    if sc["addB"]:
        sim.addB(*sc["addB"])
    sim.precalc()


def register(sim, sc, shift=0):
    """the registered operators of a scene; shift: the sub-steps a resumed run has behind it"""
    ce, pe = sc["collide_every"], sc["pair_every"]
    assert sim.collideEvery(ce["every"], ce["kind"], species=ce["species"], **dict(ce["kw"], epoch=ce["kw"]["epoch"] + shift)) == 0
    assert sim.collidePairEvery(pe["every"], pe["a"], pe["b"], **dict(pe["kw"], epoch=pe["kw"]["epoch"] + shift)) == 0


def twin_of(fp, sc, a, path):
    a.saveCheckpoint(path)
    b = build(fp, sc)
    b.loadCheckpoint(path)
    return b


def particles_of(sim, sc):
    return [sim.getParticles(species=sp) for sp in range(len(sc["counts"]))]


def fields_of(fp, sim, sc, density=True, face_b=True):
    """the fields as bytes.  Full EM: density() first unless density=False (the charge grid of the current positions);
    face_b=False leaves an open chained lattice step open (B of the integer time is not asked for)"""
    yee = sc["solver"] == "yee"
    if yee and density:
        sim.density()
    which = [("E", fp.F3_E), ("rho", fp.F3_RHO_FIXED)]
    if yee:
        which += [("edge_E", fp.F3_EDGE_E), ("J", fp.F3_J_FIXED)] + ([("face_B", fp.F3_FACE_B)] if face_b else [])
    return {name: sim.readField(w).tobytes() for name, w in which}


def same_particles(pa, pb):
    return all(bits(x["position"], y["position"]) and bits(x["velocity"], y["velocity"]) for x, y in zip(pa, pb))


def add_counts(total, got):
    for key, v in got.items():
        total[key] = total.get(key, 0) + v


# ---------------------------------------------------------------------------------------------- the operations
def apply(sim, sc, st, files):
    """one state-changing operation of the model on a handle; what it returned"""
    kind, out = st["kind"], None
    if kind == "substeps":
        sim.substeps(st["k"])
    elif kind == "sort":
        sim.sort()
    elif kind in ("set", "setRange"):
        n = sc["counts"][st["species"]] if kind == "set" else st["count"]
        pos, vel = model.particles(sc["seed"], st["tag"], n)
        kw = dict(position=pos if st["what"] != "velocity" else None, velocity=vel if st["what"] != "position" else None)
        if kind == "set":
            sim.set(species=st["species"], **kw)
        else:
            sim.setRange(st["first"], species=st["species"], **kw)
    elif kind == "load":
        out = sim.load(species=st["species"], first=st["first"], count=st["count"], seed=st["seed"], stream=st["stream"], lo=st["lo"], hi=st["hi"],
                       drift=st["drift"], vth=st["vth"], lattice=st["lattice"], paired=st["paired"], position=st["what"] != "velocity",
                       velocity=st["what"] != "position")
    elif kind.startswith("collide_"):
        out = sim.collide(st["what"], **st["kw"])
    elif kind.startswith("pair_"):
        out = sim.collidePair(st["a"], st["b"], **st["kw"])
    elif kind == "loadCheckpoint":
        sim.loadCheckpoint(files[st["file"]])
    else:
        raise AssertionError(kind)
    if st["precalc"]:
        sim.precalc()
    return out


def deposits(sc, st):
    """the grids an operation writes afresh (a twin's other grids are those of a fresh handle)"""
    if st["precalc"]:
        return {"rho"}
    if st["kind"] == "substeps":
        return {"J"} if sc["solver"] == "yee" else {"rho"}
    return set()


def manual_substeps(fp, b, sc, k, t, sums, due):
    """the manual equivalent of substeps(k) on a handle with the scene's operators registered, from the test's own count t of
    A's sub-steps; the counts go to sums, the rows of the sub-steps where a recorder is due to `due`"""
    ce, pe, rec = sc["collide_every"], sc["pair_every"], sc["recorders"]
    for _ in range(k):
        b.substeps(1)
        t += 1
        if t % ce["every"] == 0:
            add_counts(sums["collide"], b.collide(ce["kind"], species=ce["species"], **dict(ce["kw"], epoch=t + ce["kw"]["epoch"])))
        if t % pe["every"] == 0:
            add_counts(sums["pair"], b.collidePair(pe["a"], pe["b"], **dict(pe["kw"], epoch=t + pe["kw"]["epoch"])))
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


# ---------------------------------------------------------------------------------------------- the reads
def read(fp, a, sc, r, files, tmp_path, rho_current):
    """one reading call on A; those that return exact integers against the numpy references over A.getParticles()"""
    kind, sp = r["kind"], r["species"]
    shape = sc["shape"]
    if kind == "saveCheckpoint":
        path = tmp_path / ("saved%d.ckpt" % r["file"])
        a.saveCheckpoint(path)
        assert len(files) == r["file"]
        files.append(path)
        return
    p = a.getParticles(species=sp)
    n = sc["counts"][sp]
    ids = np.arange(n, dtype=np.uint32)
    if kind == "getParticles":
        assert p["position"].shape == (n, 3) and np.all((p["position"] >= 0) & (p["position"] < 1))
    elif kind == "getRange":
        got = a.getRange(r["first"], r["count"], r["stride"], species=sp)
        rows = r["first"] + r["stride"] * np.arange(r["count"])
        assert bits(got["position"], p["position"][rows]) and bits(got["velocity"], p["velocity"][rows])
    elif kind == "getCells":
        cells = a.getCells(species=sp)
        assert bits(cells, a.getRange(0, n, 1, species=sp, cells=True)["cells"]) and cells.min() >= 0 and cells.max() < np.prod(shape)
    elif kind == "count":
        assert a.count(r["where"], species=sp, every=r["every"]) == sref.count(ids, p["position"], p["velocity"], r["where"], r["every"])
    elif kind == "select":
        got, want = a.select(r["where"], species=sp, every=r["every"]), sref.select(ids, p["position"], p["velocity"], r["where"], r["every"])
        assert got["matched"] == want["matched"] and bits(got["ids"], want["ids"])
        assert bits(got["position"], want["position"]) and bits(got["velocity"], want["velocity"])
    elif kind in ("histogram_lds", "histogram_global"):
        got = a.histogram(r["axes"], r["bins"], r["ranges"], species=sp)
        want, outside = hr.histogram(p["position"], p["velocity"], r["axes"], r["bins"], r["ranges"])
        assert got["outside"] == outside and np.array_equal(got["counts"], want) and int(want.sum()) + outside == n
    elif kind == "moments":
        got = a.moments(r["which"], species=sp)
        want, rejected = mref.moments(p["position"], p["velocity"], shape, r["which"])
        assert got["rejected"] == rejected == 0
        for name in ("N", "FX", "FY", "FZ"):
            assert np.array_equal(got[name], want[name]), name
        if rho_current:      # the charge grid is the deposit of these positions: the sum over the species of Z N, bit for bit
            total = np.zeros_like(got["N"])
            for s2 in range(len(sc["counts"])):
                total += int(round(sc["charges"][s2] / sc["charges"][0])) * a.moments("n", species=s2)["N"]
            assert np.array_equal(total, a.readField(fp.F3_RHO_FIXED).reshape(total.shape))
    elif kind == "energy":
        e = a.energy()
        assert e["count"].tolist() == sc["counts"] and np.all(e["kinetic"] > 0)
    elif kind == "series":
        tr = np.array(r["tracers"])
        got = a.series(points=r["points"], tracers=tr, species=sp)
        want = np.concatenate([p["position"][tr], p["velocity"][tr]], axis=1).astype(np.float64)
        assert bits(np.ascontiguousarray(got["tracers"][:, :6]), want) and np.all(got["tracers"][:, 6] == 1) and np.all(np.isfinite(got["points"]))
    elif kind == "modes":
        got = a.modes(r["modes"], r["fields"])
        assert all(np.all(np.isfinite(got[f])) for f in r["fields"])
    elif kind == "readField":
        e = a.readField(fp.F3_E)
        assert e.shape == (np.prod(shape), 4) and np.all(np.isfinite(e))
        if sc["solver"] == "yee":
            assert np.all(np.isfinite(a.readField(fp.F3_FACE_B)))       # (forms B of the integer time: closes an open lattice step)
        charge = int(a.readField(fp.F3_RHO_FIXED).astype(object).sum())
        if rho_current:
            assert charge == sum(int(round(sc["charges"][s2] / sc["charges"][0])) * sc["counts"][s2] for s2 in range(len(sc["counts"]))) << 42
    else:
        raise AssertionError(kind)


# ---------------------------------------------------------------------------------------------- relations 1 and 2
def run_sequence(fp, sc, steps, tmp_path, monkeypatch):
    if sc["staged"]:
        monkeypatch.setenv("FPIC_TWO_LEVEL_MIN", "1")
    a, c = build(fp, sc), build(fp, sc)
    for sim in (a, c):
        start(sim, sc)
        if sc["registered"]:
            register(sim, sc)
    if sc["registered"]:
        rec = sc["recorders"]
        a.recordEnergy(rec["energy"]["every"], rec["energy"]["capacity"])
        a.recordSeries(rec["series"]["every"], rec["series"]["capacity"], points=rec["series"]["points"], tracers=np.array(rec["series"]["tracers"]),
                       species=rec["series"]["species"])
        a.recordModes(rec["modes"]["every"], rec["modes"]["capacity"], rec["modes"]["modes"], rec["modes"]["fields"])
    sums, due = dict(collide={}, pair={}), dict(energy=[], series=[], modes=[])
    files, t = [], 0
    passes0 = a.stats()["sort_passes"]
    rho_current = True          # precalc() has deposited the charge of these positions
    before_p, before_f = particles_of(a, sc), fields_of(fp, a, sc)
    for index, st in enumerate(steps):
        where = "seed %d step %d %s" % (sc["seed"], index, st["kind"])
        b = twin_of(fp, sc, a, tmp_path / "twin.ckpt")
        passes = a.stats()["sort_passes"]
        got_a = apply(a, sc, st, files)
        apply(c, sc, st, files)
        if st["kind"] == "substeps" and sc["registered"]:
            t = manual_substeps(fp, b, sc, st["k"], t, sums, due)
            got_b = None
        else:
            got_b = apply(b, sc, st, files)
            t += st.get("k", 0)
        assert got_a == got_b, (where, got_a, got_b)
        pa, pb = particles_of(a, sc), particles_of(b, sc)
        for sp, (x, y) in enumerate(zip(pa, pb)):
            assert bits(x["position"], y["position"]), (where, "position of species", sp, int((x["position"] != y["position"]).any(axis=1).sum()))
            assert bits(x["velocity"], y["velocity"]), (where, "velocity of species", sp, int((x["velocity"] != y["velocity"]).any(axis=1).sum()))
        face_b = model.compares_face_b(index)        # (every other step leaves A's chained lattice step open for what follows)
        fa, fb = fields_of(fp, a, sc, face_b=face_b), fields_of(fp, b, sc, face_b=face_b)
        fresh = deposits(sc, st) | ({"rho"} if sc["solver"] == "yee" else set())      # (full EM: density() came first on both)
        for name in fa:
            if name in ("rho", "J") and name not in fresh:
                assert fa[name] == before_f[name], (where, name, "written by an operation that deposits nothing")
            else:
                assert fa[name] == fb[name], (where, name)
        b.destroy()
        # the operation did something: A's bytes moved, or it returned a positive count
        moved = not same_particles(pa, before_p) or any(fa[name] != before_f[name] for name in fa if name in before_f)
        counted = bool(got_a) and (got_a if isinstance(got_a, int) else max(got_a.get("collided", 0), got_a.get("pairs", 0))) > 0
        assert moved or counted or (st["kind"] == "sort" and a.stats()["sort_passes"] > passes), where
        if st["kind"].startswith("collide_") or st["kind"].startswith("pair_"):
            assert counted and moved, (where, got_a)
        if st.get("expect_sort_pass"):      # (precalc() binned: the other species' re-binning is pending now)
            assert a.stats()["sort_passes"] > passes, where
        before_p, before_f = pa, fa
        if deposits(sc, st) & {"rho"}:
            rho_current = True
        elif (st["kind"] in model.POSITION_KINDS and st["what"] != "velocity") or st["kind"] == "loadCheckpoint" or sc["solver"] == "yee":
            rho_current = False
        for r in st["reads"]:
            read(fp, a, sc, r, files, tmp_path, rho_current and sc["solver"] != "yee")
        if index == len(steps) // 2:      # the midpoint: C's lattice step stays open (no density(), no B of the integer time)
            assert same_particles(particles_of(a, sc), particles_of(c, sc)), (where, "A and C")
            fa, fc = fields_of(fp, a, sc, density=False, face_b=False), fields_of(fp, c, sc, density=False, face_b=False)
            assert all(fa[name] == fc[name] for name in fa if not (name == "rho" and sc["solver"] == "yee")), (where, "fields of A and C")
    # the end: A, read and saved and copied all the way, is C, which was not
    assert same_particles(particles_of(a, sc), particles_of(c, sc)), (sc["seed"], "A and C at the end")
    fa, fc = fields_of(fp, a, sc), fields_of(fp, c, sc)
    assert all(fa[name] == fc[name] for name in fa), (sc["seed"], "fields of A and C at the end")
    assert a.stats()["sort_passes"] > passes0
    if sc["registered"]:
        assert a.collisionStats(0) == sums["collide"] == c.collisionStats(0) and a.pairStats(0) == sums["pair"] == c.pairStats(0)
        assert sums["collide"]["collided"] > 0 and sums["pair"]["pairs"] > 0
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
            assert dropped == len(due[name]) - cap > 0, (name, dropped, len(due[name]))           # the ring wrapped
            assert labels[name] == [tt for tt, _ in due[name][-cap:]], (name, labels[name])
            assert rows[name] == [row for _, row in due[name][-cap:]], (sc["seed"], name)
            assert len(set(rows[name])) == cap                                                  # (a row in the wrong slot would show)
    a.destroy()
    c.destroy()


@pytest.mark.parametrize("seed", model.SEEDS)
def test_any_state_against_a_fresh_twin_and_reading_changes_nothing(fp, tmp_path, monkeypatch, seed):
    t0 = time.perf_counter()
    run_sequence(fp, model.scene(seed), model.sequence(seed), tmp_path, monkeypatch)
    print("seed %d: %.2f s" % (seed, time.perf_counter() - t0))


@pytest.mark.parametrize("name", sorted(model.NAMED))
def test_named_sequence(fp, tmp_path, monkeypatch, name):
    """the written-out sequences of tests/sequence_model.py (NAMED), under relations 1 and 2"""
    t0 = time.perf_counter()
    sc, steps = model.NAMED[name]()
    run_sequence(fp, sc, steps, tmp_path, monkeypatch)
    print("named %s: %.2f s" % (name, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------- relation 3: the decomposition
def gathered(ranks):
    parts = [s.domainGet() for s in ranks]
    ids = np.concatenate([p["ids"] for p in parts])
    order = np.argsort(ids, kind="stable")
    return ids[order], np.concatenate([p["position"] for p in parts])[order], np.concatenate([p["velocity"] for p in parts])[order]


def group_read(one, group, r):
    kind = r["kind"]
    if kind == "count":
        assert one.count(r["where"], every=r["every"]) == group.count(r["where"], every=r["every"])
    elif kind == "select":
        x, y = one.select(r["where"], every=r["every"]), group.select(r["where"], every=r["every"])
        assert x["matched"] == y["matched"] == sum(y["matched_members"]) and bits(x["ids"], y["ids"])
        assert bits(x["position"], y["position"]) and bits(x["velocity"], y["velocity"])
    elif kind == "histogram":
        x, y = one.histogram(r["axes"], r["bins"], r["ranges"]), group.histogram(r["axes"], r["bins"], r["ranges"])
        assert x["outside"] == y["outside"] and np.array_equal(x["counts"], y["counts"]) and int(x["counts"].sum()) > 0
    elif kind == "moments":
        x, y = one.moments(r["which"]), group.moments(r["which"])
        assert x["rejected"] == y["rejected"] == 0 and all(np.array_equal(x[k], y[k]) for k in ("N", "FX", "FY", "FZ"))
    elif kind == "energy":
        x, y = one.energy(), group.energy()
        assert x["count"].tolist() == y["count"].tolist() and bits(x["speed_max"], y["speed_max"])
    else:
        raise AssertionError(kind)


@pytest.mark.parametrize("index", range(len(model.GROUP_CASES)))
def test_a_decomposition_under_the_same_sequence(fp, monkeypatch, index):
    t0 = time.perf_counter()
    case, steps = model.group_case(index), model.group_sequence(index)
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
    ce = case["collide_every"]
    assert one.collideEvery(ce["every"], ce["kind"], **ce["kw"]) == group.collideEvery(ce["every"], ce["kind"], **ce["kw"]) == 0
    refused = 0
    before = gathered(ranks)
    for i, st in enumerate(steps):
        where = "case %d step %d %s" % (index, i, st["kind"])
        kind = st["kind"]
        if kind == "step":
            one.step()
            group.step()
        elif kind.startswith("collide_"):
            x, y = one.collide(st["what"], **st["kw"]), group.collide(st["what"], **st["kw"])
            assert x == y and x["collided"] > 0, (where, x, y)
        elif kind == "reload":
            assert one.load(**st["population"]) == n == sum(group.load(**st["population"])), where
            one.precalc()
            group.precalc()
        elif kind == "pair_refused":
            held = gathered(ranks)
            for owner in (group, ranks[0]):
                for call in (lambda: owner.collidePair(0, log_lambda=10.0), lambda: owner.collidePairEvery(1, 0, log_lambda=10.0)):
                    with pytest.raises(fp.FusionPicError, match="cannot pair a cell alone") as e:
                        call()
                    assert e.value.code == -5 and "needs an undecomposed handle" in str(e.value)
            assert all(bits(x, y) for x, y in zip(held, gathered(ranks))), where
            refused += 1
        else:
            raise AssertionError(kind)
        ids, pos, vel = gathered(ranks)
        want = one.getParticles()
        assert np.array_equal(ids, np.arange(n)), where
        assert bits(pos, want["position"]), (where, int((pos != want["position"]).any(axis=1).sum()))
        assert bits(vel, want["velocity"]), (where, int((vel != want["velocity"]).any(axis=1).sum()))
        assert one.collisionStats(0) == group.collisionStats(0), where
        # the operation did something (a vacuous equality cannot pass): every operation but the refusal moves velocities
        assert bits(vel, before[2]) == (kind == "pair_refused") and (kind not in ("step", "reload") or not bits(pos, before[1])), where
        before = (ids, pos, vel)
        for r in st["reads"]:
            group_read(one, group, r)
    stats = [s.domainStats() for s in ranks]
    assert refused == 1 and sum(s["migrated"] for s in stats) > 0 and sum(s["lost"] for s in stats) == 0
    assert one.collisionStats(0)["applications"] > 0 and one.collisionStats(0)["collided"] > 0
    for s in ranks + [one]:
        s.destroy()
    print("group case %d: %.2f s" % (index, time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------- the resume
@pytest.mark.parametrize("solver,precision", model.RESUME)
def test_a_run_with_registered_operators_resumes_bit_for_bit(fp, tmp_path, solver, precision):
    """N sub-steps with a background operator every e1-th and a binary operator every e2-th sub-step; the same run cut after t
    sub-steps, t a common multiple of e1 and e2, saved, loaded into a fresh handle on which the operators are registered with
    epoch + t, and run for N - t: the same particles and fields, and the two parts' counts add up to the whole run's.  (The
    phase of `every` counts a handle's own sub-steps: a cut that is no common multiple cannot reproduce the run.)"""
    t0 = time.perf_counter()
    sc = model.resume_scene(solver, precision)
    t, n = model.RESUME_T, model.RESUME_N
    assert all(t % e == 0 for e in model.RESUME_EVERY) and 0 < t < n and (n - t) % 2 == 1
    whole, first, rest = build(fp, sc), build(fp, sc), build(fp, sc)
    for sim in (whole, first):
        start(sim, sc)
        register(sim, sc)
    whole.substeps(n)
    first.substeps(t)
    first.saveCheckpoint(tmp_path / "cut.ckpt")
    rest.loadCheckpoint(tmp_path / "cut.ckpt")
    register(rest, sc, shift=t)
    rest.substeps(n - t)
    assert same_particles(particles_of(whole, sc), particles_of(rest, sc))
    fw, fr = fields_of(fp, whole, sc), fields_of(fp, rest, sc)
    assert all(fw[name] == fr[name] for name in fw), [name for name in fw if fw[name] != fr[name]]
    assert not same_particles(particles_of(first, sc), particles_of(rest, sc))
    # (the comparison has teeth: the same resumption with the epochs off by one sub-step is another run)
    wrong = build(fp, sc)
    wrong.loadCheckpoint(tmp_path / "cut.ckpt")
    register(wrong, sc, shift=t + 1)
    wrong.substeps(n - t)
    assert not same_particles(particles_of(whole, sc), particles_of(wrong, sc))
    wrong.destroy()
    for stats in ("collisionStats", "pairStats"):
        total = {}
        for sim in (first, rest):
            add_counts(total, getattr(sim, stats)(0))
        assert total == getattr(whole, stats)(0) and total["applications"] == n // model.RESUME_EVERY[stats == "pairStats"], (stats, total)
    assert whole.collisionStats(0)["collided"] > 0 and whole.pairStats(0)["pairs"] > 0 and rest.pairStats(0)["pairs"] > 0
    for sim in (whole, first, rest):
        sim.destroy()
    print("resume %s %s: %.2f s" % (solver, precision, time.perf_counter() - t0))
