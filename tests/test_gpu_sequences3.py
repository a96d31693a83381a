"""Generation 3 of the random call sequences on the CART3D box: the sinks and the sources — remove() / removeEvery() /
renumber(), inject() / injectEvery(), reserve(), population(), the only operators that change a species' count, its id span and
its capacity — among every operator and read of generations 1 and 2, whose helpers this module uses.  tests/sequence_model.py
(generation 3) turns a seed into the scene (on a box of unit edges: select() returns the stored values exactly) and the steps;
tests/test_sequence_model.py proves on the CPU that the committed SEEDS3 reach the states meant here and that no committed
removal is vacuous on the initial particles.  Everything below is equality bit for bit or of exact integers: no tolerance
anywhere.

A thinned species has no caller's order, so every handle is compared through select() of each species — population(), the rows
(ids, position, velocity) as bytes — fields_of(), and the returned dictionaries through exact().  What depends on n is carried by
the model as a fraction or a rule and resolved against A.population() just before the call; WHICH species are thinned the model
knows, and the replay holds that against population() at every step.

Relation 1, the fresh twin, whenever no species of A is thinned (grown and reserved species count): B is built, reserved to A's
capacities and loaded from A.saveCheckpoint(); both get the operation, the new kinds included.
Relation 1T, the mate.  While a species is thinned saveCheckpoint is refused (asserted at every such step), so no fresh twin can be
made.  The mate M runs beside A from the start of EVERY scene (on a scene without registered operators it need only exist from
the checkpoint before the first removal; the longer life asks more, not less, and until the first removal A is held to the
fresh twin from its own file at the same steps), gets every state-changing operation A gets and no
read, and lives another binning life: sort_interval + 2 (mod 4), the opposite setting of the staged binning, an explicit sort()
before every operation.  A and M hold the same ids in other slots; after every step their rows, populations, fields and returned
values agree — no result depends on slots or bins.  With operators registered on A (and C), M has none and does the manual loop in
the hook's full order (diag_after_substep): substeps(1), the forces, collide, collideGas, collidePair, fusionYield,
fusionSpectrum, the sinks in registration order, the sources (application k with epoch + k), then the recorder rows; A's seven
stats families, removeStats and injectStats are the integer sums of what M's one-shot calls returned, A's three histories are M's
rows, and the count of every energy row is population() at its sub-step.
Relation 2, the unread copy: C gets the state-changing operations only; A equals it at the midpoint and at the end.

The references, on A's select() rows read just before the call (cells computed from the rows as the model's initial_state
does): remove* results and survivors against remove_reference.remove (result exact, doubles included); inject*: the old rows
untouched, the new ids id span + l, the tallies against inject_reference.tally_fast of the new rows, the positions of every
axis the rule forms without a transcendental function against inject_reference.stored bit for bit; the velocities and a flux
source's normal position within the reference's own error as tests/test_gpu_inject.py states it (the reference's logarithm and
circular functions differ from the device's in the last places: one unit in the last place of the rounded reference in fp32,
velocity_bound / flux_bounds in fp64 — the only inequalities of this module, and the reference's, not the library's); and
wherever the stored velocities ARE inject_reference.stored's bits, the whole result against inject_reference.application.  The
hook's applications are held the same way, on the mate's one-shot calls.  Every test prints how many applications were held
whole, and test_turnover[poisson_fft-fp32] asserts that some were.  count, select, both histograms and moments against
their references; fusionYield and fusionSpectrum against fusion_want / spectrum_want and collideGas against gas_want with the
true ids.  After renumber the rows are the old rows in ascending old id with the ids 0 .. n-1 and the fields are untouched.
Refusals: on a thinned species set, setRange, load, load(density=...), load(radial=...), getParticles, getRange, getCells and
saveCheckpoint raise FPIC_ERR_STATE naming fpic_renumber; renumber of a thinned species with operators registered raises it
naming "registered" (on C; on A, which also records a series, fpic_renumber names the series first: both are asserted);
inject of capacity - n + 1 raises FPIC_ERR_INVALID_ARG naming fpic_reserve — each with the rows, fields, population() and
stats()["sort_passes"] as they were.  The model counts them as coverage, not as skips.
The named sequences: turnover (source against sink over forty sub-steps, the id span three times the capacity; the `none` case
carries the ledger in the 128-bit fixed point), rewinds (files of three sizes into a thinned and a grown handle: stale slots),
hook_overflow (a registered source whose third application does not fit: an API error, and the handle equals the mate that
stopped before that source).  The two resumes: a source alone through a file, and with a sink (clear, renumber, register again).

What the sequences found (fixed with them): reserve() across a stride AFTER collidePairEvery, fusionYieldEvery or
fusionSpectrumEvery had been registered made the next due sub-step fail ("a registered fpic_pair operator found species 1 larger
than at its registration"): the cell index those operators share is sized at registration and the hook never grows it.  Seeds
176 and 2568 reach it (a reserve step, and a one-shot source that reserves first, on scenes with registered operators);
fpic_reserve now regrows the index itself, and tests/test_gpu_inject.py holds that alone.

Where a fused re-binning push meets the new kinds: a sink or source that applies un-bins its species, from inside the hook too,
and the scenes with registered operators carry a source due every sub-step — their species are binned afresh every sub-step.  The
re-binning conditions of tests/test_sequence_model.py therefore rest on the five seeds without registered operators that can
re-bin (8, 89, 3060, 3317, 4778: electrostatic or `none`, sort_interval > 0); the forced substeps after their first removal is a
re-binning push on the species just thinned.

Wall times on an MI355X, one run of the module on its own (11.5 s in all; tests/test_gpu_sequences2.py on its own: 17.8 s, its 12
seeds 13.1 s, the resets 0.4 s, its 6 group cases 2.0 s, its resumes 0.2 s):
    relations 1, 1T and 2, 12 seeds    6.9 s together: 0.23 to 0.39 s each, 2.0 s and 1.8 s for the first electrostatic and the first
                                       full-EM seed of the process (the transform library and the code objects are loaded there)
    turnover, 3 cases                  1.3 s together
    rewinds                            0.2 s
    hook_overflow                      0.03 s
    the resumes, 2 x 2                 0.3 s together
In that run all 207 fp32 applications of a source (one-shot and the hook's) were held to inject_reference.application whole; none
of the 157 fp64 ones was (every one within velocity_bound / flux_bounds).
A negative control of the whole construction, run once by hand and not kept: with fpic_inject giving a thinned species the ids
n + l instead of id span + l (a value, never an address: the ids stay below the id span, an unthinned species is untouched) 14 of
the 21 tests fail.  Eight of the twelve seeds: the five with registered operators (82, 176, 648, 1986, 2568) at sub-step 2, where
the pair source's application into species 0, which the first sink has just thinned, "touched the old rows" on the mate (two rows
of one id come back in slot order); 24, 3060 and 3975 at their first one-shot injection into a thinned species (inject_volume,
inject_pair, inject_pair), at the comparison with the mate.  The three turnovers fail at sub-step 2 in the same way, hook_overflow
after the refused sub-step, and both resumes with a sink.  What passes: seeds 8, 89, 3317 and 4778, which inject into no thinned
species (8 and 3317 draw no injection, 89 injects before its first removal, 4778 into the other species), rewinds (it grows
before it thins) and both resumes with a source alone.  Of the single-operation modules, tests/test_gpu_inject.py sees it in
test_a_thinned_species and test_order_in_the_hook (both precisions; its other 39 tests and all of tests/test_gpu_remove.py pass)."""
import time

import numpy as np
import pytest

import histogram_reference as hr
import inject_reference as ir
import load_reference as lr
import moments_reference as mref
import remove_reference as rr
import select_reference as sref
import sequence_model as model
import test_gpu_sequences as g1
import test_gpu_sequences2 as g2
from test_gpu_inject import flux_bounds
from test_gpu_load import velocity_bound
from test_gpu_remove import refused, same_result as same_removal
from test_gpu_sequences2 import add_ints, equal_sums, exact, ints_of

pytestmark = pytest.mark.gpu

DTYPE = dict(fp32=np.float32, fp64=np.float64)
FIELD_KINDS = ("E", "edge_E", "face_B")      # what a checkpoint carries; rho and J are the deposit of a handle's own last call


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


# ---------------------------------------------------------------------------------------------- handles and what is compared
def build3(fp, sc, monkeypatch, mate=False, capacities=None):
    """a handle of the scene; mate: the other binning life (the staged binning is read from the environment at creation)"""
    staged = sc["staged"] != mate
    if staged:
        monkeypatch.setenv("FPIC_TWO_LEVEL_MIN", "1")
    else:
        monkeypatch.delenv("FPIC_TWO_LEVEL_MIN", raising=False)
    sim = fp.makeCylindricalParticlePusher(sc["spec"], precision=sc["precision"], sort_interval=(sc["sort_interval"] + 2) % 4 if mate else sc["sort_interval"])
    for sp in range(1, len(sc["counts"])):
        assert sim.addSpecies(sc["masses"][sp], sc["charges"][sp], sc["counts"][sp]) == sp
    for sp, cap in enumerate(capacities or []):
        assert sim.reserve(sp, cap) == max(cap, sc["counts"][sp])
    return sim


def start3(sim, sc):
    for sp, n in enumerate(sc["counts"]):
        pos, vel = model.particles3(sc["seed"], 1000 + sp, n)
        sim.set(position=pos, velocity=vel, species=sp)
    if sc["solver"] == "none":
        sim.set(E=np.zeros(tuple(sc["shape"]) + (3,)) if sc.get("zero_field") else model.given_field3(sc["seed"]))
    if sc["addB"]:
        sim.addB(*sc["addB"])
    sim.precalc()


def rows(sim, sp):
    r = sim.select(species=sp)
    return r["ids"], r["position"], r["velocity"]


def same_rows(x, y):
    return all(g1.bits(p, q) for p, q in zip(x, y))


def snap(fp, sim, sc, density=True, face_b=True):
    ns = len(sc["counts"])
    return dict(pop=[sim.population(sp) for sp in range(ns)], rows=[rows(sim, sp) for sp in range(ns)], fields=g1.fields_of(fp, sim, sc, density=density, face_b=face_b))


def thinned_of(pops):
    return [sp for sp, p in enumerate(pops) if p["id_span"] != p["n"]]


def assert_same(x, y, where, names=None):
    """two snapshots: the populations, the rows and the fields (names: only these; None: all both hold)"""
    assert x["pop"] == y["pop"], (where, x["pop"], y["pop"])
    for sp, (p, q) in enumerate(zip(x["rows"], y["rows"])):
        assert g1.bits(p[0], q[0]), (where, "ids of species", sp)
        assert g1.bits(p[1], q[1]), (where, "position of species", sp, int((p[1] != q[1]).any(axis=1).sum()))
        assert g1.bits(p[2], q[2]), (where, "velocity of species", sp, int((p[2] != q[2]).any(axis=1).sum()))
    for name in x["fields"]:
        if name in y["fields"] and (names is None or name in names):
            assert x["fields"][name] == y["fields"][name], (where, name)


def state_of(snapshot, sc):
    """what the references take, from the rows: the stored fractions (a unit box) and velocities, the true ids, the cells"""
    return [dict(frac=r[1], vel=r[2], cell=model.cells_of(r[1], sc["shape"]), ids=r[0].astype(np.int64)) for r in snapshot["rows"]]


def twin3(fp, sc, a, path, monkeypatch, pops):
    a.saveCheckpoint(path)
    b = build3(fp, sc, monkeypatch, capacities=[p["capacity"] for p in pops])
    b.loadCheckpoint(path)
    return b


# ---------------------------------------------------------------------------------------------- registration and the manual loop
def register3(sim, sc, shift=0, applied=None):
    """everything a generation-3 scene registers; shift: the sub-steps a resumed run has behind it; applied: the applications
    each source has made so far"""
    g2.register2(sim, sc, shift)
    for i, op in enumerate(sc["remove_every"]):
        assert sim.removeEvery(op["every"], where=op["where"], species=op["species"], every=op["every_id"], outside=op["outside"]) == i
    for i, op in enumerate(sc["inject_every"]):
        assert sim.injectEvery(op["every"], species=op["species"], **dict(op["kw"], epoch=op["kw"]["epoch"] + (applied[i] if applied else 0))) == i


def record3(a, sc):
    rec = sc["recorders"]
    a.recordEnergy(rec["energy"]["every"], rec["energy"]["capacity"])
    a.recordSeries(rec["series"]["every"], rec["series"]["capacity"], points=rec["series"]["points"], tracers=np.array(rec["series"]["tracers"]), species=rec["series"]["species"])
    a.recordModes(rec["modes"]["every"], rec["modes"]["capacity"], rec["modes"]["modes"], rec["modes"]["fields"])


def sinks_and_sources(m, sc, t, sums, applied, held=None):
    """the hook's last operators by hand on the mate: the sinks in registration order, then the sources (application k carries
    epoch + k); held: every application of a source is also held to the rule (check_injection), on the mate's own rows"""
    for i, op in enumerate(sc.get("remove_every", [])):
        if t % op["every"] == 0:
            add_ints(sums["remove%d" % i], m.remove(where=op["where"], species=op["species"], every=op["every_id"], outside=op["outside"]))
    for i, op in enumerate(sc.get("inject_every", [])):
        if t % op["every"] == 0:
            kw, sp = dict(op["kw"], epoch=op["kw"]["epoch"] + applied[i]), op["species"]
            before = (m.population(sp), rows(m, sp)) if held is not None else None
            got = m.inject(species=sp, **kw)
            if held is not None:
                check_injection(sc, kw, sp, before, (m.population(sp), rows(m, sp)), got, "source %d at sub-step %d" % (i, t), held)
            add_ints(sums["inject%d" % i], got)
            applied[i] += 1


def manual_substeps3(fp, m, sc, k, t, sums, due, applied, held=None, tail=None):
    """the manual equivalent of substeps(k) on the mate, which has run beside A from the start (its own count of sub-steps is
    A's: a one-shot force needs no shift of its epoch), in the hook's order; tail(m, t): the operators a later generation has
    behind the sources and before the recorder rows; returns t"""
    ce, pe, ge, fe, se, rec = sc["collide_every"], sc["pair_every"], sc["gas_every"], sc["fusion_every"], sc["spectrum_every"], sc["recorders"]
    for _ in range(k):
        m.substeps(1)
        t += 1
        for i, kw in enumerate(sc["force_on"]):
            add_ints(sums["force%d" % i], m.force(**kw))
        if t % ce["every"] == 0:
            add_ints(sums["collide"], m.collide(ce["kind"], species=ce["species"], **dict(ce["kw"], epoch=t + ce["kw"]["epoch"])))
        if t % ge["every"] == 0:
            add_ints(sums["gas"], m.collideGas(ge["kind"], **dict(ge["kw"], epoch=t + ge["kw"]["epoch"])))
        if t % pe["every"] == 0:
            add_ints(sums["pair"], m.collidePair(pe["a"], pe["b"], **dict(pe["kw"], epoch=t + pe["kw"]["epoch"])))
        if t % fe["every"] == 0:
            add_ints(sums["fusion"], m.fusionYield(fe["a"], fe["b"], grid=True, **dict(fe["kw"], epoch=t + fe["kw"]["epoch"])))
        if t % se["every"] == 0:
            add_ints(sums["spectrum"], m.fusionSpectrum(se["a"], se["b"], **dict(se["kw"], epoch=t + se["kw"]["epoch"])))
        sinks_and_sources(m, sc, t, sums, applied, held)
        if tail is not None:
            tail(m, t)
        if t % rec["energy"]["every"] == 0:
            row = np.zeros(1, dtype=fp.ENERGY_DTYPE)
            row[0] = m._energy_row("global")
            assert [int(x) for x in row["count"][0][:len(sc["counts"])]] == [m.population(sp)["n"] for sp in range(len(sc["counts"]))]      # the row counts the live particles
            row["substep"] = 0
            due["energy"].append((t, row.tobytes()))
        if t % rec["series"]["every"] == 0:
            s = rec["series"]
            got = m.series(points=s["points"], tracers=np.array(s["tracers"]), species=s["species"])
            due["series"].append((t, got["points"].tobytes() + got["tracers"].tobytes()))
        if t % rec["modes"]["every"] == 0:
            mo = rec["modes"]
            due["modes"].append((t, m._modes_rows(mo["modes"], mo["fields"], "global")[0].tobytes()))
    return t


# ---------------------------------------------------------------------------------------------- the operations
def resolve(sc, st, pops):
    """what a step's call takes that depends on the populations, read from A just before it"""
    res = dict(n=[p["n"] for p in pops], capacity=[p["capacity"] for p in pops])
    sp = st.get("species")
    if "first_frac" in st:
        res["range"] = model.resolve_range(st["first_frac"], st["count_frac"], pops[sp]["n"])
    if st["kind"] in ("inject_volume", "inject_flux"):
        res["inject"] = {sp: model.resolve_inject(st, pops[sp]["n"], pops[sp]["capacity"])}
    elif st["kind"] == "inject_pair":
        res["inject"] = {s: model.resolve_inject(st, pops[s]["n"], pops[s]["capacity"]) for s in (0, 1)}
    elif st["kind"] == "inject_refused":
        res["over"] = pops[sp]["capacity"] - pops[sp]["n"] + 1
    return res


def inject_now(sim, sp, st, res):
    reserve_to, count = res["inject"][sp]
    if reserve_to is not None:
        assert sim.reserve(sp, reserve_to) == reserve_to
    return sim.inject(species=sp, count=count, **st["kw"])


def call3(fp, sim, sc, st, res, files, shift):
    kind, sp = st["kind"], st.get("species")
    if kind == "substeps":
        return sim.substeps(st["k"])
    if kind == "sort":
        return sim.sort()
    if kind == "loadCheckpoint":
        return sim.loadCheckpoint(files[st["file"]])
    if kind in ("set", "setRange"):
        first, count = (0, res["n"][sp]) if kind == "set" else res["range"]
        pos, vel = model.particles3(sc["seed"], st["tag"], count)
        kw = dict(position=pos if st["what"] != "velocity" else None, velocity=vel if st["what"] != "position" else None)
        return sim.set(species=sp, **kw) if kind == "set" else sim.setRange(first, species=sp, **kw)
    if kind in ("load", "load_profile", "load_radial"):
        tables = dict(paired=st["paired"]) if kind == "load" else dict(radial=st["radial"]) if kind == "load_radial" else dict(density=st["density"], thermal=st["thermal"], shear=st["shear"])
        return sim.load(species=sp, first=res["range"][0], count=res["range"][1], seed=st["seed"], stream=st["stream"], lo=st["lo"], hi=st["hi"], drift=st["drift"],
                        vth=st["vth"], lattice=st["lattice"], position=st["what"] != "velocity", velocity=st["what"] != "position", **tables)
    if kind.startswith("collide_"):
        return sim.collide(st["what"], **st["kw"])
    if kind.startswith("pair_"):
        return sim.collidePair(st["a"], st["b"], **st["kw"])
    if kind.startswith("force_"):
        return sim.force(**dict(st["kw"], epoch=st["kw"]["epoch"] + shift))
    if kind.startswith("gas_"):
        return sim.collideGas(st["what"], **st["kw"])
    if kind.startswith("remove_"):
        return sim.remove(where=st["where"], species=sp, every=st["every"], outside=st["outside"])
    if kind in ("inject_volume", "inject_flux"):
        return inject_now(sim, sp, st, res)
    if kind == "inject_pair":
        return [inject_now(sim, s, st, res) for s in (0, 1)]
    if kind == "inject_refused":
        return refused(fp, lambda: sim.inject(species=sp, count=res["over"], **st["kw"]), -1, "fpic_reserve")
    if kind == "reserve":
        cap = res["capacity"][sp]
        assert sim.reserve(sp, cap - 1) == cap and sim.reserve(sp, 0) == cap      # smaller: a no-op
        return sim.reserve(sp, cap + st["extra"])
    if kind == "renumber":
        return [sim.renumber(s) for s in range(len(sc["counts"]))]
    raise AssertionError(kind)


def apply3(fp, sim, sc, st, res, files, shift=0, registered=True, recording=False):
    """one state-changing operation of generation 3 on a handle; what it returned.  A step the library must refuse is asked of
    every handle that must refuse it (registered=False: a handle with no operators registered has no reason to refuse renumber,
    and is not asked; recording=True: the handle also records a series, which fpic_renumber names first)."""
    if st["refused"]:
        if st.get("species") is not None:
            sim.population(st["species"])      # (the wrapper's own count: sinks and sources change n behind it)
        if st["kind"] == "renumber":
            if registered:
                refused(fp, lambda: call3(fp, sim, sc, st, res, files, shift), -5, "fpic_renumber", "series" if recording else "registered")
        else:
            refused(fp, lambda: call3(fp, sim, sc, st, res, files, shift), -5, "fpic_renumber")
        return None
    out = call3(fp, sim, sc, st, res, files, shift)
    if st["precalc"]:
        sim.precalc()
    return out


def deposits3(sc, st, got):
    """the grids an operation writes afresh: generation 1's, and the charge grid an electrostatic handle deposits again when a
    sink took or a source gave somebody"""
    fresh = set() if st["refused"] else g1.deposits(sc, st)
    if sc["solver"] == "poisson_fft" and (st["kind"] in model.INJECT_KINDS3 or (st["kind"] in model.REMOVE_KINDS3 and got["removed"] > 0)):
        fresh.add("rho")
    return fresh


def check_injection(sc, kw, sp, before, after, got, where, held=None):
    """one application against the rule: before, after: (population, rows) of the species.  Exact: the count, the old rows,
    the new ids, the tallies of the new rows, the positions of every axis the rule forms without a transcendental function.
    The rounded parts — the velocities, a flux source's normal position — lie within the reference's own error as
    tests/test_gpu_inject.py states it (fp32: one unit in the last place of the rounded reference; fp64: the loader's bound,
    velocity_bound / flux_bounds), and wherever the stored velocities ARE the reference's bits the whole result is
    inject_reference.application's.  held[True / False] counts the applications that were / were not held whole."""
    (pop0, r0), (pop1, r1) = before, after
    n, m = pop0["n"], pop1["n"] - pop0["n"]
    T = DTYPE[sc["precision"]]
    assert got["applications"] == 1 and got["injected"] == m > 0 and pop1["id_span"] == pop0["id_span"] + m and pop1["capacity"] >= pop1["n"], (where, got, pop0, pop1)
    assert same_rows(tuple(x[:n] for x in r1), r0), (where, "an injection touched the old rows")
    assert g1.bits(r1[0][n:], np.arange(pop0["id_span"], pop0["id_span"] + m, dtype=np.uint32)), (where, "the new ids are id span + l")
    pos, vel = r1[1][n:], r1[2][n:]
    assert [got["energy_fixed"]] + got["momentum_fixed"] == ir.tally_fast(vel), (where, "the tally of the new rows")
    req = ir.request(model.L3, sc["dt"], **{k: v for k, v in kw.items() if k not in ("first", "count", "epoch")})
    j = ir.sequence(kw["first"], m, k=0, epoch=kw.get("epoch", 0))
    want_p, want_v = ir.stored(req, j, T)
    for a in range(3):
        if not (kw["kind"] == "flux" and a == kw["axis"]):      # integers, one rounded multiply, one rounded add
            assert g1.bits(pos[:, a], want_p[:, a]), (where, "position axis", a, int((pos[:, a] != want_p[:, a]).sum()))
    assert np.all((pos >= 0) & (pos < 1))
    if kw["kind"] == "flux":
        assert np.all(vel[:, kw["axis"]] * kw["side"] > 0), where
    p64, v64 = ir.states(req, j)
    if kw["kind"] == "flux":
        bv, bp = flux_bounds(req, j)
        dpn = np.abs(pos[:, kw["axis"]].astype(np.float64) - lr.wrap01(p64.copy())[:, kw["axis"]])
        dpn = np.minimum(dpn, 1.0 - dpn)                                         # (a plane on the box's face: the wrap's two sides)
    else:
        bv, bp = velocity_bound(req, j), None
    if sc["precision"] == "fp64":
        assert np.all(np.abs(vel - v64) <= bv), (where, "velocity beyond the loader's bound", float((np.abs(vel - v64) / bv).max()))
        assert bp is None or np.all(dpn <= bp), (where, "normal position beyond its bound", float((dpn / bp).max()))
    else:
        assert np.all(np.abs(vel.astype(np.float64) - want_v.astype(np.float64)) <= np.spacing(np.abs(want_v)).astype(np.float64)), (where, "velocity beyond one ulp")
        dp = np.abs(pos.astype(np.float64) - want_p.astype(np.float64))
        assert np.all(np.minimum(dp, 1.0 - dp) <= np.spacing(np.maximum(want_p, T(2.0 ** -20))).astype(np.float64)), (where, "position beyond one ulp")
    whole = g1.bits(vel, want_v)
    if whole:
        want = ir.application(req, j, T, mass=sc["masses"][sp], charge=sc["charges"][sp], weight=sc["macro_weight"])
        assert exact(got) == exact(want), (where, got, want)
    if held is not None:
        held[whole] += 1
    assert got["charge"] == (float(m) * sc["charges"][sp]) * sc["macro_weight"]


def check_new_kind(fp, a, sc, st, res, got, before, after, passes, rho_current, where, held=None):
    """a step of a new kind on A against its reference"""
    kind, sp = st["kind"], st.get("species")
    others = [s for s in range(len(sc["counts"])) if s != sp and kind != "inject_pair" and kind != "renumber"]
    for s in others:
        assert same_rows(before["rows"][s], after["rows"][s]) and before["pop"][s] == after["pop"][s], (where, "another species changed", s)
    if kind.startswith("remove_"):
        survivors, want = rr.remove(*before["rows"][sp], where=st["where"], every=st["every"], outside=st["outside"], mass=sc["masses"][sp], charge=sc["charges"][sp],
                                    weight=sc["macro_weight"])
        same_removal(got, want)
        assert same_rows(after["rows"][sp], survivors), (where, "the survivors")
        n = before["pop"][sp]["n"]
        if kind == "remove_nothing":
            assert got["removed"] == 0 and got["scanned"] == n and a.stats()["sort_passes"] == passes, (where, got)
            assert_same(before, after, where)
        else:
            assert 0 < got["removed"] < n, (where, "a vacuous removal at run time: replace the seed", got["removed"], n)
            assert after["pop"][sp] == dict(n=n - got["removed"], capacity=before["pop"][sp]["capacity"], id_span=before["pop"][sp]["id_span"]), (where, after["pop"][sp])
    elif kind in ("inject_volume", "inject_flux"):
        check_injection(sc, st["kw"], sp, (before["pop"][sp], before["rows"][sp]), (after["pop"][sp], after["rows"][sp]), got, where, held)
        assert after["pop"][sp]["n"] - before["pop"][sp]["n"] == res["inject"][sp][1]
    elif kind == "inject_pair":
        for s in (0, 1):
            check_injection(sc, st["kw"], s, (before["pop"][s], before["rows"][s]), (after["pop"][s], after["rows"][s]), got[s], where, held)
        m = res["inject"][0][1]
        assert m == res["inject"][1][1] and all(g1.bits(after["rows"][0][c][-m:], after["rows"][1][c][-m:]) for c in (1, 2)), (where, "the pair does not coincide")
        if sc["solver"] == "poisson_fft" and rho_current:      # a neutral pair: the charge grid it re-deposits is the one before
            assert after["fields"]["rho"] == before["fields"]["rho"], (where, "a neutral pair changed the charge grid")
    elif kind == "inject_refused":
        assert a.stats()["sort_passes"] == passes
        assert_same(before, after, where)
    elif kind == "reserve":
        assert got == res["capacity"][sp] + st["extra"] == after["pop"][sp]["capacity"]
        assert dict(after["pop"][sp], capacity=0) == dict(before["pop"][sp], capacity=0) and same_rows(before["rows"][sp], after["rows"][sp]), where
        assert all(after["fields"][name] == before["fields"][name] for name in after["fields"] if name in before["fields"]), (where, "reserve changed a field")
    elif kind == "renumber":
        for s, n in enumerate(got):
            r0, r1 = before["rows"][s], after["rows"][s]
            assert n == len(r0[0]) and after["pop"][s] == dict(n=n, capacity=before["pop"][s]["capacity"], id_span=n), (where, after["pop"][s])
            assert g1.bits(r1[0], np.arange(n, dtype=np.uint32)) and g1.bits(r1[0], np.sort(rr.renumber(r0[0]))) and g1.bits(r1[1], r0[1]) and g1.bits(r1[2], r0[2]), where
        assert all(after["fields"][name] == before["fields"][name] for name in after["fields"] if name in before["fields"]), (where, "renumber changed a field")


# ---------------------------------------------------------------------------------------------- the reads
def read3(fp, a, sc, r, files, tmp_path, rho_current, sums, thinned, where):
    """one reading call on A, held to the references over A's select() rows read just before; thinned: the species thinned now"""
    kind, sp = r["kind"], r["species"]
    shape = sc["shape"]
    if kind in model.STATS_KINDS2:
        return g2.read2(fp, a, sc, r, files, tmp_path, rho_current, sums, dict(fusion={}, spectrum={}))
    if kind == "removeStats":
        assert all(equal_sums(ints_of(a.removeStats(i)), sums["remove%d" % i]) for i in range(len(sc["remove_every"]))), where
        return
    if kind == "injectStats":
        assert all(equal_sums(ints_of(a.injectStats(i)), sums["inject%d" % i]) for i in range(len(sc["inject_every"]))), where
        return
    ns = len(sc["counts"])
    if kind == "saveCheckpoint":
        assert r["refused"] == bool(thinned), (where, kind)
        if r["refused"]:
            return refused(fp, lambda: a.saveCheckpoint(tmp_path / "refused.ckpt"), -5, "fpic_renumber")
        path = tmp_path / ("saved%d.ckpt" % r["file"])
        a.saveCheckpoint(path)
        assert len(files) == r["file"]
        files.append(path)
        return
    ids, pos, vel = rows(a, sp)
    pop = a.population(sp)
    n = pop["n"]
    assert len(ids) == n
    if kind in model.CALLER_ORDER_READS3:
        assert r["refused"] == (sp in thinned), (where, kind)
        call = dict(getParticles=lambda: a.getParticles(species=sp), getCells=lambda: a.getCells(species=sp), getRange=lambda: a.getRange(0, 1, 1, species=sp))[kind]
        if r["refused"]:
            return refused(fp, call, -5, "fpic_renumber")
        assert g1.bits(ids, np.arange(n, dtype=np.uint32))
        if kind == "getParticles":
            p = call()
            assert g1.bits(p["position"], pos) and g1.bits(p["velocity"], vel), where
        elif kind == "getRange":
            first, count = model.resolve_range(r["first_frac"], r["count_frac"], n, r["stride"])
            got = a.getRange(first, count, r["stride"], species=sp)
            at = first + r["stride"] * np.arange(count)
            assert g1.bits(got["position"], pos[at]) and g1.bits(got["velocity"], vel[at]), where
        else:
            cells = call()
            assert g1.bits(cells, a.getRange(0, n, 1, species=sp, cells=True)["cells"]) and np.array_equal(cells, model.cells_of(pos, shape)), (where, "the cells of the rows")
    elif kind == "count":
        assert a.count(r["where"], species=sp, every=r["every"]) == sref.count(ids, pos, vel, r["where"], r["every"]), where
    elif kind == "select":
        got, want = a.select(r["where"], species=sp, every=r["every"]), sref.select(ids, pos, vel, r["where"], r["every"])
        assert got["matched"] == want["matched"] and g1.bits(got["ids"], want["ids"]), where
        assert g1.bits(got["position"], want["position"]) and g1.bits(got["velocity"], want["velocity"]), where
    elif kind in ("histogram_lds", "histogram_global"):
        got = a.histogram(r["axes"], r["bins"], r["ranges"], species=sp)
        want, outside = hr.histogram(pos, vel, r["axes"], r["bins"], r["ranges"])
        assert got["outside"] == outside and np.array_equal(got["counts"], want) and int(want.sum()) + outside == n, where
    elif kind == "moments":
        got = a.moments(r["which"], species=sp)
        want, rejected = mref.moments(pos, vel, shape, r["which"])
        assert got["rejected"] == rejected == 0
        for name in ("N", "FX", "FY", "FZ"):
            assert np.array_equal(got[name], want[name]), (where, name)
        if rho_current:      # the charge grid is the deposit of these positions: the sum over the species of Z N, bit for bit
            total = np.zeros_like(got["N"])
            for s2 in range(ns):
                total += int(round(sc["charges"][s2] / sc["charges"][0])) * a.moments("n", species=s2)["N"]
            assert np.array_equal(total, a.readField(fp.F3_RHO_FIXED).reshape(total.shape)), (where, "the charge grid")
    elif kind == "energy":
        e = a.energy()
        assert e["count"].tolist() == [a.population(s)["n"] for s in range(ns)], where
    elif kind == "series":
        tr = np.array(model.resolve_tracers(r["tracer_fracs"], pop["id_span"], ids))
        got = a.series(points=r["points"], tracers=tr, species=sp)["tracers"]
        at = {int(i): k for k, i in enumerate(ids)}
        dead = 0
        for row, i in zip(got, tr):
            if int(i) in at:      # a live tracer's row is its select() row
                k = at[int(i)]
                assert g1.bits(np.ascontiguousarray(row[:6]), np.concatenate([pos[k], vel[k]]).astype(np.float64)) and row[6] == 1, (where, "tracer", int(i))
            else:
                assert np.all(row == 0), (where, "the row of a dead tracer", int(i))
                dead += 1
        assert dead >= (1 if pop["id_span"] > n else 0), where
    elif kind == "modes":
        got = a.modes(r["modes"], r["fields"])
        assert all(np.all(np.isfinite(got[f])) for f in r["fields"])
    elif kind == "readField":
        e = a.readField(fp.F3_E)
        assert e.shape == (np.prod(shape), 4) and np.all(np.isfinite(e))
        if sc["solver"] == "yee":
            assert np.all(np.isfinite(a.readField(fp.F3_FACE_B)))
        charge = int(a.readField(fp.F3_RHO_FIXED).astype(object).sum())
        if rho_current:
            assert charge == sum(int(round(sc["charges"][s2] / sc["charges"][0])) * a.population(s2)["n"] for s2 in range(ns)) << 42, where
    elif kind in ("fusionYield", "fusionSpectrum"):
        which = {r["a"]} | ({r["b"]} if r["b"] is not None else set())
        state = [None] * ns
        for s2 in which:
            i2, p2, v2 = rows(a, s2)
            state[s2] = dict(frac=p2, vel=v2, cell=model.cells_of(p2, shape), ids=i2.astype(np.int64))
        if kind == "fusionYield":
            got = a.fusionYield(r["a"], r["b"], grid=True, **r["kw"])
            want = model.fusion_want(sc, state, r["a"], r["b"], r["kw"])[1]
            grid = got.pop("grid")
            assert np.array_equal(grid.ravel(), want["grid"]) and int(grid.sum()) == want["reactions_exact"], (where, int(grid.sum()), want["reactions_exact"])
        else:
            got = a.fusionSpectrum(r["a"], r["b"], **r["kw"])
            want = model.spectrum_want(sc, state, r["a"], r["b"], r["kw"])
            assert (got["bins"], got["under"], got["over"]) == (want["bins"], want["under"], want["over"]), (where, got["bins"], want["bins"])
            assert sum(got["bins"]) + got["under"] + got["over"] == got["reactions_exact"] and np.array_equal(got["edges"], want["edges"])
        assert {k: got[k] for k in g2.COUNTS} == dict(applications=1, **{k: int(want[k]) for k in g2.COUNTS[1:]}), (where, {k: got[k] for k in g2.COUNTS})
    else:
        raise AssertionError(kind)


# ---------------------------------------------------------------------------------------------- relations 1, 1T and 2
def families_of(sc):
    return g2.FAMILIES + tuple("remove%d" % i for i in range(len(sc.get("remove_every", [])))) + tuple("inject%d" % i for i in range(len(sc.get("inject_every", []))))


def stats3_of(sim, sc):
    """the integers of every registered family of a handle (a scene that registers only sinks and sources: only theirs)"""
    out = g2.stats_of(sim) if "collide_every" in sc else {}
    for i in range(len(sc["remove_every"])):
        out["remove%d" % i] = ints_of(sim.removeStats(i))
    for i in range(len(sc["inject_every"])):
        out["inject%d" % i] = ints_of(sim.injectStats(i))
    return out


def end_of_registered_run(a, c, sc, sums, due, t, families=None, stats=None):
    """the end of a run with registered operators: A's and C's totals are the sums of the mate's one-shot results, every
    family was due as often as its period says, A's three histories are the mate's rows"""
    families, stats = families or families_of, stats or stats3_of
    have, theirs = stats(a, sc), stats(c, sc)
    for key in families(sc):
        assert equal_sums(have[key], sums[key]) and have[key] == theirs[key], (sc["seed"], key, {k: v for k, v in have[key].items() if k != "grid"}, {k: v for k, v in sums[key].items() if k != "grid"})
    lo, hi = sc["force_window"]
    assert sums["force0"]["applications"] == hi - lo + 1 and sums["force1"]["applications"] == t
    assert all(sums[key]["applications"] == t // sc[key + "_every"]["every"] >= 3 for key in ("collide", "pair", "gas", "fusion", "spectrum"))
    assert all(sums["remove%d" % i]["applications"] == t // op["every"] and sums["remove%d" % i]["removed"] > 0 for i, op in enumerate(sc["remove_every"]))
    assert all(sums["inject%d" % i]["injected"] == op["kw"]["count"] * (t // op["every"]) > 0 for i, op in enumerate(sc["inject_every"]))
    rec = sc["recorders"]
    erows, edropped = a.energyHistory()
    hist, sdropped = a.seriesHistory()
    msub, mout, _, mdropped = a._modes_history_rows("global")
    erows = erows.copy()
    assert int(erows["substep"][-1]) == t // rec["energy"]["every"] * rec["energy"]["every"]
    labels = dict(energy=[int(x) for x in erows["substep"]], series=hist["substep"].tolist(), modes=msub.tolist())
    erows["substep"] = 0
    got_rows = dict(energy=[erows[i:i + 1].tobytes() for i in range(len(erows))],
                    series=[hist["points"][i].tobytes() + hist["tracers"][i].tobytes() for i in range(len(hist["substep"]))],
                    modes=[mout[i].tobytes() for i in range(len(msub))])
    for name, dropped in (("energy", edropped), ("series", sdropped), ("modes", mdropped)):
        cap = rec[name]["capacity"]
        assert dropped == len(due[name]) - cap > 0, (name, dropped, len(due[name]))
        assert labels[name] == [tt for tt, _ in due[name][-cap:]], (name, labels[name])
        assert got_rows[name] == [row for _, row in due[name][-cap:]], (sc["seed"], name)


def run_sequence3(fp, sc, steps, tmp_path, monkeypatch):
    ns = len(sc["counts"])
    caps = model.reserved3(sc, model.substeps_of(steps)) if sc["registered"] else None
    a, c, m = build3(fp, sc, monkeypatch, capacities=caps), build3(fp, sc, monkeypatch, capacities=caps), build3(fp, sc, monkeypatch, mate=True, capacities=caps)
    for sim in (a, c, m):
        start3(sim, sc)
    if sc["registered"]:
        register3(a, sc)
        register3(c, sc)
        record3(a, sc)
    for sp in range(ns):      # once per seed: on an unthinned species select() IS getParticles(), bit for bit
        p, r = a.getParticles(species=sp), rows(a, sp)
        assert g1.bits(r[0], np.arange(sc["counts"][sp], dtype=np.uint32)) and g1.bits(p["position"], r[1]) and g1.bits(p["velocity"], r[2])
    sums, due, applied = {k: {} for k in families_of(sc)}, dict(energy=[], series=[], modes=[]), [0] * len(sc.get("inject_every", []))
    files, t, twins, mated, held = [], 0, 0, 0, {True: 0, False: 0}
    passes0 = a.stats()["sort_passes"]
    rho_current = True
    before = snap(fp, a, sc)
    for index, st in enumerate(steps):
        kind = st["kind"]
        where = "seed %d step %d %s" % (sc["seed"], index, kind)
        thinned = thinned_of(before["pop"])
        assert thinned == st["thinned"], (where, "the model's thinned species", thinned, st["thinned"])
        res = resolve(sc, st, before["pop"])
        manual = kind == "substeps" and sc["registered"]      # (the mate does the hook by hand; a fresh twin would only do the same)
        if thinned:      # no fresh twin of a thinned handle can be made
            refused(fp, lambda: a.saveCheckpoint(tmp_path / "refused.ckpt"), -5, "fpic_renumber")
        b = None if thinned or manual else twin3(fp, sc, a, tmp_path / "twin.ckpt", monkeypatch, before["pop"])
        passes = a.stats()["sort_passes"]
        got_a = apply3(fp, a, sc, st, res, files, recording=sc["registered"])
        apply3(fp, c, sc, st, res, files)
        m.sort()
        if manual:
            t = manual_substeps3(fp, m, sc, st["k"], t, sums, due, applied, held)
        else:
            got_m = apply3(fp, m, sc, st, res, files, registered=False)
            assert exact(got_a) == exact(got_m), (where, "A and the mate", got_a, got_m)
            t += st.get("k", 0)
        face_b = model.compares_face_b(index)
        after = snap(fp, a, sc, face_b=face_b)
        assert_same(after, snap(fp, m, sc, face_b=face_b), where + " (the mate)")
        mated += bool(thinned)
        fresh = deposits3(sc, st, got_a) | ({"rho"} if sc["solver"] == "yee" else set())
        for name in after["fields"]:
            if name in ("rho", "J") and name not in fresh and name in before["fields"]:
                assert after["fields"][name] == before["fields"][name], (where, name, "written by an operation that deposits nothing")
        if b is not None:      # relation 1: the fresh twin (its own count of sub-steps is 0, A's is t)
            got_b = apply3(fp, b, sc, st, res, files, shift=t - st.get("k", 0), registered=False)
            assert exact(got_a) == exact(got_b), (where, "A and the fresh twin", got_a, got_b)
            assert_same(after, snap(fp, b, sc, face_b=face_b), where + " (the fresh twin)", names=FIELD_KINDS + tuple(fresh))
            b.destroy()
            twins += 1
        if st["refused"]:
            assert a.stats()["sort_passes"] == passes, where
            assert_same(before, after, where + " (refused)")
        elif kind in model.NEW_KINDS3:
            check_new_kind(fp, a, sc, st, res, got_a, before, after, passes, rho_current and sc["solver"] != "yee", where, held)
        elif kind.startswith("gas_"):
            want = model.gas_want(sc, state_of(before, sc), st["what"], st["kw"])
            assert {k: got_a[k] for k in ("candidates", "collided", "below", "above")} == want, (where, got_a, want)
        elif kind in ("load", "load_profile", "load_radial"):
            assert got_a == res["range"][1], (where, got_a)
        elif kind.startswith("force_"):
            assert st["t"] == t and got_a["applications"] == int(st["active"]), (where, st["t"], t, got_a)
        assert thinned_of(after["pop"]) == st["thinned_after"], (where, "the model's thinned species afterwards", thinned_of(after["pop"]), st["thinned_after"])
        if fresh & {"rho"} and sc["solver"] != "yee":
            rho_current = True
        elif (kind in model.POSITION_KINDS2 and st["what"] != "velocity" and not st["refused"]) or kind == "loadCheckpoint" or sc["solver"] == "yee" or \
                (kind in model.REMOVE_KINDS3 + model.INJECT_KINDS3 and sc["solver"] == "none"):
            rho_current = False
        if manual and sc["solver"] == "none":      # (the hook's sinks and sources deposit nothing under a given field: the grid is the push's)
            rho_current = False
        before = after
        for r in st["reads"]:
            read3(fp, a, sc, r, files, tmp_path, rho_current and sc["solver"] != "yee", sums, st["thinned_after"], where + " read " + r["kind"])
        if index == len(steps) // 2 or index == len(steps) - 1:      # relation 2 (at the midpoint C's lattice step stays open)
            end = index == len(steps) - 1
            sa, sc_ = snap(fp, a, sc, density=end, face_b=end), snap(fp, c, sc, density=end, face_b=end)
            assert_same(sa, sc_, where + " (A and C)", names=None if end else [name for name in sa["fields"] if not (name == "rho" and sc["solver"] == "yee")])
            before = sa if end else before
    assert a.stats()["sort_passes"] > passes0 and mated > 0 and (sc["registered"] or twins > 0), (sc["seed"], mated, twins)
    if sc["registered"]:
        end_of_registered_run(a, c, sc, sums, due, t)
    for sim in (a, c, m):
        sim.destroy()
    return held


@pytest.mark.parametrize("seed", model.SEEDS3)
def test_generation_3_sinks_and_sources_among_everything_else(fp, tmp_path, monkeypatch, seed):
    t0 = time.perf_counter()
    sc = model.scene3(seed)
    held = run_sequence3(fp, sc, model.sequence3(seed), tmp_path, monkeypatch)
    print("generation 3 seed %d (%s): %.2f s; injections held whole %d, within the reference's error %d" % (seed, sc["precision"], time.perf_counter() - t0, held[True], held[False]))


# ---------------------------------------------------------------------------------------------- the named sequences
@pytest.mark.parametrize("solver,precision", model.TURNOVER_CASES)
def test_turnover(fp, tmp_path, monkeypatch, solver, precision):
    """source against sink over forty sub-steps: A has both registered, the mate applies them by hand and lives another binning
    life; reads of every kind on A after every piece; the id span ends at three times the capacity; the `none` case balances
    the ledger word for word"""
    t0 = time.perf_counter()
    sc, reads = model.NAMED3["turnover"](solver, precision)
    tv = sc["turnover"]
    a, m = build3(fp, sc, monkeypatch, capacities=sc["capacities"]), build3(fp, sc, monkeypatch, mate=True, capacities=sc["capacities"])
    sc["remove_every"] = [dict(every=tv["sink_every"], species=1, where=tv["sink"]["where"], every_id=None, outside=False)]
    sc["inject_every"] = [dict(every=1, species=s, kw=tv["source"]) for s in tv["feeds"]]
    for sim in (a, m):
        start3(sim, sc)
    for i, op in enumerate(sc["remove_every"]):
        assert a.removeEvery(op["every"], where=op["where"], species=op["species"]) == i
    for i, op in enumerate(sc["inject_every"]):
        assert a.injectEvery(op["every"], species=op["species"], **op["kw"]) == i
    first = snap(fp, a, sc)
    sums, applied, t, held = {k: {} for k in families_of(sc)}, [0] * len(sc["inject_every"]), 0, {True: 0, False: 0}
    rho_current = True
    for index, (k, row) in enumerate(zip(tv["pieces"], reads)):
        where = "turnover %s %s piece %d" % (solver, precision, index)
        a.substeps(k)
        for _ in range(k):
            m.sort()
            m.substeps(1)
            t += 1
            sinks_and_sources(m, sc, t, sums, applied, held)
        sa = snap(fp, a, sc)
        assert_same(sa, snap(fp, m, sc), where)
        thinned = thinned_of(sa["pop"])
        assert thinned == ([1] if t >= 2 else []), (where, thinned)
        for r in row:
            if r["kind"] == "saveCheckpoint":
                r = dict(r, refused=bool(thinned), file=0)
            read3(fp, a, sc, r, [], tmp_path, rho_current and solver == "poisson_fft", sums, thinned, where + " read " + r["kind"])
        assert_same(sa, snap(fp, a, sc), where + " (the reads changed something)")
    assert t == 40 and held[True] + held[False] == sum(applied) == 40 * len(tv["feeds"])
    assert precision != "fp32" or held[True] > 0, ("no fp32 application was held to the whole reference", held)
    have = stats3_of(a, sc)
    for key in have:
        assert equal_sums(have[key], sums[key]), (key, have[key], sums[key])
    pop = a.population(1)
    assert pop["id_span"] == model.N1 + 40 * tv["count"] == 4590 >= 3 * pop["capacity"] and pop["capacity"] == tv["capacity"] and 0 < pop["n"] < tv["capacity"], pop
    assert sums["remove0"]["removed"] > 0 and pop["n"] == model.N1 + 40 * tv["count"] - sums["remove0"]["removed"]
    if tv["zero_field"]:      # the ledger: no velocity ever changes, so what species 1 holds is what it held, plus the sources, minus the sink
        src = sums["inject%d" % tv["feeds"].index(1)]
        want = [x + y - z for x, y, z in zip(ir.tally_fast(first["rows"][1][2]), [src["energy_fixed"]] + src["momentum_fixed"], [sums["remove0"]["energy_fixed"]] + sums["remove0"]["momentum_fixed"])]
        assert ir.tally_fast(rows(a, 1)[2]) == want, "the ledger of the 128-bit tallies"
        assert pop["n"] == model.N1 + src["injected"] - sums["remove0"]["removed"]
    for sim in (a, m):
        sim.destroy()
    print("turnover %s %s: %.2f s; injections held whole %d, within the reference's error %d" % (solver, precision, time.perf_counter() - t0, held[True], held[False]))


def test_rewinds(fp, tmp_path, monkeypatch):
    """files of three sizes loaded into a thinned and into a grown handle (stale slots behind n), beside a mate of another
    binning life; a grown file is refused by a fresh handle until it reserves"""
    t0 = time.perf_counter()
    sc = model.NAMED3["rewinds"]()
    rw = sc["rewinds"]
    a, m = build3(fp, sc, monkeypatch), build3(fp, sc, monkeypatch, mate=True)
    for sim in (a, m):
        start3(sim, sc)
    files, saved = [tmp_path / ("file%d.ckpt" % i) for i in range(3)], {}

    def both(where, call, check=None):
        before = snap(fp, a, sc)
        got = call(a)
        m.sort()
        assert exact(got) == exact(call(m)), (where, got)
        after = snap(fp, a, sc)
        assert_same(after, snap(fp, m, sc), "rewinds: " + where)
        if check:
            check(before, after, got)
        return after

    def save(i):
        a.saveCheckpoint(files[i])
        saved[i] = snap(fp, a, sc)

    def load(i):
        after = both("load file %d" % i, lambda s: s.loadCheckpoint(files[i]))
        assert after["pop"] == [dict(p, capacity=q["capacity"]) for p, q in zip(saved[i]["pop"], after["pop"])] and not thinned_of(after["pop"])
        assert all(same_rows(x, y) for x, y in zip(after["rows"], saved[i]["rows"])), ("rewinds: the rows of file", i)
        assert all(after["fields"][name] == saved[i]["fields"][name] for name in FIELD_KINDS if name in after["fields"])

    def removal(where, sp, req):
        def check(before, after, got):
            survivors, want = rr.remove(*before["rows"][sp], mass=sc["masses"][sp], charge=sc["charges"][sp], weight=sc["macro_weight"], **req)
            same_removal(got, want)
            assert same_rows(after["rows"][sp], survivors) and 0 < got["removed"] < before["pop"][sp]["n"], (where, got)
        return both(where, lambda s: s.remove(species=sp, **req), check)

    save(0)
    for sp, (src, count) in enumerate(zip(rw["sources"], rw["grow"])):
        both("reserve", lambda s: s.reserve(sp, sc["counts"][sp] + count))
        both("inject", lambda s: s.inject(species=sp, **src),
             lambda before, after, got: check_injection(sc, src, sp, (before["pop"][sp], before["rows"][sp]), (after["pop"][sp], after["rows"][sp]), got, "rewinds inject"))
    save(1)                                                                             # grown
    grown = [p["n"] for p in saved[1]["pop"]]
    assert grown[:2] == [sc["counts"][0] + rw["grow"][0], sc["counts"][1] + rw["grow"][1]]
    both("substeps", lambda s: s.substeps(rw["substeps"][0]))
    after = removal("the thinning removal", 0, rw["remove"])
    assert thinned_of(after["pop"]) == [0] and after["pop"][0]["n"] > sc["counts"][0]
    refused(fp, lambda: a.saveCheckpoint(tmp_path / "refused.ckpt"), -5, "fpic_renumber")
    load(0)                                                                             # into the thinned handle: n shrinks, stale slots behind it
    both("substeps", lambda s: s.substeps(rw["substeps"][1]))
    load(1)                                                                             # n grows again within the capacity
    both("substeps", lambda s: s.substeps(rw["substeps"][2]))
    after = removal("the halving removal", 0, rw["odd"])
    if after["pop"][0]["n"] % 2 == 0:                                                   # down to an odd n: the particle of the smallest id leaves too
        x0 = float(after["rows"][0][1][0, 0])
        after = removal("one more", 0, dict(where={"x": (x0, float(np.nextafter(after["rows"][0][1].dtype.type(x0), 2)))}))
    assert after["pop"][0]["n"] % 2 == 1

    def renumbered(before, after, got):
        assert got == [len(r[0]) for r in before["rows"][:2]] and not thinned_of(after["pop"])
        for r0, r1 in zip(before["rows"][:2], after["rows"][:2]):
            assert g1.bits(r1[0], np.arange(len(r0[0]), dtype=np.uint32)) and g1.bits(r1[1], r0[1]) and g1.bits(r1[2], r0[2])
        assert all(after["fields"][name] == before["fields"][name] for name in after["fields"])
    both("renumber", lambda s: [s.renumber(sp) for sp in range(2)], renumbered)
    save(2)
    both("substeps", lambda s: s.substeps(rw["substeps"][3]))
    fresh = build3(fp, sc, monkeypatch)
    start3(fresh, sc)
    held = snap(fp, fresh, sc)
    refused(fp, lambda: fresh.loadCheckpoint(files[1]), -1, "fpic_reserve")             # the grown file, without reserve: nothing changed
    assert_same(held, snap(fp, fresh, sc), "rewinds: a refused load")
    for sp in range(2):
        fresh.reserve(sp, grown[sp])
    fresh.loadCheckpoint(files[1])
    assert all(same_rows(x, y) for x, y in zip(snap(fp, fresh, sc)["rows"], saved[1]["rows"]))
    fresh.loadCheckpoint(files[2])                                                      # and the file of the odd, renumbered species
    assert all(same_rows(x, y) for x, y in zip(snap(fp, fresh, sc)["rows"], saved[2]["rows"]))
    fresh.substeps(rw["substeps"][3])
    assert_same(snap(fp, a, sc), dict(snap(fp, fresh, sc), pop=snap(fp, a, sc)["pop"]), "rewinds: the fresh handle after file 2", names=FIELD_KINDS)
    for sim in (a, m, fresh):
        sim.destroy()
    print("rewinds: %.2f s" % (time.perf_counter() - t0))


def test_hook_overflow(fp, monkeypatch):
    """a registered source whose third application does not fit: substeps(5) raises FPIC_ERR_STATE naming fpic_reserve (an API
    error, no GPU fault) and leaves the handle the mate is in after three manual sub-steps with the hook's operators up to and
    excluding that source; after reserve() the run goes on"""
    t0 = time.perf_counter()
    sc = model.NAMED3["hook_overflow"]()
    hk = sc["hook"]
    a, m = build3(fp, sc, monkeypatch, capacities=sc["capacities"]), build3(fp, sc, monkeypatch, mate=True, capacities=sc["capacities"])
    for sim in (a, m):
        start3(sim, sc)
    ce = hk["collide"]
    assert a.collideEvery(1, ce["kind"], species=ce["species"], **ce["kw"]) == 0
    assert a.removeEvery(1, where=hk["sink"]["where"], species=hk["sink"]["species"]) == 0
    for i, src in enumerate(hk["sources"]):
        assert a.injectEvery(1, species=src["species"], **src["kw"]) == i
    applied, t = [0, 0], 0

    def manual(k, fits):
        nonlocal t
        for _ in range(k):
            m.sort()
            m.substeps(1)
            t += 1
            m.collide(ce["kind"], species=ce["species"], **dict(ce["kw"], epoch=t + ce["kw"]["epoch"]))
            m.remove(where=hk["sink"]["where"], species=hk["sink"]["species"])
            for i, src in enumerate(hk["sources"]):
                pop = m.population(src["species"])
                if ir.fits(pop["n"], pop["capacity"], pop["id_span"], src["kw"]["count"]):
                    m.inject(species=src["species"], **dict(src["kw"], epoch=src["kw"]["epoch"] + applied[i]))
                    applied[i] += 1
                else:
                    assert not fits and i == 1 and t == 3, (t, i, pop)

    before = snap(fp, a, sc)
    refused(fp, lambda: a.substeps(5), -5, "fpic_reserve")
    manual(3, fits=False)
    after = snap(fp, a, sc)
    assert_same(after, snap(fp, m, sc), "hook_overflow: after the refused sub-step")
    assert applied == [3, 2] and [a.injectStats(i)["applications"] for i in range(2)] == applied and a.removeStats(0)["applications"] == 3 and a.collisionStats(0)["applications"] == 3
    assert after["pop"][1] == dict(n=model.N1 + 2 * 96, capacity=sc["capacities"][1], id_span=model.N1 + 2 * 96) and not g1.bits(after["rows"][0][2], before["rows"][0][2])
    for sim in (a, m):
        assert sim.reserve(1, model.N1 + 5 * 96) == model.N1 + 5 * 96
    a.substeps(2)
    manual(2, fits=True)
    assert_same(snap(fp, a, sc), snap(fp, m, sc), "hook_overflow: after reserve")
    assert applied == [5, 4] and a.population(1)["n"] == model.N1 + 4 * 96
    for sim in (a, m):
        sim.destroy()
    print("hook_overflow: %.2f s" % (time.perf_counter() - t0))


# ---------------------------------------------------------------------------------------------- the resumes
def clear_all(sim):
    for call in ("clearCollisions", "clearForces", "clearGas", "clearPairs", "clearFusion", "clearFusionSpectra", "clearRemovals", "clearInjections"):
        getattr(sim, call)()


@pytest.mark.parametrize("sink", [False, True], ids=["source", "source_and_sink"])
@pytest.mark.parametrize("solver,precision", model.RESUME)
def test_a_run_with_sources_and_sinks_resumes_bit_for_bit(fp, tmp_path, monkeypatch, solver, precision, sink):
    """(i) a source alone beside the generation-2 families (the species grow, none is thinned): N sub-steps in one run against
    T and N - T through a file and a fresh handle that reserves, then registers with epoch = the applications made so far.
    (ii) with a sink as well a thinned species has no file: both runs clear every registration at T, renumber and register
    again; only one of them goes through the file."""
    t0 = time.perf_counter()
    sc = model.resume_scene3(solver, precision, sink)
    t, n = model.RESUME_T, model.RESUME_N
    made = [t // op["every"] for op in sc["inject_every"]]
    whole, first, rest = (build3(fp, sc, monkeypatch, capacities=sc["capacities"]) for _ in range(3))
    for sim in (whole, first):
        start3(sim, sc)
        register3(sim, sc)
    if sink:
        for sim in (whole, first):
            sim.substeps(t)
            assert thinned_of([sim.population(0)]) == [0]
            part = stats3_of(sim, sc)
            clear_all(sim)
            assert [sim.renumber(sp) for sp in range(2)] == [sim.population(sp)["n"] for sp in range(2)]
        register3(whole, sc, shift=0, applied=made)      # (its own count of sub-steps goes on: no shift but the sources')
        whole.substeps(n - t)
    else:
        whole.substeps(n)
        first.substeps(t)
        part = stats3_of(first, sc)
    first.saveCheckpoint(tmp_path / "cut.ckpt")
    rest.loadCheckpoint(tmp_path / "cut.ckpt")
    register3(rest, sc, shift=t, applied=made)
    rest.substeps(n - t)
    sw, sr = snap(fp, whole, sc), snap(fp, rest, sc)
    assert_same(sw, sr, "resume")
    assert not same_rows(snap(fp, first, sc)["rows"][0], sr["rows"][0])
    total, tail = stats3_of(whole, sc), stats3_of(rest, sc)
    for key in families_of(sc):
        assert (tail[key] if sink else g2.plus(part[key], tail[key])) == total[key], (key, {k: v for k, v in total[key].items() if k != "grid"})
    assert all(total["inject%d" % i]["injected"] == op["kw"]["count"] * ((n - t if sink else n) // op["every"]) > 0 for i, op in enumerate(sc["inject_every"]))
    assert not sink or (part["remove0"]["removed"] > 0 and total["remove0"]["removed"] > 0)
    assert [p["n"] for p in sw["pop"][:2]] == [sc["counts"][sp] + sc["inject_every"][sp]["kw"]["count"] * (n // 2) - (part["remove0"]["removed"] + total["remove0"]["removed"] if sink and sp == 0 else 0)
                                               for sp in range(2)]
    for sim in (whole, first, rest):
        sim.destroy()
    print("generation 3 resume %s %s sink=%s: %.2f s" % (solver, precision, sink, time.perf_counter() - t0))
