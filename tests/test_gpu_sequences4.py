"""Generation 4 of the random call sequences on the CART3D box: the ioniser and the burner — ionize() / ionizeEvery(), burn() /
burnEvery(), the operators that couple the most state (a burner is a sink on two species and a source on up to two others in
one application; an ioniser appends to two species, one of which may be its own projectile species) — among every operator and
read of generations 1 to 3, whose helpers this module uses.  tests/sequence_model.py (generation 4) turns a seed into the scene
(generation 3's, with the product species, a separate electron species on half the seeds and the two targets of the refusals
behind its own) and the steps; tests/test_sequence_model.py proves on the CPU that the committed SEEDS4 reach the states meant
here and that no committed burn or ionisation is vacuous on the initial particles.  Everything below is equality bit for bit
or of exact integers, but for the ioniser's rounded velocities, which lie within tests/test_gpu_ionize.py's value_bound (fp32:
plus half a float spacing): that module's own statement of the reference's error, no new number.

The relations are generation 3's (tests/test_gpu_sequences3.py): 1, the fresh twin from saveCheckpoint whenever nobody is
thinned; 1T, the mate from the start of every scene, which lives the other binning life and sorts before every operation —
with operators registered on A and C the mate does the hook by hand in the hook's full order: generation 3's, then the
ionisers in registration order, then the burners in registration order (the second burns the first one's products of the same
sub-step: the chain), then the recorder rows; A's ionizeStats and burnStats are the integer sums of the mate's one-shot
results; 2, the unread copy at the midpoint and at the end.

The references, on A's select() rows read just before the call: a burn step against burn_reference.application — every count,
every fixed-point word of the four groups and the doubles derived from them, the survivors of both reactants (rows, ids,
order), the products' ids (id span + l in ascending id of the species_a reactant), positions and stored velocities, accepted ==
burnt + blocked, the other species untouched: no tolerance, the rule has no transcendental (tests/test_gpu_burn.py); an
ionise step against ionize_reference.application — the event set and the counts, the new ids and their places, the copied
positions, the three groups of exact tallies exactly, the rounded velocities within value_bound.  The events are the
reference's: the replay reserves every target to n + events (an exact fit) on a scene without registered operators, to its
capacity plus the events on one with; the target of ionize_refused / burn_refused is one slot short and the call raises
FPIC_ERR_INVALID_ARG naming fpic_reserve with rows, fields, populations and sort_passes as they were; ionize_nothing /
burn_nothing return their counts and change nothing.  The hook's applications are held the same way, on the mate's one-shot
calls.  On an electrostatic handle whose charge grid is current the grid's integer sum is the same after an ionisation; after
a burn it is the sum over the species of Z N (read3).  While a burn has left a species thinned, saveCheckpoint and every
caller-order call on it are refused naming fpic_renumber; renumber with burners and ionisers registered is refused (A names
its series first, C "registered", as in generation 3).  At run time every burn kind with events has 4 <= burnt and leaves
somebody of every reactant, every ionize has ionised > 0.

What the model does otherwise than one might expect.  On a scene with registered operators the product species p3 is emptied
before the run (thinned from the start): the second burner's reactant is then thinned whatever the first has produced, and the
model knows who is thinned without knowing when the chain first reacts; no save is possible there, so relation 1 rests on
the seven scenes without registered operators.  The forced block of every seed ends with a removal of every second id of p3:
every later burn of the seed puts its products into a thinned species.  The refusals have two species of their own (a capacity
only grows).  g_threshold lies at or below the table's start, as the library requires.  burner_fails_behind_an_ioniser takes
the room from the mate's own events, so the third application is EXACTLY one slot short.

The named scenes: chain (a like burner on species 0 into species 2 and 3, an unlike burner on species 2 with 1, an ioniser
whose projectiles are species 2; twenty sub-steps in pieces of 1, 2, 3 and 5, each operator with events on at least three;
the `none` case carries the ledger of the 128-bit tallies of all five species), reserve_after_register, hook_order,
burner_fails_behind_an_ioniser; and the 2 x 2 resumes.

What the sequences found: nothing.  Seed 103 was replaced by 13 (its burn_like on the 750 ions had 2 events
on the GPU); no seed reached a fault or a disagreement.

Wall times on an MI355X, one run of the module on its own (18.6 s in all; tests/test_gpu_sequences3.py on its own in the same
session: 11.4 s — 1.6 times generation 3's, with up to four more species, 26 to 34 steps a seed and a reference per
application of the hook):
    relations 1, 1T and 2, 12 seeds    13.5 s together: 0.56 to 1.28 s each, 2.8 s and 2.4 s for the first `none` / full-EM and
                                       the first electrostatic seed of the process (the libraries and code objects are loaded there)
    chain, 2 cases                     0.7 s together
    reserve_after_register             0.12 s
    hook_order, 2 precisions           0.15 s together
    burner_fails_behind_an_ioniser     0.12 s
    the resumes, 2 x 2                 0.4 s together
In that run all 101 fp32 applications of an ioniser with events (one-shot and the hook's) stored the rounded reference's
bits; the largest fp64 |dv| / bound was 0.352.
A negative control of the whole construction, run once by hand and not kept: with fpic_burn giving a product the ids n + l
instead of id span + l (a value, never an address: the ids stay below the id span, a product species that is not thinned is
untouched) 14 of the 22 tests fail.  All twelve seeds: the five with registered operators (0, 2, 12, 111, 129) at an
application of the first burner into the emptied p3 on sub-step 2 or 3, where the mate's application is held to
burn_reference.application ("product_a": the new ids); of the seven without, which fail at their first burn behind the
product's removal, five (13, 21, 131, 165, 187) at the comparison with the mate — two rows of one id come back in slot order:
"position of species" 2 or 3 — and two (59 at step 25 burn_untracked, 149 at step 20 burn_like) against
burn_reference.application on A.  Both chains fail in the same way as the registered seeds, once the second burner has thinned
species 2.  What passes: reserve_after_register, hook_order (2), burner_fails_behind_an_ioniser and the four resumes, none of
which burns into a thinned product (the resumes renumber at the cut).  Before the product's removal was added to the block
only the five seeds with registered operators noticed (7 of 22 tests), which is why it was added.
Of the single-operation modules, tests/test_gpu_burn.py sees it in test_a_product_species_that_starts_empty alone (its other
37 tests pass).
"""
import time

import numpy as np
import pytest

import burn_reference as bref
import sequence_model as model
import test_gpu_sequences as g1
import test_gpu_sequences3 as g3
from test_gpu_burn import check_against
from test_gpu_ionize import check_application as check_ionisation
from test_gpu_remove import refused
from test_gpu_sequences2 import add_ints, equal_sums, exact
from test_gpu_sequences3 import apply3, assert_same, build3, check_new_kind, manual_substeps3, read3, rows, same_rows, snap, start3, thinned_of

pytestmark = pytest.mark.gpu

BURN_KINDS = model.BURN_KINDS4 + ("burn_nothing", "burn_refused")


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


# ---------------------------------------------------------------------------------------------- handles, registration, totals
def start4(sim, sc):
    """start3, and the species a scene empties before the run (a product species that starts empty: thinned from here on)"""
    start3(sim, sc)
    for sp in sc.get("empty", []):
        assert sim.remove(species=sp)["removed"] == sc["counts"][sp] and sim.population(sp)["n"] == 0


def flat(got):
    """the exact integers of an ionize or burn result: the counts, and the fixed-point words of every group under group.word"""
    out = {}
    for k, v in got.items():
        if isinstance(v, dict):
            out[k + ".energy_fixed"], out[k + ".momentum_fixed"] = v["energy_fixed"], list(v["momentum_fixed"])
        elif isinstance(v, int) and not isinstance(v, bool):
            out[k] = v
    return out


def ionize_call(sim, op, epoch=None):
    kw = dict(op["kw"], epoch=op["kw"]["epoch"] if epoch is None else epoch)
    return sim.ionize(electron=op["electron"], ion=op["ion"], g_threshold=op["g_threshold"], **kw)


def burn_call(sim, op, epoch=None):
    kw = dict(op["kw"], epoch=op["kw"]["epoch"] if epoch is None else epoch)
    return sim.burn(op["a"], op["b"], products=tuple(op["products"]), q_value=op["q_value"], other_mass=op["other_mass"], **kw)


def register4(sim, sc, shift=0, applied=None):
    g3.register3(sim, sc, shift, applied)
    register_new(sim, sc, shift)


def register_new(sim, sc, shift=0):
    for i, op in enumerate(sc.get("ionize_every", [])):
        assert sim.ionizeEvery(op["every"], electron=op["electron"], ion=op["ion"], g_threshold=op["g_threshold"], **dict(op["kw"], epoch=op["kw"]["epoch"] + shift)) == i
    for i, op in enumerate(sc.get("burn_every", [])):
        assert sim.burnEvery(op["every"], op["a"], op["b"], products=tuple(op["products"]), q_value=op["q_value"], other_mass=op["other_mass"],
                             **dict(op["kw"], epoch=op["kw"]["epoch"] + shift)) == i


def new_families(sc):
    return tuple("ionize%d" % i for i in range(len(sc.get("ionize_every", [])))) + tuple("burn%d" % i for i in range(len(sc.get("burn_every", []))))


def families4(sc):
    return (g3.families_of(sc) if "collide_every" in sc else ()) + new_families(sc)


def new_stats(sim, sc):
    out = {"ionize%d" % i: flat(sim.ionizeStats(i)) for i in range(len(sc.get("ionize_every", [])))}
    out.update({"burn%d" % i: flat(sim.burnStats(i)) for i in range(len(sc.get("burn_every", [])))})
    return out


def stats4_of(sim, sc):
    return dict(g3.stats3_of(sim, sc) if "collide_every" in sc else {}, **new_stats(sim, sc))


# ---------------------------------------------------------------------------------------------- one application against its reference
def held_of(sim, species):
    return {k: (rows(sim, k), sim.population(k)) for k in species if k is not None}


def state_of_rows(held, sc):
    return {k: dict(frac=r[1], vel=r[2], cell=model.cells_of(r[1], sc["shape"]), ids=r[0].astype(np.int64)) for k, (r, _) in held.items()}


def burn_reference_of(sc, op, held, epoch=None):
    """burn_reference.application of a request to the rows `held` ({species: (rows, population)})"""
    p3, p4 = op["products"]
    pops = [(held[k][1]["n"], held[k][1]["id_span"]) if k is not None else (0, 0) for k in (p3, p4)]
    return model.burn_want(sc, state_of_rows(held, sc), op, epoch=epoch, pops=pops)[1]


def ionize_reference_of(sc, op, held, epoch=None):
    pops = [(held[k][1]["n"], held[k][1]["id_span"]) for k in (op["electron"], op["ion"])]
    return model.ionize_want(sc, state_of_rows(held, sc), op, epoch=epoch, pops=pops)


def check_burn(sim, sc, op, held, got, app, where):
    a, b, (p3, p4) = op["a"], op["b"], op["products"]
    try:
        check_against(sim, app, (a, b, p3, p4), held, got, sc["masses"], sc["charges"], weight=sc["macro_weight"], other=(op["other_mass"], 0.0))
    except AssertionError as e:
        raise AssertionError((where, "a burn against burn_reference.application") + e.args) from e


def check_ionize(sim, sc, op, held, got, epoch, figures, where):
    """test_gpu_ionize.check_application on this box; figures[precision]: [applications, those whose every stored velocity is
    the rounded reference's bits] in fp32, the largest |dv| / bound in fp64"""
    e, i, p = op["electron"], op["ion"], op["species"]
    kw = dict({k: v for k, v in op["kw"].items() if k != "species"}, g_threshold=op["g_threshold"], epoch=op["kw"]["epoch"] if epoch is None else epoch)
    try:
        worst = check_ionisation(sim, sc["precision"], kw, e, held[p][0], [held[e], held[i]], got, ion=i, lengths=sc["L"], weight=sc["macro_weight"],
                                 masses=(sc["masses"][p], sc["masses"][e], sc["masses"][i]), charges=(sc["charges"][p], sc["charges"][e], sc["charges"][i]), projectile=p)
    except AssertionError as err:
        raise AssertionError((where, "an ionisation against ionize_reference.application") + err.args) from err
    if got["ionised"]:
        if sc["precision"] == "fp32":
            figures["fp32"][0] += 1
            figures["fp32"][1] += worst == 0.0
        else:
            figures["fp64"] = max(figures["fp64"], worst)


def new_figures():
    return dict(fp32=[0, 0], fp64=0.0, hook_ionised=0, hook_burnt=[0, 0])


def hook_tail(sc, sums, figures, check=True):
    """the hook's last operators by hand on the mate, behind the sources: the ionisers in registration order, then the burners
    in registration order, each application held to its reference on the mate's own rows"""
    def tail(m, t):
        for i, op in enumerate(sc.get("ionize_every", [])):
            if t % op["every"] == 0:
                epoch = t + op["kw"]["epoch"]
                held = held_of(m, {op["species"], op["electron"], op["ion"]}) if check else None
                got = ionize_call(m, op, epoch)
                if check:
                    check_ionize(m, sc, op, held, got, epoch, figures, "ioniser %d at sub-step %d" % (i, t))
                add_ints(sums["ionize%d" % i], flat(got))
                figures["hook_ionised"] += got["ionised"]
        for i, op in enumerate(sc.get("burn_every", [])):
            if t % op["every"] == 0:
                epoch = t + op["kw"]["epoch"]
                if check:
                    held = held_of(m, {op["a"], op["b"]} | set(op["products"]))
                    app = burn_reference_of(sc, op, held, epoch)
                got = burn_call(m, op, epoch)
                if check:
                    check_burn(m, sc, op, held, got, app, "burner %d at sub-step %d" % (i, t))
                add_ints(sums["burn%d" % i], flat(got))
                figures["hook_burnt"][i] += got["burnt"]
    return tail


# ---------------------------------------------------------------------------------------------- the steps of the new kinds
def resolve4(sc, st, before):
    """what a step of a new kind takes that depends on A's state: the reference's application on A's rows, and the capacities
    its targets are reserved to first"""
    held = {k: (before["rows"][k], before["pop"][k]) for k in range(len(sc["counts"]))}
    if st["kind"] in model.IONIZE_KINDS4:
        req, app = ionize_reference_of(sc, st, held)
    else:
        app = burn_reference_of(sc, st, held)
    reserve = model.resolve_events4(st, before["pop"], app["m"], sc["registered"])
    if st["kind"] in ("ionize_refused", "burn_refused"):
        short = st["short"]
        assert app["m"] >= 1 and reserve[short] >= before["pop"][short]["capacity"], ("the refusal's target has more room than one slot short", app["m"], before["pop"][short])
    return dict(app=app, held=held, reserve=reserve)


def reserve4(sim, res):
    for sp, cap in sorted(res["reserve"].items()):
        sim.reserve(sp, cap)


def call4(fp, sim, sc, st):
    kind = st["kind"]
    call = (lambda: ionize_call(sim, st)) if kind in model.IONIZE_KINDS4 else (lambda: burn_call(sim, st))
    if kind in ("ionize_refused", "burn_refused"):
        return refused(fp, call, -1, "fpic_reserve", "nothing was changed")
    return call()


def apply4(fp, sim, sc, st, res, files, shift=0, registered=True, recording=False):
    if st["kind"] in model.NEW_KINDS4:
        return call4(fp, sim, sc, st)
    return apply3(fp, sim, sc, st, res, files, shift=shift, registered=registered, recording=recording)


def deposits4(sc, st, got):
    if st["kind"] not in model.NEW_KINDS4:
        return g3.deposits3(sc, st, got)
    events = got is not None and (got.get("ionised", 0) > 0 or got.get("burnt", 0) > 0)
    return {"rho"} if sc["solver"] == "poisson_fft" and events else set()


def charge_sum(fp, sim):
    return int(sim.readField(fp.F3_RHO_FIXED).astype(object).sum())


def check_kind4(fp, a, sc, st, res, got, before, after, passes, rho_current, figures, where):
    """a step of a generation-4 kind on A against its reference"""
    kind, app, held = st["kind"], res["app"], res["held"]
    touched = {0, st["electron"], st["ion"]} if kind in model.IONIZE_KINDS4 else {st["a"], st["b"]} | set(st["products"])
    for s in range(len(sc["counts"])):
        if s not in touched:
            assert same_rows(before["rows"][s], after["rows"][s]) and before["pop"][s] == after["pop"][s], (where, "another species changed", s)
    if kind in ("ionize_refused", "burn_refused", "ionize_nothing", "burn_nothing"):
        assert a.stats()["sort_passes"] == passes, where
        assert_same(before, after, where + " (nothing may change)")
        if kind == "ionize_nothing":
            assert got["ionised"] == 0 and got["candidates"] == int(app["candidate"].sum()) > 0 and got["below"] == got["candidates"], (where, got)
        elif kind == "burn_nothing":
            assert got["burnt"] == 0 == got["accepted"] and {k: got[k] for k in ("pairs", "below", "above", "cells")} == {k: app[k] for k in ("pairs", "below", "above", "cells")}, (where, got)
        return
    if kind == "ionize":
        check_ionize(a, sc, st, held, got, None, figures, where)
        assert got["ionised"] > 0, (where, "a vacuous ionisation at run time: replace the seed", got)
        if rho_current:      # an electron and an ion of opposite charge at one place: the grid's integer sum stays
            assert int(np.frombuffer(after["fields"]["rho"], dtype=np.int64).astype(object).sum()) == int(np.frombuffer(before["fields"]["rho"], dtype=np.int64).astype(object).sum()), (where, "the charge")
    else:
        check_burn(a, sc, st, held, got, app, where)
        left = [after["pop"][st["a"]]["n"]] + ([after["pop"][st["b"]]["n"]] if st["b"] is not None else [])
        assert got["burnt"] >= 4 and min(left) >= 1 and got["accepted"] == got["burnt"] + got["blocked"], (where, "a vacuous burn at run time: replace the seed", got["burnt"], left)
        if st["saturated"]:
            assert got["saturated"] > 0 and got["blocked"] > 0, (where, got)


def read4(fp, a, sc, r, files, tmp_path, rho_current, sums, thinned, where):
    if r["kind"] in ("ionizeStats", "burnStats"):
        have = new_stats(a, sc)
        assert all(equal_sums(have[key], sums[key]) for key in have if key.startswith(r["kind"][:-5])), (where, have)
        return
    return read3(fp, a, sc, r, files, tmp_path, rho_current, sums, thinned, where)


# ---------------------------------------------------------------------------------------------- relations 1, 1T and 2
def run_sequence4(fp, sc, steps, tmp_path, monkeypatch):
    total = model.substeps_of(steps)
    caps = model.reserved4(sc, total) if sc["registered"] else None
    a, c, m = build3(fp, sc, monkeypatch, capacities=caps), build3(fp, sc, monkeypatch, capacities=caps), build3(fp, sc, monkeypatch, mate=True, capacities=caps)
    for sim in (a, c, m):
        start4(sim, sc)
    if sc["registered"]:
        register4(a, sc)
        register4(c, sc)
        g3.record3(a, sc)
    sums, due, applied = {k: {} for k in families4(sc)}, dict(energy=[], series=[], modes=[]), [0] * len(sc.get("inject_every", []))
    files, t, twins, mated, held3, figures = [], 0, 0, 0, {True: 0, False: 0}, new_figures()
    tail = hook_tail(sc, sums, figures)
    passes0 = a.stats()["sort_passes"]
    rho_current = not (sc.get("empty") and sc["solver"] == "none")      # (under a given field the emptying removal deposits nothing)
    before = snap(fp, a, sc)
    for index, st in enumerate(steps):
        kind = st["kind"]
        where = "seed %d step %d %s" % (sc["seed"], index, kind)
        new = kind in model.NEW_KINDS4
        thinned = thinned_of(before["pop"])
        assert thinned == st["thinned"], (where, "the model's thinned species", thinned, st["thinned"])
        if new:
            res = resolve4(sc, st, before)
            for sim in (a, c, m):      # (a reserve changes no row and no field: tests/test_gpu_sequences3.py holds that)
                reserve4(sim, res)
            before["pop"] = [a.population(sp) for sp in range(len(sc["counts"]))]
        else:
            res = g3.resolve(sc, st, before["pop"])
        manual = kind == "substeps" and sc["registered"]
        if thinned:
            refused(fp, lambda: a.saveCheckpoint(tmp_path / "refused.ckpt"), -5, "fpic_renumber")
        b = None if thinned or manual else g3.twin3(fp, sc, a, tmp_path / "twin.ckpt", monkeypatch, before["pop"])
        passes = a.stats()["sort_passes"]
        got_a = apply4(fp, a, sc, st, res, files, recording=sc["registered"])
        apply4(fp, c, sc, st, res, files)
        m.sort()
        if manual:
            t = manual_substeps3(fp, m, sc, st["k"], t, sums, due, applied, held3, tail=tail)
        else:
            got_m = apply4(fp, m, sc, st, res, files, registered=False)
            assert exact(got_a) == exact(got_m), (where, "A and the mate", got_a, got_m)
            t += st.get("k", 0)
        face_b = model.compares_face_b(index)
        after = snap(fp, a, sc, face_b=face_b)
        assert_same(after, snap(fp, m, sc, face_b=face_b), where + " (the mate)")
        mated += bool(thinned)
        fresh = deposits4(sc, st, got_a) | ({"rho"} if sc["solver"] == "yee" else set())
        for name in after["fields"]:
            if name in ("rho", "J") and name not in fresh and name in before["fields"]:
                assert after["fields"][name] == before["fields"][name], (where, name, "written by an operation that deposits nothing")
        if b is not None:
            got_b = apply4(fp, b, sc, st, res, files, shift=t - st.get("k", 0), registered=False)
            assert exact(got_a) == exact(got_b), (where, "A and the fresh twin", got_a, got_b)
            assert_same(after, snap(fp, b, sc, face_b=face_b), where + " (the fresh twin)", names=g3.FIELD_KINDS + tuple(fresh))
            b.destroy()
            twins += 1
        if st["refused"]:
            assert a.stats()["sort_passes"] == passes, where
            assert_same(before, after, where + " (refused)")
        elif new:
            check_kind4(fp, a, sc, st, res, got_a, before, after, passes, rho_current and sc["solver"] == "poisson_fft", figures, where)
        elif kind in model.NEW_KINDS3:
            check_new_kind(fp, a, sc, st, res, got_a, before, after, passes, rho_current and sc["solver"] != "yee", where, held3)
        elif kind.startswith("gas_"):
            want = model.gas_want(sc, g3.state_of(before, sc), st["what"], st["kw"])
            assert {k: got_a[k] for k in ("candidates", "collided", "below", "above")} == want, (where, got_a, want)
        elif kind in ("load", "load_profile", "load_radial"):
            assert got_a == res["range"][1], (where, got_a)
        elif kind.startswith("force_"):
            assert st["t"] == t and got_a["applications"] == int(st["active"]), (where, st["t"], t, got_a)
        assert thinned_of(after["pop"]) == st["thinned_after"], (where, "the model's thinned species afterwards", thinned_of(after["pop"]), st["thinned_after"])
        changed_n = kind in model.REMOVE_KINDS3 + model.INJECT_KINDS3 + ("ionize",) + model.BURN_KINDS4
        if fresh & {"rho"} and sc["solver"] != "yee":
            rho_current = True
        elif (kind in model.POSITION_KINDS2 and st["what"] != "velocity" and not st["refused"]) or kind == "loadCheckpoint" or sc["solver"] == "yee" or \
                (changed_n and sc["solver"] == "none"):
            rho_current = False
        if manual and sc["solver"] == "none":
            rho_current = False
        before = after
        for r in st["reads"]:
            read4(fp, a, sc, r, files, tmp_path, rho_current and sc["solver"] != "yee", sums, st["thinned_after"], where + " read " + r["kind"])
        if index == len(steps) // 2 or index == len(steps) - 1:
            end = index == len(steps) - 1
            sa, sc_ = snap(fp, a, sc, density=end, face_b=end), snap(fp, c, sc, density=end, face_b=end)
            assert_same(sa, sc_, where + " (A and C)", names=None if end else [name for name in sa["fields"] if not (name == "rho" and sc["solver"] == "yee")])
            before = sa if end else before
    assert a.stats()["sort_passes"] > passes0 and mated > 0 and (sc["registered"] or twins > 0), (sc["seed"], mated, twins)
    if sc["registered"]:
        g3.end_of_registered_run(a, c, sc, sums, due, t, families=families4, stats=stats4_of)
        io, burners = sc["ionize_every"][0], sc["burn_every"]
        assert sums["ionize0"]["applications"] == t // io["every"] >= 3 and sums["ionize0"]["ionised"] > 0, sums["ionize0"]
        assert all(sums["burn%d" % i]["applications"] == t // op["every"] >= 3 for i, op in enumerate(burners)) and sums["burn0"]["burnt"] > 0      # (no application of the hook was refused)
    for sim in (a, c, m):
        sim.destroy()
    return figures, held3


def report(name, sc, t0, figures):
    print("%s (%s %s): %.2f s; fp32 ionisations bit-equal to the rounded reference %d of %d, largest fp64 |dv| / bound %.3f; the hook ionised %d, burnt %s"
          % (name, sc["solver"], sc["precision"], time.perf_counter() - t0, figures["fp32"][1], figures["fp32"][0], figures["fp64"], figures["hook_ionised"], figures["hook_burnt"]))


@pytest.mark.parametrize("seed", model.SEEDS4)
def test_generation_4_ionisation_and_burn_among_everything_else(fp, tmp_path, monkeypatch, seed):
    t0 = time.perf_counter()
    sc = model.scene4(seed)
    figures, _ = run_sequence4(fp, sc, model.sequence4(seed), tmp_path, monkeypatch)
    report("generation 4 seed %d" % seed, sc, t0, figures)


# ---------------------------------------------------------------------------------------------- the named scenes
def pair_of(fp, sc, monkeypatch, capacities=None):
    """A and the mate of a named scene, started"""
    a, m = build3(fp, sc, monkeypatch, capacities=capacities or sc["capacities"]), build3(fp, sc, monkeypatch, mate=True, capacities=sc["capacities"])
    for sim in (a, m):
        start4(sim, sc)
    return a, m


def same_but_capacity(x, y, where):
    """assert_same of two snapshots whose handles were given different room"""
    assert_same(dict(x, pop=[dict(p, capacity=0) for p in x["pop"]]), dict(y, pop=[dict(p, capacity=0) for p in y["pop"]]), where)


def tally(vel):
    g = bref.iref.gain(vel)
    return [g["energy_fixed"]] + g["momentum_fixed"]


def words(sums, key, group):
    return [sums[key].get(group + ".energy_fixed", 0)] + sums[key].get(group + ".momentum_fixed", [0, 0, 0])


@pytest.mark.parametrize("solver,precision", model.CHAIN_CASES)
def test_chain(fp, tmp_path, monkeypatch, solver, precision):
    """the second burner burns what the first has made on the same sub-step, and the ioniser's projectiles are the first
    burner's products: A has all three registered, the mate applies them by hand (every application against its reference) and
    lives another binning life; the `none` case balances the ledger of every species word for word"""
    t0 = time.perf_counter()
    sc = model.NAMED4["chain"](solver, precision)
    roles = sc["roles"]
    a, m = pair_of(fp, sc, monkeypatch)
    register_new(a, sc)
    first = snap(fp, a, sc)
    sums, figures, t = {k: {} for k in families4(sc)}, new_figures(), 0
    tail = hook_tail(sc, sums, figures)
    active = {k: 0 for k in sums}
    for index, k in enumerate(sc["pieces"]):
        a.substeps(k)
        for _ in range(k):
            m.sort()
            m.substeps(1)
            t += 1
            was = {key: sums[key].get("ionised", 0) + sums[key].get("burnt", 0) for key in sums}
            tail(m, t)
            for key in sums:
                active[key] += sums[key].get("ionised", 0) + sums[key].get("burnt", 0) > was[key]
        sa = snap(fp, a, sc)
        assert_same(sa, snap(fp, m, sc), "chain %s %s piece %d" % (solver, precision, index))
        have = new_stats(a, sc)
        assert all(equal_sums(have[key], sums[key]) for key in have), ("chain piece", index)
        assert a.energy()["count"].tolist() == [p["n"] for p in sa["pop"]]
    assert t == 20 and all(n >= 3 for n in active.values()), ("every operator has events on at least three sub-steps", active)
    assert thinned_of(sa["pop"]) == [0, 1, roles["p3"]], sa["pop"]
    refused(fp, lambda: a.saveCheckpoint(tmp_path / "refused.ckpt"), -5, "fpic_renumber")
    refused(fp, lambda: a.renumber(0), -5, "registered")
    if sc["zero_field"]:      # the ledger: no velocity changes but by the three operators
        now = [tally(r[2]) for r in sa["rows"]]
        was = [tally(r[2]) for r in first["rows"]]
        z = [0, 0, 0, 0]
        gains = {0: z, 1: words(sums, "ionize0", "ion"), roles["p3"]: [x + y for x, y in zip(words(sums, "burn0", "product_a"), words(sums, "ionize0", "primary"))],
                 roles["p4"]: [x + y for x, y in zip(words(sums, "burn0", "product_b"), words(sums, "burn1", "product_a"))], roles["electron"]: words(sums, "ionize0", "electron")}
        losses = {0: words(sums, "burn0", "reactant_a"), 1: words(sums, "burn1", "reactant_b"), roles["p3"]: words(sums, "burn1", "reactant_a"), roles["p4"]: z, roles["electron"]: z}
        for sp in range(len(sc["counts"])):
            assert now[sp] == [w + g - l for w, g, l in zip(was[sp], gains[sp], losses[sp])], ("the ledger of the 128-bit tallies of species", sp)
        assert words(sums, "burn0", "reactant_b") == z
    for sim in (a, m):
        sim.destroy()
    report("chain", sc, t0, figures)


def test_reserve_after_register(fp, monkeypatch):
    """reserve() across a stride on a reactant, a product and the ion target AFTER burnEvery and ionizeEvery were registered
    beside collidePairEvery and fusionYieldEvery on the same species: the next sub-steps, on which all are due, are the
    mate's by hand"""
    t0 = time.perf_counter()
    sc = model.NAMED4["reserve_after_register"]()
    plan, pe, fe = sc["plan"], sc["pair_every"], sc["fusion_every"]
    a, m = pair_of(fp, sc, monkeypatch)
    assert a.collidePairEvery(pe["every"], pe["a"], pe["b"], **pe["kw"]) == 0 and a.fusionYieldEvery(fe["every"], fe["a"], fe["b"], **fe["kw"]) == 0
    register_new(a, sc)
    sums, figures, t = {k: {} for k in ("pair", "fusion") + new_families(sc)}, new_figures(), 0
    tail = hook_tail(sc, sums, figures)

    def manual(k):
        nonlocal t
        for _ in range(k):
            m.sort()
            m.substeps(1)
            t += 1
            add_ints(sums["pair"], m.collidePair(pe["a"], pe["b"], **dict(pe["kw"], epoch=t + pe["kw"]["epoch"])))
            add_ints(sums["fusion"], m.fusionYield(fe["a"], fe["b"], grid=True, **dict(fe["kw"], epoch=t + fe["kw"]["epoch"])))
            tail(m, t)

    a.substeps(plan["before"])
    manual(plan["before"])
    assert_same(snap(fp, a, sc), snap(fp, m, sc), "reserve_after_register: before the reserves")
    for sp in plan["reserve"]:
        cap = a.population(sp)["capacity"]
        assert cap // 1024 != (cap + plan["extra"]) // 1024
        for sim in (a, m):
            assert sim.reserve(sp, cap + plan["extra"]) == cap + plan["extra"]
    a.substeps(plan["after"])
    manual(plan["after"])
    assert_same(snap(fp, a, sc), snap(fp, m, sc), "reserve_after_register: after the reserves")
    have = dict(new_stats(a, sc), pair=g3.ints_of(a.pairStats(0)), fusion=g3.ints_of(dict(a.fusionStats(0), grid=a.fusionGrid(0))))
    for key in sums:
        assert equal_sums(have[key], sums[key]) and sums[key]["applications"] == t == 5, (key, have[key])
    assert sums["ionize0"]["ionised"] > 0 and sums["burn0"]["burnt"] > 0 and sums["pair"]["pairs"] > 0 and sums["fusion"]["pairs"] > 0
    for sim in (a, m):
        sim.destroy()
    report("reserve_after_register", sc, t0, figures)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_hook_order(fp, monkeypatch, precision):
    """a source of a fast beam, an ioniser only the beam (and the fast fifth) reaches, and a like burner on the species that
    receives the secondaries, all due on sub-step 1: the ioniser saw the particles injected on that sub-step, the burner the
    ones ionised on it, and the recorded row counts them all"""
    t0 = time.perf_counter()
    sc = model.NAMED4["hook_order"](precision)
    roles, src = sc["roles"], sc["inject_every"][0]
    a, m = pair_of(fp, sc, monkeypatch)
    assert a.injectEvery(1, species=src["species"], **src["kw"]) == 0
    register_new(a, sc)
    a.recordEnergy(1)
    sums, figures = {k: {} for k in ("inject0",) + new_families(sc)}, new_figures()
    tail = hook_tail(sc, sums, figures)
    for t in range(1, sc["substeps"] + 1):
        a.substeps(1)
        m.sort()
        m.substeps(1)
        span0, e_before = m.population(0)["id_span"], m.population(roles["electron"])
        g3.sinks_and_sources(m, sc, t, sums, [t - 1])
        before = rows(m, 0)
        tail(m, t)
        after = rows(m, 0)
        primaries = before[0][(after[2][:len(before[0])] != before[2]).any(axis=1)]
        assert (primaries >= span0).sum() > 100, ("the ioniser did not see the particles injected on its sub-step", t, int((primaries >= span0).sum()))
        if t == 1:      # one particle before the sub-step: every pair the burner found holds a secondary of this sub-step
            assert e_before["n"] == 1 and sums["burn0"]["burnt"] > 10, ("the burner did not see the particles ionised on its sub-step", sums["burn0"])
        sa = snap(fp, a, sc)
        assert_same(sa, snap(fp, m, sc), "hook_order %s sub-step %d" % (precision, t))
        row, _ = a.energyHistory()
        assert [int(x) for x in row["count"][-1][:len(sc["counts"])]] == [p["n"] for p in sa["pop"]], "the recorded row counts the new particles"
    have = dict(new_stats(a, sc), inject0=g3.ints_of(a.injectStats(0)))
    assert all(equal_sums(have[key], sums[key]) for key in have)
    assert sums["inject0"]["injected"] == sc["substeps"] * src["kw"]["count"] and sums["ionize0"]["below"] > 0
    for sim in (a, m):
        sim.destroy()
    report("hook_order", sc, t0, figures)


def test_burner_fails_behind_an_ioniser(fp, monkeypatch):
    """the burner's third application is one slot short: substeps(5) raises FPIC_ERR_STATE naming fpic_reserve (an API error,
    no GPU fault) and leaves the handle the mate is in after three manual sub-steps with the hook's operators up to and
    excluding that burner — the ioniser's application of that sub-step in place and settled; after reserve() the run goes on"""
    t0 = time.perf_counter()
    sc = model.NAMED4["burner_fails_behind_an_ioniser"]()
    p3, io, bu = sc["roles"]["p3"], sc["ionize_every"][0], sc["burn_every"][0]
    m = build3(fp, sc, monkeypatch, mate=True, capacities=sc["capacities"])
    start4(m, sc)
    sums, figures = {k: {} for k in new_families(sc)}, new_figures()
    events, t = [], 0

    def manual(burns):
        nonlocal t
        m.sort()
        m.substeps(1)
        t += 1
        held = held_of(m, {0, io["electron"], io["ion"]})
        got = ionize_call(m, io, t + io["kw"]["epoch"])
        check_ionize(m, sc, io, held, got, t + io["kw"]["epoch"], figures, "the ioniser at sub-step %d" % t)
        add_ints(sums["ionize0"], flat(got))
        held = held_of(m, {bu["a"], bu["b"]} | set(bu["products"]))
        app = burn_reference_of(sc, bu, held, t + bu["kw"]["epoch"])
        events.append(app["m"])
        if burns:
            got = burn_call(m, bu, t + bu["kw"]["epoch"])
            check_burn(m, sc, bu, held, got, app, "the burner at sub-step %d" % t)
            add_ints(sums["burn0"], flat(got))

    for k in range(sc["fails_at"]):
        manual(burns=k + 1 < sc["fails_at"])
    room = model.room_of(sc["counts"][p3], events)
    assert len(events) == 3 and min(events) >= 4 and sc["counts"][p3] + events[0] + events[1] <= room < sc["counts"][p3] + sum(events), (events, room)
    caps = list(sc["capacities"])
    caps[p3] = room
    a = build3(fp, sc, monkeypatch, capacities=caps)
    start4(a, sc)
    register_new(a, sc)
    refused(fp, lambda: a.substeps(5), -5, "fpic_reserve", "nothing was changed")
    same_but_capacity(snap(fp, a, sc), snap(fp, m, sc), "burner_fails_behind_an_ioniser: after the refused sub-step")
    have = new_stats(a, sc)
    assert all(equal_sums(have[key], sums[key]) for key in have) and have["ionize0"]["applications"] == 3 and have["burn0"]["applications"] == 2, have
    assert a.population(p3) == dict(n=room + 1 - events[2], capacity=room, id_span=room + 1 - events[2])
    assert a.reserve(p3, sc["capacities"][p3]) == sc["capacities"][p3]
    a.substeps(2)
    for _ in range(2):
        manual(burns=True)
    assert_same(snap(fp, a, sc), snap(fp, m, sc), "burner_fails_behind_an_ioniser: after reserve")
    have = new_stats(a, sc)
    assert all(equal_sums(have[key], sums[key]) for key in have) and have["ionize0"]["applications"] == 5 and have["burn0"]["applications"] == 4, have
    for sim in (a, m):
        sim.destroy()
    report("burner_fails_behind_an_ioniser", sc, t0, figures)


# ---------------------------------------------------------------------------------------------- the resumes
def clear_all4(sim):
    g3.clear_all(sim)
    sim.clearIonization()
    sim.clearBurn()


@pytest.mark.parametrize("burner", [False, True], ids=["ioniser", "ioniser_and_burner"])
@pytest.mark.parametrize("solver,precision", model.RESUME)
def test_a_run_with_an_ioniser_and_a_burner_resumes_bit_for_bit(fp, tmp_path, monkeypatch, solver, precision, burner):
    """(i) an ioniser alone beside generation 3's sources (the species grow, none is thinned): N sub-steps in one run against T
    and N - T through a file and a fresh handle that reserves, then registers again with shifted epochs.  (ii) with a burner as
    well a thinned species has no file: both runs clear every registration at T (clearIonization and clearBurn among them),
    renumber and register again; only one of them goes through the file."""
    t0 = time.perf_counter()
    sc = model.resume_scene4(solver, precision, burner)
    ns = len(sc["counts"])
    t, n = model.RESUME_T, model.RESUME_N
    made = [t // op["every"] for op in sc["inject_every"]]
    whole, first, rest = (build3(fp, sc, monkeypatch, capacities=sc["capacities"]) for _ in range(3))
    for sim in (whole, first):
        start4(sim, sc)
        register4(sim, sc)
    if burner:
        for sim in (whole, first):
            sim.substeps(t)
            assert thinned_of([sim.population(sp) for sp in range(ns)]) == [0, 1]
            refused(fp, lambda: sim.saveCheckpoint(tmp_path / "refused.ckpt"), -5, "fpic_renumber")
            refused(fp, lambda: sim.renumber(0), -5, "registered")
            part = stats4_of(sim, sc)
            clear_all4(sim)
            assert [sim.renumber(sp) for sp in range(ns)] == [sim.population(sp)["n"] for sp in range(ns)]
        register4(whole, sc, shift=0, applied=made)
        whole.substeps(n - t)
    else:
        whole.substeps(n)
        first.substeps(t)
        part = stats4_of(first, sc)
    first.saveCheckpoint(tmp_path / "cut.ckpt")
    rest.loadCheckpoint(tmp_path / "cut.ckpt")
    register4(rest, sc, shift=t, applied=made)
    rest.substeps(n - t)
    sw, sr = snap(fp, whole, sc), snap(fp, rest, sc)
    assert_same(sw, sr, "resume")
    assert not same_rows(snap(fp, first, sc)["rows"][0], sr["rows"][0])
    total, tail = stats4_of(whole, sc), stats4_of(rest, sc)
    for key in families4(sc):
        assert (tail[key] if burner else g3.g2.plus(part[key], tail[key])) == total[key], (key, {k: v for k, v in total[key].items() if k != "grid"})
    assert part["ionize0"]["ionised"] > 0 and total["ionize0"]["ionised"] > 0 and total["ionize0"]["applications"] == (n - t if burner else n) // sc["ionize_every"][0]["every"]
    assert not burner or (part["burn0"]["burnt"] > 0 and total["burn0"]["burnt"] > 0)
    for sim in (whole, first, rest):
        sim.destroy()
    print("generation 4 resume %s %s burner=%s: %.2f s" % (solver, precision, burner, time.perf_counter() - t0))
