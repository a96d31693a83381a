"""The electron-impact ionisation (fpic_ionize*) on the GPU against the numpy restatement of its rule
(tests/ionize_reference.py, proved on the CPU by tests/test_ionize_reference.py, where the conditions of the scenes compared
here — tests/ionize_scenes.py — are shown to hold): the event set, the counts, the ids and places of the new rows, their
copied positions and all three groups of exact tallies bit for bit; the rounded velocities within a bound; every projectile
count and event count at which a pass takes another path; both forms of every choice the host makes on either side of its
threshold; the independence of slots; both kinds of electron target, thinned and grown species; neutrality; the fit rule with
nothing changed on a refusal; the registered form against a manual loop, a fresh twin, the order in the hook; the operators and
diagnostics on the ionised targets with a checkpoint; the refusals.

THE BOUND of the rounded velocities (fp64; value_bound below), derived as tests/test_gpu_gas.value_bound is, with its
constant ULPS (tests/test_gpu_collide.py: the device's normals, cospi and sinpi) and one spacing per further operation on
either side; nothing new is measured.  With e_vb, e_d, e_g as there (the partner, the difference, the relative speed):
    gg = g g                e_gg  = 2 g e_g + e_g^2 + spacing(gg)
    gp2 = gg - thr^2        e_gp2 = e_gg + spacing(max(gg, thr^2, gp2))            (thr^2 is the same double on both sides)
    a1 = r gp2              e_a1  = r e_gp2 + spacing(a1)                          (r is exact: a word)
    a2 = gp2 - a1           e_a2  = e_gp2 + e_a1 + spacing(max(gp2, a1, a2))
    g1 = sqrt(a1)           e_g1  = e_a1 / g1 + spacing(g1)     (|sqrt x - sqrt y| = |x - y| / (sqrt x + sqrt y) <= |x - y| / sqrt y;
                                                                  g1 = 0: sqrt(e_a1)); g2 likewise from a2
    n = nhat(words)         e_n   = ULPS s spacing(cospi, sinpi) + 2 spacing(n) on x and y, 0 on z (test_gpu_gas's e_nh)
    t = g1 n                e_t   = e_g1 |n| + g1 e_n + spacing(t)
    v' = vb + t             e_v   = e_vb + e_t + spacing(max(|vb|, |t|, |v'|))
The secondary takes g2 and its own direction, the ion e_vb alone.  An fp32 handle stores the float nearest to a double within
that bound of the reference's: |stored - reference| <= bound + half a float spacing.
Largest observed |dv| / bound on an MI355X (test_against_the_reference prints them): fp64 0.216 (the window and the
whole-box scene, 100003 projectiles), 0.376 (the table that starts at the threshold), 0.429 (P_max = 1, 4101 projectiles);
fp32: no stored velocity that is not bit-equal to the rounded reference, which the test asserts."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import force_reference as fref
import histogram_reference as hr
import ionize_reference as ref
import ionize_scenes as sc
import moments_reference as mr
from helpers import ROOT
from test_gas_reference import DT, L, ME, QE, SHAPE, density_for, scene
from test_gpu_collide import ULPS
from test_gpu_gas import spacing, spec_of
from test_gpu_gas import W as WEIGHT
from test_gpu_histogram import MP, PRECISIONS, em_dt
from test_gpu_remove import bits, refused, rows, same_boxes, same_rows, twin_of, unit_box

pytestmark = pytest.mark.gpu

DTYPE = {"fp32": np.float32, "fp64": np.float64}
MI = sc.MI


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def filled(fp, precision, n, third=False, ni=3, room=None, **kw):
    """scene(n) as species 0 (electrons) of the gas scenes' box, ni cold ions as species 1 and, with `third`, a species 2 of
    electrons to receive the secondaries; room: the particles every target can grow by"""
    sim = fp.makeCylindricalParticlePusher(spec_of(n, **kw), precision=precision)
    frac, vel = scene(n)
    sim.set(position=frac * np.array(L), velocity=vel)
    assert sim.addSpecies(MI, QE, ni) == 1
    fi, vi = scene(ni, seed=2)
    sim.set(position=fi * np.array(L), velocity=vi * 0.01, species=1)
    if third:
        assert sim.addSpecies(ME, -QE, 2) == 2
        fe, ve = scene(2, seed=3)
        sim.set(position=fe * np.array(L), velocity=ve, species=2)
    if room:
        for k in range(3 if third else 2):
            sim.reserve(k, sim.population(k)["n"] + room)
    return sim


def value_bound(req, ids, v, out):
    """(primary, secondary, ion) bounds per component for the events `ids` with double velocities v: the module docstring"""
    n = ref.normals(req, ids)
    th = req["vth"] * n
    vb = req["drift"] + th
    e_vb = ULPS * req["vth"] * spacing(n) + 2 * spacing(np.maximum(np.abs(th), np.abs(vb)))
    d = v - vb
    e_d = e_vb + spacing(np.maximum.reduce([np.abs(v), np.abs(vb), np.abs(d)]))
    g = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    e_g = e_d.sum(axis=1) + 6 * spacing(g)
    gg, thr2 = g * g, req["thr"] * req["thr"]
    e_gg = 2 * g * e_g + e_g * e_g + spacing(gg)
    gp2 = gg - thr2
    e_gp2 = e_gg + spacing(np.maximum.reduce([gg, np.full_like(gg, thr2), np.abs(gp2)]))
    r = ref.share(req, ids)
    a1 = r * gp2
    e_a1 = r * e_gp2 + spacing(a1)
    a2 = gp2 - a1
    e_a2 = e_gp2 + e_a1 + spacing(np.maximum.reduce([np.abs(gp2), np.abs(a1), np.abs(a2)]))
    w0, w2 = ref.words(req, ids, 0), ref.words(req, ids, 2)
    bounds = []
    for a, e_a, wc, wp in ((a1, e_a1, w0[2], w0[3]), (a2, e_a2, w2[1], w2[2])):
        root = np.sqrt(np.maximum(a, 0.0))
        e_root = np.where(root > 0, e_a / np.where(root > 0, root, 1.0), np.sqrt(e_a)) + spacing(root)
        c = 1.0 - 2.0 * ((wc.astype(np.float64) + 0.5) * 2.0 ** -32)
        s = np.sqrt(1.0 - c * c)
        phi2 = 2.0 * (wp.astype(np.float64) * 2.0 ** -32)
        circ = np.stack([ref.cospi(phi2), ref.sinpi(phi2)], axis=1)
        nh = ref.nhat(wc, wp)
        e_nh = np.zeros_like(nh)
        e_nh[:, :2] = ULPS * s[:, None] * spacing(circ) + 2 * spacing(nh[:, :2])
        t = root[:, None] * nh
        e_t = e_root[:, None] * np.abs(nh) + root[:, None] * e_nh + spacing(t)
        bounds.append(e_vb + e_t + spacing(np.maximum.reduce([np.abs(vb), np.abs(t), np.abs(vb + t)])))
    return bounds[0], bounds[1], e_vb


def same_gain(got, vel, count, mass, charge, weight=WEIGHT):
    """a target's group of the result against the exact sums of the rows it gained, and the doubles derived from them"""
    want = ref.gain(vel)
    assert got["energy_fixed"] == want["energy_fixed"] and got["momentum_fixed"] == want["momentum_fixed"], (got, want)
    d = ref.derived(want, count, mass, charge, weight)
    assert got["energy"] == d["energy"] and got["momentum"] == d["momentum"] and got["charge"] == d["charge"], (got, d)


def check_application(sim, precision, kw, electron, before, targets, got, figures=None, known=None, ion=1, lengths=L, weight=WEIGHT, masses=(ME, ME, MI),
                      charges=(-QE, -QE, QE), projectile=0):
    """one application `got` of the request kw to the projectile rows `before` (ids, position, velocity of species 0, read
    before it), `targets` the (rows, population) of the electron and the ion species before it: everything exact, and the
    rounded velocities within the bound.  projectile, ion: the projectile species and the ion target; lengths, weight: the box's;
    masses, charges: of the projectile, the electron and the ion species (the defaults are this module's box)"""
    T = DTYPE[precision]
    req = ref.request(lengths, **kw)
    (rows_e, pop_e), (rows_i, pop_i) = targets
    app = ref.application(req, before[0], before[1], before[2], pop_e["n"], pop_e["id_span"], pop_i["n"], pop_i["id_span"], known=known)
    assert ref.margins_hold(req, app)
    m = app["m"]
    assert {k: got[k] for k in ("candidates", "below", "above", "ionised")} == ref.counts(app) and got["applications"] == 1
    after = rows(sim, projectile)
    new_e, new_i = rows(sim, electron), rows(sim, ion)
    old = slice(0, len(before[0]))
    # the projectiles: the same ids and positions; exactly the primaries have new velocities
    assert bits(after[0][old], before[0]) and bits(after[1][old], before[1])
    changed = (after[2][old] != before[2]).any(axis=1)
    assert np.array_equal(changed, app["event"]), (int(changed.sum()), m)
    # the new rows: behind the old ones, ids from the id span on in the order of the primaries' ids, the primaries' positions
    for name, held, (was, pop) in (("electron", new_e, targets[0]), ("ion", new_i, targets[1])):
        assert len(held[0]) == pop["n"] + m
        if not (electron == projectile and name == "electron"):                # (the projectile species' own old rows: checked above)
            assert same_rows(tuple(x[:pop["n"]] for x in held), was), name
        assert bits(held[0][pop["n"]:], (pop["id_span"] + np.arange(m)).astype(np.uint32)), name
        assert bits(held[1][pop["n"]:], app[name]["position"]), name
        now = sim.population(electron if name == "electron" else ion)
        assert now["n"] == pop["n"] + m and now["id_span"] == pop["id_span"] + m
    ve, vi = new_e[2][pop_e["n"]:], new_i[2][pop_i["n"]:]
    # the tallies: the integers Python computes from the read-back rows, and the doubles derived from them
    t = fref.tallies(before[2], after[2][old], app["event"])
    p = got["primary"]
    assert p["energy_fixed"] == t["work_fixed"] and p["momentum_fixed"] == t["impulse_fixed"] and p["charge"] == 0.0
    d = fref.derived(t, masses[0], weight)
    assert p["energy"] == d["work"] and p["momentum"] == d["impulse"]
    same_gain(got["electron"], ve, m, masses[1], charges[1], weight)
    same_gain(got["ion"], vi, m, masses[2], charges[2], weight)
    if not m:
        return 0.0
    # the rounded velocities
    ev = np.flatnonzero(app["event"])
    order = ev[np.argsort(app["rank"][ev])]
    b1, b2, b3 = value_bound(req, before[0][order], before[2][order].astype(np.float64), app)
    worst = 0.0
    for stored, want, bound in ((after[2][old][order], app["v1"][order], b1), (ve, app["vs"][order], b2), (vi, app["vb"][order], b3)):
        dv = np.abs(stored.astype(np.float64) - want)
        allowed = bound + (0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) if T == np.float32 else 0.0)
        assert np.all(dv <= allowed), (precision, float((dv / allowed).max()))
        worst = max(worst, float((dv / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if T == np.float64 else float((stored != want.astype(np.float32)).mean()))
    if figures is not None:
        figures.append(worst)
    return worst


def run_scene(fp, precision, name, n, third=False, state="loaded", figures=None):
    kw = sc.keywords(name)
    req, out = sc.reference(name, n)
    m = int(out["event"].sum())
    sim = filled(fp, precision, n, third=third, room=m)
    if state == "sorted":
        sim.sort()
    electron = 2 if third else 0
    before = rows(sim, 0)
    frac, vel = scene(n)
    T = DTYPE[precision]
    assert bits(before[2], vel.astype(T)) and bits(before[1], frac.astype(T))          # the handle stores what the reference was given
    targets = [(rows(sim, k), sim.population(k)) for k in (electron, 1)]
    got = sim.ionize(species=0, electron=electron, ion=1, **kw)
    assert got["ionised"] == m
    assert bits(before[0], np.arange(n, dtype=np.uint32))
    worst = check_application(sim, precision, kw, electron, before, targets, got, figures, known=out)          # (the same arguments: the shared reference)
    sim.destroy()
    return worst


# ---- 1. against the reference
@pytest.mark.parametrize("name,n", [("window", 100003), ("whole", 100003), ("at threshold", 100003), ("dense", 4101)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_reference(fp, precision, name, n):
    for third, state in ((False, "loaded"), (True, "sorted")):
        worst = run_scene(fp, precision, name, n, third=third, state=state)
        if precision == "fp64":
            print("fp64 %s n=%d %s: largest |dv| / bound %.3f" % (name, n, state, worst))
            assert 0 < worst <= 1.0
        else:
            print("fp32 %s n=%d %s: share of stored values NOT bit-equal to the rounded reference %.2e" % (name, n, state, worst))
            assert worst == 0.0


# ---- 2. sizes
@pytest.mark.parametrize("name", ["window", "whole", "at threshold"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_projectile_counts(fp, precision, name):
    sizes = [n for s, n in sc.exact_cases() if s == name]
    assert sizes[:9] == sc.SIZES
    for k, n in enumerate(sizes):
        run_scene(fp, precision, name, n, third=bool(k % 2), state="sorted" if k % 3 == 1 else "loaded")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_event_counts(fp, precision):
    """none, one, then past a lane's vector, a wave, a workgroup of the generation pass and the queue's entries; ids in more
    than one chunk of the popcount scan; id spans that are no multiple of 32 (test_ionize_reference.py holds the counts)"""
    for name in sc.SPARSE:
        run_scene(fp, precision, name, sc.SPARSE_N, third=(name == "one event"))
    for k, n in enumerate(sc.DENSE_SIZES):
        run_scene(fp, precision, "dense", n, third=bool(k % 2))


def test_no_event_changes_nothing_and_k_zero_launches_nothing(fp):
    sim = filled(fp, "fp32", sc.SPARSE_N, room=10, solver="poisson_fft")
    sim.precalc()
    sim.substeps(2)
    held = [rows(sim, k) for k in range(2)]
    e, rho = sim.readField(fp.F3_E), sim.readField(fp.F3_RHO_FIXED)
    # (the positions have moved: whatever the counts are, a request of density 0 has K = 0)
    zero = sim.ionize(species=0, ion=1, **dict(sc.SPARSE["no event"], density=0.0))
    assert zero["applications"] == 0 and zero["candidates"] == 0 and zero["ionised"] == 0
    got = sim.ionize(species=0, ion=1, **dict(sc.SPARSE["no event"], density=1e-30))          # K = 0 as well: x_max underflows
    assert got["ionised"] == 0
    assert all(same_rows(rows(sim, k), held[k]) for k in range(2)) and bits(sim.readField(fp.F3_E), e) and bits(sim.readField(fp.F3_RHO_FIXED), rho)
    sim.substeps(1)                                                            # still binned, still ready
    sim.destroy()


# ---- 3. both forms of every choice of the host, on either side of its threshold
@pytest.mark.parametrize("window", ["narrow", "wide", "whole"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_both_forms_on_either_side_of_their_thresholds(fp, precision, window):
    names = [name for name in sc.THRESHOLD_SCENES if name.endswith(window)]
    assert len(names) == 5
    for k, name in enumerate(names):
        run_scene(fp, precision, name, sc.THRESHOLD_N, third=bool(k % 2), state="sorted" if k % 2 else "loaded")


def digest(fp, precision):
    sim = filled(fp, precision, 100003, room=2000)
    sim.sort()
    got = sim.ionize(species=0, ion=1, **sc.SCENES["window"])
    out = [got["candidates"], got["below"], got["above"], got["ionised"], str(got["primary"]["energy_fixed"]), str(got["electron"]["energy_fixed"]), str(got["ion"]["momentum_fixed"])]
    for k in range(2):
        r = rows(sim, k)
        out += [hashlib.sha256(r[0].tobytes()).hexdigest(), hashlib.sha256(r[1].tobytes()).hexdigest(), hashlib.sha256(r[2].tobytes()).hexdigest()]
    sim.destroy()
    return out


FORMS_SCRIPT = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import fusionpic as fp
import test_gpu_ionize as t
print(json.dumps({p: t.digest(fp, p) for p in ("fp32", "fp64")}))
"""


@pytest.mark.parametrize("forms", [5, 6, 9, 10])
def test_the_forms_behind_the_test_switch_give_the_same_particles(fp, forms):
    """FPIC_IONIZE_FORMS is read once, so each value gets a process of its own: the word (1) or the window (2) first, in the
    wave-shared loop (4) or through the queue (8), whatever the host would choose for the scene"""
    env = dict(os.environ, FPIC_IONIZE_FORMS=str(forms))
    raw = subprocess.check_output([sys.executable, "-c", FORMS_SCRIPT, os.path.join(ROOT, "fusion-sim_amd"), os.path.join(ROOT, "tests")], env=env, timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    for precision in PRECISIONS:
        want = digest(fp, precision)
        assert out[precision] == want and want[3] > 400, (forms, precision)


# ---- 4. independence of slots
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_result_does_not_depend_on_the_slots(fp, precision):
    """as loaded, after fpic_sort, and after re-binning pushes have permuted the slots (the state is then uploaded again: an
    upload to a binned species goes through its ids and keeps the permutation)"""
    n = 20011
    kw = sc.SCENES["window"]
    frac, vel = scene(n)
    results = []
    for state in ("loaded", "sorted", "pushed"):
        sim = filled(fp, precision, n, room=500)
        if state == "sorted":
            sim.sort()
        if state == "pushed":
            sim.substeps(9)                                                    # (past the re-binning of the eighth sub-step)
            sim.set(position=frac * np.array(L), velocity=vel)
            fi, vi = scene(3, seed=2)
            sim.set(position=fi * np.array(L), velocity=vi * 0.01, species=1)
        got = sim.ionize(species=0, ion=1, **kw)
        results.append((got, rows(sim, 0), rows(sim, 1)))
        sim.destroy()
    first = results[0]
    assert first[0]["ionised"] > 50
    for got, r0, r1 in results[1:]:
        assert got == first[0] and same_rows(r0, first[1]) and same_rows(r1, first[2])


# ---- 5. thinned and grown species
@pytest.mark.parametrize("third", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_thinned_and_grown_species(fp, precision, third):
    """a thinned projectile (its ids lie below a span that is no multiple of 32), a thinned target whose id span grows, and
    targets grown by reserve() from a capacity of a few particles"""
    n = 20011
    sim = filled(fp, precision, n, third=third, ni=300)
    electron = 2 if third else 0
    assert sim.remove(where={"x": (0.25, 0.5)}, species=0)["removed"] > 1000
    assert sim.remove(where={"z": (0.0, 0.5)}, species=1)["removed"] > 50
    for k in {0, 1, electron}:
        sim.reserve(k, sim.population(k)["capacity"] + 700)
    kw = sc.SCENES["window"]
    for epoch in (3, 4):                                                       # twice: the second application reads the grown species
        before = rows(sim, 0)
        targets = [(rows(sim, k), sim.population(k)) for k in (electron, 1)]
        assert targets[1][1]["id_span"] > targets[1][1]["n"] and (third or epoch == 4 or targets[0][1]["id_span"] == n)
        got = sim.ionize(species=0, electron=electron, ion=1, **dict(kw, epoch=epoch))
        assert 20 < got["ionised"] < 350
        if electron == 0 and epoch == 4:
            assert (before[0] >= n).any()                                      # secondaries of the first application are projectiles now
        check_application(sim, precision, dict(kw, epoch=epoch), electron, before, targets, got)
    refused(fp, lambda: sim.getParticles(species=1), -5, "fpic_renumber")       # a thinned target stays thinned
    if third:
        assert sim.getParticles(species=2)["position"].shape[0] == sim.population(2)["n"]      # one that was not stays so
    sim.destroy()


# ---- 6. neutrality
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_application_adds_no_net_charge(fp, precision, solver):
    sim, spec = ionising_box(fp, precision, solver)
    sim.precalc()
    sim.substeps(3)
    sim.density()
    rho = sim.readField(fp.F3_RHO_FIXED)
    fields = [sim.readField(w) for w in ((fp.F3_EDGE_E, fp.F3_FACE_B) if solver == "yee" else (fp.F3_E,))]
    got = sim.ionize(**ION_UNIT)
    assert got["ionised"] > 50 and got["electron"]["charge"] == -got["ion"]["charge"] != 0.0
    sim.density()
    assert bits(sim.readField(fp.F3_RHO_FIXED), rho)
    # (full EM: the fields stay; electrostatic: the re-deposit gives the same grid, so the same solve)
    assert all(bits(sim.readField(w), f) for w, f in zip((fp.F3_EDGE_E, fp.F3_FACE_B) if solver == "yee" else (fp.F3_E,), fields))
    sim.destroy()


FLAT = np.full(2, 3.0e-19)
UNIT_TAU = 1e-9
ION_UNIT = dict(species=0, ion=1, g_threshold=0.01, sigma=FLAT, g_lo=0.01, g_hi=0.5, tau=UNIT_TAU, density=density_for(0.5 * 2.0 ** 32, FLAT, 0.01, 0.5, UNIT_TAU),
                drift=(0.0, 0.0, 0.001), vth=0.002, seed=0x1051E0DD, stream=1)


def ionising_box(fp, precision, solver, n=4000, ni=1500, room=3000):
    """test_gpu_remove's unit box (electrons, and ions of the opposite charge) with room to grow"""
    sim, spec = unit_box(fp, precision, solver, n, ni=ni, weight=2e9)
    for k in range(2):
        sim.reserve(k, sim.population(k)["n"] + room)
    return sim, spec


# ---- 7. the fit
@pytest.mark.parametrize("short", ["electron", "ion"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_slot_short_is_refused_and_changes_nothing(fp, precision, short):
    n = 4101
    kw = sc.DENSE
    m = int(sc.reference("dense", n)[1]["event"].sum())
    sim = filled(fp, precision, n, third=True, solver="poisson_fft")
    sim.reserve(2, 2 + m - (1 if short == "electron" else 0))
    sim.reserve(1, 3 + m - (1 if short == "ion" else 0))
    sim.precalc()
    index = sim.ionizeEvery(1000, species=0, electron=2, ion=1, **kw)
    held = [rows(sim, k) for k in range(3)]
    pops = [sim.population(k) for k in range(3)]
    e = sim.readField(fp.F3_E)
    refused(fp, lambda: sim.ionize(species=0, electron=2, ion=1, **kw), -1, "." + short + " <- ", "fpic_reserve", "nothing was changed")
    assert all(same_rows(rows(sim, k), held[k]) for k in range(3)) and [sim.population(k) for k in range(3)] == pops
    assert bits(sim.readField(fp.F3_E), e)
    stats = sim.ionizeStats(index)
    assert stats["applications"] == 0 and stats["candidates"] == 0 and stats["ionised"] == 0 and stats["primary"]["energy_fixed"] == 0
    sim.substeps(1)                                                            # the box is as it was: still binned, still ready
    sim.destroy()
    # at the exact capacity it succeeds
    sim = filled(fp, precision, n, third=True)
    sim.reserve(2, 2 + m)
    sim.reserve(1, 3 + m)
    assert sim.ionize(species=0, electron=2, ion=1, **kw)["ionised"] == m
    assert sim.population(2) == dict(n=2 + m, capacity=2 + m, id_span=2 + m) and sim.population(1)["n"] == sim.population(1)["capacity"] == 3 + m
    sim.destroy()


def test_an_ioniser_that_overflows_in_mid_run_leaves_the_earlier_applications(fp):
    sim, spec = ionising_box(fp, "fp32", "poisson_fft", room=0)
    twin, _ = ionising_box(fp, "fp32", "poisson_fft", room=3000)
    twin.precalc()
    assert twin.ionizeEvery(1, **ION_UNIT) == 0
    twin.substeps(1)
    first = twin.ionizeStats(0)["ionised"]
    assert first > 50
    # the room for the first application and five particles more
    sim.reserve(0, 4000 + first + 5)
    sim.reserve(1, 1500 + first + 5)
    sim.precalc()
    index = sim.ionizeEvery(1, **ION_UNIT)
    sim.substeps(1)
    assert sim.ionizeStats(index)["applications"] == 1 and sim.ionizeStats(index)["ionised"] == first
    assert all(same_rows(rows(sim, k), rows(twin, k)) for k in range(2))
    held = [rows(sim, k) for k in range(2)]
    refused(fp, lambda: sim.substeps(1), -5, "fpic_reserve", "nothing was changed")
    stats = sim.ionizeStats(index)
    assert stats == dict(twin.ionizeStats(0))                                   # the earlier application is intact, nothing was added
    assert sim.population(0)["n"] == 4000 + first and sim.population(1)["n"] == 1500 + first
    assert all(bits(rows(sim, k)[0], held[k][0]) for k in range(2))              # nobody new (the sub-step itself has pushed them)
    sim.destroy()
    twin.destroy()


# ---- 8. twins
GAS_ON = dict(density=2e19, tau=1e-9, sigma=np.full(16, 3e-19), g_lo=0.0, g_hi=0.5, vth=0.01, seed=9)
SOURCE_ON = dict(kind="volume", species=0, lo=(0.4, 0.4, 0.4), hi=(0.6, 0.6, 0.6), seed=42, stream=2, vth=0.05, first=0, count=200)
SINK_ON = dict(where={"x": (0.0, 0.05)}, species=1)
ION_B = dict(ION_UNIT, seed=0x1051E0EE, stream=2, epoch=50, lo=(0.25, 0.0, 0.0), hi=(0.75, 1.0, 1.0))


@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_registered_equals_manual(fp, precision, solver):
    """two ionisers, a gas operator, a source and a sink: the hook's order is gas, remove, inject, ionize"""
    a, spec = ionising_box(fp, precision, solver)
    b, _ = ionising_box(fp, precision, solver)
    for s in (a, b):
        s.precalc()
    assert [a.ionizeEvery(1, **ION_UNIT), a.ionizeEvery(2, **ION_B)] == [0, 1]
    assert a.collideGasEvery(1, "exchange", **GAS_ON) == 0 and a.injectEvery(2, **SOURCE_ON) == 0 and a.removeEvery(3, **SINK_ON) == 0
    steps = 4
    a.substeps(steps)
    totals = [dict(applications=0, candidates=0, below=0, above=0, ionised=0, sums=[0] * 12) for _ in range(2)]
    for k in range(1, steps + 1):
        b.substeps(1)
        b.collideGas("exchange", **dict(GAS_ON, epoch=k))
        if k % 3 == 0:
            b.remove(**SINK_ON)
        if k % 2 == 0:
            b.inject(**dict(SOURCE_ON, first=(k // 2 - 1) * 200))
        for every, kw, total in ((1, ION_UNIT, totals[0]), (2, ION_B, totals[1])):
            if k % every == 0:
                got = b.ionize(**dict(kw, epoch=k + kw.get("epoch", 0)))
                for key in ("applications", "candidates", "below", "above", "ionised"):
                    total[key] += got[key]
                total["sums"] = [x + y for x, y in zip(total["sums"], flat_sums(got))]
    for k in range(2):
        assert same_rows(rows(a, k), rows(b, k))
        assert a.population(k) == b.population(k)
    assert bits(a.readField(fp.F3_E), b.readField(fp.F3_E))
    for index, total in enumerate(totals):
        got = a.ionizeStats(index)
        assert {key: got[key] for key in ("applications", "candidates", "below", "above", "ionised")} == {key: total[key] for key in total if key != "sums"}
        assert flat_sums(got) == total["sums"] and got == a.ionizeStats(index, "local")
    assert [t["applications"] for t in totals] == [4, 2] and all(t["ionised"] > 20 for t in totals)
    # clearIonization leaves the gas operators, the sources and the sinks
    refused(fp, lambda: a.renumber(1), -5, "registered")
    a.clearIonization()
    refused(fp, lambda: a.ionizeStats(0), -1, ".index <- no such registered ioniser")
    assert a.gasStats(0)["applications"] == steps and a.injectStats(0)["applications"] == 2 and a.removeStats(0)["applications"] == 1
    for s in (a, b):
        s.destroy()


def flat_sums(got):
    return [x for name in ("primary", "electron", "ion") for x in [got[name]["energy_fixed"]] + got[name]["momentum_fixed"]]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fresh_twin(fp, precision):
    """a box after an application steps as a fresh box that was given the grown populations"""
    sim, spec = ionising_box(fp, precision, "poisson_fft")
    sim.precalc()
    sim.substeps(5)
    got = sim.ionize(**ION_UNIT)
    assert got["ionised"] > 50 and sim.population(0)["n"] == 4000 + got["ionised"] and sim.population(1)["n"] == 1500 + got["ionised"]
    twin = twin_of(fp, sim, spec, precision)
    twin.precalc()
    same_boxes(fp, sim, twin)
    for _ in range(5):
        sim.substeps(1)
        twin.substeps(1)
        same_boxes(fp, sim, twin)
    sim.destroy()
    twin.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_order_in_the_hook(fp, precision):
    """the ionisers run after the sources: a beam injected on a sub-step can ionise on it, and a row recorded on that sub-step
    counts the new particles"""
    sim, spec = ionising_box(fp, precision, "poisson_fft")
    sim.precalc()
    # only the beam is fast enough for the table: the thermal electrons (sigma 0.03) lie below g_lo = 0.6
    beam = dict(kind="volume", species=0, lo=(0.4, 0.4, 0.4), hi=(0.6, 0.6, 0.6), seed=77, stream=5, vth=0.001, drift=(0.0, 0.0, 0.8), first=0, count=500)
    kw = dict(ION_UNIT, g_threshold=0.6, g_lo=0.6, g_hi=0.9, density=density_for(0.9 * 2.0 ** 32, FLAT, 0.6, 0.9, UNIT_TAU))
    source, index = sim.injectEvery(1, **beam), sim.ionizeEvery(1, **kw)
    sim.recordEnergy(1)
    sim.substeps(1)
    stats = sim.ionizeStats(index)
    assert sim.injectStats(source)["injected"] == 500 and stats["applications"] == 1
    assert stats["ionised"] > 100 and stats["below"] > 0                        # the fresh beam ionised on its own sub-step
    ids, pos, vel = rows(sim, 0)
    assert sim.population(0)["n"] == 4000 + 500 + stats["ionised"] == len(ids)
    ions = rows(sim, 1)
    born = ions[1][1500:]
    assert len(born) == stats["ionised"] and np.all((born >= 0.4) & (born < 0.6))    # where the beam is
    row, _ = sim.energyHistory()
    assert int(row["count"][-1][0]) == len(ids) and int(row["count"][-1][1]) == 1500 + stats["ionised"]
    sim.destroy()


# ---- 9. the operators and diagnostics on the ionised targets, and a checkpoint
@pytest.mark.parametrize("precision", PRECISIONS)
def test_operators_and_diagnostics_on_the_ionised_targets(fp, precision, tmp_path):
    """the box whose species grew by ionisation against the fresh box of the grown populations (twin_of): the per-particle and
    the cell operators, which act by id and stored state, do the same to both; the diagnostics of the grown box against their
    references; sort, the series, a sink and a source after the ioniser; the checkpoint of the (unthinned) box"""
    a, spec = ionising_box(fp, precision, "poisson_fft")
    a.precalc()
    a.substeps(2)
    m = a.ionize(**ION_UNIT)["ionised"]
    assert m > 50
    b = twin_of(fp, a, spec, precision)
    b.precalc()
    same_boxes(fp, a, b)
    before = rows(a, 1)
    fusion = dict(sigma=np.linspace(1e-28, 4e-28, 16), g_lo=0.0, g_hi=0.5, tau=1e-9, seed=5, stream=2, epoch=1)
    text = lambda g: {k: np.asarray(v).tolist() for k, v in g.items()}
    operators = [
        ("collide elastic", lambda s: s.collide("elastic", nu_tau=0.8, vth=0.02, mass_ratio=2.0, seed=7, epoch=3)),
        ("collide relax", lambda s: s.collide("relax", nu_tau=0.1, vth=0.01, seed=8, species=1)),
        ("collideGas", lambda s: s.collideGas("exchange", species=1, **GAS_ON)),
        ("force", lambda s: s.force(waves=[dict(amp=5e4, mode=(1, 0, 2), nu=0.0)])),       # (a static wave: the two boxes are at different sub-steps)
        ("collidePair", lambda s: s.collidePair(0, 1, log_lambda=10.0, tau=1e-9, seed=3)),
        ("fusionYield", lambda s: s.fusionYield(0, 1, **fusion)),
        ("fusionSpectrum", lambda s: s.fusionSpectrum(1, axis="cm", bins=8, lo=0.0, hi=4000 * fp.KEV, **fusion)),
    ]
    for name, op in operators:
        ga, gb = text(op(a)), text(op(b))
        assert all(same_rows(rows(a, k), rows(b, k)) for k in range(2)), name
        assert ga == gb, (name, ga, gb)
        assert name not in ("collidePair", "fusionYield", "fusionSpectrum") or ga["pairs"] > 0
    same_boxes(fp, a, b)
    ra = [rows(a, k) for k in range(2)]
    assert not bits(ra[1][2][1500:], before[2][1500:])                          # (the operators reached the new ions)
    a.sort()
    assert all(same_rows(rows(a, k), ra[k]) for k in range(2))
    got = a.histogram("vx", 32, (-0.1, 0.1), species=1)
    counts, outside = hr.histogram(ra[1][1], ra[1][2], ["vx"], [32], [(-0.1, 0.1)])
    assert np.array_equal(got["counts"], counts) and got["outside"] == outside
    mo = a.moments("order1", species=1)
    want, _ = mr.moments(ra[1][1], ra[1][2], (8, 8, 8), "order1")
    assert all(np.array_equal(mo[key], want[key]) for key in ("N", "FX", "FY", "FZ"))
    last = 4000 + m - 1
    tr = a.series(tracers=[0, last])["tracers"]
    assert np.array_equal(tr[1][3:6], ra[0][2][last].astype(np.float64))
    ma, mb = a.modes([(1, 0, 0), (0, 2, 1)]), b.modes([(1, 0, 0), (0, 2, 1)])
    assert all(np.asarray(ma[k]).tobytes() == np.asarray(mb[k]).tobytes() for k in ma)
    # the checkpoint of the grown, unthinned box
    path = str(tmp_path / "ionised.ckpt")
    a.saveCheckpoint(path)
    for _ in range(3):
        for s in (a, b):
            s.substeps(3)                                                      # (past the re-binning of the eighth sub-step)
        same_boxes(fp, a, b)
    want = [rows(a, k) for k in range(2)], a.readField(fp.F3_E)
    fresh, _ = ionising_box(fp, precision, "poisson_fft")
    fresh.loadCheckpoint(path)
    assert fresh.population(0)["n"] == 4000 + m and fresh.population(1)["n"] == 1500 + m
    fresh.substeps(9)
    assert all(same_rows(rows(fresh, k), want[0][k]) for k in range(2)) and bits(fresh.readField(fp.F3_E), want[1])
    fresh.destroy()
    # a sink and a source after the ioniser, and a second application on the stepped box
    held = rows(a, 1)
    assert a.remove(where={"x": (0.0, 0.1)}, species=1)["removed"] == int((held[1][:, 0] < 0.1).sum()) > 0
    assert a.inject(**dict(SOURCE_ON, species=1))["injected"] == 200
    assert a.ionize(**dict(ION_UNIT, epoch=9))["ionised"] > 50
    a.substeps(2)
    assert a.population(0)["n"] == a.count() and a.population(1)["n"] == a.count(species=1)
    a.destroy()
    b.destroy()


# ---- 10. refusals
def test_refusals(fp):
    from helpers import make_spec
    rz = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    ok = dict(sc.SCENES["whole"], species=0, ion=1)
    for call in (lambda: rz.ionize(**ok), lambda: rz.ionizeEvery(1, **ok), lambda: rz.ionizeStats(0), rz.clearIonization):
        refused(fp, call, -5, "needs a CART3D handle")
    rz.destroy()
    sim = filled(fp, "fp32", 1000, third=True, room=500)
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(species=3), ".species <- no such species"), (dict(species=-1), ".species <- no such species"),
        (dict(electron=3), ".electron <- no such species"), (dict(electron=-1), ".electron <- no such species"),
        (dict(ion=3), ".ion <- no such species"), (dict(ion=-1), ".ion <- no such species"),
        (dict(ion=0), ".ion <- must differ from species and from electron"), (dict(electron=1), ".ion <- must differ from species and from electron"),
        (dict(g_threshold=-1e-9), ".g_threshold <- must be finite and not negative"), (dict(g_threshold=inf), ".g_threshold <- "), (dict(g_threshold=nan), ".g_threshold <- "),
        (dict(g_threshold=0.0500001), ".g_lo <- the table must start at or above g_threshold"),
        (dict(density=-1.0), ".density <- must be finite and not negative"), (dict(tau=0.0), ".tau <- must be positive and finite"),
        (dict(sigma=[1e-19]), ".n <- must be 2 .. FPIC_GAS_TABLE_MAX (4096)"), (dict(g_lo=-0.1, g_threshold=0.0), ".g_lo <- must be finite and not negative"),
        (dict(g_hi=0.05), ".g_hi <- must be finite and above g_lo"), (dict(sigma=[1e-19, -1e-19]), ".sigma <- every entry must be finite and not negative"),
        (dict(drift=(0, nan, 0)), ".drift <- must be finite"), (dict(vth=(0, -1e-3, 0)), ".vth <- must be finite and not negative"),
        (dict(lo=(-1e-9, 0, 0)), ".lo, .hi <- the window must lie within 0 <= lo < hi <= L"),
        (dict(taper=(None, [1.0], None)), ".taper_n <- a table has 2 .. FPIC_GAS_TAPER_MAX nodes (0: none)"),
        (dict(taper=(None, None, [1.0, 1.0000001])), ".taper <- the nodes must lie in [0, 1]"),
        (dict(density=1e300, sigma=[1e300, 1e300]), ".sigma <- the candidate bound density c tau max(sigma g) is not a finite number"),
    ]
    held = [rows(sim, k) for k in range(3)]
    for bad, message in cases:
        kw = dict(ok, **bad)
        for call in (lambda: sim.ionize(**kw), lambda: sim.ionizeEvery(1, **kw)):
            with pytest.raises(fp.FusionPicError) as e:
                call()
            assert message in str(e.value) and e.value.code == -1, (bad, str(e.value))
    assert sim.ionize(**dict(ok, g_threshold=0.05))["candidates"] > 0            # g_lo == g_threshold is allowed
    for every in (0, -1):
        refused(fp, lambda: sim.ionizeEvery(every, **ok), -1, ".every <- must be at least 1")
    lib = sim._lib
    good = lambda: fp._ionize_spec(DT, list(L), **ok)
    assert lib.fpic_ionize(sim._h, None, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_ionize_register(sim._h, None, 1, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_ionize_stats(sim._h, 0, 0, None) == -1 and b".out <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    for poke in (lambda s: s.reserved.__setitem__(2, 1.0), lambda s: setattr(s, "reserved_i", 1), lambda s: setattr(s, "reserved_n", 1), lambda s: setattr(s, "reserved_u", 1)):
        s, keep = good()
        poke(s)
        for rc in (lib.fpic_ionize(sim._h, s, None), lib.fpic_ionize_register(sim._h, s, 1, None)):
            assert rc == -1 and b".reserved <- must be zero" in lib.fpic_last_error(sim._h)
    for index in (0, -1):
        refused(fp, lambda: sim.ionizeStats(index), -1, ".index <- no such registered ioniser")
    assert sim.collideGasEvery(1, "exchange", **GAS_ON) == 0 and sim.injectEvery(1000, count=1, vth=0.01) == 0
    assert [sim.ionizeEvery(1000 + k, **dict(ok, seed=k)) for k in range(fp.IONIZE_MAX_OPS)] == list(range(fp.IONIZE_MAX_OPS))
    refused(fp, lambda: sim.ionizeEvery(1, **ok), -1, ".spec <- FPIC_IONIZE_MAX_OPS (8) ionisers are registered already")
    refused(fp, lambda: sim.ionizeStats(fp.IONIZE_MAX_OPS), -1, ".index <- no such registered ioniser")
    with pytest.raises(fp.FusionPicError, match=r"\.scope <- "):
        sim._check(lib.fpic_ionize_stats(sim._h, 0, 7, fp.IonizeResult()))
    # clearIonization leaves the gas operators and the sources; renumber is refused while an ioniser is registered
    sim.clearGas()
    sim.clearInjections()
    assert sim.remove(where={"x": (0.0, 0.5)}, species=0)["removed"] > 0          # (renumber has something to do: the species is thinned)
    refused(fp, lambda: sim.renumber(0), -5, "registered")
    assert sim.collideGasEvery(1, "exchange", **GAS_ON) == 0 and sim.injectEvery(1000, species=1, count=1, vth=0.01) == 0
    sim.clearIonization()
    assert sim.gasStats(0)["applications"] == 0 and sim.injectStats(0)["applications"] == 0
    refused(fp, lambda: sim.renumber(0), -5, "registered")                       # (the gas operator and the source still are)
    sim.clearGas()
    sim.clearInjections()
    assert sim.renumber(0) == sim.population(0)["n"]
    s, keep = good()
    assert lib.fpic_ionize(sim._h, s, None) == 0                                # `out` is optional
    sim.destroy()
    del held


def test_a_decomposition_is_refused(fp):
    sims = [unit_box(fp, "fp32", "poisson_fft", 100, ni=50, b=False)[0] for _ in range(2)]
    for r, s in enumerate(sims):
        s.domainInit(r, 2, ghost_planes=1)
    group = fp.BoxGroup(sims)
    for owner in sims + [group]:
        for call in (lambda: owner.ionize(**ION_UNIT), lambda: owner.ionizeEvery(1, **ION_UNIT), lambda: owner.ionizeStats(0), owner.clearIonization):
            refused(fp, call, -5, "undecomposed")
    for s in sims:
        s.destroy()


# ---- 7b. the id bound of a thinned target
ID_END = (1 << 32) - 1


def raise_id_span(sim, species, span, room):
    """brings the id span of a species to `span` and leaves it empty of all but nothing: a thinned species keeps its span when
    a sink empties it and a source starts behind it, so cycles of inject and remove walk the span up by `room` a time"""
    sim.reserve(species, room)
    sim.remove(species=species)                                              # every particle: the species is thinned from here on
    while True:
        at = sim.population(species)["id_span"]
        if at == span:
            return
        assert sim.inject("volume", species=species, count=min(room, span - at), vth=0.01, seed=3)["injected"] > 0
        assert sim.remove(species=species)["removed"] > 0


@pytest.mark.parametrize("short", ["electron", "ion"])
def test_the_id_bound_of_a_thinned_target(fp, short):
    """id span + M <= 2^32 - 1: refused one id past the bound with nothing changed, done at the bound, where the last new
    particle takes the id 2^32 - 2"""
    n = 4101
    m = int(sc.reference("dense", n)[1]["event"].sum())
    room = 1 << 27
    target = 2 if short == "electron" else 1
    for past in (1, 0):
        sim = filled(fp, "fp32", n, third=True)
        raise_id_span(sim, target, ID_END - m + past, room)
        assert sim.population(target) == dict(n=0, capacity=room, id_span=ID_END - m + past)
        sim.reserve(3 - target, sim.population(3 - target)["n"] + 3 * m)      # (the other target has room for more than one application)
        held = [rows(sim, k) for k in range(3)]
        pops = [sim.population(k) for k in range(3)]
        call = lambda: sim.ionize(species=0, electron=2, ion=1, **sc.DENSE)
        if past:
            refused(fp, call, -1, "." + short + " <- ", "ids below %d" % (ID_END - m + 1), "nothing was changed")
            assert all(same_rows(rows(sim, k), held[k]) for k in range(3)) and [sim.population(k) for k in range(3)] == pops
        else:
            assert call()["ionised"] == m
            ids, pos, vel = rows(sim, target)
            assert bits(ids, np.arange(ID_END - m, ID_END, dtype=np.uint32)) and int(ids[-1]) == (1 << 32) - 2
            assert sim.population(target) == dict(n=m, capacity=room, id_span=ID_END)
            primaries = np.flatnonzero((rows(sim, 0)[2] != held[0][2]).any(axis=1))
            assert bits(pos, held[0][1][primaries])                          # by rank: the primaries' positions in ascending id
            other = rows(sim, 3 - target)
            assert bits(other[1][-m:], pos)
            refused(fp, lambda: sim.ionize(species=0, electron=2, ion=1, **dict(sc.DENSE, epoch=7)), -1, "." + short + " <- ")     # the span is full
        sim.destroy()


# ---- 11. the JavaScript host
def test_ionize_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    n, ni = 4000, 500
    spec = spec_of(n, solver="poisson_fft")
    populations = [dict(species=0, seed=123456789, stream=3, drift=[0.0, 0.01, 0.0], vth=0.05), dict(species=1, seed=5, stream=4, vth=0.001)]
    listed = lambda kw: {k: (v.tolist() if isinstance(v, np.ndarray) else [None if t is None else list(map(float, t)) for t in v] if k == "taper" else list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
    now = listed(dict(sc.SCENES["window"], species=0, ion=1, seed=0x1051E0123456))     # (below 2^53: JSON carries it as a number)
    on = listed(dict(sc.DENSE, species=0, electron=0, ion=1, density=sc.DENSE["density"] * 1e-11, seed=77))
    camel = lambda kw: {dict(g_lo="gLo", g_hi="gHi", g_threshold="gThreshold").get(k, k): v for k, v in kw.items()}       # the JavaScript host's names
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, populations=populations, ion=[MI, QE, ni], room=3000, now=camel(now), on=camel(on))))
    script = r"""
const fs = require('fs');
const crypto = require('crypto');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.addSpecies(inp.ion[0], inp.ion[1], inp.ion[2]);
for (const p of inp.populations) sim.load(p);
for (const k of [0, 1]) sim.reserve(k, sim.population(k).n + inp.room);
sim.precalc();
const group = (g) => ({energy_fixed: g.energyFixed.toString(), momentum_fixed: g.momentumFixed.map((x) => x.toString()), energy: g.energy, momentum: Array.from(g.momentum), charge: g.charge});
const plain = (r) => ({applications: r.applications, candidates: r.candidates, below: r.below, above: r.above, ionised: r.ionised,
  primary: group(r.primary), electron: group(r.electron), ion: group(r.ion)});
const first = plain(sim.ionize(inp.now));
const held = sim.getParticles(null, 1).position.length / 3;
const index = sim.ionizeEvery(2, inp.on);
sim.step(2);
const stats = plain(sim.ionizeStats(index));
const local = plain(sim.ionizeStats(index, 'local'));
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const rows = [0, 1].map((k) => { const r = sim.select({species: k}); return [sha(r.ids), sha(r.position), sha(r.velocity)]; });
const counts = [0, 1].map((k) => [sim.population(k).n, sim.getParticles(null, k).position.length / 3]);
const errors = [];
const ok = inp.on;
const tries = [() => sim.ionize({}), () => sim.ionize(7), () => sim.ionize(Object.assign({}, ok, {ion: undefined})), () => sim.ionize(Object.assign({}, ok, {ion: 0})),
  () => sim.ionize(Object.assign({}, ok, {electron: 1})), () => sim.ionize(Object.assign({}, ok, {electron: 0.5})), () => sim.ionize(Object.assign({}, ok, {ion: 5})),
  () => sim.ionize(Object.assign({}, ok, {gThreshold: 'x'})), () => sim.ionize(Object.assign({}, ok, {gThreshold: 1})), () => sim.ionize(Object.assign({}, ok, {sigma: [1e-19]})),
  () => sim.ionize(Object.assign({}, ok, {density: -1})), () => sim.ionize(Object.assign({}, ok, {taper: [null, [1], null]})), () => sim.ionizeEvery(0, ok),
  () => sim.ionizeEvery(1.5, ok), () => sim.ionizeStats(4), () => sim.ionizeStats(0.5)];
for (const t of tries) { try { t(); errors.push(null); } catch (err) { errors.push(String(err.message)); } }
sim.clearIonization();
let cleared = null;
try { sim.ionizeStats(0); } catch (err) { cleared = String(err.message); }
console.log(JSON.stringify({first: first, held: held, index: index, stats: stats, local: local, rows: rows, counts: counts, errors: errors, cleared: cleared}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    sim = fp.makeCylindricalParticlePusher(spec)
    assert sim.addSpecies(MI, QE, ni) == 1
    for p in populations:
        sim.load(**p)
    for k in range(2):
        sim.reserve(k, sim.population(k)["n"] + 3000)
    sim.precalc()

    def text(r):
        g = lambda x: dict(x, energy_fixed=str(x["energy_fixed"]), momentum_fixed=[str(v) for v in x["momentum_fixed"]])
        return dict(r, primary=g(r["primary"]), electron=g(r["electron"]), ion=g(r["ion"]))
    first = text(sim.ionize(**now))
    held = len(sim.getParticles(species=1)["position"])
    index = sim.ionizeEvery(2, **on)
    sim.step(2)
    stats = text(sim.ionizeStats(index))
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    want = [[sha(x) for x in rows(sim, k)] for k in range(2)]
    counts = [[sim.population(k)["n"], len(sim.getParticles(species=k)["position"])] for k in range(2)]
    sim.destroy()
    assert out["first"] == first and first["ionised"] > 5 and first["electron"]["energy_fixed"] != "0"
    assert out["held"] == held == ni + first["ionised"]                      # the getter's length check has asked the library
    assert out["index"] == index == 0 and out["stats"] == stats == out["local"] and stats["applications"] >= 1 and stats["ionised"] > 50
    assert out["rows"] == want and out["counts"] == counts and all(a == b for a, b in counts)
    assert all(err is not None and " <- " in err for err in out["errors"]), out["errors"]
    assert out["cleared"] is not None and ".index <- no such registered ioniser" in out["cleared"]
