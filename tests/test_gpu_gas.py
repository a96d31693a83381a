"""The windowed background collisions (fpic_gas*) on the GPU against the numpy restatement of their rule
(tests/gas_reference.py, proved on the CPU by tests/test_gas_reference.py, where the scenes used here are defined and their
margins are shown to hold): who collides exactly, the rounded values within a bound, the exact tallies, both forms of every
choice the host makes on either side of its threshold, the registered form against a manual loop, a decomposition that must
hold the same particles as one handle (as a group, and as ranks with a communicator whose GLOBAL tallies must be one
handle's), the refusals, and the JavaScript host.

The bound of the rounded parts is the one tests/test_gpu_collide.py builds, with its constant: ULPS = 4 x 2.29 + REF_ULPS
ulps on each normal and on cospi / sinpi, carried through vth, g M, plus one rounding per operation of the rule on either
side (one spacing).  The window, the tapers, the table lookup and the acceptance are decided exactly: the margins proved on
the CPU put every decision out of reach of those few ulps.  Met on an MI355X at 100003 particles (fp64): largest |dv| / bound
0.216 (exchange), 0.220 (elastic); fp32: no stored value that is not bit-equal to the rounded reference.

The decomposition runs on (8, 8, 24) nodes, not 16^3: three slabs of a full-EM box need 24 planes."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gas_reference as ref
from helpers import ROOT
from test_gas_reference import (BACKGROUND, DT, G_HI, G_LO, L, ME, P30, QE, SCENES, SHAPE, SIZES, TABLE, TAPERS, THRESHOLD_SCENES, WINDOW, big_n, code, compact_range,
                                density_for, gas, margins_hold, reference, scene, window_first_max)
from test_gpu_collide import ULPS
from test_gpu_histogram import PRECISIONS, em_dt

pytestmark = pytest.mark.gpu

DTYPE = {"fp32": np.float32, "fp64": np.float64}
W = 2.5e5
N_BIG = big_n()                                  # just above one full trip of the grid-stride loop: a second trip and a ragged tail
assert N_BIG == 2048 * 256 * 4 + 1027 and N_BIG % 4 == 3
BIG = 100003


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def spec_of(n, solver="none", dt=DT, shape=SHAPE, lengths=L, **kw):
    s = dict(radius=lengths[0], length_y=lengths[1], height=lengths[2], nr=shape[0], ny=shape[1], nz=shape[2], dt=dt, nparticles=0, count=n,
             particle_mass=ME, particle_charge=-QE, geometry="cart3d", solver=solver, macro_weight=W)
    s.update(kw)
    return s


def filled(fp, precision, n, **kw):
    sim = fp.makeCylindricalParticlePusher(spec_of(n, **kw), precision=precision)
    frac, vel = scene(n)
    sim.set(position=frac * np.array(L), velocity=vel)
    return sim


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def spacing(x):
    return np.spacing(np.maximum(np.abs(x), np.finfo(np.float64).tiny))


def value_bound(req, ids, v):
    """|v' - v'_ref| allowed per component for double velocities v: test_gpu_collide.value_bound on this operator's words"""
    n = ref.normals(req, ids)
    th = req["vth"] * n
    vb = req["drift"] + th
    e_vb = ULPS * req["vth"] * spacing(n) + 2 * spacing(np.maximum(np.abs(th), np.abs(vb)))
    if req["kind"] == ref.EXCHANGE:
        return e_vb
    d = v - vb
    e_d = e_vb + spacing(np.maximum.reduce([np.abs(v), np.abs(vb), np.abs(d)]))
    g = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    e_g = e_d.sum(axis=1) + 6 * spacing(g)                      # |dg / dd_a| <= 1; three squares, two sums, the root
    w = ref.words(req, ids, 0)
    c = 1.0 - 2.0 * ((w[2].astype(np.float64) + 0.5) * 2.0 ** -32)
    s = np.sqrt(1.0 - c * c)
    phi2 = 2.0 * (w[3].astype(np.float64) * 2.0 ** -32)
    circ = np.stack([ref.cospi(phi2), ref.sinpi(phi2)], axis=1)
    nh = ref.direction(req, ids)
    e_nh = np.zeros_like(nh)
    e_nh[:, :2] = ULPS * s[:, None] * spacing(circ) + 2 * spacing(nh[:, :2])      # the root, the product
    t = g[:, None] * nh
    e_t = e_g[:, None] * np.abs(nh) + g[:, None] * e_nh + spacing(t)
    r = d - t
    e_r = e_d + e_t + spacing(np.maximum.reduce([np.abs(d), np.abs(t), np.abs(r)]))
    q = req["M"] * r
    e_q = req["M"] * e_r + spacing(q)
    return e_q + spacing(np.maximum.reduce([np.abs(v), np.abs(q), np.abs(v - q)]))


def check_tallies(got, before, after, collided, applications=1):
    """3. the returned integers are those Python computes from the read-back velocities, and the doubles are derived from them"""
    t = ref.tallies(before, after, collided)
    assert got["applications"] == applications and got["collided"] == t["collided"]
    assert got["energy_fixed"] == t["energy_fixed"] and got["momentum_fixed"] == t["momentum_fixed"], (got, t)
    d = ref.derived(t, ME, W)
    assert got["energy"] == d["energy"] and got["momentum"] == d["momentum"], (got, d)
    return t


def check_scene(fp, precision, name, n, sort):
    """one application of a scene to scene(n): 1. the decisions, 2. the values, 3. the tallies.  Returns largest |dv| / bound
    (fp64) or the share of stored values bit-equal to the rounded reference (fp32)."""
    T = DTYPE[precision]
    kind, kw = (SCENES.get(name) or THRESHOLD_SCENES[name])[:2]
    req, out = reference(name, n)
    frac, vel = scene(n)
    sim = filled(fp, precision, n)
    if sort:
        sim.sort()
    before = sim.getParticles()
    assert bits(before["velocity"], vel.astype(T)) and bits(before["position"], frac.astype(T))    # the handle stores what the reference was given
    got = sim.collideGas(kind, **kw)
    after = sim.getParticles()
    sim.destroy()
    hit = out["collided"]
    changed = (after["velocity"] != before["velocity"]).any(axis=1)
    assert np.array_equal(changed, hit), (name, n, precision, sort, int(changed.sum()), int(hit.sum()))
    assert {k: got[k] for k in ("candidates", "collided", "below", "above")} == ref.counts(out), (name, n, precision, sort)
    assert bits(after["velocity"][~hit], before["velocity"][~hit]) and bits(after["position"], before["position"])
    check_tallies(got, before["velocity"], after["velocity"], hit)
    if not hit.any():
        return 0.0
    want = out["v"][hit]
    if T == np.float32:
        equal = after["velocity"][hit] == want.astype(np.float32)
        return float(equal.mean())
    dv = np.abs(after["velocity"][hit] - want)
    bound = value_bound(req, np.arange(n)[hit], vel[hit])
    assert np.all(dv <= bound), (name, n, precision, float((dv / bound).max()))
    return float((dv / bound).max())


# ---- 1. who collides, exactly (with 2. and 3. at every size)
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("kind", ["exchange", "elastic"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_decisions(fp, precision, kind, sort):
    for n in SIZES + [N_BIG]:
        check_scene(fp, precision, kind, n, sort)


def test_nothing_to_collide_launches_nothing(fp):
    sim = filled(fp, "fp32", 257)
    before = sim.getParticles()
    zero = dict(applications=0, candidates=0, collided=0, below=0, above=0, energy_fixed=0, momentum_fixed=[0, 0, 0], energy=0.0, momentum=[0.0, 0.0, 0.0])
    assert sim.collideGas("exchange", **dict(gas("exchange", P30, 3), density=0.0)) == zero
    assert sim.collideGas("elastic", **dict(gas("elastic", P30, 3), sigma=np.zeros(16))) == zero
    assert bits(sim.getParticles()["velocity"], before["velocity"])
    # P_max = 1 on the whole box with a table that covers every speed: everybody is a candidate (the acceptance is g / g_hi)
    kw = dict(gas("exchange", P30, 3, sigma=np.full(2, 3e-19), g_lo=0.0, g_hi=0.5), density=1e32)
    req = ref.request(L, ref.EXCHANGE, **kw)
    want = ref.apply(req, np.arange(257), *scene(257))
    assert margins_hold(req, want)
    every = sim.collideGas("exchange", **kw)
    assert every["candidates"] == 257 and 20 < every["collided"] == int(want["collided"].sum()) < 257 and every["below"] == every["above"] == 0
    assert np.array_equal((sim.getParticles()["velocity"] != before["velocity"]).any(axis=1), want["collided"])
    sim.destroy()


# ---- 2. the values
@pytest.mark.parametrize("kind", ["exchange", "elastic"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_values_within_the_bound(fp, precision, kind):
    """fp64: within the bound (largest |dv| / bound on an MI355X: 0.216 exchange, 0.220 elastic); fp32: bit-equal to the
    rounded reference"""
    for sort in (False, True):
        figure = check_scene(fp, precision, kind, BIG, sort)
        if precision == "fp32":
            print("fp32 %s sorted=%s n=%d: share of stored values bit-equal to the rounded reference %.6f" % (kind, sort, BIG, figure))
            assert figure == 1.0
        else:
            print("fp64 %s sorted=%s n=%d: largest |dv| / bound %.3f" % (kind, sort, BIG, figure))
            assert 0 < figure <= 1.0


# ---- 3. the tallies
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_term_outside_the_fixed_point_range_makes_its_double_nan(fp, precision):
    n = 257
    sim = filled(fp, precision, n)
    vel = scene(n)[1].copy()
    vel[5] = (200.0, 0.0, 0.0)                                              # |v|^2 = 40000 >= 2^15: the energy's term is outside, vx itself inside
    vel[9] = (0.0, -40000.0, 0.0)                                           # vy itself outside (and |v|^2)
    sim.set(velocity=vel)
    but = lambda *who: np.isin(np.arange(n), who, invert=True)
    # one application per planted particle, with a flat table that reaches its speed (the acceptance is g / g_hi = 0.8) and
    # the first epoch at which the reference has it collide
    for who, g_hi, axis in ((5, 250.0, None), (9, 5.0e4, 1)):
        before = sim.getParticles()
        kw = dict(gas("exchange", P30, 3, sigma=np.full(2, 3e-19), g_lo=0.0, g_hi=g_hi), density=1e32)
        for epoch in range(1, 64):
            kw["epoch"] = epoch
            req = ref.request(L, ref.EXCHANGE, **kw)
            out = ref.apply(req, np.arange(n), before["position"], before["velocity"].astype(np.float64))
            if out["collided"][who] and margins_hold(req, out):
                break
        hit = out["collided"]
        assert hit[who]
        got = sim.collideGas("exchange", **kw)
        after = sim.getParticles()
        assert np.array_equal((after["velocity"] != before["velocity"]).any(axis=1), hit) and got["collided"] == int(hit.sum()) and got["applications"] == 1
        tally = lambda mask: ref.tallies(before["velocity"], after["velocity"], mask)
        # a term outside the range adds nothing to its sum and makes the sum's double NaN; the other sums are untouched
        assert np.isnan(got["energy"]) and got["energy_fixed"] == tally(hit & but(who))["energy_fixed"]
        whole = tally(hit)
        d = ref.derived(whole, ME, W)
        for a in range(3):
            if a == axis:
                assert np.isnan(got["momentum"][a]) and got["momentum_fixed"][a] == tally(hit & but(who))["momentum_fixed"][a]
            else:
                assert got["momentum_fixed"][a] == whole["momentum_fixed"][a] and got["momentum"][a] == d["momentum"][a]
    sim.destroy()


# ---- 4. both forms of every choice of the host, on either side of its threshold
@pytest.mark.parametrize("window", ["narrow", "wide", "whole"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_both_forms_on_either_side_of_their_thresholds(fp, precision, window):
    """the word and the window first (the narrow window lies below kGasWindowFirstMax, the wide one above, the whole box has
    no window), the wave-shared loop and the queue (K just below, just above and between kGasCompactMin and kGasCompactMax)
    give the particles the reference gives"""
    lo, hi = compact_range()
    names = [name for name in THRESHOLD_SCENES if name.endswith(window)]
    assert len(names) == 5 and 0.375 < window_first_max() < 0.5625
    for name in names:
        for n in SIZES:
            check_scene(fp, precision, name, n, sort=(n % 2 == 1))


FORMS_SCRIPT = r"""
import hashlib, json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import fusionpic as fp
import test_gpu_gas as t
out = {}
for precision in ("fp32", "fp64"):
    for kind in ("exchange", "elastic"):
        sim = t.filled(fp, precision, t.BIG)
        sim.sort()
        got = sim.collideGas(kind, **t.SCENES[kind][1])
        out[precision + kind] = [got["candidates"], got["collided"], got["below"], got["above"], str(got["energy_fixed"]), hashlib.sha256(sim.getParticles()["velocity"].tobytes()).hexdigest()]
        sim.destroy()
print(json.dumps(out))
"""


@pytest.mark.parametrize("forms", [5, 6, 9, 10])
def test_the_forms_behind_the_test_switch_give_the_same_particles(fp, forms):
    """FPIC_GAS_FORMS is read once, so each value gets a process of its own: the word (1) or the window (2) first, in the
    wave-shared loop (4) or through the queue (8), whatever the host would choose for the scene"""
    env = dict(os.environ, FPIC_GAS_FORMS=str(forms))
    raw = subprocess.check_output([sys.executable, "-c", FORMS_SCRIPT, os.path.join(ROOT, "fusion-sim_amd"), os.path.join(ROOT, "tests")], env=env, timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    for precision in PRECISIONS:
        for kind in ("exchange", "elastic"):
            sim = filled(fp, precision, BIG)
            sim.sort()
            got = sim.collideGas(kind, **SCENES[kind][1])
            want = [got["candidates"], got["collided"], got["below"], got["above"], str(got["energy_fixed"]), hashlib.sha256(sim.getParticles()["velocity"].tobytes()).hexdigest()]
            sim.destroy()
            assert out[precision + kind] == want and got["collided"] > 100, (forms, precision, kind)


# ---- 5. the registered form equals the manual loop
@pytest.mark.parametrize("solver", ["none", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_registered_equals_manual(fp, precision, solver):
    n = 4099
    dt = em_dt(SHAPE, L) if solver == "yee" else DT
    a, b = (filled(fp, precision, n, solver=solver, dt=dt) for _ in range(2))
    for s in (a, b):
        s.precalc()
    relax = dict(nu_tau=0.2, seed=53, drift=0.0, vth=0.01)
    gas_ops = [(2, "elastic", dict(gas("elastic", P30, 61, stream=1, epoch=100, taper=TAPERS, **WINDOW), tau=2 * dt)),
               (1, "exchange", dict(gas("exchange", 0.01 * 2.0 ** 32, 62, stream=2), tau=dt))]
    pair = dict(log_lambda=10.0, seed=51, stream=1)
    # registered in another order than they run: the background operators first, then the gas, then the pairs
    assert a.collidePairEvery(1, 0, **pair) == 0
    assert [a.collideGasEvery(every, kind, **kw) for every, kind, kw in gas_ops] == [0, 1]
    assert a.collideEvery(1, "relax", **relax) == 0
    steps = 4
    a.substeps(steps)
    sums = [dict(ref.ZERO, applications=0, candidates=0, below=0, above=0) for _ in gas_ops]
    for k in range(1, steps + 1):
        b.substeps(1)
        b.collide("relax", epoch=k, **relax)
        for (every, kind, kw), total in zip(gas_ops, sums):
            if k % every == 0:
                got = b.collideGas(kind, **dict(kw, epoch=k + kw["epoch"]))
                total.update(ref.add_tallies(total, got))
                for key in ("applications", "candidates", "below", "above"):
                    total[key] += got[key]
        b.collidePair(0, tau=dt, epoch=k, **pair)
    pa, pb = a.getParticles(), b.getParticles()
    assert bits(pa["velocity"], pb["velocity"]) and bits(pa["position"], pb["position"])
    for i, total in enumerate(sums):
        got = a.gasStats(i)
        d = ref.derived(total, ME, W)
        assert got == dict(total, energy=d["energy"], momentum=d["momentum"]), (i, got, total)
        assert a.gasStats(i, "local") == got
    assert [s["applications"] for s in sums] == [2, 4] and all(s["collided"] > 0 for s in sums)
    # clearGas leaves the operators of collideEvery and collidePairEvery in place, clearCollisions those of collideGasEvery
    a.clearGas()
    with pytest.raises(fp.FusionPicError, match=r"\.index <- "):
        a.gasStats(0)
    assert a.collisionStats(0)["applications"] == steps and a.pairStats(0)["applications"] == steps
    a.substeps(1)
    b.substeps(1)
    b.collide("relax", epoch=steps + 1, **relax)
    b.collidePair(0, tau=dt, epoch=steps + 1, **pair)
    assert bits(a.getParticles()["velocity"], b.getParticles()["velocity"])
    assert a.collideGasEvery(1, "exchange", **gas_ops[1][2]) == 0           # a new registration starts from zero
    a.clearCollisions()
    with pytest.raises(fp.FusionPicError, match=r"\.index <- "):
        a.collisionStats(0)
    a.substeps(1)
    b.substeps(1)
    got = b.collideGas("exchange", **dict(gas_ops[1][2], epoch=steps + 2))
    b.collidePair(0, tau=dt, epoch=steps + 2, **pair)
    assert bits(a.getParticles()["velocity"], b.getParticles()["velocity"])
    stats = a.gasStats(0)
    assert stats["applications"] == 1 and {k: stats[k] for k in got if k != "applications"} == {k: got[k] for k in got if k != "applications"}
    a.destroy()
    b.destroy()


# ---- 6. a decomposition holds the same particles
DSHAPE = (8, 8, 24)                                                          # (three slabs of a full-EM box need 2 (G + 2) <= nz / 3 planes)
DL = (2.0 ** -7, 2.0 ** -7, 3 * 2.0 ** -7)


DN = 20011
POPULATION = dict(seed=0xABCDEF, stream=6, drift=(0.0, 0.0, 0.1), vth=0.03)


def decomposed_op():
    return dict(gas("elastic", P30, 71, stream=4, epoch=7, taper=TAPERS), lo=(DL[0] / 4, 0.0, DL[2] / 8), hi=(3 * DL[0] / 4, DL[1], 7 * DL[2] / 8))


def decomposed_handle(fp, precision, solver):
    dt = em_dt(DSHAPE, DL) if solver == "yee" else DT
    return fp.makeCylindricalParticlePusher(spec_of(DN, solver=solver, dt=dt, shape=DSHAPE, lengths=DL, macro_weight=1e3), precision=precision)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_decomposition_holds_the_same_particles(fp, precision, solver, world):
    n, population, op = DN, POPULATION, decomposed_op()
    make = lambda: decomposed_handle(fp, precision, solver)
    one = make()
    assert one.load(**population) == n
    sims = []
    for r in range(world):
        s = make()
        s.domainInit(r, world, ghost_planes=2, migrate_every=2, distributed_solve=0)
        sims.append(s)
    g = fp.BoxGroup(sims)
    assert sum(g.load(count=n, **population)) == n
    one.precalc()
    g.precalc()
    first = (one.collideGas("elastic", **op), g.collideGas("elastic", **op))
    assert first[0] == first[1] and 0 < first[0]["collided"] < first[0]["candidates"] < n
    assert one.collideGasEvery(1, "elastic", **op) == g.collideGasEvery(1, "elastic", **op) == 0
    one.step(4)
    g.step(4)
    stats = [m.domainStats() for m in g.sims]
    assert sum(s["migrated"] for s in stats) > 0 and sum(s["lost"] for s in stats) == 0
    want = one.getParticles()
    parts = [m.domainGet() for m in g.sims]
    ids = np.concatenate([p["ids"] for p in parts])
    order = np.argsort(ids, kind="stable")
    assert np.array_equal(ids[order], np.arange(n))
    for key in ("position", "velocity"):
        assert bits(np.concatenate([p[key] for p in parts])[order], want[key]), key
    whole, summed = one.gasStats(0), g.gasStats(0)
    applications = whole["applications"]
    assert whole == summed and applications >= 4 and 0 < whole["collided"] < whole["candidates"] < applications * n, (whole, summed)
    assert len({m.gasStats(0, "local")["candidates"] for m in g.sims}) > 1
    g.clearGas()
    one.destroy()
    for m in g.sims:
        m.destroy()


# ---- the communicator: ranks as threads of one process over the stand-in RCCL (tests/fake_rccl, as test_gpu_energy.py)
COMM_DRIVER = r"""
import json, os, sys, threading
sys.path.insert(0, os.path.join(sys.argv[1], "fusion-sim_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import fusionpic as fp
import test_gpu_gas as t
world, precision = int(sys.argv[2]), sys.argv[3]
uid = fp.commUniqueId()
out, err = [None] * world, [None] * world
def rank_main(r):
    try:
        s = t.decomposed_handle(fp, precision, "poisson_fft")
        s.commInit(uid, r, world)
        s.domainInit(r, world, ghost_planes=2, migrate_every=2, distributed_solve=0)
        s.load(count=t.DN, **t.POPULATION)
        s.precalc()
        s.collideGasEvery(1, "elastic", **t.decomposed_op())
        s.step(4)
        stats = s.gasStats(0, "global")
        out[r] = dict(stats, energy_fixed=str(stats["energy_fixed"]), momentum_fixed=[str(x) for x in stats["momentum_fixed"]], local=s.gasStats(0, "local")["candidates"])
        s.destroy()
    except Exception as e:
        err[r] = repr(e)
threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
for th in threads: th.start()
for th in threads: th.join()
print(json.dumps({"error": err} if any(err) else {"ranks": out}))
"""


@pytest.mark.parametrize("world,precision", [(2, "fp32"), (3, "fp64")])
def test_communicator_global_tallies_are_one_handles(fp, world, precision):
    """GLOBAL with a communicator adds the ranks' 128-bit sums exactly (four 32-bit limbs through the shared rank-sum): every
    rank reports the integers of one handle that holds the whole box"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "fake_rccl")])
    env = dict(os.environ, FPIC_RCCL_LIBRARY=os.path.join(ROOT, "tests", "fake_rccl", "libfakerccl.so"))
    raw = subprocess.check_output([sys.executable, "-c", COMM_DRIVER, ROOT, str(world), precision], env=env, timeout=240)
    res = json.loads(raw.decode().strip().splitlines()[-1])
    assert "error" not in res, res
    one = decomposed_handle(fp, precision, "poisson_fft")
    assert one.load(**POPULATION) == DN
    one.precalc()
    assert one.collideGasEvery(1, "elastic", **decomposed_op()) == 0
    one.step(4)
    whole = one.gasStats(0)
    one.destroy()
    want = dict(whole, energy_fixed=str(whole["energy_fixed"]), momentum_fixed=[str(x) for x in whole["momentum_fixed"]])
    for r in res["ranks"]:
        assert {k: v for k, v in r.items() if k != "local"} == want, (r, want)
    assert whole["collided"] > 0 and whole["energy_fixed"] != 0 and len({r["local"] for r in res["ranks"]}) > 1


# ---- 7. refusals; the next valid call succeeds
def test_refusals(fp):
    from helpers import make_spec
    rz = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    ok = gas("exchange", P30, 1)
    for call in (lambda: rz.collideGas("exchange", **ok), lambda: rz.collideGasEvery(1, "exchange", **ok), lambda: rz.gasStats(0), rz.clearGas):
        with pytest.raises(fp.FusionPicError, match="needs a CART3D handle") as e:
            call()
        assert e.value.code == -5
    rz.destroy()
    sim = filled(fp, "fp32", 1000)
    nan, inf = float("nan"), float("inf")
    window = ".lo, .hi <- the window must lie within 0 <= lo < hi <= L"
    cases = [
        (2, {}, ".kind <- must be 0 (exchange) or 1 (elastic)"), (-1, {}, ".kind <- must be 0"), ("exchange", dict(species=1), ".species <- no such species"),
        ("exchange", dict(species=-1), ".species <- no such species"),
        ("exchange", dict(density=-1.0), ".density <- must be finite and not negative"), ("exchange", dict(density=inf), ".density <- must be finite"), ("exchange", dict(density=nan), ".density <- "),
        ("exchange", dict(tau=0.0), ".tau <- must be positive and finite"), ("exchange", dict(tau=inf), ".tau <- must be positive and finite"), ("exchange", dict(tau=nan), ".tau <- "),
        ("exchange", dict(sigma=[1e-19]), ".n <- must be 2 .. FPIC_GAS_TABLE_MAX (4096)"), ("exchange", dict(sigma=np.ones(4097) * 1e-19), ".n <- must be 2 .. FPIC_GAS_TABLE_MAX (4096)"),
        ("exchange", dict(g_lo=-0.1), ".g_lo <- must be finite and not negative"), ("exchange", dict(g_lo=nan), ".g_lo <- "),
        ("exchange", dict(g_hi=G_LO), ".g_hi <- must be finite and above g_lo"), ("exchange", dict(g_hi=inf), ".g_hi <- must be finite and above g_lo"),
        ("exchange", dict(sigma=[1e-19, -1e-19]), ".sigma <- every entry must be finite and not negative"), ("exchange", dict(sigma=[1e-19, nan]), ".sigma <- every entry"),
        ("exchange", dict(sigma=[inf, 1e-19]), ".sigma <- every entry"),
        ("exchange", dict(drift=(0, nan, 0)), ".drift <- must be finite"), ("exchange", dict(vth=(0, -1e-3, 0)), ".vth <- must be finite and not negative"), ("exchange", dict(vth=inf), ".vth <- "),
        ("elastic", dict(mass_ratio=0.0), ".mass_ratio <- must be positive (+inf: a fixed target) for FPIC_GAS_ELASTIC"), ("elastic", dict(mass_ratio=nan), ".mass_ratio <- must be positive"),
        ("exchange", dict(mass_ratio=2.0), ".mass_ratio <- must be 0 for FPIC_GAS_EXCHANGE"),
        ("exchange", dict(lo=(0, nan, 0)), ".lo, .hi <- must be finite"), ("exchange", dict(hi=inf), ".lo, .hi <- must be finite"),
        ("exchange", dict(lo=(-1e-9, 0, 0)), window), ("exchange", dict(hi=(L[0], L[1], L[2] * 1.001)), window), ("exchange", dict(lo=L[0] / 2, hi=L[0] / 2), window),
        ("exchange", dict(lo=L[0] / 2, hi=L[0] / 4), window),
        ("exchange", dict(taper=(None, [1.0], None)), ".taper_n <- a table has 2 .. FPIC_GAS_TAPER_MAX nodes (0: none)"), ("exchange", dict(taper=(np.ones(1026), None, None)), ".taper_n <- a table has 2 .."),
        ("exchange", dict(taper=(None, None, [1.0, 1.0000001])), ".taper <- the nodes must lie in [0, 1]"), ("exchange", dict(taper=(None, None, [-1e-9, 1.0])), ".taper <- the nodes must lie in [0, 1]"),
        ("exchange", dict(taper=([0.5, nan], None, None)), ".taper <- the nodes must lie in [0, 1]"),
        ("exchange", dict(density=1e300, sigma=[1e300, 1e300]), ".sigma <- the candidate bound density c tau max(sigma g) is not a finite number"),
    ]
    before = sim.getParticles()
    for kind, bad, message in cases:
        kw = dict(ok, **bad)
        for call in (lambda: sim.collideGas(kind, **kw), lambda: sim.collideGasEvery(1, kind, **kw)):
            with pytest.raises(fp.FusionPicError) as e:
                call()
            assert message in str(e.value) and e.value.code == -1, (kind, bad, str(e.value))
    for every in (0, -1):
        with pytest.raises(fp.FusionPicError, match=r"\.every <- must be at least 1"):
            sim.collideGasEvery(every, "exchange", **ok)
    lib = sim._lib
    good = lambda: fp._gas_spec(DT, list(L), "exchange", **ok)
    assert lib.fpic_gas(sim._h, None, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_gas_register(sim._h, None, 1, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_gas_stats(sim._h, 0, 0, None) == -1 and b".out <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    for poke in (lambda s: s.reserved.__setitem__(2, 1.0), lambda s: setattr(s, "reserved_i", 1), lambda s: setattr(s, "reserved_u", 1)):
        s, keep = good()
        poke(s)
        for rc in (lib.fpic_gas(sim._h, s, None), lib.fpic_gas_register(sim._h, s, 1, None)):
            assert rc == -1 and b".reserved <- must be zero" in lib.fpic_last_error(sim._h)
    s, keep = good()
    s.taper_n[0] = 2                                                         # a null table with a node count
    assert lib.fpic_gas(sim._h, s, None) == -1 and b"null but its node count is not zero" in lib.fpic_last_error(sim._h)
    s, keep = good()
    s.sigma = None
    assert lib.fpic_gas(sim._h, s, None) == -1 and b".sigma <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    for index in (0, -1):
        with pytest.raises(fp.FusionPicError, match=r"\.index <- no such registered operator"):
            sim.gasStats(index)
    now = sim.getParticles()
    assert bits(now["velocity"], before["velocity"]) and bits(now["position"], before["position"])   # nothing refused has touched a particle
    assert sim.collideEvery(1, "relax", nu_tau=0.1, vth=0.01) == 0
    assert [sim.collideGasEvery(1 + k % 2, "exchange", **dict(ok, seed=k)) for k in range(fp.GAS_MAX_OPS)] == list(range(fp.GAS_MAX_OPS))
    with pytest.raises(fp.FusionPicError, match=r"\.spec <- FPIC_GAS_MAX_OPS \(8\) operators are registered already"):
        sim.collideGasEvery(1, "exchange", **ok)
    with pytest.raises(fp.FusionPicError, match=r"\.index <- no such registered operator"):
        sim.gasStats(fp.GAS_MAX_OPS)
    with pytest.raises(fp.FusionPicError, match=r"\.scope <- "):
        sim._check(lib.fpic_gas_stats(sim._h, 0, 7, fp.GasResult()))
    sim.precalc()
    sim.substeps(2)
    assert sim.gasStats(0)["applications"] == 2 and sim.gasStats(1)["applications"] == 1 and sim.gasStats(0)["collided"] > 0
    # clearGas leaves the operators of collideEvery in place, and clearCollisions those of collideGasEvery
    sim.clearGas()
    assert sim.collisionStats(0)["applications"] == 2
    assert sim.collideGasEvery(1, "exchange", **ok) == 0
    sim.clearCollisions()
    sim.substeps(1)
    assert sim.gasStats(0)["applications"] == 1
    with pytest.raises(fp.FusionPicError, match=r"\.index <- "):
        sim.collisionStats(0)
    sim.clearGas()
    s, keep = good()
    assert lib.fpic_gas(sim._h, s, None) == 0                                # `out` is optional
    assert sim.collideGas("exchange", **ok)["candidates"] > 0 and sim.collideGasEvery(1, "exchange", **ok) == 0
    sim.destroy()


# ---- 8. the JavaScript host
def test_gas_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    n = 4000
    spec = spec_of(n)
    population = dict(seed=123456789, stream=3, drift=[0.0, 0.01, 0.0], vth=0.05)
    listed = lambda kw: {k: (v.tolist() if isinstance(v, np.ndarray) else [None if t is None else list(map(float, t)) for t in v] if k == "taper" else list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
    now = listed(dict(gas("elastic", P30, 81, stream=2, epoch=5, taper=TAPERS, **WINDOW), kind="elastic"))
    on = listed(dict(gas("exchange", 0.05 * 2.0 ** 32, 82, stream=3), kind="exchange"))
    camel = lambda kw: {dict(g_lo="gLo", g_hi="gHi", mass_ratio="massRatio").get(k, k): v for k, v in kw.items()}       # the JavaScript host's names
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, population=population, now=camel(now), on=camel(on))))
    script = r"""
const fs = require('fs');
const crypto = require('crypto');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.load(inp.population);
sim.precalc();
const plain = (r) => ({applications: r.applications, candidates: r.candidates, collided: r.collided, below: r.below, above: r.above,
  energy_fixed: r.energyFixed.toString(), momentum_fixed: r.momentumFixed.map((x) => x.toString()), energy: r.energy, momentum: Array.from(r.momentum)});
const first = plain(sim.collideGas(inp.now));
const index = sim.collideGasEvery(2, inp.on);
sim.step(2);
const stats = plain(sim.gasStats(index));
const local = plain(sim.gasStats(index, 'local'));
const r = sim.select({});
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const errors = [];
const ok = inp.on;
const tries = [() => sim.collideGas(Object.assign({}, ok, {kind: 'relax'})), () => sim.collideGas({}), () => sim.collideGas(7), () => sim.collideGas(Object.assign({}, ok, {sigma: [1e-19]})),
  () => sim.collideGas(Object.assign({}, ok, {sigma: 'x'})), () => sim.collideGas(Object.assign({}, ok, {species: 3})), () => sim.collideGas(Object.assign({}, ok, {epoch: -1})),
  () => sim.collideGas(Object.assign({}, ok, {taper: [null, [1], null]})), () => sim.collideGas(Object.assign({}, ok, {taper: [null, [0.5, 2], null]})),
  () => sim.collideGas(Object.assign({}, ok, {drift: [1, 2]})), () => sim.collideGas(Object.assign({}, ok, {density: -1})), () => sim.collideGasEvery(0, ok),
  () => sim.collideGasEvery(1, Object.assign({}, ok, {lo: 1})), () => sim.gasStats(4), () => sim.gasStats(0.5)];
for (const t of tries) { try { t(); errors.push(null); } catch (err) { errors.push(String(err.message)); } }
sim.clearGas();
let cleared = null;
try { sim.gasStats(0); } catch (err) { cleared = String(err.message); }
console.log(JSON.stringify({first: first, index: index, stats: stats, local: local, ids: sha(r.ids), position: sha(r.position), velocity: sha(r.velocity), errors: errors, cleared: cleared}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    sim = fp.makeCylindricalParticlePusher(spec)
    sim.load(**population)
    sim.precalc()
    text = lambda r: dict(r, energy_fixed=str(r["energy_fixed"]), momentum_fixed=[str(x) for x in r["momentum_fixed"]])
    call = lambda kw: (kw["kind"], {k: v for k, v in kw.items() if k != "kind"})
    kind, kw = call(now)
    first = text(sim.collideGas(kind, **kw))
    kind, kw = call(on)
    index = sim.collideGasEvery(2, kind, **kw)
    sim.step(2)
    stats = text(sim.gasStats(index))
    want = sim.select()
    sim.destroy()
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    assert out["first"] == first and 0 < first["collided"] < first["candidates"] < n and first["energy_fixed"] != "0"
    assert out["index"] == index == 0 and out["stats"] == stats == out["local"] and stats["applications"] >= 1 and stats["collided"] > 0
    assert (out["ids"], out["position"], out["velocity"]) == (sha(want["ids"]), sha(want["position"]), sha(want["velocity"]))
    assert all(err is not None and " <- " in err for err in out["errors"]), out["errors"]
    assert out["cleared"] is not None and ".index <- " in out["cleared"]
