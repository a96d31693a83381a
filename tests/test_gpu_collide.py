"""The collision operator (fpic_collide*) on the GPU against the numpy restatement of its rule (tests/collide_reference.py,
proved on the CPU by tests/test_collide_reference.py): who collides exactly, the rounded values within a bound built from
measured deviations, the null-collision test, independence of the slot, the registered form against a manual loop, a
decomposition that must hold the same particles as one handle, the physics of repeated charge exchange, the refusals, and the
JavaScript host.

The bound of the rounded parts.  The rule's rounded functions are the loader's: the Box-Muller normals and cospi / sinpi of the
device's maths library, for which the ROCm on the machine states no ulp bounds.  The loader's kernel was measured against
50-digit values (scripts/probe_load.py ulps): largest deviation 2.29 float64 ulps.  Four times that bounds the kernel; the
reference's own deviation (below REF_ULPS, tests/test_collide_reference.py) is added because the comparison is with the
reference.  Every other operation of the rule is one rounding, counted once on either side.  Met on an MI355X at 100003
particles (fp64): largest |dv| / bound 0.429 (exchange), 0.353 (elastic), 0.282 (relax); fp32: no stored value that is not
bit-equal to the rounded reference.

EXCHANGE and ELASTIC have two passes chosen by P_max (fes_collide_kernels.hpp); test_both_passes_on_either_side_of_their_
thresholds runs both.  The decomposition test does not reach the arrivals of a riding migration: a migration and the push that
consumes it finish inside one sub-step, so no call and no hook meets a tail or a dead slot."""
import hashlib
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import collide_reference as ref
import load_reference as lref
from helpers import ROOT
from test_collide_reference import REF_ULPS
from test_gpu_histogram import PRECISIONS, box_spec, em_dt

pytestmark = pytest.mark.gpu

KERNEL_ULPS_MEASURED = 2.29    # the loader's device functions (tests/test_gpu_load.py)
ULPS = 4 * KERNEL_ULPS_MEASURED + REF_ULPS

SHAPE = (16, 16, 16)
L = (0.016, 0.016, 0.016)
SIZES = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 100003]
BIG = 100003
BACKGROUND = dict(drift=(0.01, 0.0, -0.02), vth=(0.05, 0.02, 0.1))


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def box(fp, precision, n, dt=5e-12, **kw):
    spec = box_spec(SHAPE, L, n, dt, macro_weight=1e15 * np.prod(L) / n, **kw)
    return fp.makeCylindricalParticlePusher(spec, precision=precision)


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


_scene = {}


def scene(n, seed=1, vth=0.05):
    """positions (metres) and velocities (c) of n particles, computed once per (n, seed, vth) and never changed"""
    key = (n, seed, vth)
    if key not in _scene:
        pos = np.random.default_rng(seed).random((n, 3)) * L
        vel = lref.velocities(lref.request(L, seed=seed, stream=11, drift=(0.0, 0.02, 0.0), vth=vth), np.arange(n))
        pos.setflags(write=False)
        vel.setflags(write=False)
        _scene[key] = (pos, vel)
    return _scene[key]


def filled(fp, precision, n, seed=1, vth=0.05, **kw):
    sim = box(fp, precision, n, **kw)
    pos, vel = scene(n, seed, vth)
    sim.set(position=pos, velocity=vel)
    return sim


def counts_of(out):
    return dict(candidates=int(out["candidate"].sum()), collided=int(out["collided"].sum()), clipped=int(out["clipped"].sum()))


def same_counts(got, out, applications=1):
    return got == dict(counts_of(out), applications=applications)


# ---- 1. who collides, exactly
def test_who_collides_exactly(fp):
    kw = dict(nu_tau=-math.log(0.7), seed=0xC0FFEE0123456789, stream=5, epoch=3, **BACKGROUND)
    req = ref.request(ref.EXCHANGE, **kw)
    assert abs(req["K"] * 2.0 ** -32 - 0.3) < 1e-9
    for n in SIZES:
        ids = np.arange(n)
        sets = {}
        for precision in PRECISIONS:
            sim = filled(fp, precision, n)
            before = sim.getParticles()
            got = sim.collide("exchange", **kw)
            after = sim.getParticles()
            want = ref.stored(req, ids, before["velocity"])
            changed = (after["velocity"] != before["velocity"]).any(axis=1)
            assert np.array_equal(changed, want["candidate"]), (n, precision)
            assert got["candidates"] == got["collided"] == int(want["candidate"].sum()) and got["clipped"] == 0 and got["applications"] == 1
            assert bits(after["velocity"][~changed], before["velocity"][~changed]) and bits(after["position"], before["position"])
            sets[precision] = changed
            # nu_tau = 0 changes nothing and returns zeros; +inf collides all
            assert sim.collide("exchange", **dict(kw, nu_tau=0.0)) == dict(applications=0, candidates=0, collided=0, clipped=0)
            assert bits(sim.getParticles()["velocity"], after["velocity"])
            every = sim.collide("exchange", **dict(kw, nu_tau=math.inf, epoch=4))
            assert every == dict(applications=1, candidates=n, collided=n, clipped=0)
            assert (sim.getParticles()["velocity"] != after["velocity"]).any(axis=1).all()
            sim.destroy()
        assert np.array_equal(sets["fp32"], sets["fp64"])


def compact_range():
    """kCollideCompactMin, kCollideCompactMax of the kernel header: the K between which the compacting pass serves a request"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_collide_kernels.hpp")).read()
    m = re.search(r"kCollideCompactMin\s*=\s*1ull\s*<<\s*(\d+)\s*,\s*kCollideCompactMax\s*=\s*1ull\s*<<\s*(\d+)\s*;", text)
    return 1 << int(m.group(1)), 1 << int(m.group(2))


def test_both_passes_on_either_side_of_their_thresholds(fp):
    """the plain and the compacting pass give the same particles: requests just below, at and just above the two thresholds"""
    lo, hi = compact_range()
    assert 0 < lo < hi < 1 << 32
    for target, inside in ((lo * 0.999, False), (lo * 1.001, True), ((lo * hi) ** 0.5, True), (hi * 0.999, True), (hi * 1.001, False)):
        kw = dict(nu_tau=-math.log1p(-target * 2.0 ** -32), seed=0xBADC0DE, stream=8, epoch=1, **BACKGROUND)
        req = ref.request(ref.EXCHANGE, **kw)
        assert (lo <= req["K"] <= hi) == inside and abs(req["K"] - target) < 4
        for n in SIZES:
            ids = np.arange(n)
            for precision in PRECISIONS:
                sim = filled(fp, precision, n)
                before = sim.getParticles()
                got = sim.collide("exchange", **kw)
                after = sim.getParticles()
                sim.destroy()
                want = ref.stored(req, ids, before["velocity"])
                changed = (after["velocity"] != before["velocity"]).any(axis=1)
                assert np.array_equal(changed, want["candidate"]) and same_counts(got, want), (target, n, precision)
                assert bits(after["velocity"][~changed], before["velocity"][~changed]) and bits(after["position"], before["position"])
                if precision == "fp64":
                    assert np.all(np.abs(after["velocity"] - want["v"]) <= value_bound(req, ids, before["velocity"]))
    # the null-collision form and a sorted species in the compacting pass
    kw = dict(nu_tau=0.01, sigma_tau=0.3, g_max=0.15, mass_ratio=2.0, seed=2027, stream=2, epoch=4, **BACKGROUND)
    req = ref.request(ref.ELASTIC, **kw)
    assert lo <= req["K"] <= hi
    n, ids = BIG, np.arange(BIG)
    for precision in PRECISIONS:
        sim = filled(fp, precision, n)
        sim.sort()
        before = sim.getParticles()
        want = ref.stored(req, ids, before["velocity"])
        cand = want["candidate"]
        x, ux = ref.acceptance(req, ids, want["g"])
        assert not (np.abs(ux - x)[cand] < 1e-9 * req["x_max"]).any() and not (np.abs(want["g"] - req["g_max"])[cand] < 1e-9 * req["g_max"]).any()
        assert 0 < want["clipped"].sum() < want["collided"].sum() < cand.sum()
        got = sim.collide("elastic", **kw)
        after = sim.getParticles()
        sim.destroy()
        assert same_counts(got, want)
        changed = (after["velocity"] != before["velocity"]).any(axis=1)
        assert np.array_equal(changed, want["collided"]) and bits(after["velocity"][~changed], before["velocity"][~changed])
        if precision == "fp64":
            assert np.all(np.abs(after["velocity"] - want["v"]) <= value_bound(req, ids, before["velocity"]))


# ---- 2. the rounded values
def spacing(x):
    return np.spacing(np.maximum(np.abs(x), np.finfo(np.float64).tiny))


def value_bound(req, ids, v):
    """|v' - v'_ref| allowed per component for double velocities v: ULPS ulps on each normal and on cospi / sinpi, carried
    through vth, g M and sv, plus one rounding per operation of the rule (half an ulp on either side: one spacing)"""
    n = ref.normals(req, ids)
    if req["kind"] == ref.RELAX:
        r = v - req["drift"]
        p, k = req["decay"] * r, req["sv"] * n
        q = p + k
        scale = np.maximum.reduce([np.abs(r), np.abs(p), np.abs(k), np.abs(q), np.abs(req["drift"] + q), np.abs(v)])
        return ULPS * req["sv"] * spacing(n) + 5 * spacing(scale)
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
    circ = np.stack([lref.cospi(phi2), lref.sinpi(phi2)], axis=1)
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


ROUNDED = {
    "exchange": dict(nu_tau=math.inf, seed=77, stream=2, epoch=5, **BACKGROUND),
    "elastic": dict(nu_tau=math.inf, mass_ratio=3.0, seed=78, stream=3, epoch=6, **BACKGROUND),
    "relax": dict(nu_tau=0.5, seed=79, stream=4, epoch=7, **BACKGROUND),
}


@pytest.mark.parametrize("kind", sorted(ROUNDED))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rounded_values_within_the_bound(fp, precision, kind):
    n, ids, kw = BIG, np.arange(BIG), ROUNDED[kind]
    req = ref.request(fp.COLLIDE_KINDS[kind], **kw)
    sim = filled(fp, precision, n)
    before = sim.getParticles()
    got = sim.collide(kind, **kw)
    after = sim.getParticles()
    sim.destroy()
    want = ref.stored(req, ids, before["velocity"])
    assert got == dict(applications=1, candidates=0 if kind == "relax" else n, collided=n, clipped=0)
    assert bits(after["position"], before["position"])
    if precision == "fp64":
        dv = np.abs(after["velocity"] - want["v"])
        bound = value_bound(req, ids, before["velocity"])
        print("fp64 %s: largest |dv| / bound %.3f, share bit-equal %.3f" % (kind, (dv / bound).max(), (dv == 0).mean()))
        assert np.all(dv <= bound)
    else:
        off = after["velocity"] != want["v"]
        print("fp32 %s: share not bit-equal %.2e" % (kind, off.mean()))
        assert np.all(np.abs(after["velocity"].astype(np.float64) - want["v"].astype(np.float64)) <= np.spacing(np.abs(want["v"])).astype(np.float64))
        assert off.mean() <= 1e-4


# ---- 3. the null-collision method
NULL = dict(nu_tau=0.05, sigma_tau=4.0, g_max=0.15, mass_ratio=2.0, seed=2026, stream=1, epoch=9, **BACKGROUND)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_null_collision(fp, precision):
    n, ids = BIG, np.arange(BIG)
    req = ref.request(ref.ELASTIC, **NULL)
    sim = filled(fp, precision, n)
    before = sim.getParticles()
    want = ref.stored(req, ids, before["velocity"])
    # the reference alone: no decision of a candidate hangs on the last bits (the seed was chosen so that this holds)
    cand = want["candidate"]
    x, ux = ref.acceptance(req, ids, want["g"])
    assert not (np.abs(ux - x)[cand] < 1e-9 * req["x_max"]).any()
    assert not (np.abs(want["g"] - req["g_max"])[cand] < 1e-9 * req["g_max"]).any()
    assert 0 < want["clipped"].sum() < want["collided"].sum() < cand.sum() < n       # every branch is taken
    assert (want["clipped"] & ~want["collided"]).sum() == 0                          # (a clipped candidate has x = x_max)
    got = sim.collide("elastic", **NULL)
    after = sim.getParticles()
    sim.destroy()
    print("null collision %s: %s" % (precision, got))
    assert same_counts(got, want)
    changed = (after["velocity"] != before["velocity"]).any(axis=1)
    assert np.array_equal(changed, want["collided"])
    assert bits(after["velocity"][~changed], before["velocity"][~changed]) and bits(after["position"], before["position"])
    if precision == "fp64":
        assert np.all(np.abs(after["velocity"] - want["v"]) <= value_bound(req, ids, before["velocity"]))


# EXCHANGE with the null-collision form, handed out by the wave-shared loop (P_max above 2^-3) and by the LDS queue (inside
# [2^-8, 2^-3]): 2051 slots are three workgroups' turns, the last group of four partial
EXCHANGE_NULL = {"loop": dict(nu_tau=0.1, sigma_tau=2.0, g_max=0.15, seed=2028, stream=3, epoch=2, **BACKGROUND),
                 "queue": dict(nu_tau=0.01, sigma_tau=0.3, g_max=0.15, seed=2029, stream=4, epoch=2, **BACKGROUND)}


@pytest.mark.parametrize("form", sorted(EXCHANGE_NULL))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_exchange_null_collision_in_both_passes(fp, precision, form):
    n, ids, kw = 2051, np.arange(2051), EXCHANGE_NULL[form]
    req = ref.request(ref.EXCHANGE, **kw)
    lo, hi = compact_range()
    assert (lo <= req["K"] <= hi) == (form == "queue")
    sim = filled(fp, precision, n)
    before = sim.getParticles()
    want = ref.stored(req, ids, before["velocity"])
    cand = want["candidate"]
    x, ux = ref.acceptance(req, ids, want["g"])
    assert not (np.abs(ux - x)[cand] < 1e-9 * req["x_max"]).any() and not (np.abs(want["g"] - req["g_max"])[cand] < 1e-9 * req["g_max"]).any()
    assert cand[:1024].any() and cand[1024:2048].any() and 0 < want["clipped"].sum() < want["collided"].sum() < cand.sum() < n
    got = sim.collide("exchange", **kw)
    after = sim.getParticles()
    sim.destroy()
    assert same_counts(got, want)
    changed = (after["velocity"] != before["velocity"]).any(axis=1)
    assert np.array_equal(changed, want["collided"])
    assert bits(after["velocity"][~changed], before["velocity"][~changed]) and bits(after["position"], before["position"])
    if precision == "fp64":
        assert np.all(np.abs(after["velocity"] - want["v"]) <= value_bound(req, ids, before["velocity"]))


# ---- 4. independence of the slot: no tolerance
@pytest.mark.parametrize("precision", PRECISIONS)
def test_slot_independence(fp, precision):
    n = 4099
    requests = [("exchange", dict(nu_tau=0.4, seed=5, stream=1, epoch=2, **BACKGROUND)),
                ("elastic", dict(nu_tau=0.1, sigma_tau=3.0, g_max=0.2, mass_ratio=1.0, seed=6, stream=2, epoch=2, **BACKGROUND)),
                ("relax", dict(nu_tau=0.3, seed=7, stream=3, epoch=2, **BACKGROUND))]

    def run(sort, epoch):
        sim = filled(fp, precision, n)
        if sort:
            sim.sort()
        counts = [sim.collide(kind, **dict(kw, epoch=epoch)) for kind, kw in requests]
        out = sim.getParticles()
        sim.destroy()
        return counts, out

    plain, a = run(False, 2)
    sorted_, b = run(True, 2)
    assert plain == sorted_ and bits(a["velocity"], b["velocity"]) and bits(a["position"], b["position"])
    again, c = run(True, 2)
    assert again == plain and bits(c["velocity"], a["velocity"])                      # the same epoch on a fresh copy: the same bytes
    other, d = run(True, 3)
    assert other[0]["collided"] != 0 and (d["velocity"] != a["velocity"]).any(axis=1).mean() > 0.9
    pos, vel = scene(n)
    first = ref.candidates(ref.request(ref.EXCHANGE, **requests[0][1]), np.arange(n))
    assert not np.array_equal(first, ref.candidates(ref.request(ref.EXCHANGE, **dict(requests[0][1], epoch=3)), np.arange(n)))
    assert plain[0]["candidates"] == int(first.sum())


# ---- 5. the registered form equals the manual loop
@pytest.mark.parametrize("precision", PRECISIONS)
def test_registered_equals_manual(fp, precision):
    n = 4099
    ops = [(2, "exchange", dict(nu_tau=0.3, seed=15, stream=1, **BACKGROUND)), (3, "relax", dict(nu_tau=0.2, seed=16, stream=2, **BACKGROUND))]
    a, b = filled(fp, precision, n, solver="none"), filled(fp, precision, n, solver="none")
    for s in (a, b):
        s.precalc()
    assert [a.collideEvery(every, kind, **kw) for every, kind, kw in ops] == [0, 1]
    a.recordEnergy(1, 64)
    a.step(6)
    rows, dropped = a.energyHistory()
    assert dropped == 0 and list(rows["substep"]) == list(range(1, 13))
    sums = [dict(applications=0, candidates=0, collided=0, clipped=0) for _ in ops]
    for k in range(1, 13):
        b.substeps(1)
        pre = b.energy()["kinetic"][0]
        for (every, kind, kw), total in zip(ops, sums):
            if k % every == 0:
                for key, v in b.collide(kind, epoch=k, **kw).items():
                    total[key] += v
        post = b.energy()["kinetic"][0]
        # the row recorded after sub-step k holds the kinetic energy after the collisions of that sub-step (the two sums run
        # over the same 4099 values: they differ by less than n 2^-53 of the value if the order of the sum differs at all)
        assert abs(rows["kinetic"][k - 1][0] - post) <= 1e-12 * post, k
        if k % 2 == 0 or k % 3 == 0:
            assert abs(post - pre) > 1e-9 * pre, k                       # (and that is not the energy before them)
    pa, pb = a.getParticles(), b.getParticles()
    assert bits(pa["velocity"], pb["velocity"]) and bits(pa["position"], pb["position"])
    stats = [a.collisionStats(i) for i in range(2)]
    assert stats == sums and [s["applications"] for s in stats] == [6, 4]
    assert stats[0]["collided"] > 0 and stats[1]["collided"] == 4 * n and stats[1]["candidates"] == 0
    assert a.collisionStats(0, "local") == stats[0]
    # cleared: the handle runs on like one that never registered
    a.clearCollisions()
    with pytest.raises(fp.FusionPicError, match=r"\.index <- "):
        a.collisionStats(0)
    a.step(2)
    b.step(2)
    pa, pb = a.getParticles(), b.getParticles()
    assert bits(pa["velocity"], pb["velocity"]) and bits(pa["position"], pb["position"])
    # a new registration starts from zero
    assert a.collideEvery(1, "exchange", nu_tau=math.inf) == 0
    a.substeps(1)
    assert a.collisionStats(0) == dict(applications=1, candidates=n, collided=n, clipped=0)
    a.destroy()
    b.destroy()


# ---- 6. a decomposition holds the same particles
def members(fp, world, precision, capacity, every=2, **kw):
    sims = []
    for r in range(world):
        s = box(fp, precision, capacity, **kw)
        s.domainInit(r, world, ghost_planes=2, migrate_every=every, distributed_solve=0)
        sims.append(s)
    return sims


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_decomposition_holds_the_same_particles(fp, precision):
    n, world = 20011, 2
    population = dict(seed=0xABCDEF, stream=6, drift=(0.0, 0.0, 0.1), vth=0.03)
    background = dict(drift=(0.0, 0.0, 0.1), vth=(0.03, 0.03, 0.03))
    ops = [("exchange", dict(nu_tau=0.2, seed=25, stream=1, **background)), ("relax", dict(nu_tau=0.1, seed=26, stream=2, **background)),
           ("elastic", dict(nu_tau=0.05, mass_ratio=1.0, seed=27, stream=3, **background))]          # (the third in the compacting pass)
    one = box(fp, precision, n, solver="none")
    assert one.load(**population) == n
    g = fp.BoxGroup(members(fp, world, precision, n, solver="none"))
    assert sum(g.load(count=n, **population)) == n
    one.precalc()
    g.precalc()
    for kind, kw in ops:
        assert one.collideEvery(1, kind, **kw) == g.collideEvery(1, kind, **kw)
    one.step(4)
    g.step(4)
    stats = [m.domainStats() for m in g.sims]
    assert sum(s["migrated"] for s in stats) > 0 and sum(s["lost"] for s in stats) == 0
    want = one.getParticles()
    parts = [m.domainGet() for m in g.sims]
    ids = np.concatenate([p["ids"] for p in parts])
    order = np.argsort(ids, kind="stable")
    assert np.array_equal(ids[order], np.arange(n))
    for k in ("position", "velocity"):
        assert bits(np.concatenate([p[k] for p in parts])[order], want[k]), k
    for i in range(len(ops)):
        whole, summed = one.collisionStats(i), g.collisionStats(i)
        assert whole == summed and whole["applications"] == 8, (i, whole, summed)
    assert one.collisionStats(1)["collided"] == 8 * n
    one.destroy()
    for m in g.sims:
        m.destroy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_registered_equals_manual_under_full_em(fp, precision):
    n = 4099
    ops = [(1, "elastic", dict(nu_tau=0.3, mass_ratio=2.0, seed=35, stream=1, **BACKGROUND)), (2, "relax", dict(nu_tau=0.2, seed=36, stream=2, **BACKGROUND))]
    a, b = (filled(fp, precision, n, vth=0.03, dt=em_dt(SHAPE, L), solver="yee") for _ in range(2))
    for s in (a, b):
        s.precalc()
    for every, kind, kw in ops:
        a.collideEvery(every, kind, **kw)
    a.step(2)
    for k in range(1, 5):
        b.substeps(1)
        for every, kind, kw in ops:
            if k % every == 0:
                b.collide(kind, epoch=k, **kw)
    pa, pb = a.getParticles(), b.getParticles()
    assert bits(pa["velocity"], pb["velocity"]) and bits(pa["position"], pb["position"])
    assert a.collisionStats(0)["applications"] == 4 and a.collisionStats(1) == dict(applications=2, candidates=0, collided=2 * n, clipped=0)
    a.destroy()
    b.destroy()


# ---- 7. physics end to end
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_cold_beam_under_charge_exchange(fp, precision):
    n, speed, rounds = BIG, 0.125, 10
    kw = dict(nu_tau=-math.log(0.8), seed=45, stream=1)
    req = ref.request(ref.EXCHANGE, **kw)
    p = req["K"] * 2.0 ** -32
    assert abs(p - 0.2) < 1e-9
    sim = box(fp, precision, n)
    vel = np.zeros((n, 3))
    vel[:, 0] = speed
    sim.set(position=scene(n)[0], velocity=vel)
    hits = [sim.collide("exchange", epoch=k, **kw) for k in range(rounds)]           # the background: cold and at rest
    v = sim.getParticles()["velocity"].astype(np.float64)
    sim.destroy()
    assert np.all((v[:, 0] == speed) | (v[:, 0] == 0)) and not v[:, 1:].any()
    keep = (1 - p) ** rounds
    never = int((v[:, 0] == speed).sum())
    sigma = math.sqrt(keep * (1 - keep) / n)
    assert abs(v[:, 0].mean() / speed - keep) <= 5 * sigma
    assert abs(never / n - keep) <= 5 * sigma
    assert all(h["candidates"] == h["collided"] and h["clipped"] == 0 for h in hits)
    total = sum(h["collided"] for h in hits)
    assert abs(total - rounds * n * p) <= 5 * math.sqrt(rounds * n * p * (1 - p))
    # the never-collided share from the per-application counts: each application spares 1 - collided / n
    # (each factor 1 - c / n has the relative standard deviation sqrt(p / ((1 - p) n)); ten independent factors)
    from_counts = math.prod(1 - h["collided"] / n for h in hits)
    assert abs(from_counts - keep) <= 5 * keep * math.sqrt(rounds * p / ((1 - p) * n))


# ---- 8. refusals; the next valid call succeeds
def test_refusals(fp):
    from helpers import make_spec
    rz = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    for call in (lambda: rz.collide("exchange", nu_tau=1.0), lambda: rz.collideEvery(1, "exchange", nu_tau=1.0), lambda: rz.collisionStats(0), rz.clearCollisions):
        with pytest.raises(fp.FusionPicError, match="needs a CART3D handle") as e:
            call()
        assert e.value.code == -5
    rz.destroy()
    sim = filled(fp, "fp32", 1000)
    nan, inf = float("nan"), float("inf")
    null = dict(sigma_tau=1.0, g_max=0.5)
    cases = [
        ("exchange", dict(species=1), ".species <- no such species"), ("relax", dict(species=-1, nu_tau=1.0), ".species <- no such species"),
        (3, dict(), ".kind <- must be 0 (exchange), 1 (elastic) or 2 (relax)"), (-1, dict(), ".kind <- must be 0"),
        ("exchange", dict(nu_tau=nan), ".nu_tau <- must not be NaN"), ("exchange", dict(sigma_tau=nan), ".sigma_tau <- must not be NaN"),
        ("exchange", dict(g_max=nan), ".g_max <- must not be NaN"), ("elastic", dict(mass_ratio=nan), ".mass_ratio <- must not be NaN"),
        ("exchange", dict(nu_tau=-0.1), ".nu_tau <- must not be negative"), ("exchange", dict(sigma_tau=-1.0, g_max=1.0), ".sigma_tau <- must be finite and not negative"),
        ("elastic", dict(sigma_tau=inf, g_max=1.0), ".sigma_tau <- must be finite and not negative"),
        ("exchange", dict(sigma_tau=1.0), ".g_max <- must be positive and finite when sigma_tau > 0"),
        ("exchange", dict(sigma_tau=1.0, g_max=inf), ".g_max <- must be positive and finite when sigma_tau > 0"),
        ("exchange", dict(sigma_tau=1.0, g_max=-1.0), ".g_max <- must be positive and finite when sigma_tau > 0"),
        ("exchange", dict(nu_tau=inf, **null), ".nu_tau <- +inf needs sigma_tau == 0"), ("exchange", dict(nu_tau=1.0, g_max=0.5), ".g_max <- must be 0 when sigma_tau == 0"),
        ("exchange", dict(nu_tau=1.0, drift=inf), ".drift <- must be finite"), ("exchange", dict(nu_tau=1.0, drift=(0, nan, 0)), ".drift <- must be finite"),
        ("exchange", dict(nu_tau=1.0, vth=-0.1), ".vth <- must be finite and not negative"), ("relax", dict(nu_tau=1.0, vth=(0, 0, inf)), ".vth <- must be finite and not negative"),
        ("exchange", dict(nu_tau=1.0, vth=nan), ".vth <- must be finite and not negative"),
        ("elastic", dict(nu_tau=1.0, mass_ratio=0.0), ".mass_ratio <- must be positive"), ("elastic", dict(nu_tau=1.0, mass_ratio=-2.0), ".mass_ratio <- must be positive"),
        ("exchange", dict(nu_tau=1.0, mass_ratio=1.0), ".mass_ratio <- must be 0 for a kind other than FPIC_COLLIDE_ELASTIC"),
        ("relax", dict(nu_tau=1.0, mass_ratio=inf), ".mass_ratio <- must be 0 for a kind other than FPIC_COLLIDE_ELASTIC"),
        ("relax", dict(nu_tau=1.0, **null), ".sigma_tau <- must be 0 for FPIC_COLLIDE_RELAX"), ("relax", dict(), ".nu_tau <- must be positive and finite for FPIC_COLLIDE_RELAX"),
        ("relax", dict(nu_tau=inf), ".nu_tau <- must be positive and finite for FPIC_COLLIDE_RELAX"),
    ]
    before = sim.getParticles()
    for kind, kw, message in cases:
        for call in (lambda: sim.collide(kind, **kw), lambda: sim.collideEvery(1, kind, **kw)):
            with pytest.raises(fp.FusionPicError) as e:
                call()
            assert message in str(e.value) and e.value.code == -1, (kind, kw, str(e.value))
    lib = sim._lib
    s = fp._collide_spec(5e-12, "exchange", nu_tau=1.0)
    s.reserved[2] = 1.0
    assert lib.fpic_collide(sim._h, s, None) == -1 and b".reserved <- must be zero" in lib.fpic_last_error(sim._h)
    assert lib.fpic_collide(sim._h, None, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_collide_register(sim._h, None, 1, None) == -1 and b".spec <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    assert lib.fpic_collide_stats(sim._h, 0, 0, None) == -1 and b".out <- Non-optional property is undefined!" in lib.fpic_last_error(sim._h)
    for every in (0, -1):
        with pytest.raises(fp.FusionPicError, match=r"\.every <- must be at least 1"):
            sim.collideEvery(every, "exchange", nu_tau=1.0)
    for index in (0, -1):
        with pytest.raises(fp.FusionPicError, match=r"\.index <- no such registered operator"):
            sim.collisionStats(index)
    assert bits(sim.getParticles()["velocity"], before["velocity"])                  # nothing refused has touched a particle
    assert [sim.collideEvery(1 + k, "exchange", nu_tau=0.0) for k in range(fp.COLLIDE_MAX_OPS)] == list(range(fp.COLLIDE_MAX_OPS))
    with pytest.raises(fp.FusionPicError, match=r"\.spec <- FPIC_COLLIDE_MAX_OPS \(8\) operators are registered already"):
        sim.collideEvery(1, "exchange", nu_tau=1.0)
    with pytest.raises(fp.FusionPicError, match=r"\.index <- no such registered operator"):
        sim.collisionStats(fp.COLLIDE_MAX_OPS)
    with pytest.raises(fp.FusionPicError, match=r"\.scope <- "):
        sim._check(lib.fpic_collide_stats(sim._h, 0, 7, fp.CollideResult()))
    # K = 0 registered: the applications are counted, nothing runs
    sim.precalc()
    sim.step(3)
    assert sim.collisionStats(0) == dict(applications=6, candidates=0, collided=0, clipped=0)
    assert sim.collisionStats(5) == dict(applications=1, candidates=0, collided=0, clipped=0)
    sim.clearCollisions()
    assert lib.fpic_collide(sim._h, fp._collide_spec(5e-12, "exchange", nu_tau=1.0), None) == 0     # `out` is optional
    assert sim.collide("relax", nu_tau=1.0, vth=0.01)["collided"] == 1000
    sim.destroy()


# ---- 9. the JavaScript host
def test_collide_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    n = 4000
    spec = box_spec(SHAPE, L, n, 5e-12, solver="none", macro_weight=1e15 * np.prod(L) / n)
    population = dict(seed=123456789, stream=3, drift=[0.0, 0.01, 0.0], vth=0.02)
    now = dict(kind="elastic", nuTau=0.2, sigmaTau=3.0, gMax=0.1, drift=[0.01, 0.0, -0.02], vth=[0.05, 0.02, 0.1], massRatio=2.0, seed=99, stream=4, epoch=7)
    every = dict(kind="relax", nu=2e10, vth=0.03, seed=5)
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, population=population, now=now, every=every)))
    script = r"""
const fs = require('fs');
const crypto = require('crypto');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.load(inp.population);
sim.precalc();
const first = sim.collide(inp.now);
const index = sim.collideEvery(2, inp.every);
sim.step(2);
const stats = sim.collisionStats(index);
const local = sim.collisionStats(index, 'local');
const r = sim.select({});
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const errors = [];
const tries = [() => sim.collide({kind: 'coulomb'}), () => sim.collide({kind: 'relax'}), () => sim.collide({kind: 'exchange', nu: 1, nuTau: 1}), () => sim.collide(7),
  () => sim.collide({kind: 'exchange', vth: [1, 2]}), () => sim.collide({kind: 'exchange', nuTau: 1, species: 3}), () => sim.collide({kind: 'exchange', seed: -1}),
  () => sim.collideEvery(0, {kind: 'exchange', nuTau: 1}), () => sim.collideEvery(1.5, {kind: 'exchange', nuTau: 1}), () => sim.collisionStats(4), () => sim.collide({})];
for (const t of tries) { try { t(); errors.push(null); } catch (err) { errors.push(String(err.message)); } }
sim.clearCollisions();
let cleared = null;
try { sim.collisionStats(0); } catch (err) { cleared = String(err.message); }
console.log(JSON.stringify({first: first, index: index, stats: stats, local: local, ids: sha(r.ids), position: sha(r.position), velocity: sha(r.velocity), errors: errors, cleared: cleared}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    sim = fp.makeCylindricalParticlePusher(spec)
    sim.load(**population)
    sim.precalc()
    first = sim.collide("elastic", nu_tau=0.2, sigma_tau=3.0, g_max=0.1, drift=now["drift"], vth=now["vth"], mass_ratio=2.0, seed=99, stream=4, epoch=7)
    index = sim.collideEvery(2, "relax", nu=2e10, vth=0.03, seed=5)
    sim.step(2)
    stats = sim.collisionStats(index)
    want = sim.select()
    sim.destroy()
    sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()
    assert out["first"] == first and first["collided"] > 0 and first["clipped"] > 0
    assert out["index"] == index == 0 and out["stats"] == stats == out["local"] and stats == dict(applications=2, candidates=0, collided=2 * n, clipped=0)
    assert (out["ids"], out["position"], out["velocity"]) == (sha(want["ids"]), sha(want["position"]), sha(want["velocity"]))
    assert all(err is not None and " <- " in err for err in out["errors"]), out["errors"]
    assert out["cleared"] is not None and ".index <- " in out["cleared"]
