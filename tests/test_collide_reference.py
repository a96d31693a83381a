"""The numpy restatement of the collision rule (tests/collide_reference.py) proved on the CPU: its words against the loader
reference's generator at the new tag, the candidate and acceptance fractions, the scattering direction, the conserved speed
on a fixed target, and the relaxation's stationary Maxwellian — each over 2 10^5 ids with fixed seeds and within 5 standard
errors computed from N.  The kernel is compared with this reference in tests/test_gpu_collide.py.

Deviation of the reference's rounded parts from 50-digit values (mpmath; numpy.longdouble where mpmath is missing) over
ULP_PARTICLES ids, in float64 ulps of the value (measured here, asserted below REF_ULPS): normals 2.69, cospi / sinpi 1.68."""
import math

import numpy as np
import pytest

import collide_reference as ref
import load_reference as lref

N = 200000
IDS = np.arange(N, dtype=np.uint64)
ULP_PARTICLES = 20000
# The reference's own deviation stays below this (tests/test_gpu_collide.py adds it to the kernel's bound), as
# test_load_reference.REF_ULPS: libm's log, sin and cos within 1 ulp, sqrt within 1/2, the product pi r and the constant pi
# within 1 more, the final product within 1/2
REF_ULPS = 4.0


def test_words_are_the_loaders_generator_at_the_new_tag():
    req = ref.request(ref.EXCHANGE, nu_tau=1.0, seed=0x0123456789ABCDEF, stream=5, epoch=77)
    ids = np.array([0, 1, 2, 0xFFFFFFFF, 123456789], dtype=np.uint64)
    for b in (0, 1):
        mine = ref.words(req, ids, b)
        theirs = lref.philox(ids, 77, 5, 0xC0110 + b, 0x89ABCDEF, 0x01234567)
        assert all(np.array_equal(m, t) for m, t in zip(mine, theirs))
    # the constants tests/native/collide_core_test.cpp holds the library's words to
    w = np.stack(ref.words(req, np.array([0, 1, 0xFFFFFFFF]), 0), axis=1)
    assert ["%08x" % int(x) for x in w.ravel()] == WORDS_OF_THREE_IDS
    # another epoch, stream or block: other words
    assert not np.array_equal(ref.words(req, ids, 0)[0], ref.words(dict(req, epoch=78), ids, 0)[0])
    assert not np.array_equal(ref.words(req, ids, 0)[0], ref.words(dict(req, stream=6), ids, 0)[0])
    assert not np.array_equal(ref.words(req, ids, 0)[0], ref.words(req, ids, 1)[0])


WORDS_OF_THREE_IDS = "373469d3 feeda24b 6bb82344 614548a1 e8427845 0b69b034 0cc70f85 709c2f32 12b30ae2 d221c64b b8af0f74 80a771b8".split()


def test_host_side_numbers():
    r = ref.request(ref.EXCHANGE, nu_tau=0.0)
    assert r["K"] == 0 and r["p_max"] == 0
    assert ref.request(ref.EXCHANGE, nu_tau=math.inf)["K"] == 1 << 32
    assert ref.request(ref.EXCHANGE, nu_tau=50.0)["K"] == 1 << 32           # P_max rounds to 1
    assert ref.request(ref.EXCHANGE, nu_tau=math.log(2.0))["K"] in (1 << 31, (1 << 31) - 1)
    r = ref.request(ref.ELASTIC, nu_tau=0.25, sigma_tau=2.0, g_max=0.5, mass_ratio=3.0)
    assert r["x_max"] == 1.25 and r["M"] == 0.75 and r["K"] == int(math.ldexp(-math.expm1(-1.25), 32))
    assert ref.request(ref.ELASTIC)["M"] == 1.0
    r = ref.request(ref.RELAX, nu_tau=0.5, vth=(1.0, 2.0, 0.0))
    assert r["decay"] == math.exp(-0.5) and list(r["sv"]) == [math.sqrt(-math.expm1(-1.0)), math.sqrt(-math.expm1(-1.0)) * 2.0, 0.0]


@pytest.mark.parametrize("nu_tau", [1e-3, 0.05, -math.log(0.7), 3.0])
def test_candidate_fraction(nu_tau):
    req = ref.request(ref.EXCHANGE, nu_tau=nu_tau, seed=101, stream=1, epoch=3)
    p = req["K"] * 2.0 ** -32
    got = ref.candidates(req, IDS).mean()
    assert abs(got - p) <= 5 * math.sqrt(p * (1 - p) / N)
    assert abs(p - (1 - math.exp(-nu_tau))) < 2.0 ** -31


def test_null_collision_acceptance_of_a_cold_beam_through_a_cold_background():
    speed = 0.03125                                           # g = 2^-5 exactly
    req = ref.request(ref.EXCHANGE, nu_tau=0.1, sigma_tau=20.0, g_max=0.0625, seed=102, stream=2, epoch=9)
    v = np.zeros((N, 3))
    v[:, 0] = speed
    out = ref.apply(req, IDS, v)
    assert np.all(out["g"] == speed) and not out["clipped"].any()
    nc = int(out["candidate"].sum())
    p = (0.1 + 20.0 * speed) / req["x_max"]
    assert abs(out["collided"].sum() / nc - p) <= 5 * math.sqrt(p * (1 - p) / nc)
    assert not (out["collided"] & ~out["candidate"]).any()
    # everybody who collided took the partner's velocity (the cold background: its drift), the others kept theirs
    assert np.all(out["v"][out["collided"]] == 0) and np.array_equal(out["v"][~out["collided"]], v[~out["collided"]])
    # a faster beam than the bound: every candidate is clipped, and accepted with certainty short of u x_max < x_max rounding
    v[:, 0] = 0.125
    out = ref.apply(req, IDS, v)
    assert np.array_equal(out["clipped"], out["candidate"]) and np.array_equal(out["collided"], out["candidate"])


def test_direction_is_a_unit_vector_uniform_on_the_sphere():
    req = ref.request(ref.ELASTIC, nu_tau=1.0, seed=103, stream=3, epoch=1)
    nh = ref.direction(req, IDS)
    norm2 = (nh[:, 0] * nh[:, 0] + nh[:, 1] * nh[:, 1]) + nh[:, 2] * nh[:, 2]
    assert np.abs(norm2 - 1.0).max() <= 4 * np.spacing(1.0)
    for a in range(3):
        assert abs(nh[:, a].mean()) <= 5 * math.sqrt(1.0 / 3.0 / N)
        assert abs((nh[:, a] ** 2).mean() - 1.0 / 3.0) <= 5 * math.sqrt(4.0 / 45.0 / N)       # var of n_a^2 = 1/5 - 1/9
    assert np.abs(nh[:, 2]).max() < 1.0


def test_elastic_on_a_cold_fixed_target_keeps_the_speed():
    drift = np.array([0.01, -0.02, 0.005])
    req = ref.request(ref.ELASTIC, nu_tau=math.inf, drift=drift, vth=0.0, seed=104, stream=4)
    rng = np.random.default_rng(104)
    v = rng.normal(0.0, 0.05, size=(N, 3))
    out = ref.apply(req, IDS, v)
    assert out["collided"].all() and req["M"] == 1.0
    w = out["v"] - drift
    after = np.sqrt((w[:, 0] ** 2 + w[:, 1] ** 2) + w[:, 2] ** 2)
    # every component of v' - drift carries at most three roundings of the rule (t, r, v') and the subtraction here, each
    # half an ulp of the larger of |v|, |drift| and g; the direction's norm is 1 to 4 ulps of its square
    scale = np.maximum(np.maximum(np.abs(v).max(axis=1), np.abs(drift).max()), out["g"])
    worst = (np.abs(after - out["g"]) / np.spacing(scale)).max()
    print("speed after / before a fixed cold target: largest deviation %.2f ulps" % worst)
    assert worst <= 8
    assert (np.abs(out["v"] - v).max(axis=1) > 0).mean() > 0.999


def test_relax_far_beyond_the_relaxation_time_draws_the_background():
    drift, vth = np.array([0.01, -0.02, 0.0]), np.array([0.05, 0.02, 0.1])
    req = ref.request(ref.RELAX, nu_tau=40.0, drift=drift, vth=vth, seed=105, stream=5, epoch=2)
    v = np.full((N, 3), 0.3)
    out = ref.apply(req, IDS, v)
    assert out["collided"].all() and not out["candidate"].any()
    for a in range(3):
        assert abs(out["v"][:, a].mean() - drift[a]) <= 5 * vth[a] / math.sqrt(N)
        assert abs(out["v"][:, a].var() - vth[a] ** 2) <= 5 * vth[a] ** 2 * math.sqrt(2.0 / N)


def test_relax_leaves_the_backgrounds_maxwellian_stationary():
    drift, vth = np.array([0.01, -0.02, 0.0]), np.array([0.05, 0.02, 0.1])
    v = lref.velocities(lref.request((1.0, 1.0, 1.0), seed=7, stream=9, drift=drift, vth=vth), IDS)
    req = ref.request(ref.RELAX, nu_tau=0.5, drift=drift, vth=vth, seed=106, stream=6, epoch=4)
    for k in range(3):
        v = ref.apply(dict(req, epoch=req["epoch"] + k), IDS, v)["v"]
        for a in range(3):
            z = (v[:, a] - drift[a]) / vth[a]
            assert abs(z.mean()) <= 5 / math.sqrt(N)
            assert abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / N)
            assert abs((z ** 4).mean() - 3.0) <= 5 * math.sqrt(96.0 / N)          # var of z^4 = 105 - 9
    # and it does move every particle: decay = exp(-1/2) of the old deviation is kept
    first = lref.velocities(lref.request((1.0, 1.0, 1.0), seed=7, stream=9, drift=drift, vth=vth), IDS)
    once = ref.apply(req, IDS, first)["v"]
    c = np.corrcoef(((first - drift) / vth)[:, 0], ((once - drift) / vth)[:, 0])[0, 1]
    assert abs(c - math.exp(-0.5)) <= 5 * (1 - math.exp(-1.0)) / math.sqrt(N)


def _exact_parts(req, ids):
    """50-digit (or long double) values of the three normals and of cospi(2 phi), sinpi(2 phi): (hi, lo) float64 [n][5]"""
    w1 = [x.astype(np.uint64) for x in ref.words(req, ids, 1)]
    w0 = [x.astype(np.uint64) for x in ref.words(req, ids, 0)]
    hi, lo = np.empty((len(ids), 5)), np.empty((len(ids), 5))
    try:
        import mpmath
    except ImportError:
        mpmath = None
    if mpmath is None:
        ld = np.longdouble
        two32, pi = ld(2) ** 32, ld(np.pi) + ld(1.2246467991473532e-16)
        f = lambda w: w.astype(ld)
        r1, r3 = np.sqrt(-2 * np.log((f(w1[0]) + ld(0.5)) / two32)), np.sqrt(-2 * np.log((f(w1[2]) + ld(0.5)) / two32))
        a2, a4, p2 = 2 * pi * f(w1[1]) / two32, 2 * pi * f(w1[3]) / two32, 2 * pi * f(w0[3]) / two32
        vals = np.stack([r1 * np.cos(a2), r1 * np.sin(a2), r3 * np.cos(a4), np.cos(p2), np.sin(p2)], axis=1)
        hi[:] = vals.astype(np.float64)
        lo[:] = (vals - hi.astype(ld)).astype(np.float64)
        return hi, lo
    with mpmath.workdps(50):
        two32 = mpmath.mpf(2) ** 32
        for k in range(len(ids)):
            r1 = mpmath.sqrt(-2 * mpmath.log((mpmath.mpf(int(w1[0][k])) + 0.5) / two32))
            r3 = mpmath.sqrt(-2 * mpmath.log((mpmath.mpf(int(w1[2][k])) + 0.5) / two32))
            u2, u4, phi = mpmath.mpf(int(w1[1][k])) / two32, mpmath.mpf(int(w1[3][k])) / two32, mpmath.mpf(int(w0[3][k])) / two32
            vals = (r1 * mpmath.cospi(2 * u2), r1 * mpmath.sinpi(2 * u2), r3 * mpmath.cospi(2 * u4), mpmath.cospi(2 * phi), mpmath.sinpi(2 * phi))
            for c, x in enumerate(vals):
                hi[k, c] = float(x)
                lo[k, c] = float(x - mpmath.mpf(hi[k, c]))
    return hi, lo


def test_rounded_parts_against_fifty_digits():
    req = ref.request(ref.ELASTIC, nu_tau=1.0, seed=0x0123456789ABCDEF, stream=7, epoch=11)
    ids = np.arange(ULP_PARTICLES, dtype=np.uint64)
    hi, lo = _exact_parts(req, ids)
    phi2 = 2.0 * (ref.words(req, ids, 0)[3].astype(np.float64) * 2.0 ** -32)
    got = np.concatenate([ref.normals(req, ids), lref.cospi(phi2)[:, None], lref.sinpi(phi2)[:, None]], axis=1)
    d = np.abs((got - hi) - lo) / np.spacing(np.maximum(np.abs(hi), np.finfo(np.float64).tiny))
    exact_zero = hi == 0                                       # cospi / sinpi at a multiple of a quarter turn: exact
    assert np.all(got[exact_zero] == 0)
    d[exact_zero] = 0
    print("reference against 50 digits, largest deviation in ulps: normals %.3f %.3f %.3f, cospi %.3f, sinpi %.3f" % tuple(d.max(axis=0)))
    assert d.max() < REF_ULPS
