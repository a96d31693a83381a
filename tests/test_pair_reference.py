"""The numpy restatement of the binary collision rule (tests/pair_reference.py) proved on the CPU: the pairing tables by hand,
the conservation laws of one pair, the deflection, the two degenerate branches, its rounded functions against 50-digit
values, the isotropisation rate of a bi-Maxwellian against the closed form, and — for tests/test_gpu_pair.py — how far the
reference moves on the GPU test's own scenes when its rounded functions are replaced by correctly rounded ones.

Measured here (printed by the tests, asserted against the constants below):
  rounded functions against 50 digits, float64 ulps of the value (with the half ulp of the rounded 50-digit value): first
      normal 3.5, cospi 2.5, sinpi 2.5 (REF_ULPS = 4).
  isotropisation (test_isotropisation_rate...): measured / closed-form rate 1.035, standard error over 8 seeds 0.039, the same
      with tau / 2: 0.991; tolerance = 3 standard errors + |difference of the two| (not fixed in advance, see the test).
  the double reference against its 50-digit twin on the scenes of tests/pair_scene.py, as a share of the bound
      `value_bound(out, REF_ULPS)`: single-stage particles 0.352, chains and triples 0.038 -> AMPLIFICATION = 4 x 0.038 = 0.16;
      fp32: none of the 3978 stored particles differs (the condition of the GPU test is a share below 1e-3)."""
import math

import mpmath
import numpy as np
import pytest

import load_reference as lref
import pair_reference as ref
import pair_scene as scene

EPS = 2.0 ** -53
ULP = 2.0 ** -52                 # the largest relative size of one ulp of a double; half an ulp on either side of a comparison is one
# The reference's own rounded functions stay below this many ulps of 50-digit values (asserted below): libm's log and cos or
# sin within 1 ulp, sqrt within 1/2, the product pi r and the constant pi within 1 more, the final product within 1/2 —
# as test_collide_reference.REF_ULPS
REF_ULPS = 4.0
# chains and triples: the deviation of a particle that took part in several pairs, as a multiple of the sum of its pairs'
# single-stage bounds: 4 x the largest share measured below on the scenes (0.038), rounded up
AMPLIFICATION = 0.16
FP32_SHARE = 1e-3


def value_bound(out, ulps, side="a", amplification=1.0):
    """The bound of |v - reference| per particle and component when every rounded function of the rule (the first normal,
    cospi, sinpi) may be off by `ulps` ulps.  One ulp is at most ULP = 2^-52 of the value, and an operation rounded on either
    side of the comparison (half an ulp each) adds at most one ULP.  delta carries the normal's error and two roundings:
    e = (ulps + 2) ULP relative; sinT has at most that relative error and omc twice it (d ln sinT / d ln delta = (1 - d2) /
    (1 + d2), d ln omc / d ln delta = 2 / (1 + d2)); cs and sn add `ulps` ULP; the at most eight operations behind a term of du
    (d2, 1 + d2, the division, and the products) one ULP each: a term is off by (2 (ulps + 2) + ulps + 8) ULP of its
    magnitude.  The products f du and the sums v + f du add ULP (|f du| + |v'|) per pair.  scale = the sum over the particle's
    pairs of f times the magnitudes of du's terms."""
    s, stages, v = out["scale_" + side], out["stages_" + side], np.abs(out["v" + side].astype(np.float64))
    own = (3 * ulps + 12) * ULP * s + 2 * ULP * stages[:, None] * (v.max(axis=1)[:, None] + s)
    return np.where(stages[:, None] > 1, amplification, 1.0) * own


# ---- the pairing tables, by hand
def test_unlike_pairing_tables():
    want = {
        (1, 1): [(0, 0)],
        (2, 1): [(0, 0), (1, 0)],
        (5, 1): [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)],
        (5, 2): [(0, 0), (1, 1), (2, 0), (3, 1), (4, 0)],
        (7, 3): [(0, 0), (1, 1), (2, 2), (3, 0), (4, 1), (5, 2), (6, 0)],
        (4, 4): [(0, 0), (1, 1), (2, 2), (3, 3)],
    }
    for (nm, nf), pairs in want.items():
        assert ref.pairing_unlike(nm, nf) == [(j, q, float(nf)) for j, q in pairs], (nm, nf)
    assert ref.pairing_unlike(3, 0) == []
    # (Na, Nb) = (3, 4): species b is the many one; a tie goes to species a
    req = ref.request(10.0, 1e-9, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, seed=5)
    for na, nb, a_many in ((3, 4, False), (4, 4, True), (5, 2, True)):
        ids_a, ids_b = np.arange(na), 100 + np.arange(nb)
        plan = ref.schedule(req, np.zeros(na), ids_a, np.zeros(nb), ids_b)
        ids = np.concatenate([ids_a, ids_b])
        sorted_of = lambda x: [int(i) for i in sorted(x, key=lambda i: (int(ref.keys(req, [i])[0]), int(i)))]
        sa, sb = sorted_of(ids_a), sorted_of(ids_b)
        many, few = (sa, sb) if a_many else (sb, sa)
        got = [(int(ids[o]), int(ids[p]), nl, int(t)) for o, p, nl, t in zip(plan["owner"], plan["partner"], plan["n_l"], plan["stage"])]
        assert got == [(many[j], few[j % len(few)], float(len(few)), j // len(few)) for j in range(len(many))]
        assert plan["cells"] == 1


def test_like_pairing_tables():
    want = {
        0: [], 1: [],
        2: [(0, 1, 2.0)],
        3: [(0, 1, 1.5), (1, 2, 1.5), (2, 0, 1.5)],
        4: [(0, 1, 4.0), (2, 3, 4.0)],
        5: [(0, 1, 2.5), (1, 2, 2.5), (2, 0, 2.5), (3, 4, 5.0)],
        6: [(0, 1, 6.0), (2, 3, 6.0), (4, 5, 6.0)],
        7: [(0, 1, 3.5), (1, 2, 3.5), (2, 0, 3.5), (3, 4, 7.0), (5, 6, 7.0)],
    }
    for n, pairs in want.items():
        assert ref.pairing_like(n) == pairs, n
    # the order inside a cell is (key, id), whatever order the particles are handed in
    req = ref.request(10.0, 1e-9, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, seed=9, like=True)
    ids = np.array([40, 7, 19, 3, 88])
    s = sorted(ids, key=lambda i: (int(ref.keys(req, [i])[0]), int(i)))
    plan = ref.schedule(req, np.zeros(5), ids)
    assert [(int(ids[o]), int(ids[p])) for o, p in zip(plan["owner"], plan["partner"])] == [(s[0], s[1]), (s[1], s[2]), (s[2], s[0]), (s[3], s[4])]
    assert list(plan["stage"]) == [0, 1, 2, 0] and list(plan["n_l"]) == [2.5, 2.5, 2.5, 5.0]
    assert len(set(int(k) for k in ref.keys(req, ids))) == 5 and s != sorted(ids)


def test_words_are_the_loaders_generator_at_the_new_tag():
    req = ref.request(10.0, 1e-9, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, seed=0x0123456789ABCDEF, stream=5, epoch=77)
    ids = np.array([0, 1, 0xFFFFFFFF], dtype=np.uint64)
    for b in (0, 1):
        assert all(np.array_equal(m, t) for m, t in zip(ref.words(req, ids, b), lref.philox(ids, 77, 5, 0xC0120 + b, 0x89ABCDEF, 0x01234567)))
    assert ["%08x" % int(x) for x in np.stack(ref.words(req, ids, 0), axis=1).ravel()] == WORDS_OF_THREE_IDS


# the constants tests/native/pair_core_test.cpp holds the library's words to
WORDS_OF_THREE_IDS = "db3527ce eab17efb 45a4aec9 3dc11ec5 af769be6 05f58b6a f8cee517 ec47426d a05ed635 cfa18e33 4e01cffc 096542b2".split()


# ---- one pair
N = 20000


def _pairs(seed, ma=scene.ME, mb=scene.MP, like=False):
    rng = np.random.default_rng(seed)
    req = ref.request(10.0, 1e-9, ma, scene.QE, mb, -scene.QE, scene.weight(1, 0.01, var=0.3, ma=ma, mb=mb, qb=-scene.QE), 1.0, seed=seed, stream=2, epoch=4, like=like)
    vo, vp = rng.normal(0, 0.01, (N, 3)), rng.normal(0, 0.01 if like else 0.001, (N, 3))
    return req, np.arange(N), vo, vp


@pytest.mark.parametrize("like", [False, True])
def test_a_pair_conserves_momentum_and_energy(like):
    ld = np.longdouble
    ma, mb = scene.ME, scene.ME if like else scene.MP
    req, ids, vo, vp = _pairs(21, ma, mb, like)
    new_o, new_p, counted, strong, var, mag = ref.collide(req, ids, np.ones(N), np.full(N, req["fa"]), np.full(N, req["fb"]), vo, vp)
    assert counted.all() and 0 < strong.sum() < N
    # momentum per component: m_o f_o = m_ab = m_p f_p up to the four roundings of a mass factor (2 EPS relative); the product
    # f du and the sum v + f du are one rounding each: |error| <= m (2.5 EPS |f du| + 0.5 EPS |v'|) per member
    mo, mp = ld(ma), ld(mb)
    p0 = mo * vo.astype(ld) + mp * vp.astype(ld)
    p1 = mo * new_o.astype(ld) + mp * new_p.astype(ld)
    bound = 3 * EPS * (ma * (req["fa"] * mag + np.abs(new_o)) + mb * (req["fb"] * mag + np.abs(new_p)))
    worst = float((np.abs(p1 - p0) / bound).max())
    print("momentum of a pair: largest error / bound %.3f" % worst)
    assert worst <= 1
    # kinetic energy: |u'| = |u| holds to the roundings of du (six operations and two rounded functions of 4 ulps per term: within
    # 16 EPS of a term's magnitude), so the energy of the relative motion m_ab |u|^2 / 2 moves by at most 2 x 16 EPS of m_ab |u| mag;
    # the centre-of-mass part moves with the momentum error above
    ke = lambda m, v: (ld(0.5) * m * (v.astype(ld) ** 2).sum(axis=1))
    e0, e1 = ke(mo, vo) + ke(mp, vp), ke(mo, new_o) + ke(mp, new_p)
    u = np.abs(vo - vp).max(axis=1)
    vmax = np.maximum(np.abs(new_o).max(axis=1), np.abs(new_p).max(axis=1))
    ebound = 32 * EPS * req["mab"] * u * mag.sum(axis=1) + 3 * vmax * bound.sum(axis=1)
    worst = float((np.abs(e1 - e0) / ebound).max())
    print("kinetic energy of a pair: largest error / bound %.3f" % worst)
    assert worst <= 1


def test_the_deflection_keeps_the_relative_speed_and_turns_by_theta():
    ld = np.longdouble
    req, ids, vo, vp = _pairs(22)
    new_o, new_p, counted, strong, var, mag = ref.collide(req, ids, np.ones(N), np.full(N, req["fa"]), np.full(N, req["fb"]), vo, vp)
    u0, u1 = (vo - vp).astype(ld), (new_o - new_p).astype(ld)
    g0, g1 = np.sqrt((u0 ** 2).sum(axis=1)), np.sqrt((u1 ** 2).sum(axis=1))
    # u' = u + (f_o + f_p) du with f_o + f_p = 1 up to 4 EPS; a term of du within 16 EPS of its magnitude (as above), the sums
    # v + f du within EPS |v|: |g' - g| <= 24 EPS (sum of the magnitudes + |v_o| + |v_p|)
    slack = 24 * EPS * (mag.sum(axis=1) + np.abs(vo).sum(axis=1) + np.abs(vp).sum(axis=1))
    assert np.all(np.abs(g1 - g0) <= slack)
    # 1 - cos of the angle between u and u' is omc = 2 d2 / (1 + d2), recomputed here in long double from the same words
    n0, cs, sn = ref.parts_of(req, ids)
    delta = np.sqrt(var.astype(ld)) * n0.astype(ld)
    omc = 2 * delta ** 2 / (1 + delta ** 2)
    one_minus_cos = 1 - (u0 * u1).sum(axis=1) / (g0 * g1)
    assert np.all(np.abs(one_minus_cos - omc) <= 64 * EPS + slack / g0)
    assert omc.max() > 1.0 and omc.min() < 1e-3                     # small and large angles both occur


def test_the_axial_and_the_resting_branch():
    req, ids, vo, vp = _pairs(23)
    vo, vp = vo[:64].copy(), vp[:64].copy()
    vp[:32, :2] = vo[:32, :2]                                       # up == 0: the relative velocity lies along z
    vp[32:] = vo[32:]                                               # g == 0
    f = np.full(64, 0.5)
    new_o, new_p, counted, strong, var, mag = ref.collide(req, ids[:64], np.ones(64), f, f, vo, vp)
    assert counted[:32].all() and not counted[32:].any() and not strong[32:].any()
    assert np.array_equal(new_o[32:], vo[32:]) and np.array_equal(new_p[32:], vp[32:])
    n0, cs, sn = ref.parts_of(req, ids[:32])
    g = np.abs(vo[:32, 2] - vp[:32, 2])
    delta = np.sqrt(req["kappa"] / ((g * g) * g)) * n0
    sinT, omc = (2.0 * delta) / (1.0 + delta * delta), (2.0 * (delta * delta)) / (1.0 + delta * delta)
    du = np.stack([(g * sinT) * cs, (g * sinT) * sn, -(g * omc)], axis=1)
    assert np.array_equal(new_o[:32], vo[:32] + 0.5 * du) and np.array_equal(new_p[:32], vp[:32] - 0.5 * du)
    assert np.isfinite(new_o).all() and np.isfinite(new_p).all()
    # and in a cell: a resting pair is not counted and keeps its bits, its cell is still a cell with a pair
    like = ref.request(10.0, 1e-9, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, like=True)
    v = np.array([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3]], dtype=np.float32)
    out = ref.apply(like, [0, 0], [0, 1], v)
    assert out["pairs"] == 0 and out["cells"] == 1 and out["va"].tobytes() == v.tobytes()


# ---- the rounded functions against 50 digits
def exact_parts(req, owners):
    """the three rounded functions of a pair from 50-digit values, correctly rounded to float64 (the twin's `parts`)"""
    w0, w1 = ref.words(req, owners, 0), ref.words(req, owners, 1)
    out = np.empty((3, len(np.atleast_1d(owners))))
    with mpmath.workdps(50):
        two32 = mpmath.mpf(2) ** 32
        for k in range(out.shape[1]):
            r1 = mpmath.sqrt(-2 * mpmath.log((mpmath.mpf(int(w1[0][k])) + 0.5) / two32))
            phi = mpmath.mpf(int(w0[1][k])) / two32
            out[0, k] = float(r1 * mpmath.cospi(2 * mpmath.mpf(int(w1[1][k])) / two32))
            out[1, k] = float(mpmath.cospi(2 * phi))
            out[2, k] = float(mpmath.sinpi(2 * phi))
    return out[0], out[1], out[2]


def test_rounded_parts_against_fifty_digits():
    req = ref.request(10.0, 1e-9, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, seed=0x0123456789ABCDEF, stream=7, epoch=11)
    ids = np.arange(20000, dtype=np.uint64)
    got, want = np.stack(ref.parts_of(req, ids)), np.stack(exact_parts(req, ids))
    d = np.abs(got - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny)) + 0.5      # (`want` is itself rounded: half an ulp)
    d[want == 0] = 0
    assert np.all(got[want == 0] == 0)
    print("reference against 50 digits, largest deviation in ulps: first normal %.3f, cospi %.3f, sinpi %.3f" % tuple(d.max(axis=1)))
    assert d.max() < REF_ULPS


# ---- the reference against its 50-digit twin on the scenes of the GPU test
def scene_runs(dtype, parts=None):
    """(like, unlike) outputs of the reference on the two scenes of tests/pair_scene.py, velocities stored as dtype"""
    s = scene.like_scene()
    req = ref.request(scene.LOG_LAMBDA, scene.TAU, scene.ME, scene.QE, scene.ME, scene.QE, s["W"], scene.DV, seed=31, stream=1, epoch=2, like=True)
    like = ref.apply(req, scene.cell_index(s["pos"]), np.arange(len(s["pos"])), s["vel"].astype(dtype), parts=parts)
    s = scene.unlike_scene()
    req = ref.request(scene.LOG_LAMBDA, scene.TAU, scene.ME, scene.QE, scene.MP, -scene.QE, s["W"], scene.DV, seed=32, stream=1, epoch=2)
    unlike = ref.apply(req, scene.cell_index(s["pos_a"]), np.arange(len(s["pos_a"])), s["vel_a"].astype(dtype),
                       scene.cell_index(s["pos_b"]), np.arange(len(s["pos_b"])), s["vel_b"].astype(dtype), parts=parts)
    return like, unlike


def test_the_reference_against_its_fifty_digit_twin_on_the_gpu_scenes():
    single = chained = 0.0
    for dtype in (np.float64, np.float32):
        differing = total = 0
        for mine, twin in zip(scene_runs(dtype), scene_runs(dtype, exact_parts)):
            assert (mine["pairs"], mine["strong"], mine["cells"]) == (twin["pairs"], twin["strong"], twin["cells"])
            for side in ("a", "b"):
                if mine["v" + side] is None:
                    continue
                if dtype is np.float32:
                    differing += int((mine["v" + side] != twin["v" + side]).any(axis=1).sum())
                    total += len(mine["v" + side])
                    continue
                share = np.abs(mine["v" + side] - twin["v" + side]) / np.maximum(value_bound(mine, REF_ULPS, side), np.finfo(np.float64).tiny)
                stages = mine["stages_" + side]
                single = max(single, float(share[stages == 1].max()))
                if (stages > 1).any():
                    chained = max(chained, float(share[stages > 1].max()))
        if dtype is np.float32:
            print("fp32: %d of %d stored particles differ from the 50-digit twin" % (differing, total))
            assert differing <= FP32_SHARE * total
    print("double reference against its 50-digit twin, share of value_bound(REF_ULPS): single-stage %.3f, chains and triples %.3f" % (single, chained))
    assert single <= 1                                              # the single-stage bound holds for the reference itself
    assert 4 * chained <= AMPLIFICATION


# ---- physics: the isotropisation of a bi-Maxwellian
def _nu_t(n, t_par, t_perp, m, q, log_lambda):
    """NRL Plasma Formulary (2019) p. 33, in SI: dT_perp/dt = -(1/2) dT_par/dt = -nu_T (T_perp - T_par),
    nu_T = 2 sqrt(pi) q^4 n lambda / ((4 pi eps0)^2 m^(1/2) (k T_par)^(3/2)) A^-2 [-3 + (A + 3) atan(sqrt A) / sqrt A],
    A = T_perp / T_par - 1 > 0; temperatures as (v_th / c)^2"""
    a = t_perp / t_par - 1.0
    kt = m * ref.C ** 2 * t_par
    pre = 2.0 * math.sqrt(math.pi) * q ** 4 * n * log_lambda / ((4.0 * math.pi * ref.EPS0) ** 2 * math.sqrt(m) * kt ** 1.5)
    return pre * (-3.0 + (a + 3.0) * math.atan(math.sqrt(a)) / math.sqrt(a)) / a ** 2


def test_isotropisation_rate_of_a_bi_maxwellian():
    """One species in 8 cells of 2000 particles with T_perp = 2 T_par, var = 0.05 at the thermal speed (0.2 % of the pairs are
    `strong`), 16 applications.  T_perp - T_par decays at 3 nu_T (the formulary's two equations added); the measured rate
    -ln(dT_16 / dT_0) / (16 tau) is divided by 3 nu_T evaluated at the measured temperatures (the mean of start and end).
    The tolerance is not fixed in advance: three standard errors of that ratio over 8 seeds, plus the time-step bias
    estimated as the difference to the same run with tau / 2 and 32 applications.  Measured: 1.035 with standard error 0.039;
    tau / 2: 0.991; so the tolerance is 0.16."""
    n_cell, cells, v_par, log_lambda, dv = 2000, 8, 0.01, 10.0, 1e-9
    v_perp = v_par * math.sqrt(2.0)
    k1 = ref.request(log_lambda, 1.0, scene.ME, scene.QE, scene.ME, scene.QE, 1.0, dv, like=True)["kappa"]
    tau = 0.05 * v_par ** 3 / (k1 * n_cell)
    n = n_cell * cells
    cell, ids = np.repeat(np.arange(cells), n_cell), np.arange(n)

    def ratio(seed, tau, steps):
        rng = np.random.default_rng(seed)
        v = np.stack([rng.normal(0, v_perp, n), rng.normal(0, v_perp, n), rng.normal(0, v_par, n)], axis=1)
        temps = lambda v: (v.var(axis=0)[2], 0.5 * (v.var(axis=0)[0] + v.var(axis=0)[1]))
        t0 = temps(v)
        e0 = (v ** 2).sum()
        for k in range(steps):
            v = ref.apply(ref.request(log_lambda, tau, scene.ME, scene.QE, scene.ME, scene.QE, 1.0, dv, seed=seed, epoch=k, like=True), cell, ids, v)["va"]
        assert abs((v ** 2).sum() / e0 - 1) < 1e-12
        t1 = temps(v)
        rate = -math.log((t1[1] - t1[0]) / (t0[1] - t0[0])) / (steps * tau)
        return rate / (3.0 * 0.5 * (_nu_t(n_cell / dv, *t0, scene.ME, scene.QE, log_lambda) + _nu_t(n_cell / dv, *t1, scene.ME, scene.QE, log_lambda)))

    full = np.array([ratio(s, tau, 16) for s in range(8)])
    half = np.array([ratio(100 + s, tau / 2, 32) for s in range(8)])
    error = full.std(ddof=1) / math.sqrt(len(full))
    bias = abs(full.mean() - half.mean())
    print("isotropisation: measured / closed-form rate %.3f, standard error %.3f; with tau / 2: %.3f" % (full.mean(), error, half.mean()))
    assert abs(full.mean() - 1.0) <= 3 * error + bias
    assert 3 * error + bias < 0.5                                   # (and the tolerance says something)
