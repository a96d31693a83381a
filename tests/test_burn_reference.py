"""The numpy restatement of the fusion burn (tests/burn_reference.py) alone, on the CPU: hand-made cells, the books
(accepted = burnt + blocked, no particle in two events), the saturated counts per cell, conservation of momentum and energy per
event within a bound derived from the operation count, the statistics of the acceptance, and the conditions of every scene the
GPU test (tests/test_gpu_burn.py) compares exactly.

THE COUNT OF AN ODD LIKE CELL when every pair is accepted: like_pair gives a cell of N = 2 t + 1 >= 3 particles the triple
(s0,s1), (s1,s2), (s2,s0) — one chain, of which the first pair reacts — and the (N - 3) / 2 disjoint pairs (s[3+2k], s[4+2k]):
1 + (N - 3) / 2 = (N - 1) / 2 = floor(N / 2) events, as in an even cell (N / 2 disjoint pairs).  s2 of the triple is left over.

THE BOUNDS of the per-event identities, with e = 2^-53 (one rounding, relative) and everything evaluated in exact rationals
from the doubles the rule produced.  Both products are built on the same computed V, so V enters exactly.
  momentum, per component:  w3 = fl(V + fl(u3 n)), w4 = fl(V - fl(u4 n)), u4 = fl(r34 u3), r34 = fl(m3 / m4).  With a = u3 n:
      |m3 w3 + m4 w4 - (m3 + m4) V| <= m3 (e |w3| + e |a|) + m4 (e |w4| + 3 e r34 |a|) (1 + 3 e) <= e (m3 |w3| + m4 |w4| + 4.5 m3 |a|)
      (m4 r34 = m3 (1 + e)): five roundings in all, each counted once.
  energy:  1/2 m3 |w3 - V|^2 c^2 + 1/2 m4 |w4 - V|^2 c^2 against Et = fl(q_value + K) held to 0.  Exactly, u3^2 = Et kf and |n| = 1
      make it Et.  Relative roundings on the way to the squares: kf 4 (m3 + m4, the product, the division, / (c c)), c c 1,
      Et kf 1, the square root 1 (and it halves what came before: 3 + 1 on u3, 8 on u3^2), u3 n_i 1 each (2 on the square),
      |n|^2 - 1 at most 10 (x x twice, their sum, 1 - s, the root, 2 x r, 1 - 2 s), product 4 besides r34 1 and u4 1 (4 on the
      square) and m4 r34^2 against m3^2 / m4 2: 8 + 2 + 10 + 4 + 2 = 26, taken as 32 e Et.  Absolutely, the sums V + a round
      to w with at most e |w_i| each, which moves m c^2 |d|^2 / 2 by m c^2 |d_i| e |w_i| per component (first order; twice that
      is allowed for the second order)."""
from fractions import Fraction

import numpy as np
import pytest

import burn_reference as ref
import burn_scenes as sc
from test_fusion_host import KEV, KT_KEV, MD, MT, gamow_of_g, quadrature

EPS = Fraction(1, 2 ** 53)
FLAT = np.full(2, 1e-28)


def saturated(like, m4=sc.MN, **kw):
    """every pair of every speed below 1 is inside the table and has P >= 1"""
    return ref.request(FLAT, 0.0, 1.0, 1e30, 1e10, 1.0, sc.MD, sc.MD if like else sc.MT, sc.MA, m4, q_value=sc.Q_DT, like=like, **kw)


def cells(counts, seed, vth=0.01):
    """(cell, ids, pos, vel) of counts[c] particles in cell c, shuffled"""
    rng = np.random.default_rng(seed)
    cell = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(cell)
    n = len(cell)
    return dict(cell=cell, ids=rng.permutation(3 * n + 5)[:n], pos=rng.random((n, 3)), vel=rng.normal(0, vth, (n, 3)))


def books(app, A, B):
    assert app["accepted"] == app["burnt"] + app["blocked"] and app["burnt"] == app["m"]
    if app["m"]:
        a, b = np.asarray(A["ids"])[app["event_a"]], np.asarray((A if B is None else B)["ids"])[app["event_b"]]
        assert len(set(a.tolist())) == len(a) and len(set(b.tolist())) == len(b)
        if B is None:
            assert not set(a.tolist()) & set(b.tolist())
        assert np.all(np.diff(a.astype(np.int64)) > 0)                         # the events in ascending id of their species_a reactant
    assert int((~app["keep_a"]).sum()) == app["m"] * (2 if B is None else 1)


# ---- hand-made cells
def test_hand_made_unlike_cells():
    req = saturated(False)
    # (1, 1): one pair, one event
    A, B = cells([1], 1), cells([1], 2)
    app = ref.application(req, A, B, 0, 0)
    books(app, A, B)
    assert (app["pairs"], app["accepted"], app["blocked"], app["burnt"], app["saturated"], app["cells"]) == (1, 1, 0, 1, 1, 1)
    assert not app["keep_a"].any() and not app["keep_b"].any()
    # (3, 1): one chain of three; only the middle pair is accepted: it reacts
    A, B = cells([3], 3), cells([1], 4)
    plan = ref.schedule(req, A["cell"], A["ids"], B["cell"], B["ids"])
    assert plan["chain"].tolist() == [0, 0, 0] and plan["place"].tolist() == [0, 1, 2] and plan["n_l"].tolist() == [1.0, 1.0, 1.0]
    accepted = np.array([False, True, False])
    assert ref.resolve(plan["chain"], plan["place"], accepted).tolist() == [False, True, False]
    assert ref.resolve(plan["chain"], plan["place"], np.array([False, True, True])).tolist() == [False, True, False]      # the lower place wins
    assert ref.resolve(plan["chain"], plan["place"], np.array([True, True, True])).tolist() == [True, False, False]
    app = ref.application(req, A, B, 0, 0)                                      # all three accepted: the first reacts, two are blocked
    books(app, A, B)
    assert (app["accepted"], app["blocked"], app["burnt"]) == (3, 2, 1)
    order = np.lexsort((A["ids"], ref.keys(req, A["ids"])))
    assert app["event_a"].tolist() == [order[0]] and int(app["keep_a"].sum()) == 2      # the first of the sorted many
    # the few species may be species_a
    app = ref.application(req, B, A, 0, 0)
    assert (app["accepted"], app["blocked"], app["burnt"]) == (3, 2, 1) and not app["keep_a"].any() and int(app["keep_b"].sum()) == 2


def test_hand_made_like_cells():
    req = saturated(True)
    A = cells([3], 5)
    plan = ref.schedule(req, A["cell"], A["ids"])
    assert plan["chain"].tolist() == [0, 0, 0] and plan["place"].tolist() == [0, 1, 2] and plan["n_l"].tolist() == [1.5, 1.5, 1.5]
    order = np.lexsort((A["ids"], ref.keys(req, A["ids"])))
    assert plan["owner"].tolist() == [order[0], order[1], order[2]] and plan["partner"].tolist() == [order[1], order[2], order[0]]
    app = ref.application(req, A, None, 0, 0)
    books(app, A, None)
    assert (app["accepted"], app["blocked"], app["burnt"]) == (3, 2, 1) and app["keep_a"].tolist() == [k == order[2] for k in range(3)]
    assert ref.resolve(plan["chain"], plan["place"], np.array([False, True, True])).tolist() == [False, True, False]
    A = cells([2], 6)
    app = ref.application(req, A, None, 0, 0)
    books(app, A, None)
    assert (app["pairs"], app["accepted"], app["blocked"], app["burnt"]) == (1, 1, 0, 1) and not app["keep_a"].any()
    assert ref.application(req, cells([1], 7), None, 0, 0)["m"] == 0


def test_saturated_counts_per_cell():
    counts_a, counts_b = [1, 5, 7, 64, 65, 130, 0, 3], [1, 1, 3, 64, 64, 7, 4, 0]
    A, B = cells(counts_a, 8), cells(counts_b, 9)
    app = ref.application(saturated(False), A, B, 0, 0)
    books(app, A, B)
    assert app["saturated"] == app["accepted"] == app["pairs"] == sum(max(a, b) for a, b in zip(counts_a, counts_b) if min(a, b))
    for c, (a, b) in enumerate(zip(counts_a, counts_b)):
        assert int((~app["keep_a"][A["cell"] == c]).sum()) == min(a, b) == int((~app["keep_b"][B["cell"] == c]).sum()), c
    counts = [0, 1, 2, 3, 4, 5, 63, 64, 65, 129]
    A = cells(counts, 10)
    app = ref.application(saturated(True), A, None, 0, 0)
    books(app, A, None)
    for c, n in enumerate(counts):
        assert int((~app["keep_a"][A["cell"] == c]).sum()) == 2 * (n // 2), c        # (the module docstring: floor(N / 2) events)
        assert ref.odd_cell_pairs(n)[1] == n // 2
    assert app["blocked"] == 2 * sum(1 for n in counts if n % 2 and n >= 3)
    # an overfull cell is skipped and counted
    A, B = cells([5, 9], 11), cells([5, 2], 12)
    app = ref.application(saturated(False), A, B, 0, 0, cell_max=8)
    assert (app["overfull_cells"], app["overfull_particles"], app["cells"], app["burnt"]) == (1, 11, 1, 5)
    # max sigma = 0 and an empty species: nothing
    zero = ref.request(np.zeros(2), 0.0, 1.0, 1.0, 1e10, 1.0, sc.MD, sc.MT, sc.MA, sc.MN)
    assert ref.application(zero, A, B, 0, 0)["m"] == 0 and ref.decide(zero, A["cell"], A["ids"], A["vel"], B["cell"], B["ids"], B["vel"])["pairs"] == 0


# ---- conservation per event
@pytest.mark.parametrize("like,m4,q", [(False, sc.MN, sc.Q_DT), (True, sc.MP, 4.03e6 * sc.QP), (False, sc.MP, -3e-15)], ids=["d-t", "d-d", "endothermic"])
def test_every_event_conserves_momentum_and_energy(like, m4, q):
    A, B = cells([40, 7, 130], 13, vth=0.003), (None if like else cells([40, 9, 6], 14, vth=0.003))
    req = ref.request(FLAT, 0.0, 1.0, 1e30, 1e10, 1.0, sc.MD, sc.MD if like else sc.MT, sc.MA, m4, q_value=q, like=like, seed=99)
    app = ref.application(req, A, B, 0, 0, tracked_b=False)                     # (w4 stays a double: the identities are the rule's, before any cast)
    assert app["m"] > 40 and ref.conditions_hold(app)
    F = Fraction
    m3, m4, cc = F(sc.MA), F(m4), F(ref.C) ** 2
    et = np.where(req["q_value"] + app["K"] > 0, req["q_value"] + app["K"], 0.0)
    assert q > 0 or ((et == 0).any() and (et > 0).any())                        # the endothermic case holds Et to 0 somewhere
    worst_p = worst_e = F(0)
    for k in range(app["m"]):
        V, w3, w4, n = ([F(float(x)) for x in app[name][k]] for name in ("V", "w3", "w4", "n"))
        e3 = e4 = slack = F(0)
        u3 = float(np.sqrt(et[k] * req["kf"]))
        for i in range(3):
            a = abs(F(u3) * n[i])
            bound = EPS * (m3 * abs(w3[i]) + m4 * abs(w4[i]) + F(9, 2) * m3 * a)
            miss = abs(m3 * w3[i] + m4 * w4[i] - (m3 + m4) * V[i])
            assert miss <= bound, (k, i, float(miss / bound) if bound else None)
            worst_p = max(worst_p, miss / bound if bound else F(0))
            d3, d4 = w3[i] - V[i], w4[i] - V[i]
            e3 += d3 * d3
            e4 += d4 * d4
            slack += 2 * cc * EPS * (m3 * abs(d3) * abs(w3[i]) + m4 * abs(d4) * abs(w4[i]))
        got = m3 * cc * e3 / 2 + m4 * cc * e4 / 2
        bound = 32 * EPS * F(float(et[k])) + slack
        assert abs(got - F(float(et[k]))) <= bound, (k, float(abs(got - F(float(et[k]))) / bound) if bound else None)
        worst_e = max(worst_e, abs(got - F(float(et[k]))) / bound if bound else F(0))
    print("largest miss / bound: momentum %.3f, energy %.3f over %d events" % (float(worst_p), float(worst_e), app["m"]))


# ---- statistics
def test_the_acceptance_has_the_probability():
    """8 cells of about 2000 + 2000 at 10 keV with the cross-section of the reactivity test (tests/test_fusion_host.py), tau such
    that the mean P is about 1e-2 (from the reactivity's quadrature: P = W N_L tau <sigma v> / dV with N_L = 2000): over 8 seeds the accepted pairs lie within three standard errors of the sum of P, and the
    blocked share stays below max P x (chain length - 1)"""
    vth_d, vth_t = (np.sqrt(KT_KEV * KEV / m) / ref.C for m in (MD, MT))
    mab = MD * MT / (MD + MT)
    g_lo, g_hi = (np.sqrt(2.0 * e * KEV / mab) / ref.C for e in (0.2, 300.0))
    S = gamow_of_g(g_lo + np.arange(4096) * ((g_hi - g_lo) / 4095), mab)
    W, dV = 1e12, 1e-9
    tau = 1e-2 * dV / (W * 2000.0 * quadrature(np.sqrt(vth_d ** 2 + vth_t ** 2), mab))
    accepted = expected = variance = blocked = 0.0
    p_max, chain_max = 0.0, 0
    for seed in range(401, 409):
        rng = np.random.default_rng(seed)
        na, nb = rng.integers(1900, 2049, 8), rng.integers(1900, 2049, 8)
        ca, cb = np.repeat(np.arange(8), na), np.repeat(np.arange(8), nb)
        va, vb = rng.normal(0, vth_d, (len(ca), 3)), rng.normal(0, vth_t, (len(cb), 3))
        req = ref.request(S, g_lo, g_hi, tau, W, dV, MD, MT, sc.MA, sc.MN, q_value=sc.Q_DT, seed=seed)
        out = ref.decide(req, ca, np.arange(len(ca)), va, cb, np.arange(len(cb)), vb)
        P = np.minimum(out["P"], 1.0)
        accepted += out["accepted"]
        blocked += out["blocked"]
        expected += float(P.sum())
        variance += float((P * (1.0 - P)).sum())
        p_max = max(p_max, float(P.max()))
        chain_max = max(chain_max, int(np.bincount(out["plan"]["chain"]).max()))
        assert out["accepted"] == out["burnt"] + out["blocked"]
    print("accepted %d, sum P %.1f, standard error %.1f; blocked / accepted %.2e, chain bound %.2e (max P %.3g, chain length %d)" %
          (accepted, expected, np.sqrt(variance), blocked / accepted, p_max * (chain_max - 1), p_max, chain_max))
    assert 0.8e-2 < expected / (8 * 16000) < 1.2e-2 and p_max < 1.0 and chain_max == 2 and accepted > 1000
    assert abs(accepted - expected) <= 3.0 * np.sqrt(variance)
    assert blocked / accepted <= p_max * (chain_max - 1)


# ---- the scenes of the GPU test
@pytest.mark.parametrize("name", sc.SCENES)
def test_the_conditions_of_the_gpu_scenes(name):
    p = sc.particles(name)
    for dtype in (np.float32, np.float64):
        A, B = sc.stored(name, dtype)
        # a handle of either precision stores what the reference is given: the velocities are float32 values, the cell of a
        # stored fraction is the cell the scene put the particle in
        for side, given in ((A, p["a"]), (B, p["b"])):
            if side is None:
                continue
            pos, vel = given
            assert np.array_equal(side["vel"].astype(np.float64), np.asarray(vel, dtype=np.float64))
            c = np.floor(np.asarray(pos)).astype(np.int64)
            assert np.array_equal(side["cell"], c[:, 0] + p["shape"][0] * (c[:, 1] + p["shape"][1] * c[:, 2]))
    for which in sc.TAUS:
        for tracked in (False, True):
            req, app = sc.reference(name, which, np.float32, tracked_b=tracked)
            assert ref.conditions_hold(app)
            A, B = sc.stored(name, np.float32)
            books(app, A, B)
            assert (which != "saturated" or (app["saturated"] > 0 and app["blocked"] > 0)) and (which != "many" or app["blocked"] > 0)
    like = sc.reference("like", "many")[1]
    assert sc.RANK_MAX + 1 in np.bincount(sc.stored("like", np.float32)[0]["cell"]) and (like["g"] == 0).sum() == 1 and like["what"][like["g"] == 0][0] == 1
    full = sc.reference("full", "saturated")[1]
    assert full["overfull_cells"] == 2 and full["cells"] == 4 and sc.reference("full", "rare")[1]["m"] > 0
    full = sc.reference("full_like", "saturated")[1]
    assert full["overfull_cells"] == 1 and full["overfull_particles"] == sc.PAIR_CELL_MAX + 1 and full["cells"] == 4 and sc.reference("full_like", "rare")[1]["m"] > 0
    assert np.bincount(sc.stored("full_like", np.float32)[0]["cell"])[sc._full[0]:sc._full[0] + 5].tolist() == sc.FULL_LIKE_COUNTS
    counts = np.bincount(sc.stored("unlike", np.float32)[0]["cell"], minlength=4096), np.bincount(sc.stored("unlike", np.float32)[1]["cell"], minlength=4096)
    pairs = set(zip(counts[0].tolist(), counts[1].tolist()))
    assert {(1, 1), (130, 7), (7, 130), (64, 64), (65, 64)} <= pairs
