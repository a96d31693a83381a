"""The rule of the fusion yield tally (fpic_fusion) restated in numpy float64 and Python integers, from the text of
include/fusionpic.h and DESIGN.md 4.18.  It shares no code with the library: Philox4x32-10 is load_reference.py's, everything
else is float64 in the stated operation order (numpy never fuses a multiply with an add; every operation is one of
+ - x / sqrt, so the library can and must agree bit for bit), and the sums are Python integers.

    req = request(sigma, g_lo, g_hi, tau, W, dV, seed=..., stream=..., epoch=..., like=False)
    out = apply(req, ncells, cell_a, ids_a, v_a, cell_b, ids_b, v_b)      v: the STORED velocities, float32 or float64 (n, 3)
    out["grid"]           int64 (ncells,): the cells' tallies in units of 2**req["e"] reactions
    out["reactions_exact"], out["yield_hi"], out["yield_lo"]              the total as a Python integer and as the two words
    out["pairs"], out["below"], out["above"], out["cells"], out["overfull_cells"], out["overfull_particles"], out["unit_exponent"]
    out["weights"]        the sum of N_L over all pairs (a float that is exact: halves)
    like species: apply(req, ncells, cell, ids, v) with request(..., like=True).
"""
import math
from fractions import Fraction

import numpy as np

from load_reference import philox

TAG = 0xF0510
SEED = 0xF0510D7
C = 2.998e8
CELL_MAX = 2048
Q_BITS = 40
EXPONENT_MIN = -1000


def y_bound(W, tau, dV, s_max, g_hi):
    W, tau, dV, s_max, g_hi = (float(x) for x in (W, tau, dV, s_max, g_hi))
    return ((((W * W) * float(CELL_MAX)) * tau) / dV) * (s_max * (g_hi * C))


def exponent(bound):
    """the smallest integer e with bound < 2**(e + 40), not below EXPONENT_MIN; 0 for a zero bound"""
    if not bound > 0:
        return 0
    e = math.frexp(bound)[1] - Q_BITS          # bound = m 2**ex, 0.5 <= m < 1
    assert Fraction(2) ** (e + Q_BITS - 1) <= Fraction(bound) < Fraction(2) ** (e + Q_BITS)
    return max(e, EXPONENT_MIN)


def request(sigma, g_lo, g_hi, tau, W, dV, seed=SEED, stream=0, epoch=0, like=False):
    """the host's part of a request (rule_of)"""
    S = np.array(sigma, dtype=np.float64)
    g_lo, g_hi, tau, W, dV = (float(x) for x in (g_lo, g_hi, tau, W, dV))
    n = len(S)
    s_max = float(S.max()) if n else 0.0
    e = exponent(y_bound(W, tau, dV, s_max, g_hi))
    return dict(S=S, n=n, g_lo=g_lo, g_hi=g_hi, inv_dg=float(n - 1) / (g_hi - g_lo), s_max=s_max, ww=W * W, tau=tau, dv=dV, e=e, unit=math.ldexp(1.0, -e),
                like=bool(like), seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32, stream=stream, epoch=epoch & 0xFFFFFFFF)


def keys(req, ids):
    return philox(np.asarray(ids, dtype=np.uint64), req["epoch"], req["stream"], TAG, req["seed_lo"], req["seed_hi"])[0].astype(np.uint64)


def pairing_unlike(nm, nf):
    """(many j, few q, N_L)"""
    return [] if nf == 0 else [(j, j % nf, float(nf)) for j in range(nm)]


def pairing_like(n):
    """(owner, partner, N_L)"""
    if n < 2:
        return []
    if n % 2 == 0:
        return [(2 * t, 2 * t + 1, float(n)) for t in range(n // 2)]
    return [(0, 1, n / 2.0), (1, 2, n / 2.0), (2, 0, n / 2.0)] + [(3 + 2 * t, 4 + 2 * t, float(n)) for t in range((n - 3) // 2)]


def sigma_at(req, g):
    """the interpolated cross-section at speeds inside [g_lo, g_hi)"""
    S, n = req["S"], req["n"]
    t = (g - req["g_lo"]) * req["inv_dg"]
    k = np.minimum(np.floor(t).astype(np.int64), n - 2)
    s = S[k] + (t - k.astype(np.float64)) * (S[k + 1] - S[k])
    return np.minimum(s, req["s_max"])


def tally(req, n_l, vo, vp):
    """one pair each: N_L (array) and float64 velocities (n, 3).  Returns q (a list of Python integers), what (0 inside, 1
    below, 2 above) and g"""
    n_l = np.asarray(n_l, dtype=np.float64)
    ux, uy, uz = vo[:, 0] - vp[:, 0], vo[:, 1] - vp[:, 1], vo[:, 2] - vp[:, 2]
    g = np.sqrt((ux * ux + uy * uy) + uz * uz)
    what = np.where(g < req["g_lo"], 1, np.where(~(g < req["g_hi"]), 2, 0))
    inside = what == 0
    q = np.zeros(len(g), dtype=np.float64)
    if inside.any():
        gi = g[inside]
        sigma = sigma_at(req, gi)
        y = ((((req["ww"] * n_l[inside]) * req["tau"]) / req["dv"])) * (sigma * (gi * C))
        q[inside] = np.floor(y * req["unit"])
    assert np.all(q < 2.0 ** Q_BITS)
    return [int(x) for x in q], what, g


def schedule(req, cell_a, ids_a, cell_b=None, ids_b=None, cell_max=CELL_MAX):
    """Who pairs with whom: arrays (owner, partner, N_L, cell) of indices into the concatenation (species a, then species b),
    and the counts of cells"""
    cell_a, ids_a = np.asarray(cell_a, dtype=np.int64), np.asarray(ids_a, dtype=np.uint64)
    na = len(ids_a)
    like = req["like"]
    if like:
        cell, ids = cell_a, ids_a
    else:
        cell = np.concatenate([cell_a, np.asarray(cell_b, dtype=np.int64)])
        ids = np.concatenate([ids_a, np.asarray(ids_b, dtype=np.uint64)])
    side = np.zeros(len(ids), dtype=np.int64) if like else (np.arange(len(ids)) >= na).astype(np.int64)
    order = np.lexsort((ids, keys(req, ids), side, cell))          # by cell, then species, then (key, id)
    owner, partner, n_l, where = [], [], [], []
    cells = overfull_cells = overfull_particles = 0
    bounds = np.flatnonzero(np.diff(cell[order])) + 1
    for group in np.split(order, bounds):
        if len(group) == 0:
            continue
        a, b = group[side[group] == 0], group[side[group] == 1]
        if len(a) > cell_max or len(b) > cell_max:
            overfull_cells += 1
            overfull_particles += len(group)
            continue
        if like:
            table = [(a[o], a[p], nl) for o, p, nl in pairing_like(len(a))]
        else:
            many, few = (a, b) if len(a) >= len(b) else (b, a)
            table = [(many[j], few[q], nl) for j, q, nl in pairing_unlike(len(many), len(few))]
        if not table:
            continue
        cells += 1
        for o, p, nl in table:
            owner.append(o); partner.append(p); n_l.append(nl); where.append(cell[group[0]])
    return dict(owner=np.array(owner, dtype=np.int64), partner=np.array(partner, dtype=np.int64), n_l=np.array(n_l, dtype=np.float64),
                cell=np.array(where, dtype=np.int64), cells=cells, overfull_cells=overfull_cells, overfull_particles=overfull_particles, na=na)


def apply(req, ncells, cell_a, ids_a, v_a, cell_b=None, ids_b=None, v_b=None, cell_max=CELL_MAX):
    """the whole tally on stored velocities (their dtype is the handle's precision)"""
    like = req["like"]
    zero = dict(pairs=0, below=0, above=0, cells=0, overfull_cells=0, overfull_particles=0, yield_hi=0, yield_lo=0, reactions_exact=0, weights=0.0,
                grid=np.zeros(ncells, dtype=np.int64))
    if not req["s_max"] > 0 or len(ids_a) == 0 or (not like and len(ids_b) == 0):      # nothing can react: nothing is launched
        return dict(zero, unit_exponent=req["e"])
    plan = schedule(req, cell_a, ids_a, cell_b, ids_b, cell_max)
    v = (np.asarray(v_a) if like else np.concatenate([v_a, v_b])).astype(np.float64)
    q, what, g = tally(req, plan["n_l"], v[plan["owner"]], v[plan["partner"]])
    sums = [0] * ncells
    for c, x in zip(plan["cell"], q):
        sums[c] += x
    total = sum(sums)
    assert all(s < 1 << 51 for s in sums)
    return dict(pairs=int((what == 0).sum()), below=int((what == 1).sum()), above=int((what == 2).sum()), cells=plan["cells"], overfull_cells=plan["overfull_cells"],
                overfull_particles=plan["overfull_particles"], yield_hi=total >> 32, yield_lo=total & 0xFFFFFFFF, reactions_exact=total, unit_exponent=req["e"],
                weights=float(plan["n_l"].sum()), grid=np.array(sums, dtype=np.int64), plan=plan, q=q, what=what, g=g)
