"""The rule of the binary Coulomb collision operator (fpic_pair; Takizuka & Abe 1977) restated in plain numpy, from the text
of include/fusionpic.h and DESIGN.md 4.17.  It shares no code with the library: Philox4x32-10 and the circular functions are
those of load_reference.py, everything else is float64 in the stated operation order (numpy never fuses a multiply with an
add).

    req = request(log_lambda, tau, ma, qa, mb, qb, W, dV, seed=..., stream=..., epoch=..., like=False)
    out = apply(req, cell_a, ids_a, v_a, cell_b, ids_b, v_b)     v: the STORED velocities, float32 or float64 (n, 3)
    out["va"], out["vb"]      the stored velocities afterwards (the same dtype; cast after every pair)
    out["pairs"], out["strong"], out["cells"], out["overfull_cells"], out["overfull_particles"]
    like species: apply(req, cell, ids, v) with request(..., like=True); out["vb"] is None.

The pairs of all cells are collided in stages: stage t holds every pair that is the (t+1)-th of both its members, so the pairs
of a stage are disjoint and one vectorised call serves them; a particle's next pair starts from the value cast to the
stored type.  `parts` replaces the three rounded functions of a pair (the first normal, cospi, sinpi) — the 50-digit twin of
tests/test_pair_reference.py hands in correctly rounded ones.
"""
import math

import numpy as np

from load_reference import cospi, philox, sinpi

TAG = 0xC0120
SEED = 0x7A1C12ABE
TWO_M32 = 2.0 ** -32
EPS0 = 8.8541878128e-12
C = 2.998e8
CELL_MAX = 2048


def request(log_lambda, tau, ma, qa, mb, qb, W, dV, seed=SEED, stream=0, epoch=0, like=False):
    """the host's part of a request (rule_of)"""
    ma, qa, mb, qb, W, dV, log_lambda, tau = (float(x) for x in (ma, qa, mb, qb, W, dV, log_lambda, tau))
    mab = (ma * mb) / (ma + mb)
    qq = qa * qb
    num = (((qq * qq) * log_lambda) * tau) * W
    den = ((((8.0 * math.pi) * (EPS0 * EPS0)) * (mab * mab)) * ((C * C) * C)) * dV
    return dict(kappa=num / den, fa=mab / ma, fb=mab / mb, mab=mab, like=bool(like), seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32, stream=stream,
                epoch=epoch & 0xFFFFFFFF)


def words(req, ids, block):
    """P(block) of the particles: four uint32 arrays"""
    return philox(np.asarray(ids, dtype=np.uint64), req["epoch"], req["stream"], TAG + block, req["seed_lo"], req["seed_hi"])


def keys(req, ids):
    return words(req, ids, 0)[0].astype(np.uint64)


def parts_of(req, owners):
    """the three rounded functions of a pair: the first normal of P(1) of the owner, cospi(2 phi) and sinpi(2 phi)"""
    w1 = words(req, owners, 1)
    u1 = (w1[0].astype(np.float64) + 0.5) * TWO_M32
    r1 = np.sqrt(-2.0 * np.log(u1))
    n0 = r1 * cospi(2.0 * (w1[1].astype(np.float64) * TWO_M32))
    phi2 = 2.0 * (words(req, owners, 0)[1].astype(np.float64) * TWO_M32)
    return n0, cospi(phi2), sinpi(phi2)


def pairing_unlike(nm, nf):
    """(many j, few q, N_L) in the order a few particle meets its partners: ascending j"""
    return [] if nf == 0 else [(j, j % nf, float(nf)) for j in range(nm)]


def pairing_like(n):
    """(owner, partner, N_L) in order"""
    if n < 2:
        return []
    if n % 2 == 0:
        return [(2 * t, 2 * t + 1, float(n)) for t in range(n // 2)]
    return [(0, 1, n / 2.0), (1, 2, n / 2.0), (2, 0, n / 2.0)] + [(3 + 2 * t, 4 + 2 * t, float(n)) for t in range((n - 3) // 2)]


def collide(req, owners, n_l, fo, fp, vo, vp, parts=None):
    """one pair each: owners' ids, N_L, the mass factors of owner and partner (arrays), float64 velocities (n, 3).
    Returns vo', vp' (float64, before the cast), counted, strong, var, and mag (n, 3): per component of du the sum of the
    magnitudes of its terms (what a bound of the rounded parts scales with)"""
    n_l, fo, fp = (np.asarray(x, dtype=np.float64) for x in (n_l, fo, fp))
    ux, uy, uz = vo[:, 0] - vp[:, 0], vo[:, 1] - vp[:, 1], vo[:, 2] - vp[:, 2]
    up2 = ux * ux + uy * uy
    up = np.sqrt(up2)
    g = np.sqrt(up2 + uz * uz)
    counted = g != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        var = (req["kappa"] * n_l) / ((g * g) * g)
        n0, cs, sn = (parts or parts_of)(req, owners)
        delta = np.sqrt(var) * n0
        d2 = delta * delta
        den = 1.0 + d2
        sinT = (2.0 * delta) / den
        omc = (2.0 * d2) / den
        ex, ey = ux / up, uy / up
        ax, bx, cx = ((ex * uz) * sinT) * cs, ((ey * g) * sinT) * sn, ux * omc
        ay, by, cy = ((ey * uz) * sinT) * cs, ((ex * g) * sinT) * sn, uy * omc
        az, cz = (up * sinT) * cs, uz * omc
        dux = (ax - bx) - cx
        duy = (ay + by) - cy
        duz = (-az) - cz
        axial = up == 0
        gs = g * sinT
        dux = np.where(axial, gs * cs, dux)
        duy = np.where(axial, gs * sn, duy)
        duz = np.where(axial, -(g * omc), duz)
        mag = np.stack([np.where(axial, np.abs(gs * cs), np.abs(ax) + np.abs(bx) + np.abs(cx)),
                        np.where(axial, np.abs(gs * sn), np.abs(ay) + np.abs(by) + np.abs(cy)),
                        np.where(axial, np.abs(g * omc), np.abs(az) + np.abs(cz))], axis=1)
    du = np.stack([dux, duy, duz], axis=1)
    new_o = vo + fo[:, None] * du
    new_p = vp - fp[:, None] * du
    new_o[~counted] = vo[~counted]
    new_p[~counted] = vp[~counted]
    mag[~counted] = 0
    return new_o, new_p, counted, counted & (var > 1.0), var, mag


def schedule(req, cell_a, ids_a, cell_b=None, ids_b=None, cell_max=CELL_MAX):
    """Who pairs with whom: arrays (owner, partner, N_L, stage) of indices into the concatenation (species a, then species b),
    and the counts of cells.  Stage t of a pair: t pairs of its members come before it."""
    cell_a, ids_a = np.asarray(cell_a, dtype=np.int64), np.asarray(ids_a, dtype=np.uint64)
    na = len(ids_a)
    like = req["like"]
    if like:
        cell, ids = cell_a, ids_a
    else:
        cell = np.concatenate([cell_a, np.asarray(cell_b, dtype=np.int64)])
        ids = np.concatenate([ids_a, np.asarray(ids_b, dtype=np.uint64)])
    side = (np.arange(len(ids)) >= na).astype(np.int64) if not like else np.zeros(len(ids), dtype=np.int64)
    order = np.lexsort((ids, keys(req, ids), side, cell))          # by cell, then species, then (key, id)
    owner, partner, n_l, stage = [], [], [], []
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
            table = pairing_like(len(a))
            if not table:
                continue
            cells += 1
            for k, (o, p, nl) in enumerate(table):
                owner.append(a[o]); partner.append(a[p]); n_l.append(nl)
                stage.append(k if len(a) % 2 and k < 3 else 0)
        else:
            many, few = (a, b) if len(a) >= len(b) else (b, a)
            table = pairing_unlike(len(many), len(few))
            if not table:
                continue
            cells += 1
            for j, q, nl in table:
                owner.append(many[j]); partner.append(few[q]); n_l.append(nl); stage.append(j // len(few))
    return dict(owner=np.array(owner, dtype=np.int64), partner=np.array(partner, dtype=np.int64), n_l=np.array(n_l, dtype=np.float64),
                stage=np.array(stage, dtype=np.int64), cells=cells, overfull_cells=overfull_cells, overfull_particles=overfull_particles, na=na)


def apply(req, cell_a, ids_a, v_a, cell_b=None, ids_b=None, v_b=None, cell_max=CELL_MAX, parts=None, plan=None):
    """the whole rule on stored velocities (their dtype is the handle's precision)"""
    like = req["like"]
    dtype = v_a.dtype
    plan = plan or schedule(req, cell_a, ids_a, cell_b, ids_b, cell_max)
    na = plan["na"]
    ids = np.asarray(ids_a, dtype=np.uint64) if like else np.concatenate([np.asarray(ids_a, dtype=np.uint64), np.asarray(ids_b, dtype=np.uint64)])
    v = (v_a if like else np.concatenate([v_a, v_b])).astype(np.float64)
    f = np.where(np.arange(len(ids)) < na, req["fa"], req["fa"] if like else req["fb"])
    pairs = strong = 0
    scale = np.zeros_like(v)                                       # per particle and component: sum over its pairs of f mag + |v'|
    stages = np.zeros(len(ids), dtype=np.int64)                    # the pairs a particle took part in
    for t in range(int(plan["stage"].max()) + 1 if len(plan["stage"]) else 0):
        at = plan["stage"] == t
        o, p = plan["owner"][at], plan["partner"][at]
        new_o, new_p, counted, hard, _, mag = collide(req, ids[o], plan["n_l"][at], f[o], f[p], v[o], v[p], parts)
        v[o[counted]] = new_o[counted].astype(dtype).astype(np.float64)
        v[p[counted]] = new_p[counted].astype(dtype).astype(np.float64)
        for who, fw, new in ((o, f[o], new_o), (p, f[p], new_p)):
            scale[who[counted]] += (fw[:, None] * mag)[counted]
            stages[who[counted]] += 1
        pairs += int(counted.sum())
        strong += int(hard.sum())
    v = v.astype(dtype)
    return dict(va=v[:na], vb=None if like else v[na:], pairs=pairs, strong=strong, cells=plan["cells"], overfull_cells=plan["overfull_cells"],
                overfull_particles=plan["overfull_particles"], plan=plan, scale_a=scale[:na], scale_b=None if like else scale[na:],
                stages_a=stages[:na], stages_b=None if like else stages[na:])
