"""The rule of the fusion burn (fpic_burn) restated in numpy float64 and Python integers, from the text of include/fusionpic.h
and DESIGN.md 4.29.  It shares no code with the library: the pair sets, N_L and the table lookup are tests/fusion_reference.py's
(the restatement of fpic_fusion, which the burn is defined on), the isotropic try tests/fusion_spectrum_reference.py's, the
exact sums tests/ionize_reference.py's gain(), Philox4x32-10 load_reference.py's; the words are this operator's own (tags
0xB0510, 0xB0511 / 0xB0512, 0xB0520 ..).  Everything else is float64 in the stated operation order (numpy never fuses a multiply
with an add; every operation is one of + - x / sqrt, so the library can and must agree bit for bit).

    req = request(sigma, g_lo, g_hi, tau, W, dV, m_a, m_b, m3, m4, q_value=.., seed=.., stream=.., epoch=.., like=False)
    out = decide(req, cell_a, ids_a, v_a, cell_b, ids_b, v_b)        v: the STORED velocities (n, 3) of the handle's dtype
        the counts, and per pair (arrays over plan["owner"]): P, what (0 inside, 1 below, 2 above), accepted, reacts, chain, place
    app = application(req, A, B, n3, span3, n4, span4, tracked_b=True)   A, B: dict(cell=, ids=, pos=, vel=) of stored arrays
        (like species: B is None); the survivors, the new rows by event number, the exact sums
"""
import numpy as np

import fusion_reference as uref
import fusion_spectrum_reference as sref
import ionize_reference as iref
from load_reference import philox

TAG = 0xB0510
ACCEPT_TAG = 0xB0511
DIR_TAG = 0xB0520
SEED = 0xB0510C0FFEE
MAX_OPS = 4
C = uref.C
CELL_MAX = uref.CELL_MAX
TWO_M32 = 2.0 ** -32
ID_END = (1 << 32) - 1


def request(sigma, g_lo, g_hi, tau, W, dV, m_a, m_b, m3, m4, q_value=0.0, seed=SEED, stream=0, epoch=0, like=False):
    """the host's part of a request: fpic_fusion's numbers, the macro weight and the outcome's numbers"""
    req = uref.request(sigma, g_lo, g_hi, tau, W, dV, seed=seed, stream=stream, epoch=epoch, like=like)
    m_a, m_b, m3, m4 = (float(x) for x in (m_a, m_b, m3, m4))
    M = m_a + m_b
    cc = C * C
    req.update(w=float(W), f_a=m_a / M, f_b=m_b / M, hk=(0.5 * ((m_a * m_b) / M)) * cc, kf=((2.0 * m4) / (m3 * (m3 + m4))) / cc, r34=m3 / m4,
               q_value=float(q_value))
    return req


def keys(req, ids):
    return philox(np.asarray(ids, dtype=np.uint64), req["epoch"], req["stream"], TAG, req["seed_lo"], req["seed_hi"])[0].astype(np.uint64)


def accept_words(req, ids, side_b):
    tag = ACCEPT_TAG + np.asarray(side_b, dtype=np.uint64)
    return philox(np.asarray(ids, dtype=np.uint64), req["epoch"], req["stream"], tag, req["seed_lo"], req["seed_hi"])[0].astype(np.float64)


def odd_cell_pairs(n):
    """the pairs of a like cell of n particles, in like_pair's order, and how many of them can react at most: an even cell has
    n / 2 disjoint pairs; an odd one the triple (s0,s1), (s1,s2), (s2,s0), of which one reacts, and (n - 3) / 2 disjoint pairs
    — 1 + (n - 3) / 2 = (n - 1) / 2 = floor(n / 2) as well"""
    return uref.pairing_like(n), n // 2


def schedule(req, cell_a, ids_a, cell_b=None, ids_b=None, cell_max=CELL_MAX):
    """fusion_reference.schedule with this operator's key, and per pair its chain and its place in it: pairs of one chain share
    a particle, and the accepted one with the lowest place reacts.  Unlike species: chain = the few particle, place = the many
    particle's place in its sorted segment.  Like species: the triple of an odd cell is one chain with the places 0, 1, 2;
    every other pair is a chain of its own.  A chain's name is an integer unique in the application."""
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
    owner, partner, n_l, chain, place = [], [], [], [], []
    cells = overfull_cells = overfull_particles = 0
    chains = 0
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
            table = []
            for k, (o, p, nl) in enumerate(uref.pairing_like(len(a))):
                triple = len(a) % 2 == 1 and k < 3
                table.append((a[o], a[p], nl, chains if triple else chains + 1 + k, k))
            chains += 1 + len(table)
        else:
            many, few = (a, b) if len(a) >= len(b) else (b, a)
            table = [(many[j], few[q], nl, chains + q, j) for j, q, nl in uref.pairing_unlike(len(many), len(few))]
            chains += len(few)
        if not table:
            continue
        cells += 1
        for o, p, nl, ch, pl in table:
            owner.append(o); partner.append(p); n_l.append(nl); chain.append(ch); place.append(pl)
    return dict(owner=np.array(owner, dtype=np.int64), partner=np.array(partner, dtype=np.int64), n_l=np.array(n_l, dtype=np.float64),
                chain=np.array(chain, dtype=np.int64), place=np.array(place, dtype=np.int64),
                cells=cells, overfull_cells=overfull_cells, overfull_particles=overfull_particles, na=na, ids=ids)


def probability(req, n_l, vo, vp):
    """one pair each: (P, what, g); P = 0 outside the table"""
    n_l = np.asarray(n_l, dtype=np.float64)
    ux, uy, uz = vo[:, 0] - vp[:, 0], vo[:, 1] - vp[:, 1], vo[:, 2] - vp[:, 2]
    g = np.sqrt((ux * ux + uy * uy) + uz * uz)
    with np.errstate(invalid="ignore"):
        what = np.where(g < req["g_lo"], 1, np.where(~(g < req["g_hi"]), 2, 0))
    inside = what == 0
    P = np.zeros(len(g), dtype=np.float64)
    if inside.any():
        gi = g[inside]
        sigma = uref.sigma_at(req, gi)
        y = ((((req["ww"] * n_l[inside]) * req["tau"]) / req["dv"])) * (sigma * (gi * C))
        P[inside] = y / req["w"]
    return P, what, g


def resolve(chain, place, accepted):
    """who reacts: of the accepted pairs of a chain the one with the lowest place"""
    reacts = np.zeros(len(chain), dtype=bool)
    least = {}
    for k in np.flatnonzero(accepted):
        c = int(chain[k])
        if c not in least or place[k] < place[least[c]]:
            least[c] = k
    reacts[list(least.values())] = True
    return reacts


def decide(req, cell_a, ids_a, v_a, cell_b=None, ids_b=None, v_b=None, cell_max=CELL_MAX):
    like = req["like"]
    zero = dict(pairs=0, below=0, above=0, cells=0, overfull_cells=0, overfull_particles=0, accepted=0, blocked=0, saturated=0, burnt=0)
    if not req["s_max"] > 0 or len(ids_a) == 0 or (not like and len(ids_b) == 0):      # nothing can react: nothing is launched
        return zero
    plan = schedule(req, cell_a, ids_a, cell_b, ids_b, cell_max)
    v = (np.asarray(v_a) if like else np.concatenate([v_a, v_b])).astype(np.float64)
    P, what, g = probability(req, plan["n_l"], v[plan["owner"]], v[plan["partner"]])
    side_b = (plan["owner"] >= plan["na"]) & (not like)
    u = accept_words(req, plan["ids"][plan["owner"]], side_b)
    accepted = (what == 0) & ((u + 0.5) * TWO_M32 < P)
    reacts = resolve(plan["chain"], plan["place"], accepted)
    return dict(pairs=int((what == 0).sum()), below=int((what == 1).sum()), above=int((what == 2).sum()), cells=plan["cells"],
                overfull_cells=plan["overfull_cells"], overfull_particles=plan["overfull_particles"], accepted=int(accepted.sum()),
                blocked=int((accepted & ~reacts).sum()), saturated=int((accepted & (P >= 1.0)).sum()), burnt=int(reacts.sum()),
                plan=plan, P=P, what=what, g=g, u=u, is_accepted=accepted, reacts=reacts, side_b=side_b)


def directions(req, ids):
    """the isotropic directions of the events whose species_a reactants have the ids `ids`: n (m, 3) and the try that was taken"""
    ids = np.asarray(ids, dtype=np.uint64)
    n = np.tile(np.array([0.0, 0.0, 1.0]), (len(ids), 1))
    tries = np.full(len(ids), sref.TRIES, dtype=np.int64)
    for a in range(sref.BLOCKS):
        w = philox(ids, req["epoch"], req["stream"], DIR_TAG + a, req["seed_lo"], req["seed_hi"])
        for t, (wa, wb) in enumerate(((w[0], w[1]), (w[2], w[3]))):
            ok, cand = sref.try_direction(wa, wb)
            take = ok & (tries == sref.TRIES)
            n[take] = cand[take]
            tries[take] = 2 * a + t
    return n, tries


def outcome(req, va, vb, n):
    """one event each: float64 (m, 3) stored velocities of the species_a and species_b reactants and the direction; (w3, w4, K)"""
    ux, uy, uz = va[:, 0] - vb[:, 0], va[:, 1] - vb[:, 1], va[:, 2] - vb[:, 2]
    g = np.sqrt((ux * ux + uy * uy) + uz * uz)
    K = req["hk"] * (g * g)
    et = req["q_value"] + K
    et = np.where(et > 0, et, 0.0)
    u3 = np.sqrt(et * req["kf"])
    u4 = req["r34"] * u3
    V = np.stack([req["f_a"] * va[:, i] + req["f_b"] * vb[:, i] for i in range(3)], axis=1)
    w3 = np.stack([V[:, i] + u3 * n[:, i] for i in range(3)], axis=1)
    w4 = np.stack([V[:, i] - u4 * n[:, i] for i in range(3)], axis=1)
    return w3, w4, K, V


def fits(n, capacity, id_span, count):
    return n + count <= capacity and id_span + count <= ID_END


def application(req, A, B, n3, span3, n4=0, span4=0, tracked_b=True, cell_max=CELL_MAX):
    """One application to stored arrays.  Returns decide()'s keys and
        m                   the events
        keep_a, keep_b      boolean masks over the rows of A and B: who stays (like species: keep_b is None)
        product_a, product_b    dict(slot, id, position, velocity) of the new rows by event number, stored values of the dtype
                            (product_b not tracked: velocity is the float64 w4, no slot and id)
        lost_a, lost_b, gain_a, gain_b    the exact sums: dict(energy_fixed, momentum_fixed, nan, count)"""
    like = req["like"]
    dtype = np.asarray(A["vel"]).dtype
    out = decide(req, A["cell"], A["ids"], A["vel"], None if like else B["cell"], None if like else B["ids"], None if like else B["vel"], cell_max)
    na = len(A["ids"])
    keep_a = np.ones(na, dtype=bool)
    keep_b = None if like else np.ones(len(B["ids"]), dtype=bool)
    empty = np.zeros((0, 3), dtype=dtype)
    if "plan" not in out or out["burnt"] == 0:
        zero = lambda: dict(iref.gain(empty), count=0)
        out.update(m=0, keep_a=keep_a, keep_b=keep_b, lost_a=zero(), lost_b=zero(), gain_a=zero(), gain_b=zero(),
                   product_a=dict(slot=np.zeros(0, dtype=np.int64), id=np.zeros(0, dtype=np.int64), position=empty, velocity=empty),
                   product_b=dict(slot=np.zeros(0, dtype=np.int64), id=np.zeros(0, dtype=np.int64), position=empty, velocity=empty))
        return out
    plan = out["plan"]
    who = np.flatnonzero(out["reacts"])
    o, p = plan["owner"][who], plan["partner"][who]
    if like:
        ra, rb = o, p                                   # owner, partner
        pos_b, vel_b = np.asarray(A["pos"]), np.asarray(A["vel"])
    else:
        ra, rb = np.where(o < na, o, p), np.where(o < na, p, o) - na
        pos_b, vel_b = np.asarray(B["pos"]), np.asarray(B["vel"])
    ids_a = np.asarray(A["ids"], dtype=np.int64)
    by_id = np.argsort(ids_a[ra], kind="stable")       # the events in ascending id of their species_a reactant
    ra, rb = ra[by_id], rb[by_id]
    assert len(set(ra.tolist())) == len(ra) and len(set(rb.tolist())) == len(rb) and (not like or not set(ra.tolist()) & set(rb.tolist()))
    m = len(ra)
    va, vb = np.asarray(A["vel"])[ra].astype(np.float64), vel_b[rb].astype(np.float64)
    n, tries = directions(req, ids_a[ra])
    w3, w4, K, V = outcome(req, va, vb, n)
    keep_a[ra] = False
    if like:
        keep_a[rb] = False
    else:
        keep_b[rb] = False
    prod_a = dict(slot=n3 + np.arange(m), id=span3 + np.arange(m), position=np.asarray(A["pos"])[ra], velocity=w3.astype(dtype))
    prod_b = dict(slot=n4 + np.arange(m), id=span4 + np.arange(m), position=pos_b[rb], velocity=w4.astype(dtype) if tracked_b else w4)
    out.update(m=m, keep_a=keep_a, keep_b=keep_b, product_a=prod_a, product_b=prod_b, event_a=ra, event_b=rb, n=n, tries=tries, w3=w3, w4=w4, K=K, V=V,
               lost_a=dict(iref.gain(np.asarray(A["vel"])[~keep_a]), count=int((~keep_a).sum())),
               lost_b=dict(iref.gain(empty if like else vel_b[~keep_b]), count=0 if like else int((~keep_b).sum())),
               gain_a=dict(iref.gain(prod_a["velocity"]), count=m), gain_b=dict(iref.gain(prod_b["velocity"]), count=m))
    return out


def conditions_hold(out):
    """the conditions of an exact comparison: the rule has no transcendental and no threshold that a last-bit difference could
    cross differently — the library computes the same double operations —, so the only conditions are those the reference's own
    shortcuts need: no direction took the fallback, and no tally term left the fixed-point range"""
    if out.get("m", 0) == 0:
        return True
    nan = any(any(out[k]["nan"]) for k in ("lost_a", "lost_b", "gain_a", "gain_b"))
    return not (out["tries"] == sref.TRIES).any() and not nan
