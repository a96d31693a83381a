"""The rule of the electron-impact ionisation of a background gas (fpic_ionize) restated in plain numpy and Python integers,
from the text of include/fusionpic.h and DESIGN.md 4.28.  It shares no code with the library.  The host-side numbers, the
window, the tapers and the table lookup are those of tests/gas_reference.py (force_reference, fusion_reference), the exact
sums those of tests/force_reference.py (the primary's before/after terms) and tests/remove_reference.py (what a target
gained); the words are this operator's own (tag 0x1051E0).  Everything else is float64 in the stated operation order.

    req = request(L, g_threshold=, density=, tau=, sigma=, g_lo=, g_hi=, drift=, vth=, lo=, hi=, taper=, seed=, stream=, epoch=)
    out = apply(req, ids, position, v)        position: the stored box fractions, v: the stored velocities, as float64 (n, 3)
    out["candidate"], out["event"], out["below"], out["above"]    boolean masks over the particles
    out["vb"], out["g"], out["x"], out["ux"], out["v1"], out["vs"]  the partner, the acceptance's numbers, the outcome (double)
    app = application(req, ids, position, v_stored, n_e, span_e, n_i, span_i)   one application on stored arrays of a dtype
"""
import numpy as np

import energy_reference as eref
import force_reference as fref
import fusion_reference as uref
import gas_reference as gref
import remove_reference as rref
from load_reference import cospi, philox, sinpi

TAG = 0x1051E0
MAX_OPS = 8
SEED = 0x1051E0C0FFEE
TWO_M32 = 2.0 ** -32
ID_END = (1 << 32) - 1


def request(L, g_threshold, density, tau, sigma, g_lo, g_hi, drift=0.0, vth=0.0, lo=None, hi=None, taper=(None, None, None), seed=SEED, stream=0,
            epoch=0, species=0, electron=None, ion=None):
    """the host's part of a request: the gas operator's numbers (column, x_max, K, the table, the window) and the threshold"""
    req = gref.request(L, gref.EXCHANGE, density, tau, sigma, g_lo, g_hi, drift, vth, None, lo, hi, taper, seed, stream, epoch)
    req["thr"] = float(g_threshold)
    return req


def words(req, ids, block):
    """W(block) of the projectiles: four uint32 arrays"""
    return philox(np.asarray(ids, dtype=np.uint64), req["epoch"], req["stream"], TAG + block, req["seed_lo"], req["seed_hi"])


def normals(req, ids):
    w = [x.astype(np.float64) for x in words(req, ids, 1)]
    r1 = np.sqrt(-2.0 * np.log((w[0] + 0.5) * TWO_M32))
    r3 = np.sqrt(-2.0 * np.log((w[2] + 0.5) * TWO_M32))
    u2, u4 = w[1] * TWO_M32, w[3] * TWO_M32
    return np.stack([r1 * cospi(2.0 * u2), r1 * sinpi(2.0 * u2), r3 * cospi(2.0 * u4)], axis=1)


def partner(req, ids):
    return req["drift"] + req["vth"] * normals(req, ids)


def nhat(wc, wp):
    """ELASTIC's direction on two words"""
    c = 1.0 - 2.0 * ((wc.astype(np.float64) + 0.5) * TWO_M32)
    s = np.sqrt(1.0 - c * c)
    phi2 = 2.0 * (wp.astype(np.float64) * TWO_M32)
    return np.stack([s * cospi(phi2), s * sinpi(phi2), c], axis=1)


def share(req, ids):
    return (words(req, ids, 2)[0].astype(np.float64) + 0.5) * TWO_M32


def drawn(req, ids):
    return words(req, ids, 0)[0].astype(np.uint64) < np.uint64(req["K"]) if req["K"] < 1 << 32 else np.ones(len(np.atleast_1d(ids)), dtype=bool)


def apply(req, ids, position, v):
    """the decisions and the outcomes for live projectiles `ids` at the stored fractions `position` with velocities v"""
    ids = np.asarray(ids, dtype=np.uint64)
    p = np.asarray(position).astype(np.float64)
    v = np.asarray(v, dtype=np.float64)
    n = len(ids)
    inside = fref.inside(req["window"], p)
    cand = inside & drawn(req, ids)
    vb = partner(req, ids)
    d = v - vb
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    tab = req["table"]
    below, above = cand & (g < tab["g_lo"]), cand & ~(g < tab["g_hi"])
    live = ~(g < tab["g_lo"]) & (g < tab["g_hi"])
    sigma = np.zeros(n)
    sigma[live] = uref.sigma_at(tab, g[live])
    rho, _ = fref.taper_value(req["window"], p)
    cr = np.full(n, req["column"]) if rho is None else req["column"] * rho
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.minimum((cr * sigma) * g, req["x_max"])
    w0 = words(req, ids, 0)
    u = (w0[1].astype(np.float64) + 0.5) * TWO_M32
    ux = u * req["x_max"]
    event = cand & live & (ux < x)
    w2 = words(req, ids, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        gp2 = g * g - req["thr"] * req["thr"]
        a1 = share(req, ids) * gp2
        a2 = gp2 - a1
        g1, g2 = np.sqrt(a1), np.sqrt(a2)
        v1 = vb + g1[:, None] * nhat(w0[2], w0[3])
        vs = vb + g2[:, None] * nhat(w2[1], w2[2])
    return dict(inside=inside, candidate=cand, event=event, below=below, above=above, live=live, g=g, x=x, ux=ux, vb=vb, v1=v1, vs=vs, gp2=gp2, g1=g1, g2=g2)


def counts(out):
    return dict(candidates=int(out["candidate"].sum()), below=int(out["below"].sum()), above=int(out["above"].sum()), ionised=int(out["event"].sum()))


def ranks(ids, event):
    """the rank of every event: the number of events whose primary has a smaller id (-1 where there is no event)"""
    ids = np.asarray(ids, dtype=np.int64)
    rank = np.full(len(ids), -1, dtype=np.int64)
    who = np.flatnonzero(event)
    rank[who[np.argsort(ids[who], kind="stable")]] = np.arange(len(who))
    return rank


def fits(n, capacity, id_span, count):
    return n + count <= capacity and id_span + count <= ID_END


def gain(vel):
    """what a target gained by the rows `vel` (stored values): energy_fixed, momentum_fixed as Python integers, and which sum
    met a term outside the range"""
    v = np.asarray(vel).astype(np.float64).reshape(-1, 3)
    cols = [eref.v_squared(v), v[:, 0], v[:, 1], v[:, 2]]
    if all(np.all(np.abs(c) < rref.FIX_RANGE) for c in cols):          # (the common case, vectorised: the same integers)
        sums, nan = [eref.fix_sum(c) for c in cols], [False] * 4
    else:
        sums, nan = rref.tally(v, np.ones(len(v), dtype=bool))
    return dict(energy_fixed=sums[0], momentum_fixed=list(sums[1:]), nan=list(nan))


def derived(g, count, mass, charge, W):
    """the doubles of a group as the library forms them"""
    ke, pm = 0.5 * mass * W * rref.C * rref.C, mass * W * rref.C
    nan = g.get("nan", [False] * 4)
    return dict(energy=float("nan") if nan[0] else ke * rref.fixed_to_double(g["energy_fixed"]),
                momentum=[float("nan") if nan[1 + a] else pm * rref.fixed_to_double(g["momentum_fixed"][a]) for a in range(3)],
                charge=(float(count) * charge) * W)


def application(req, ids, position, v_stored, n_e, span_e, n_i, span_i, known=None):
    """One application to a projectile species whose stored arrays are position, v_stored (of the handle's dtype, (n, 3)) with
    ids `ids`; n_e, span_e, n_i, span_i: the targets' populations and id spans before it.  Returns the masks of apply(), and
        v          the projectile species' stored velocities afterwards
        rank       per projectile the rank of its event or -1
        electron, ion   dict(slot, id, position, velocity) of the new rows, by rank: stored values of the dtype
        primary    the projectile species' exact gains (before / after), electron_gain, ion_gain the targets'
    known: what apply() has given for exactly these arguments, if it has been computed already"""
    dtype = v_stored.dtype
    out = dict(known) if known is not None else apply(req, ids, position, v_stored.astype(np.float64))
    ev = out["event"]
    rank = ranks(ids, ev)
    order = np.flatnonzero(ev)[np.argsort(rank[ev], kind="stable")]
    new = v_stored.copy()
    new[ev] = out["v1"][ev].astype(dtype)
    m = len(order)
    pos = np.asarray(position).astype(dtype)[order]
    out.update(v=new, rank=rank, m=m,
               electron=dict(slot=n_e + np.arange(m), id=span_e + np.arange(m), position=pos, velocity=out["vs"][order].astype(dtype)),
               ion=dict(slot=n_i + np.arange(m), id=span_i + np.arange(m), position=pos, velocity=out["vb"][order].astype(dtype)))
    t = fref.tallies(v_stored, new, ev)
    out["primary"] = dict(energy_fixed=t["work_fixed"], momentum_fixed=t["impulse_fixed"])
    out["electron_gain"] = gain(out["electron"]["velocity"])
    out["ion_gain"] = gain(out["ion"]["velocity"])
    return out


def margins_hold(req, out):
    """the conditions of an exact comparison: no candidate within 1e-9 x_max of its acceptance threshold, none within 1e-9 of an
    end of the table or of g_threshold"""
    c = out["candidate"]
    tab = req["table"]
    near_accept = np.abs(out["ux"] - out["x"])[c & out["live"]] < 1e-9 * req["x_max"]
    g = out["g"][c]
    near_end = (np.abs(g - tab["g_lo"]) < 1e-9) | (np.abs(g - tab["g_hi"]) < 1e-9) | (np.abs(g - req["thr"]) < 1e-9)
    return not near_accept.any() and not near_end.any()
