"""The rule of the windowed background collisions with a tabulated cross-section (fpic_gas) restated in plain numpy, from
the text of include/fusionpic.h and DESIGN.md 4.23.  It shares no code with the library.  The partner, the direction and the
updates are the formulas of tests/collide_reference.py on this operator's own Philox words, the window, the tapers and the exact
tallies those of tests/force_reference.py, the table lookup that of tests/fusion_reference.py; everything else is float64
in the stated operation order (numpy never fuses a multiply with an add), and the host-side numbers use math.expm1 and
math.ldexp, the libm the library calls.

    req = request(L, kind, density=, tau=, sigma=, g_lo=, g_hi=, drift=, vth=, mass_ratio=, lo=, hi=, taper=, seed=, stream=, epoch=)
    out = apply(req, ids, position, v)      position: the stored box fractions, v: the stored velocities, as float64 (n, 3)
    out["v"]           the new velocities in double (cast them to the handle's precision: stored())
    out["inside"], out["candidate"], out["collided"], out["below"], out["above"]     boolean masks over the particles
    out["g"], out["x"], out["ux"]                                                     the acceptance's numbers
    counts(out), tallies(before, after, collided), derived(t, mass, W)
"""
import math

import numpy as np

import force_reference as fref
import fusion_reference as uref
from load_reference import cospi, philox, sinpi

TAG = 0x6A500
EXCHANGE, ELASTIC = 0, 1
MAX_OPS, TABLE_MAX, TAPER_MAX = 8, 4096, 1025
SEED = 0x6A5C0111DE
C = 2.998e8
TWO_M32 = 2.0 ** -32


def _three(v):
    return np.array([v, v, v] if np.ndim(v) == 0 else list(v), dtype=np.float64)


def bound(S, g_lo, g_hi):
    """max_k b_k: b_k = max(S[k], S[k+1]) g_{k+1}, g_{k+1} = g_lo + (k+1) dg, the last interval with g_hi"""
    S = np.asarray(S, dtype=np.float64)
    n = len(S)
    dg = np.float64(g_hi - g_lo) / np.float64(n - 1)
    g1 = np.float64(g_lo) + np.arange(1, n, dtype=np.float64) * dg
    g1[-1] = g_hi
    return float(np.max(np.maximum(S[:-1], S[1:]) * g1))


def request(L, kind, density, tau, sigma, g_lo, g_hi, drift=0.0, vth=0.0, mass_ratio=None, lo=None, hi=None, taper=(None, None, None),
            seed=SEED, stream=0, epoch=0):
    """the host's part of a request (rule_of)"""
    L = _three(L)
    lo = np.zeros(3) if lo is None else _three(lo)
    hi = L.copy() if hi is None else _three(hi)
    S = np.array(sigma, dtype=np.float64)
    g_lo, g_hi, density, tau = float(g_lo), float(g_hi), float(density), float(tau)
    column = (density * C) * tau
    x_max = column * bound(S, g_lo, g_hi)
    p_max = -math.expm1(-x_max)
    K = int(math.ldexp(p_max, 32))
    if mass_ratio is None:
        mass_ratio = math.inf if kind == ELASTIC else 0.0
    M = 1.0 if math.isinf(mass_ratio) else mass_ratio / (1.0 + mass_ratio)
    lo_f, hi_f = lo / L, hi / L
    table = dict(S=S, n=len(S), g_lo=g_lo, g_hi=g_hi, inv_dg=float(len(S) - 1) / (g_hi - g_lo), s_max=float(S.max()))
    window = dict(lo_f=lo_f, hi_f=hi_f, w=hi_f - lo_f, taper=[None if t is None else np.asarray(t, dtype=np.float64) for t in taper])
    return dict(kind=kind, column=column, x_max=x_max, p_max=p_max, K=K, M=M, drift=_three(drift), vth=_three(vth), table=table, window=window,
                seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32, stream=stream, epoch=epoch & 0xFFFFFFFF)


def words(req, ids, block):
    """W(block) of the particles: four uint32 arrays"""
    return philox(np.asarray(ids, dtype=np.uint64), req["epoch"], req["stream"], TAG + block, req["seed_lo"], req["seed_hi"])


def normals(req, ids):
    """the partner's normals n[n][3]: collide_reference.normals on this operator's W(1)"""
    w = [x.astype(np.float64) for x in words(req, ids, 1)]
    r1 = np.sqrt(-2.0 * np.log((w[0] + 0.5) * TWO_M32))
    r3 = np.sqrt(-2.0 * np.log((w[2] + 0.5) * TWO_M32))
    u2, u4 = w[1] * TWO_M32, w[3] * TWO_M32
    return np.stack([r1 * cospi(2.0 * u2), r1 * sinpi(2.0 * u2), r3 * cospi(2.0 * u4)], axis=1)


def partner(req, ids):
    return req["drift"] + req["vth"] * normals(req, ids)


def direction(req, ids):
    """nhat[n][3] of ELASTIC: collide_reference.direction on this operator's W(0)"""
    w = words(req, ids, 0)
    c = 1.0 - 2.0 * ((w[2].astype(np.float64) + 0.5) * TWO_M32)
    s = np.sqrt(1.0 - c * c)
    phi2 = 2.0 * (w[3].astype(np.float64) * TWO_M32)
    return np.stack([s * cospi(phi2), s * sinpi(phi2), c], axis=1)


def drawn(req, ids):
    return words(req, ids, 0)[0].astype(np.uint64) < np.uint64(req["K"]) if req["K"] < 1 << 32 else np.ones(len(np.atleast_1d(ids)), dtype=bool)


def apply(req, ids, position, v):
    """the whole rule for live particles `ids` at the stored fractions `position` with velocities v (float64 (n, 3))"""
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
    u = (words(req, ids, 0)[1].astype(np.float64) + 0.5) * TWO_M32
    ux = u * req["x_max"]
    hit = cand & live & (ux < x)
    if req["kind"] == EXCHANGE:
        new = vb
    else:
        t = g[:, None] * direction(req, ids)
        r = d - t
        q = req["M"] * r
        new = v - q
    out = v.copy()
    out[hit] = new[hit]
    return dict(v=out, inside=inside, candidate=cand, collided=hit, below=below, above=above, g=g, x=x, ux=ux, live=live, sigma=sigma, rho=rho)


def stored(req, ids, position, v_stored):
    """what a handle holding v_stored (float32 or float64 (n, 3)) holds afterwards: the masks of apply() and `v` in that type;
    a particle that does not collide keeps its bits"""
    out = apply(req, ids, position, v_stored.astype(np.float64))
    new = v_stored.copy()
    hit = out["collided"]
    new[hit] = out["v"][hit].astype(v_stored.dtype)
    out["v"] = new
    return out


def counts(out):
    return dict(candidates=int(out["candidate"].sum()), collided=int(out["collided"].sum()), below=int(out["below"].sum()), above=int(out["above"].sum()))


def tallies(before, after, collided):
    """the exact tallies of one application from the stored velocities before and after it and who collided (the forces')"""
    t = fref.tallies(before, after, collided)
    return dict(collided=t["kicked"], energy_fixed=t["work_fixed"], momentum_fixed=t["impulse_fixed"])


def derived(t, mass, W):
    d = fref.derived(dict(work_fixed=t["energy_fixed"], impulse_fixed=t["momentum_fixed"]), mass, W)
    return dict(energy=d["work"], momentum=d["impulse"])


def add_tallies(a, b):
    return dict(collided=a["collided"] + b["collided"], energy_fixed=a["energy_fixed"] + b["energy_fixed"],
                momentum_fixed=[x + y for x, y in zip(a["momentum_fixed"], b["momentum_fixed"])])


ZERO = dict(collided=0, energy_fixed=0, momentum_fixed=[0, 0, 0])
