"""The rule of the Monte Carlo collision operator (fpic_collide) restated in plain numpy, from the text of
include/fusionpic.h and DESIGN.md 4.16.  It shares no code with the library: Philox4x32-10 and the circular functions are
those of load_reference.py, everything else is float64 in the stated operation order (numpy never fuses a multiply with an
add), and the host-side numbers use math.exp / math.expm1 / math.sqrt, the libm the library calls.

    req = request(kind, nu_tau=..., sigma_tau=..., g_max=..., drift=..., vth=..., mass_ratio=..., seed=..., stream=..., epoch=...)
    out = apply(req, ids, v)        v: float64 (n, 3), the stored velocities converted to double
    out["v"]          the new velocities in double (cast them to the handle's precision: stored())
    out["candidate"], out["collided"], out["clipped"]     boolean masks over the particles
"""
import math

import numpy as np

from load_reference import cospi, philox, sinpi

TAG = 0xC0110
EXCHANGE, ELASTIC, RELAX = 0, 1, 2
SEED = 0xC0111DE5
TWO_M32 = 2.0 ** -32


def _three(v):
    return np.array([v, v, v] if np.ndim(v) == 0 else list(v), dtype=np.float64)


def request(kind, nu_tau=0.0, sigma_tau=0.0, g_max=0.0, drift=0.0, vth=0.0, mass_ratio=None, seed=SEED, stream=0, epoch=0):
    """the host's part of a request (rule_of)"""
    nu_tau, sigma_tau, g_max = float(nu_tau), float(sigma_tau), float(g_max)
    x_max = nu_tau + sigma_tau * g_max
    p_max = -math.expm1(-x_max)
    K = 1 << 32 if math.isinf(x_max) else int(math.ldexp(p_max, 32))
    if mass_ratio is None:
        mass_ratio = math.inf if kind == ELASTIC else 0.0
    M = 1.0 if math.isinf(mass_ratio) else mass_ratio / (1.0 + mass_ratio)
    vth = _three(vth)
    spread = math.sqrt(-math.expm1(-2.0 * nu_tau))
    return dict(kind=kind, nu_tau=nu_tau, sigma_tau=sigma_tau, g_max=g_max, x_max=x_max, p_max=p_max, K=K, M=M, drift=_three(drift), vth=vth,
                decay=math.exp(-nu_tau), sv=spread * vth, seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32, stream=stream, epoch=epoch & 0xFFFFFFFF)


def words(req, ids, block):
    """W(block) of the particles: four uint32 arrays"""
    return philox(np.asarray(ids, dtype=np.uint64), req["epoch"], req["stream"], TAG + block, req["seed_lo"], req["seed_hi"])


def normals(req, ids):
    """the partner's normals n[n][3]: the loader's Box-Muller formulas on W(1)"""
    w = [x.astype(np.float64) for x in words(req, ids, 1)]
    r1 = np.sqrt(-2.0 * np.log((w[0] + 0.5) * TWO_M32))
    r3 = np.sqrt(-2.0 * np.log((w[2] + 0.5) * TWO_M32))
    u2, u4 = w[1] * TWO_M32, w[3] * TWO_M32
    return np.stack([r1 * cospi(2.0 * u2), r1 * sinpi(2.0 * u2), r3 * cospi(2.0 * u4)], axis=1)


def candidates(req, ids):
    return words(req, ids, 0)[0].astype(np.uint64) < np.uint64(req["K"]) if req["K"] < 1 << 32 else np.ones(len(np.atleast_1d(ids)), dtype=bool)


def direction(req, ids):
    """nhat[n][3] of ELASTIC"""
    w = words(req, ids, 0)
    c = 1.0 - 2.0 * ((w[2].astype(np.float64) + 0.5) * TWO_M32)
    s = np.sqrt(1.0 - c * c)
    phi2 = 2.0 * (w[3].astype(np.float64) * TWO_M32)
    return np.stack([s * cospi(phi2), s * sinpi(phi2), c], axis=1)


def partner(req, ids):
    return req["drift"] + req["vth"] * normals(req, ids)


def acceptance(req, ids, g):
    """(x, u x_max) of the null-collision test for relative speeds g"""
    x = req["nu_tau"] + req["sigma_tau"] * np.minimum(g, req["g_max"])
    u = (words(req, ids, 0)[1].astype(np.float64) + 0.5) * TWO_M32
    return x, u * req["x_max"]


def apply(req, ids, v):
    """the whole rule for live particles `ids` with velocities v (float64 (n, 3))"""
    ids = np.asarray(ids, dtype=np.uint64)
    v = np.asarray(v, dtype=np.float64)
    n = len(ids)
    out = v.copy()
    none = np.zeros(n, dtype=bool)
    if req["kind"] == RELAX:
        r = v - req["drift"]
        p = req["decay"] * r
        k = req["sv"] * normals(req, ids)
        q = p + k
        return dict(v=req["drift"] + q, candidate=none, collided=~none, clipped=none.copy(), g=None)
    cand = candidates(req, ids)
    vb = partner(req, ids)
    d = v - vb
    g = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    if req["sigma_tau"] == 0:
        hit, clipped = cand.copy(), none.copy()
    else:
        x, ux = acceptance(req, ids, g)
        hit, clipped = cand & (ux < x), cand & (g > req["g_max"])
    if req["kind"] == EXCHANGE:
        new = vb
    else:
        t = g[:, None] * direction(req, ids)
        r = d - t
        q = req["M"] * r
        new = v - q
    out[hit] = new[hit]
    return dict(v=out, candidate=cand, collided=hit, clipped=clipped, g=g)


def stored(req, ids, v_stored):
    """what a handle holding v_stored (float32 or float64 (n, 3)) holds afterwards: the masks of apply() and `v` in that type;
    a particle that does not collide keeps its bits"""
    out = apply(req, ids, v_stored.astype(np.float64))
    new = v_stored.copy()
    hit = out["collided"]
    new[hit] = out["v"][hit].astype(v_stored.dtype)
    out["v"] = new
    return out
