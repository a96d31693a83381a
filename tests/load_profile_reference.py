"""The rule of a profiled load (fpic_load_profile) restated in plain numpy, from the text of include/fusionpic.h and DESIGN.md
4.20, on top of tests/load_reference.py (the words, the normals, the displacement, the wrap).  It shares no code with the
product: the cumulative masses are summed by a Python loop, the interval is found by numpy's searchsorted (the product
bisects), everything else is float64 in the stated operation order.

    req = request(L, density=(None, None, [0, 1, 0]), thermal=..., shear=dict(axis=, component=, values=), seed=..., ...)
    warp(d, f)                               f -> (f', j, s) through one density table
    stored_positions(req, i, np.float32)     what a handle of that precision holds for the particle indices i
    velocities(req, i)"""
import numpy as np

import load_reference as ref

BELOW_ONE = 1.0 - 2.0 ** -53


def cumulative(d):
    """C[0] = 0, C[j+1] = C[j] + 0.5 (d[j] + d[j+1]), in sequence"""
    d = np.asarray(d, dtype=np.float64)
    C = np.zeros(d.size, dtype=np.float64)
    for j in range(d.size - 1):
        C[j + 1] = C[j] + np.float64(0.5) * (d[j] + d[j + 1])
    return C


def warp(d, f, C=None):
    """the fractions f (float64 array) through the density table d -> (f', j, s)"""
    d = np.asarray(d, dtype=np.float64) + 0.0
    f = np.asarray(f, dtype=np.float64)
    C = cumulative(d) if C is None else C
    K = d.size - 1
    t = f * C[K]
    j = np.minimum(np.searchsorted(C, t, side="right") - 1, K - 1)      # the largest index with C[j] <= t, held to K - 1
    r = t - C[j]
    disc = d[j] * d[j] + (2.0 * (d[j + 1] - d[j])) * r
    disc = np.where(disc < 0.0, 0.0, disc)
    den = d[j] + np.sqrt(disc)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den > 0.0, (2.0 * r) / den, 0.0)
    s = np.where(s > 1.0, 1.0, s)
    fq = (j.astype(np.float64) + s) / np.float64(K)
    fq = np.where(fq < 1.0, fq, BELOW_ONE)
    return fq, j, s


def lookup(tab, f):
    """the value of a table at the fractions f of its axis -> (value, j, s)"""
    tab = np.asarray(tab, dtype=np.float64)
    K = tab.size - 1
    g = np.asarray(f, dtype=np.float64) * np.float64(K)
    j = np.minimum(g.astype(np.int64), K - 1)
    s = g - j.astype(np.float64)
    return tab[j] + (tab[j + 1] - tab[j]) * s, j, s


def request(L, density=None, thermal=None, shear=None, **kw):
    """load_reference.request with the tables beside it"""
    req = ref.request(L, **kw)
    req["density"] = [None if t is None else np.asarray(t, dtype=np.float64) + 0.0 for t in (density or [None] * 3)]
    req["thermal"] = [None if t is None else np.asarray(t, dtype=np.float64) + 0.0 for t in (thermal or [None] * 3)]
    req["shear"] = None if shear is None else dict(axis=int(shear["axis"]), component=int(shear["component"]), values=np.asarray(shear["values"], dtype=np.float64))
    return req


def fractions(req, i):
    """f'[n][3] and the intervals j[n][3] (-1 on an axis without a density table)"""
    f = ref.fractions(req, i)
    j = np.full(f.shape, -1, dtype=np.int64)
    for a in range(3):
        if req["density"][a] is not None:
            f[:, a], j[:, a], _ = warp(req["density"][a], f[:, a])
    return f, j


def base(req, i):
    """the undisplaced positions p[n][3] (box fractions), the phase theta[n] (turns) and the fractions f'[n][3]"""
    f, _ = fractions(req, i)
    t = f * req["w_f"]
    p = req["lo_f"] + t
    theta = (req["m"][0] * p[:, 0] + req["m"][1] * p[:, 1]) + req["m"][2] * p[:, 2]
    return p, theta, f


def positions(req, i):
    p, theta, _ = base(req, i)
    return ref._displaced(req, p, theta)


def stored_positions(req, i, dtype):
    return ref.wrap01(positions(req, i).astype(dtype))


def vth_eff(req, f):
    """[n][3]: ((vth[a] sx) sy) sz, a missing table no multiply"""
    v = np.broadcast_to(req["vth"], f.shape).copy()
    for b in range(3):
        if req["thermal"][b] is not None:
            v = v * lookup(req["thermal"][b], f[:, b])[0][:, None]
    return v


def drift_eff(req, f):
    d = np.broadcast_to(req["drift"], f.shape).copy()
    if req["shear"] is not None:
        sh = req["shear"]
        d[:, sh["component"]] = d[:, sh["component"]] + lookup(sh["values"], f[:, sh["axis"]])[0]
    return d


def velocities(req, i):
    """float64 velocities in units of c"""
    i = np.asarray(i, dtype=np.uint64)
    p, theta, f = base(req, i)
    th = vth_eff(req, f) * ref.normals(req, i)
    if req["paired"]:
        th = np.where(((i & np.uint64(1)) == 1)[:, None], -th, th)
    v = drift_eff(req, f) + th
    if np.any(req["vamp"] != 0):
        return v + req["vamp"] * ref.sinpi(2.0 * (theta + req["vphase"]))[:, None]
    return v + 0.0


def stored_velocities(req, i, dtype):
    return velocities(req, i).astype(dtype)
