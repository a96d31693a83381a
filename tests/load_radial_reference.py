"""The rule of a radial load (fpic_load_radial) restated in plain numpy, from the text of include/fusionpic.h, on top of
tests/load_reference.py (the words, the normals, the displacement, the wrap) and the look-up of
tests/load_profile_reference.py.  It shares no code with the product: the cumulative masses are summed by a Python loop, the
interval is found by numpy's searchsorted (the product bisects), the halvings run on whole arrays, everything is float64 in
the stated operation order.

    req = request(L, geometry="sphere", center=, r_max=, axis=0, density=, thermal=, flow_radial=, flow_azimuthal=, flow_axial=, seed=..., ...)
    radius(geometry, d, f)                   f -> (rho, j, s) through one density table
    stored_positions(req, i, np.float32)     what a handle of that precision holds for the particle indices i
    velocities(req, i)

`variant` selects one of four deliberately WRONG rules (tests/test_load_radial_reference.py shows that each fails one of its
tests)."""
import numpy as np

import load_profile_reference as pref
import load_reference as ref

BELOW_ONE = 1.0 - 2.0 ** -53
VARIANTS = ("weight_rho", "halvings_51", "thermal_displaced", "theta_hat_sign")
F = np.float64


def coefficients(geometry, d0, d1, j):
    """a1 .. a4 of M_j (arrays or scalars); the cylinder has no a4"""
    D, J = d1 - d0, np.asarray(j, dtype=F)
    if geometry == "sphere":
        JJ = J * J
        return d0 * JJ, d0 * J + F(0.5) * (D * JJ), (d0 + (F(2.0) * J) * D) / F(3.0), F(0.25) * D
    return d0 * J, F(0.5) * (d0 + D * J), D / F(3.0), None


def mass(geometry, a, s):
    a1, a2, a3, a4 = a
    h = a3 + a4 * s if geometry == "sphere" else a3
    return (a1 + (a2 + h * s) * s) * s


def cumulative(geometry, d):
    """C[0] = 0, C[j+1] = C[j] + M_j(1), in sequence"""
    d = np.asarray(d, dtype=F)
    C = np.zeros(d.size, dtype=F)
    for j in range(d.size - 1):
        C[j + 1] = C[j] + mass(geometry, coefficients(geometry, d[j], d[j + 1], j), F(1.0))
    return C


def radius(geometry, d, f, variant=None):
    """the fractions f (float64 array) through the density table d -> (rho, j, s)"""
    law = "cylinder" if variant == "weight_rho" else geometry
    d = np.asarray(d, dtype=F) + 0.0
    f = np.asarray(f, dtype=F)
    C = cumulative(law, d)
    K = d.size - 1
    t = f * C[K]
    j = np.minimum(np.searchsorted(C, t, side="right") - 1, K - 1)
    r = t - C[j]
    a = coefficients(law, d[j], d[j + 1], j)
    lo, hi = np.zeros(f.shape), np.ones(f.shape)
    for _ in range(51 if variant == "halvings_51" else 52):
        mid = F(0.5) * (lo + hi)
        below = mass(law, a, mid) <= r
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    s = lo
    rho = (j.astype(F) + s) / F(K)
    return np.where(rho < 1.0, rho, BELOW_ONE), j, s


def request(L, geometry, center, r_max, axis=0, density=None, thermal=None, flow_radial=None, flow_azimuthal=None, flow_axial=None, **kw):
    """load_reference.request with the body beside it"""
    req = ref.request(L, **kw)
    L = ref._three(L)
    tab = lambda t: None if t is None else np.asarray(t, dtype=F) + 0.0
    req.update(geometry=geometry, axis=int(axis), c_f=ref._three(center) / L, rl=F(r_max) / L, density=np.ones(2) if density is None else tab(density),
               thermal=tab(thermal), flow_radial=tab(flow_radial), flow_azimuthal=tab(flow_azimuthal), flow_axial=tab(flow_axial))
    return req


def parts(req, i, variant=None):
    """dict of per-particle float64 arrays: f[n][3], rho, j, s, dir[n][3]; the sphere also mu, q"""
    f = ref.fractions(req, i)
    n = f.shape[0]
    out = dict(f=f)
    if req["geometry"] == "sphere":
        fr, fc = f[:, 0], f[:, 2]
    else:
        a = req["axis"]
        fr, fc = f[:, (a + 1) % 3], f[:, (a + 2) % 3]
    out["rho"], out["j"], out["s"] = radius(req["geometry"], req["density"], fr, variant)
    cs, sn = ref.cospi(2.0 * fc), ref.sinpi(2.0 * fc)
    d = np.zeros((n, 3))
    if req["geometry"] == "sphere":
        mu = 2.0 * f[:, 1] - 1.0
        q = np.sqrt(1.0 - mu * mu)
        d[:, 0], d[:, 1], d[:, 2] = q * cs, q * sn, mu
        out["mu"], out["q"] = mu, q
    else:
        d[:, (a + 1) % 3], d[:, (a + 2) % 3] = cs, sn
    out["dir"] = d
    return out


def base(req, i, variant=None):
    """the undisplaced positions p[n][3] (box fractions), the phase theta[n] (turns) and parts()"""
    pt = parts(req, i, variant)
    p = req["c_f"] + (pt["rho"][:, None] * req["rl"]) * pt["dir"]
    if req["geometry"] == "cylinder":
        a = req["axis"]
        p[:, a] = req["lo_f"][a] + pt["f"][:, a] * req["w_f"][a]
    theta = (req["m"][0] * p[:, 0] + req["m"][1] * p[:, 1]) + req["m"][2] * p[:, 2]
    return p, theta, pt


def positions(req, i, variant=None):
    p, theta, _ = base(req, i, variant)
    return ref._displaced(req, p, theta)


def stored_positions(req, i, dtype, variant=None):
    return ref.wrap01(positions(req, i, variant).astype(dtype))


def _rho_displaced(req, p, theta):
    """(the mutation) the radius of the DISPLACED position"""
    x = (ref._displaced(req, p, theta) - req["c_f"]) / req["rl"]
    if req["geometry"] == "cylinder":
        x[:, req["axis"]] = 0.0
    return np.minimum(np.sqrt((x * x).sum(axis=1)), BELOW_ONE)


def drift_eff(req, pt, variant=None):
    rho, d = pt["rho"], pt["dir"]
    out = np.broadcast_to(req["drift"], d.shape).copy()
    if req["geometry"] == "sphere":
        if req["flow_radial"] is not None:
            out = out + pref.lookup(req["flow_radial"], rho)[0][:, None] * d
        return out
    a = req["axis"]
    b, c = (a + 1) % 3, (a + 2) % 3
    if req["flow_axial"] is not None:
        out[:, a] = out[:, a] + pref.lookup(req["flow_axial"], rho)[0]
    if req["flow_radial"] is not None:
        u = pref.lookup(req["flow_radial"], rho)[0]
        out[:, b] = out[:, b] + u * d[:, b]
        out[:, c] = out[:, c] + u * d[:, c]
    if req["flow_azimuthal"] is not None:
        u = pref.lookup(req["flow_azimuthal"], rho)[0]
        sign = -1.0 if variant == "theta_hat_sign" else 1.0
        out[:, b] = out[:, b] + u * (sign * -d[:, c])
        out[:, c] = out[:, c] + u * (sign * d[:, b])
    return out


def velocities(req, i, variant=None):
    """float64 velocities in units of c"""
    i = np.asarray(i, dtype=np.uint64)
    p, theta, pt = base(req, i, variant)
    vth = np.broadcast_to(req["vth"], p.shape).copy()
    if req["thermal"] is not None:
        at = _rho_displaced(req, p, theta) if variant == "thermal_displaced" else pt["rho"]
        vth = vth * pref.lookup(req["thermal"], at)[0][:, None]
    th = vth * ref.normals(req, i)
    if req["paired"]:
        th = np.where(((i & np.uint64(1)) == 1)[:, None], -th, th)
    v = drift_eff(req, pt, variant) + th
    if np.any(req["vamp"] != 0):
        return v + req["vamp"] * ref.sinpi(2.0 * (theta + req["vphase"]))[:, None]
    return v + 0.0


def stored_velocities(req, i, dtype, variant=None):
    return velocities(req, i, variant).astype(dtype)
