"""The rule of the particle loader (fpic_load) restated in plain numpy, from the text of include/fusionpic.h and DESIGN.md
4.15.  It shares no code with the product or the oracle: Philox4x32-10 runs on uint64 arrays, everything else in float64 in
the stated operation order (numpy never fuses a multiply with an add).

    req = request(L, seed=..., stream=..., lo=..., hi=..., drift=..., vth=..., mode=..., xamp=..., ...)
    stored_positions(req, i, np.float32)     what a handle of that precision holds for the particle indices i
    stored_velocities(req, i, np.float64)

`variant` selects one of five deliberately WRONG rules (tests/test_load_reference.py shows that each differs from the right
one on a stated share of particles, so that the GPU comparison can see such a mistake)."""
import numpy as np

TAG = 0x10AD
MULT = (3518319155, 2882110345, 2360945575)
M32 = np.uint64(0xFFFFFFFF)
VARIANTS = ("swapped_words", "fma", "no_half", "theta_displaced", "round_plane")


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0, c1, c2, c3) and keys (k0, k1), arrays or scalars -> four uint32 arrays"""
    c0, c1, c2, c3, k0, k1 = (np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32 for v in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    k0, k1 = k0.copy(), k1.copy()
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0        # (below 2^64: both factors are below 2^32)
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _reduced(x):
    """|x| mod 2 — exact in float64"""
    return np.fmod(np.abs(np.asarray(x, dtype=np.float64)), 2.0)


def sinpi(x):
    """sin(pi x): exact reduction to [0, 1/2], then the function of the nearer axis"""
    x = np.asarray(x, dtype=np.float64)
    s = np.where(x < 0, -1.0, 1.0)
    r = _reduced(x)
    up = r >= 1.0
    r = np.where(up, r - 1.0, r)
    s = np.where(up, -s, s)
    r = np.where(r > 0.5, 1.0 - r, r)
    return s * np.where(r <= 0.25, np.sin(np.pi * r), np.cos(np.pi * (0.5 - r)))


def cospi(x):
    r = _reduced(x)
    r = np.where(r >= 1.0, 2.0 - r, r)
    neg = r > 0.5
    r = np.where(neg, 1.0 - r, r)
    return np.where(neg, -1.0, 1.0) * np.where(r <= 0.25, np.cos(np.pi * r), np.sin(np.pi * (0.5 - r)))


def _three(v):
    return np.array([v, v, v] if np.ndim(v) == 0 else list(v), dtype=np.float64)


def request(L, seed=0x5EEDF051, stream=0, lo=None, hi=None, drift=0, vth=0, mode=None, xamp=0, xphase=0, vamp=0, vphase=0,
            lattice=False, paired=False):
    """the host's part of a request: lengths divided by the box, the lattice shifts drawn"""
    L = _three(L)
    lo = _three(0.0 if lo is None else lo)
    hi = L if hi is None else _three(hi)
    seed_lo, seed_hi = seed & 0xFFFFFFFF, seed >> 32
    shift = [int(w[0]) for w in philox(0, stream, 2, TAG, seed_lo, seed_hi)][:3]
    return dict(seed_lo=seed_lo, seed_hi=seed_hi, stream=stream, lo_f=lo / L, w_f=(hi - lo) / L, drift=_three(drift) + 0.0, vth=_three(vth),
                m=_three(0 if mode is None else mode), xamp_f=_three(xamp) / L, xphase=float(xphase), vamp=_three(vamp), vphase=float(vphase),
                lattice=bool(lattice), paired=bool(paired), shift=shift)


def fractions(req, i, variant=None):
    """f[n][3]: exact integers scaled by 2^-32"""
    i = np.asarray(i, dtype=np.uint64)
    if req["lattice"]:
        w = [(i * np.uint64(MULT[a]) + np.uint64(req["shift"][a])) & M32 for a in range(3)]
    else:
        w = list(philox(i, req["stream"], 0, TAG, req["seed_lo"], req["seed_hi"]))[:3]
        if variant == "swapped_words":
            w[0], w[1] = w[1], w[0]
    return np.stack([x.astype(np.float64) * 2.0 ** -32 for x in w], axis=1)


def base(req, i, variant=None):
    """the undisplaced positions p[n][3] (box fractions) and the phase theta[n] (turns)"""
    f = fractions(req, i, variant)
    if variant == "fma":
        import mpmath
        with mpmath.workprec(200):   # lo + f w exactly, rounded once
            p = np.array([[float(mpmath.mpf(float(req["lo_f"][a])) + mpmath.mpf(float(f[k, a])) * mpmath.mpf(float(req["w_f"][a]))) for a in range(3)]
                          for k in range(f.shape[0])]).reshape(-1, 3)
    else:
        t = f * req["w_f"]
        p = req["lo_f"] + t
    theta = (req["m"][0] * p[:, 0] + req["m"][1] * p[:, 1]) + req["m"][2] * p[:, 2]
    return p, theta


def _displaced(req, p, theta):
    if not np.any(req["xamp_f"] != 0):
        return p
    s = sinpi(2.0 * (theta + req["xphase"]))
    return p + req["xamp_f"] * s[:, None]


def positions(req, i, variant=None):
    """float64 positions before the cast and the wrap"""
    p, theta = base(req, i, variant)
    return _displaced(req, p, theta)


def wrap01(u):
    """the upload's wrap, in the arithmetic of u's type"""
    r = u - np.floor(u)
    r[~(r < 1)] = 0
    return r


def stored_positions(req, i, dtype, variant=None):
    return wrap01(positions(req, i, variant).astype(dtype))


def normal_parts(req, i, variant=None):
    """(r1, c, s, r3, c3): the radii and the circular functions of the Box-Muller transform of the velocity block"""
    i = np.asarray(i, dtype=np.uint64)
    at = i & ~np.uint64(1) if req["paired"] else i
    w = [x.astype(np.float64) for x in philox(at, req["stream"], 1, TAG, req["seed_lo"], req["seed_hi"])]
    half = 0.0 if variant == "no_half" else 0.5
    with np.errstate(divide="ignore"):
        r1 = np.sqrt(-2.0 * np.log((w[0] + half) * 2.0 ** -32))
        r3 = np.sqrt(-2.0 * np.log((w[2] + half) * 2.0 ** -32))
    u2, u4 = w[1] * 2.0 ** -32, w[3] * 2.0 ** -32
    return r1, cospi(2.0 * u2), sinpi(2.0 * u2), r3, cospi(2.0 * u4)


def normals(req, i, variant=None):
    r1, c, s, r3, c3 = normal_parts(req, i, variant)
    return np.stack([r1 * c, r1 * s, r3 * c3], axis=1)


def velocities(req, i, variant=None):
    """float64 velocities in units of c"""
    i = np.asarray(i, dtype=np.uint64)
    th = req["vth"] * normals(req, i, variant)
    if req["paired"]:
        th = np.where(((i & np.uint64(1)) == 1)[:, None], -th, th)
    v = req["drift"] + th
    if np.any(req["vamp"] != 0):
        p, theta = base(req, i, variant)
        if variant == "theta_displaced":
            q = _displaced(req, p, theta)
            theta = (req["m"][0] * q[:, 0] + req["m"][1] * q[:, 1]) + req["m"][2] * q[:, 2]
        return v + req["vamp"] * sinpi(2.0 * (theta + req["vphase"]))[:, None]
    return v + 0.0


def stored_velocities(req, i, dtype, variant=None):
    return velocities(req, i, variant).astype(dtype)


def plane(z_stored, nz, variant=None):
    """the cell plane of a stored z: floor(z nz) in the arithmetic of z's type, nz itself wrapping to 0"""
    g = z_stored * z_stored.dtype.type(nz)
    k = (np.rint(g) if variant == "round_plane" else np.floor(g)).astype(np.int64)
    return np.where(k >= nz, k - nz, k)
