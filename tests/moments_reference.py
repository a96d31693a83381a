"""The definition of the fluid moment grids (fpic_moments, include/fusionpic.h) in numpy: int64 and float64 only, nothing
of the library.  Written from the header's contract:

  cell, weights  es3d_axis of the stored position IN THE STATE'S DTYPE: g = u * n, i = (int) g, f = g - i, i -= n if i >= n,
                 w1 = ((int)(f * 32768) + 1) >> 1; w0 = 16384 - w1; nodes (i + a, j + b, k + c) wrapped periodically
  rejected       a velocity component that is not finite or |v| >= 128: the particle adds to nothing, 1 to `rejected`
  N              wx[a] * wy[b] * wz[c] per node
  other moments  m in float64 (one multiplication for the second-order ones), t = floor(m * 2^32) as int64, split with
                 remainder along z, then y, then x: upper = (w1 * t + 8192) >> 14 (numpy's >> on int64 floors), lower = t - upper
  live           every slot, except x < 0 on a decomposed rank (dead_slots=True)
"""
import numpy as np

NAMES = ("N", "FX", "FY", "FZ", "SXX", "SYY", "SZZ", "SXY", "SXZ", "SYZ")
SETS = {"n": 0x001, "order1": 0x00F, "order2": 0x3FF}
ONE = 1 << 42
SCALE = 1 << 32
LIMIT = 128.0


def mask_of(which):
    if isinstance(which, str):
        return SETS[which]
    m = 0
    for name in which:
        m |= 1 << NAMES.index(name)
    return m


def check(species, mask, nspecies, reserved=(0, 0, 0, 0)):
    """raises ValueError naming the property for a request the library refuses"""
    if not 0 <= species < nspecies:
        raise ValueError("species")
    if mask == 0 or mask >> 10:
        raise ValueError("mask")
    if any(r != 0 for r in reserved):
        raise ValueError("reserved")


def axis(u, n):
    """(cell, upper weight) of stored coordinates u (float32 or float64 array), evaluated in u's dtype"""
    T = u.dtype.type
    g = u * T(n)
    i = g.astype(np.int32)                       # (truncation, as the C cast; g >= 0)
    f = g - i.astype(u.dtype)
    i = np.where(i >= n, i - n, i)
    w1 = ((f * T(32768)).astype(np.int32) + 1) >> 1
    return i.astype(np.int64), w1.astype(np.int64)


def rejected(v):
    """v: float64 [n][3]"""
    with np.errstate(invalid="ignore"):
        return ~((np.abs(v[:, 0]) < LIMIT) & (np.abs(v[:, 1]) < LIMIT) & (np.abs(v[:, 2]) < LIMIT))


def values(bit, v):
    """the particle values m of moment `bit` (1 .. 9), float64"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return (None, x, y, z, x * x, y * y, z * z, x * y, x * z, y * z)[bit]


def fixed(m):
    return np.floor(m * 2.0 ** 32).astype(np.int64)


def split(t, w1):
    upper = (w1 * t + 8192) >> 14
    return t - upper, upper


def mom_terms(t, wx1, wy1, wz1):
    """the eight node terms [a + 2 b + 4 c] of values t (int64 arrays)"""
    out = [None] * 8
    tz = split(t, wz1)
    for c in range(2):
        ty = split(tz[c], wy1)
        for b in range(2):
            out[2 * b + 4 * c], out[1 + 2 * b + 4 * c] = split(ty[b], wx1)
    return out


def n_terms(wx1, wy1, wz1):
    wx, wy, wz = (16384 - wx1, wx1), (16384 - wy1, wy1), (16384 - wz1, wz1)
    return [wx[e & 1] * wy[e >> 1 & 1] * wz[e >> 2] for e in range(8)]


def particle_sums(velocity, mask, live=None):
    """{name: sum of t over the accepted particles (N: their number times 2^42)}, rejected"""
    v = np.asarray(velocity).astype(np.float64)
    live = np.ones(len(v), dtype=bool) if live is None else live
    ok = live & ~rejected(v)
    out = {}
    for bit in range(10):
        if mask >> bit & 1:
            out[NAMES[bit]] = int(ok.sum()) * ONE if bit == 0 else sum(int(t) for t in fixed(values(bit, v[ok])))
    return out, int(live.sum() - ok.sum())


def moments(position, velocity, shape, which="order2", dead_slots=False):
    """({name: int64 array (nz, ny, nx)}, rejected) of the particles position / velocity ([n][3] arrays of stored values in
    the handle's dtype).  shape = (nx, ny, nz).  dead_slots: the arrays come from a decomposed rank (domainGet), whose slots
    with x < 0 hold no particle."""
    mask = mask_of(which)
    position, velocity = np.asarray(position), np.asarray(velocity)
    nx, ny, nz = shape
    v = velocity.astype(np.float64)
    live = np.ones(len(position), dtype=bool)
    if dead_slots:
        live = ~(position[:, 0] < 0)
    bad = rejected(v)
    ok = live & ~bad
    p, v = position[ok], v[ok]
    i, wx1 = axis(np.ascontiguousarray(p[:, 0]), nx)
    j, wy1 = axis(np.ascontiguousarray(p[:, 1]), ny)
    k, wz1 = axis(np.ascontiguousarray(p[:, 2]), nz)
    node = []
    for e in range(8):
        ii, jj, kk = (i + (e & 1)) % nx, (j + (e >> 1 & 1)) % ny, (k + (e >> 2)) % nz
        node.append(ii + nx * (jj + ny * kk))
    out = {}
    for bit in range(10):
        if not mask >> bit & 1:
            continue
        terms = n_terms(wx1, wy1, wz1) if bit == 0 else mom_terms(fixed(values(bit, v)), wx1, wy1, wz1)
        grid = np.zeros(nx * ny * nz, dtype=np.int64)
        for e in range(8):
            np.add.at(grid, node[e], terms[e])
        out[NAMES[bit]] = grid.reshape(nz, ny, nx)
    return out, int((live & bad).sum())
