"""The point rule of the series diagnostic (fpic_series_*, include/fusionpic.h) in numpy: float64 sums over integer weights,
nothing of the library.  Written from the header's contract:

  1. per axis u = p / L in float64, u -= floor(u), u = 0 if that is not < 1; then u is cast to the state's dtype T
  2. (i, w1) = the charge deposit's axis(u, n), evaluated in T (moments_reference.axis); w0 = 16384 - w1
  3. the eight nodes (i+a, j+b, k+c) wrapped periodically, e = a + 2 b + 4 c, W_e = wx[a] * wy[b] * wz[c] (sum 2^42)
  4. per component value = (sum_e float64(W_e) * float64(F_e)) * 2^-42: the first product starts the sum, the others are
     added in the order e = 1 .. 7, every operation rounded once
"""
import numpy as np

from moments_reference import axis

ONE = 1 << 42
POINT_COLUMNS = ("ex", "ey", "ez", "phi", "bx", "by", "bz", "present")
TRACER_COLUMNS = ("x", "y", "z", "vx", "vy", "vz", "found", "zero")


def unit(p, L):
    """step 1: float64 [n] positions along one axis of length L -> the fraction of the box in [0, 1), float64"""
    u = np.asarray(p, dtype=np.float64) / np.float64(L)
    u = u - np.floor(u)
    return np.where(u < 1, u, 0.0)


def weights(points, L, shape, dtype):
    """steps 1-3: (nodes int64 [P][8] as i + nx (j + ny k), W int64 [P][8], k int64 [P]: the cell plane that owns the point)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cell, w = [], []
    for a in range(3):
        i, w1 = axis(unit(points[:, a], L[a]).astype(dtype), shape[a])
        cell.append(i)
        w.append(np.stack([16384 - w1, w1], axis=1))
    nx, ny, nz = shape
    nodes = np.empty((len(points), 8), dtype=np.int64)
    W = np.empty((len(points), 8), dtype=np.int64)
    for e in range(8):
        a, b, c = e & 1, (e >> 1) & 1, e >> 2
        nodes[:, e] = (cell[0] + a) % nx + nx * ((cell[1] + b) % ny + ny * ((cell[2] + c) % nz))
        W[:, e] = w[0][:, a] * w[1][:, b] * w[2][:, c]
    return nodes, W, cell[2]


def interpolate(field, nodes, W):
    """step 4: field [nodes][C] in the state's dtype -> float64 [P][C]"""
    F = np.asarray(field).astype(np.float64)
    Wd = W.astype(np.float64)
    acc = Wd[:, 0, None] * F[nodes[:, 0]]
    for e in range(1, 8):
        acc = acc + Wd[:, e, None] * F[nodes[:, e]]
    return acc * 2.0 ** -42


def point_rows(points, L, shape, E, B=None):
    """the rows of `points` from E (readField(F3_E): [nodes][4]) and B (readField(F3_B_NODES) or None), in their dtype"""
    nodes, W, _ = weights(points, L, shape, np.asarray(E).dtype)
    out = np.zeros((len(nodes), 8))
    out[:, 0:4] = interpolate(E, nodes, W)
    if B is not None:
        out[:, 4:7] = interpolate(B, nodes, W)[:, :3]
    out[:, 7] = 1.0
    return out


def node_points(L, shape, form=0):
    """every node of the grid as a point, in node order: i * (L / n) (form 0) or i / n * L (form 1)"""
    ax = []
    for a in range(3):
        i = np.arange(shape[a], dtype=np.float64)
        ax.append(i * (L[a] / shape[a]) if form == 0 else i / shape[a] * L[a])
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
