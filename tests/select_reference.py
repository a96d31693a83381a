"""The rule of the particle selection (fpic_select, include/fusionpic.h) in numpy, nothing of the library.  Written from the
header's text: over (ids, pos, vel) arrays of either precision — what getParticles / domainGet return, every row a live
particle — the value of an axis is the stored number converted to float64 (v2: vx*vx + vy*vy + vz*vz in float64, added left
to right), a term matches iff lo <= q < hi (a NaN matches nothing; lo may be -inf, hi +inf), a particle is selected iff it
matches every term and passes the id rule, and the rows come back in ascending id."""
import numpy as np

AXES = {"x": 0, "y": 1, "z": 2, "vx": 3, "vy": 4, "vz": 5, "v2": 6}


def axis_value(name, pos, vel):
    """float64 values of one axis for every row"""
    a = AXES[name]
    if a < 3:
        return np.asarray(pos)[:, a].astype(np.float64)
    if a < 6:
        return np.asarray(vel)[:, a - 3].astype(np.float64)
    v = np.asarray(vel).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def selected(ids, pos, vel, where=None, every=None):
    """boolean mask over the rows"""
    ids = np.asarray(ids)
    keep = np.ones(ids.shape[0], dtype=bool)
    for name, (lo, hi) in (where or {}).items():
        lo = -np.inf if lo is None else np.float64(lo)
        hi = np.inf if hi is None else np.float64(hi)
        q = axis_value(name, pos, vel)
        with np.errstate(invalid="ignore"):
            keep &= (q >= lo) & (q < hi)
    if every is not None and every[0] > 1:
        keep &= (ids.astype(np.uint64) % np.uint64(every[0])) == np.uint64(every[1])
    return keep


def select(ids, pos, vel, where=None, every=None, capacity=None, dtype=None):
    """{ids, position, velocity, matched} as fpic_select delivers them: ascending id, the stored values cast to dtype (the
    arrays' own by default); None arrays when a given capacity is below matched"""
    ids, pos, vel = np.asarray(ids, dtype=np.uint32), np.asarray(pos), np.asarray(vel)
    keep = selected(ids, pos, vel, where, every)
    matched = int(keep.sum())
    if capacity is not None and matched > capacity:
        return {"ids": None, "position": None, "velocity": None, "matched": matched}
    rows = np.flatnonzero(keep)
    rows = rows[np.argsort(ids[rows], kind="stable")]
    dt = pos.dtype if dtype is None else np.dtype(dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        return {"ids": ids[rows].copy(), "position": pos[rows].astype(dt), "velocity": vel[rows].astype(dt), "matched": matched}


def count(ids, pos, vel, where=None, every=None):
    return int(selected(ids, pos, vel, where, every).sum())
