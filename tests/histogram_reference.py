"""The definition of the phase-space histograms (fpic_histogram, include/fusionpic.h) in numpy: float64 and Python
integers only, nothing of the library.  Written from the header's contract:

  q of an axis   x, y, z, vx, vy, vz: the stored value converted to double; v2: vx*vx + vy*vy + vz*vz, left to right
  inside         q >= lo and q < hi (a NaN is not inside)
  index          min(int(floor((q - lo) * scale)), bins - 1) with scale = bins / (hi - lo), each operation rounded once
  counts         a particle inside every axis adds 1 to counts[k0] or counts[k0, k1]; every other live one to `outside`
  live           every slot, except x < 0 on a decomposed rank (live=False turns that off for one handle's getParticles)
"""
import math

import numpy as np

AXES = {"x": 0, "y": 1, "z": 2, "vx": 3, "vy": 4, "vz": 5, "v2": 6}
MAX_BINS = 1 << 22


def scale_of(bins, lo, hi):
    return np.float64(bins) / (np.float64(hi) - np.float64(lo))


def check(axes, bins, ranges):
    """raises ValueError for a request the library refuses"""
    if len(axes) not in (1, 2) or len(bins) != len(axes) or len(ranges) != len(axes):
        raise ValueError("naxes")
    if any(a not in AXES for a in axes) or len(set(axes)) != len(axes):
        raise ValueError("axis")
    total = 1
    for b, (lo, hi) in zip(bins, ranges):
        if b < 1:
            raise ValueError("bins")
        if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
            raise ValueError("range")
        with np.errstate(over="ignore"):
            if not (np.isfinite(np.float64(hi) - np.float64(lo)) and np.isfinite(scale_of(b, lo, hi))):
                raise ValueError("range")
        total *= b
    if total > MAX_BINS:
        raise ValueError("bins")


def axis_values(name, position, velocity):
    """q of every particle, float64 (the stored arrays converted exactly)"""
    c = AXES[name]
    if c < 3:
        return np.asarray(position)[:, c].astype(np.float64)
    v = np.asarray(velocity).astype(np.float64)
    if c < 6:
        return v[:, c - 3]
    return v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]      # (numpy adds left to right, one rounding each)


def bin_index(q, bins, lo, hi):
    """(inside, k) of float64 values q on one axis; k is meaningful where inside"""
    q = np.asarray(q, dtype=np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(invalid="ignore"):
        inside = (q >= lo) & (q < hi)
    d = np.where(inside, q, lo) - lo
    t = d * scale_of(bins, lo, hi)
    k = np.minimum(np.floor(t).astype(np.int64), bins - 1)
    return inside, k


def histogram(position, velocity, axes, bins, ranges, dead_slots=False):
    """(counts: uint64 array of shape (bins0,) or (bins0, bins1), outside: int) of the particles position / velocity
    ([n][3] arrays of stored values).  axes: names; bins: ints; ranges: (lo, hi) pairs, one per axis.  dead_slots: the
    arrays come from a decomposed rank (domainGet), whose slots with x < 0 hold no particle."""
    axes = [axes] if isinstance(axes, str) else list(axes)
    bins = [bins] * len(axes) if isinstance(bins, (int, np.integer)) else [int(b) for b in bins]
    ranges = np.asarray(ranges, dtype=np.float64).reshape(-1, 2).tolist()
    check(axes, bins, ranges)
    position, velocity = np.asarray(position), np.asarray(velocity)
    n = len(position)
    live = np.ones(n, dtype=bool)
    if dead_slots:
        live = ~(position[:, 0] < 0)
    inside, flat = live.copy(), np.zeros(n, dtype=np.int64)
    for name, b, (lo, hi) in zip(axes, bins, ranges):
        ins, k = bin_index(axis_values(name, position, velocity), b, lo, hi)
        inside &= ins
        flat = flat * b + k
    total = int(np.prod(bins, dtype=np.int64))
    counts = np.bincount(flat[inside], minlength=total).astype(np.uint64).reshape(bins)
    outside = int(live.sum()) - int(inside.sum())
    return counts, outside
