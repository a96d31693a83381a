"""The rule of the absorbing particle sinks (fpic_remove, fpic_renumber; include/fusionpic.h) in numpy and Python integers,
nothing of the library.  Written from the header's text.  A species is (ids, pos, vel) IN SLOT ORDER, every row a live
particle, the arrays in the handle's precision (the stored values).  The predicate is the selection's
(tests/select_reference.py): a particle matches iff select() would return it; outside=True removes the particles that pass
the id rule and do NOT match every term.  Survivors keep every bit and their order.  The tallies are exact Python integers:
floor(q * 2^80) of the stored velocity components and of the squared norm ((x x + y y) + z z) formed in float64; a term with
|q| >= 2^15 or not finite adds nothing and makes its double NaN."""
import math
from fractions import Fraction

import numpy as np

import select_reference as sr

FIX_RANGE = 2.0 ** 15
C = 2.998e8


def removed_mask(ids, pos, vel, where=None, every=None, outside=False):
    """boolean mask over the rows: who leaves"""
    ids = np.asarray(ids)
    in_terms = sr.selected(ids, pos, vel, where, None)
    id_ok = sr.selected(ids, pos, vel, None, every)
    return id_ok & (~in_terms if outside else in_terms)


def floor_fix(q):
    """floor(q * 2^80) of a finite float, exactly"""
    return math.floor(Fraction(float(q)) * (1 << 80))


def tally(vel, gone):
    """(sums, nan): sums = [energy, mx, my, mz] as Python integers over the rows `gone`, nan[k] = sum k met a term outside
    the range"""
    v = np.asarray(vel)[gone].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        v2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    sums, nan = [0, 0, 0, 0], [False] * 4
    for k, col in enumerate([v2, v[:, 0], v[:, 1], v[:, 2]]):
        for q in col:
            if math.isfinite(q) and abs(q) < FIX_RANGE:
                sums[k] += floor_fix(q)
            else:
                nan[k] = True
    return sums, nan


def fixed_to_double(s):
    """the double nearest to s 2^-80 (ties to even) of an integer sum: Python's int / int division is correctly rounded"""
    return s / (1 << 80)


def remove(ids, pos, vel, where=None, every=None, outside=False, mass=1.0, charge=1.0, weight=1.0):
    """(survivors, result): survivors = (ids, pos, vel) of the rows that stay, in their order; result as fpic_remove's dict"""
    ids, pos, vel = np.asarray(ids, dtype=np.uint32), np.asarray(pos), np.asarray(vel)
    gone = removed_mask(ids, pos, vel, where, every, outside)
    sums, nan = tally(vel, gone)
    ke, pm = 0.5 * mass * weight * C * C, mass * weight * C
    removed = int(gone.sum())
    result = {"applications": 1, "scanned": int(ids.shape[0]), "removed": removed, "energy_fixed": sums[0], "momentum_fixed": sums[1:],
              "energy": float("nan") if nan[0] else ke * fixed_to_double(sums[0]),
              "momentum": [float("nan") if nan[1 + a] else pm * fixed_to_double(sums[1 + a]) for a in range(3)],
              "charge": (float(removed) * charge) * weight}
    keep = ~gone
    return (ids[keep].copy(), pos[keep].copy(), vel[keep].copy()), result


def add_results(parts):
    """the totals of several applications of one operator on one species (the doubles are not formed: compare the integers)"""
    out = {"applications": sum(p["applications"] for p in parts), "scanned": sum(p["scanned"] for p in parts), "removed": sum(p["removed"] for p in parts),
           "energy_fixed": sum(p["energy_fixed"] for p in parts), "momentum_fixed": [sum(p["momentum_fixed"][a] for p in parts) for a in range(3)]}
    return out


def renumber(ids):
    """the new id of every row: the number of live ids below its own"""
    ids = np.asarray(ids, dtype=np.uint32)
    order = np.argsort(ids, kind="stable")
    out = np.empty_like(ids)
    out[order] = np.arange(ids.shape[0], dtype=np.uint32)
    return out


def by_id(ids, pos, vel):
    """the rows in ascending id: what select() with no window returns"""
    order = np.argsort(np.asarray(ids), kind="stable")
    return np.asarray(ids)[order], np.asarray(pos)[order], np.asarray(vel)[order]
