"""The numpy rule of the absorbing particle sinks (tests/remove_reference.py) against hand-made cases, and the conditions of
the GPU scenes (tests/remove_scenes.py), checked here so that a GPU case cannot pass by removing nothing: every scene removes
0 < removed < n, the plain and the outside form partition the candidates, the "all" and "none" requests are what they say,
and the loop and chunk boundary cases straddle their boundaries for the constants read from the kernel header."""
import math
from fractions import Fraction

import numpy as np
import pytest

import remove_reference as rr
import remove_scenes as rs
import select_reference as sr


def hand():
    ids = np.array([4, 0, 7, 2, 9], dtype=np.uint32)      # slot order is not id order
    pos = np.array([[0.1, 0.5, 0.5], [0.3, 0.5, 0.5], [0.5, 0.5, 0.5], [0.7, 0.5, 0.5], [0.9, 0.5, 0.5]])
    vel = np.array([[0.5, 0.0, 0.0], [-0.25, 0.5, 0.0], [0.0, 0.0, 2.0 ** -40], [-(2.0 ** -81), 0.0, 0.0], [1.0, 1.0, 1.0]])
    return ids, pos, vel


def test_floor_fix_floors_towards_minus_infinity():
    assert rr.floor_fix(0.5) == 1 << 79 and rr.floor_fix(-0.5) == -(1 << 79)
    assert rr.floor_fix(2.0 ** -81) == 0 and rr.floor_fix(-(2.0 ** -81)) == -1      # a negative fraction floors down
    assert rr.floor_fix(2.0 ** -80) == 1 and rr.floor_fix(0.0) == 0 and rr.floor_fix(-0.0) == 0
    q = 0.1
    assert rr.floor_fix(q) == (Fraction(q) * (1 << 80)).__floor__()
    import energy_reference as er
    for q in (0.1, -0.3, 1e-20, -1e-20, 123.456, -32767.999):
        assert rr.floor_fix(q) == int(er.fix_floor_scalar(q))      # the energy diagnostics' fixed point


def test_hand_made_removal_is_stable_and_tallied():
    ids, pos, vel = hand()
    (sids, spos, svel), r = rr.remove(ids, pos, vel, where={"x": (0.2, 0.8)}, mass=2.0, charge=-3.0, weight=5.0)
    assert sids.tolist() == [4, 9] and spos[:, 0].tolist() == [0.1, 0.9] and np.array_equal(svel, vel[[0, 4]])
    assert (r["applications"], r["scanned"], r["removed"]) == (1, 5, 3)
    assert r["momentum_fixed"] == [-(1 << 78) + 0 - 1, 1 << 79, 1 << 40]
    assert r["energy_fixed"] == ((1 << 76) + (1 << 78)) + 1 + 0      # (0.3125; (2^-40)^2 is one unit; 2^-162 floors to zero)
    assert r["energy"] == 0.5 * 2.0 * 5.0 * rr.C * rr.C * (r["energy_fixed"] / 2 ** 80) and r["charge"] == (3.0 * -3.0) * 5.0
    assert r["momentum"][1] == 2.0 * 5.0 * rr.C * 0.5
    # the outside form removes the complement among those the id rule passes, the survivors keep their order
    (sids, _, _), r = rr.remove(ids, pos, vel, where={"x": (0.2, 0.8)}, outside=True)
    assert sids.tolist() == [0, 7, 2] and r["removed"] == 2
    (sids, _, _), r = rr.remove(ids, pos, vel, where={"x": (0.2, 0.8)}, every=(2, 0), outside=True)
    assert sids.tolist() == [0, 7, 2, 9] and r["removed"] == 1      # id 9 is outside but odd: the id rule keeps it
    (sids, _, _), r = rr.remove(ids, pos, vel, every=(2, 1))
    assert sids.tolist() == [4, 0, 2] and r["removed"] == 2
    assert rr.remove(ids, pos, vel)[1]["removed"] == 5 and rr.remove(ids, pos, vel, outside=True)[1]["removed"] == 0


def test_terms_outside_the_range_make_the_double_nan():
    ids = np.arange(3, dtype=np.uint32)
    pos = np.full((3, 3), 0.5)
    vel = np.array([[200.0, 0.0, 0.0], [np.inf, 0.0, 0.0], [0.5, 0.0, np.nan]])
    _, r = rr.remove(ids, pos, vel, where={"x": (0, 1)})
    assert r["removed"] == 3 and math.isnan(r["energy"]) and math.isnan(r["momentum"][0]) and math.isnan(r["momentum"][2]) and r["momentum"][1] == 0.0
    assert r["momentum_fixed"][0] == (200 << 80) + (1 << 79) and r["energy_fixed"] == 0      # |v|^2 = 40000, inf, nan: none is added
    _, r = rr.remove(ids, pos, vel, where={"vx": (None, 1.0)})      # a NaN matches nothing: only particle 2 is tested on vx = 0.5
    assert r["removed"] == 1 and math.isnan(r["energy"]) and r["momentum_fixed"][0] == 1 << 79


def test_renumber_ranks_the_ids():
    ids = np.array([40, 3, 17, 4000000000, 0], dtype=np.uint32)
    assert rr.renumber(ids).tolist() == [3, 1, 2, 4, 0]
    assert rr.renumber(np.zeros(0, dtype=np.uint32)).tolist() == []
    i, p, v = rr.by_id(*hand())
    assert i.tolist() == [0, 2, 4, 7, 9] and p[:, 0].tolist() == [0.3, 0.7, 0.1, 0.5, 0.9]


def test_add_results():
    a = dict(applications=1, scanned=10, removed=2, energy_fixed=5, momentum_fixed=[1, -2, 3])
    b = dict(applications=1, scanned=8, removed=0, energy_fixed=0, momentum_fixed=[0, 0, 0])
    assert rr.add_results([a, b, a]) == dict(applications=3, scanned=28, removed=4, energy_fixed=10, momentum_fixed=[2, -4, 6])


# ---- the conditions of the GPU scenes
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_scene_removes_some_and_not_all(dtype):
    pos, vel = rs.population()
    pos, vel = pos.astype(dtype), vel.astype(dtype)
    ids = np.arange(rs.N, dtype=np.uint32)
    seen = set()
    for req in rs.REQUESTS:
        (sids, _, _), r = rr.remove(ids, pos, vel, **req)
        assert 0 < r["removed"] < rs.N and len(sids) == rs.N - r["removed"], req
        seen.add((len(req["where"] or {}), req["outside"], req["every"] is not None))
        # the plain and the outside form partition the candidates (those the id rule passes)
        other = rr.removed_mask(ids, pos, vel, req["where"], req["every"], not req["outside"])
        mine = rr.removed_mask(ids, pos, vel, req["where"], req["every"], req["outside"])
        candidates = sr.selected(ids, pos, vel, None, req["every"])
        assert not (mine & other).any() and np.array_equal(mine | other, candidates)
    for terms in (1, 3, 7):
        for outside in (False, True):
            assert (terms, outside, False) in seen and (terms if terms != 1 else 1, outside, True) in seen
    assert {next(iter(w)) for w in rs.ONE_TERM} == set(sr.AXES)      # one term per axis code
    assert rr.remove(ids, pos, vel, **rs.ALL)[1]["removed"] == rs.N
    for req in rs.NONE:
        assert rr.remove(ids, pos, vel, **req)[1]["removed"] == 0


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_boundary_cases_straddle_their_boundaries(precision):
    lanes, chunk = rs.LANES[precision], rs.CHUNK
    counts = rs.boundary_counts(precision)
    assert {1, lanes - 1, lanes + 1, chunk - 1, chunk, chunk + 1}.issubset(counts)
    big = max(counts)
    assert big == rs.SCAN_TURN * chunk + 1 and -(-big // chunk) == rs.SCAN_TURN + 1      # the scan's second turn holds one chunk: a carry
    assert rs.GRID_STRIDE == rs.BLOCKS * (rs.THREADS // 64) * chunk and rs.GRID_STRIDE + 1 <= 1 << 32
    for n in counts + [rs.GRID_STRIDE - 1, rs.GRID_STRIDE + 1]:
        slots = rs.planted(n, precision)
        assert len(set(slots.tolist())) == len(slots) and slots.min() >= 0 and slots.max() == n - 1 and slots[0] == 0
        assert (n - 1) // lanes * lanes in slots      # the last (partial or full) vector
        if n > chunk:
            assert chunk - 1 in slots and chunk in slots      # the last slot of a chunk and the first of the next
            assert (n - 1) // chunk * chunk in slots
        if n > 3 * chunk:
            alone = 2 * chunk + 77
            assert alone in slots and not any(s != alone and s // chunk == alone // chunk for s in slots)      # alone in its chunk
            assert rs.SCAN_TURN * chunk - 1 in slots      # the last slot the scan's first turn covers
        assert 0 < len(slots) <= n
