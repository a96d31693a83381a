"""tests/select_reference.py (the numpy restatement of the rule of fpic_select) on hand-made cases whose answers are written
down here: the half-open interval at both ends, NaN and infinite values, infinite bounds, |v|^2 summed left to right in
double from float inputs, the id rule, ascending-id order from shuffled input, and matched > capacity."""
import numpy as np
import pytest

import select_reference as ref


def rows(values, axis, dtype=np.float64):
    """particles 0 .. n-1 whose `axis` holds `values`, everything else 0.5 / 0"""
    n = len(values)
    pos, vel = np.full((n, 3), 0.5, dtype=dtype), np.zeros((n, 3), dtype=dtype)
    a = ref.AXES[axis]
    (pos if a < 3 else vel)[:, a % 3] = values
    return np.arange(n, dtype=np.uint32), pos, vel


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lo_is_included_and_hi_is_excluded(dtype):
    lo, hi = dtype(0.25), dtype(0.75)
    vals = [np.nextafter(lo, dtype(0)), lo, np.nextafter(lo, dtype(1)), np.nextafter(hi, dtype(0)), hi, np.nextafter(hi, dtype(1))]
    ids, pos, vel = rows(vals, "y", dtype)
    got = ref.select(ids, pos, vel, {"y": (float(lo), float(hi))})
    assert got["ids"].tolist() == [1, 2, 3] and got["matched"] == 3
    assert got["position"].dtype == dtype and got["position"][:, 1].tolist() == [vals[1], vals[2], vals[3]]


def test_nan_and_infinite_values():
    ids, pos, vel = rows([np.nan, -np.inf, np.inf, 0.0, -1e300, 1e300], "vx")
    assert ref.select(ids, pos, vel, {"vx": (-1.0, 1.0)})["ids"].tolist() == [3]
    assert ref.select(ids, pos, vel, {"vx": (None, 1.0)})["ids"].tolist() == [1, 3, 4]          # -inf is inside [-inf, 1)
    assert ref.select(ids, pos, vel, {"vx": (-1.0, None)})["ids"].tolist() == [3, 5]            # +inf is not below +inf
    assert ref.select(ids, pos, vel, {"vx": (None, None)})["ids"].tolist() == [1, 3, 4, 5]      # a NaN matches nothing
    assert ref.select(ids, pos, vel, {})["ids"].tolist() == [0, 1, 2, 3, 4, 5]                  # no term: everybody
    assert ref.select(ids, pos, vel, None)["matched"] == 6
    # |v|^2 of an infinite or NaN velocity: inf resp. NaN
    assert ref.select(ids, pos, vel, {"v2": (0.0, None)})["ids"].tolist() == [3]                 # (+-1e300 squared overflows to +inf)
    assert ref.axis_value("v2", pos, vel)[[1, 2, 4, 5]].tolist() == [np.inf] * 4


def test_v2_is_summed_left_to_right_in_double_from_float_inputs():
    # y*y = z*z = 1.5625 * 2^-54: each alone is lost against 1, so (1 + y*y) + z*z = 1, while (y*y + z*z) + 1 = 1 + 2^-52
    y = np.float32(1.25 * 2.0 ** -27)
    assert float(y) == 1.25 * 2.0 ** -27                       # exact in float32
    ids = np.arange(2, dtype=np.uint32)
    pos = np.full((2, 3), 0.5, dtype=np.float32)
    vel = np.array([[1.0, y, y], [y, y, 1.0]], dtype=np.float32)
    q = ref.axis_value("v2", pos, vel)
    assert q.dtype == np.float64 and q.tolist() == [1.0, 1.0 + 2.0 ** -52]
    assert ref.select(ids, pos, vel, {"v2": (0.0, 1.0 + 2.0 ** -52)})["ids"].tolist() == [0]
    assert ref.select(ids, pos, vel, {"v2": (1.0 + 2.0 ** -52, None)})["ids"].tolist() == [1]
    # a float32 product would have rounded: 0.1f * 0.1f in float32 is not the double product of the two floats
    vel = np.array([[0.1, 0.0, 0.0]], dtype=np.float32)
    assert ref.axis_value("v2", pos[:1], vel)[0] == float(np.float32(0.1)) * float(np.float32(0.1))
    assert ref.axis_value("v2", pos[:1], vel)[0] != float(np.float32(0.1) * np.float32(0.1))


def test_the_id_rule():
    ids, pos, vel = rows(np.linspace(0.0, 0.99, 100), "x")
    assert ref.select(ids, pos, vel, None, every=(7, 3))["ids"].tolist() == list(range(3, 100, 7))
    assert ref.select(ids, pos, vel, None, every=(1, 0))["matched"] == 100
    assert ref.select(ids, pos, vel, None, every=(0, 0))["matched"] == 100
    assert ref.select(ids, pos, vel, {"x": (0.5, None)}, every=(10, 0))["ids"].tolist() == [50, 60, 70, 80, 90]
    big = np.array([2 ** 32 - 1, 2 ** 32 - 2, 5], dtype=np.uint32)
    assert ref.select(big, pos[:3], vel[:3], None, every=(2 ** 32 - 1, 0))["ids"].tolist() == [2 ** 32 - 1]
    assert ref.count(ids, pos, vel, {"x": (0.5, None)}, every=(10, 0)) == 5


def test_ascending_id_from_shuffled_input():
    rng = np.random.default_rng(3)
    n = 1000
    ids = rng.permutation(n).astype(np.uint32) + 17
    pos, vel = rng.random((n, 3)), rng.normal(0, 0.1, (n, 3))
    got = ref.select(ids, pos, vel, {"z": (0.2, 0.9), "vy": (None, 0.05)})
    assert got["matched"] == len(got["ids"]) > 0 and (np.diff(got["ids"].astype(np.int64)) > 0).all()
    at = {int(i): k for k, i in enumerate(ids)}
    for r, i in enumerate(got["ids"]):
        assert np.array_equal(got["position"][r], pos[at[int(i)]]) and np.array_equal(got["velocity"][r], vel[at[int(i)]])
    want = sorted(int(ids[k]) for k in range(n) if 0.2 <= pos[k, 2] < 0.9 and vel[k, 1] < 0.05)
    assert got["ids"].tolist() == want


def test_matched_above_capacity_delivers_nothing():
    ids, pos, vel = rows(np.linspace(0.0, 0.99, 100), "x")
    got = ref.select(ids, pos, vel, {"x": (0.0, 0.5)}, capacity=49)
    assert got["matched"] == 50 and got["ids"] is None and got["position"] is None and got["velocity"] is None
    got = ref.select(ids, pos, vel, {"x": (0.0, 0.5)}, capacity=50)
    assert got["matched"] == 50 and got["ids"].tolist() == list(range(50))
    assert ref.select(ids, pos, vel, {"x": (0.0, 0.5)}, capacity=0)["ids"] is None
    assert ref.select(ids, pos, vel, {"x": (2.0, 3.0)}, capacity=0)["ids"].tolist() == []


def test_the_cast_to_another_dtype():
    ids, pos, vel = rows([0.1, 1e300, np.nan], "vx")
    got = ref.select(ids, pos, vel, None, dtype=np.float32)
    assert got["velocity"].dtype == np.float32 and got["velocity"][0, 0] == np.float32(0.1) and np.isinf(got["velocity"][1, 0]) and np.isnan(got["velocity"][2, 0])
