"""tests/histogram_reference.py (the definition of fpic_histogram in numpy) against numpy.histogram / histogram2d where the
two rules coincide (dyadic edges and values: every subtraction and product is exact), and against hand-written cases for
the edges of the inside test, values that are not finite, the product that rounds up to `bins`, |v|^2 and dead slots."""
import numpy as np
import pytest

import histogram_reference as hr


def particles(rng, n, dtype=np.float64):
    """dyadic stored values: positions k / 1024 in [0, 1), velocities k / 4096 in [-1, 1)"""
    pos = rng.integers(0, 1024, (n, 3)).astype(dtype) / 1024
    vel = rng.integers(-4096, 4096, (n, 3)).astype(dtype) / 4096
    return pos, vel


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("axis,lo,hi,bins", [("x", 0.0, 1.0, 64), ("y", 0.25, 0.75, 16), ("z", 0.0, 0.5, 512), ("vx", -1.0, 1.0, 128),
                                             ("vy", -0.5, 0.25, 48), ("vz", -2.0, 2.0, 32)])
def test_one_axis_equals_numpy_histogram_on_dyadic_input(dtype, axis, lo, hi, bins):
    pos, vel = particles(np.random.default_rng(1), 5000, dtype)
    counts, outside = hr.histogram(pos, vel, axis, bins, (lo, hi))
    q = hr.axis_values(axis, pos, vel)
    q = q[q != hi]                                  # numpy's last bin is closed at hi; the definition's is not
    want, _ = np.histogram(q, bins=bins, range=(lo, hi))
    assert counts.dtype == np.uint64 and counts.shape == (bins,)
    assert counts.tolist() == want.tolist()
    assert int(counts.sum()) + outside == 5000
    assert outside == int(((hr.axis_values(axis, pos, vel) < lo) | (hr.axis_values(axis, pos, vel) >= hi)).sum())


def test_two_axes_equal_numpy_histogram2d_on_dyadic_input():
    pos, vel = particles(np.random.default_rng(2), 8000)
    counts, outside = hr.histogram(pos, vel, ("x", "vx"), (32, 16), ((0.0, 1.0), (-0.5, 0.5)))
    keep = vel[:, 0] != 0.5
    want, _, _ = np.histogram2d(pos[keep, 0], vel[keep, 0], bins=(32, 16), range=((0.0, 1.0), (-0.5, 0.5)))
    assert counts.shape == (32, 16)                 # row-major [bins0][bins1]
    assert counts.tolist() == want.astype(np.uint64).tolist()
    assert int(counts.sum()) + outside == 8000 and outside > 0
    # a particle inside one axis and outside the other is outside
    c, o = hr.histogram([[0.5, 0, 0]], [[0.75, 0, 0]], ("x", "vx"), (4, 4), ((0, 1), (-0.5, 0.5)))
    assert c.sum() == 0 and o == 1


def test_v2_is_added_left_to_right_in_double():
    y = 1.25 * 2.0 ** -27                           # y*y is less than half an ulp of 1, 2 y*y is more
    vel = np.array([[1.0, y, y], [y, y, 1.0], [3.0, 4.0, 12.0]])
    q = hr.axis_values("v2", np.zeros((3, 3)), vel)
    assert q.tolist() == [1.0, 1.0 + 2.0 ** -52, 169.0]
    # float32 velocities are converted first: the squares are exact in double
    v32 = np.array([[0.1, 0.2, 0.3]], dtype=np.float32)
    d = v32.astype(np.float64)[0]
    assert hr.axis_values("v2", np.zeros((1, 3)), v32)[0] == (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    c, o = hr.histogram(np.zeros((3, 3)), vel, "v2", 4, (0.0, 2.0))
    assert c.tolist() == [0, 0, 2, 0] and o == 1


def one(q, bins, lo, hi):
    inside, k = hr.bin_index(np.array([q]), bins, lo, hi)
    return bool(inside[0]), int(k[0])


def test_edges_of_the_inside_test():
    assert one(-1.0, 8, -1.0, 3.0) == (True, 0)                     # q == lo
    assert one(3.0, 8, -1.0, 3.0)[0] is False                       # q == hi
    assert one(np.nextafter(3.0, 0.0), 8, -1.0, 3.0) == (True, 7)   # the largest double below hi
    assert one(np.nextafter(-1.0, -2.0), 8, -1.0, 3.0)[0] is False
    for bad in (np.nan, np.inf, -np.inf):
        assert one(bad, 8, -1.0, 3.0)[0] is False
    vel = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [-np.inf, 0, 0], [0.0, np.nan, 0], [0.25, 0, 0]])
    c, o = hr.histogram(np.zeros((5, 3)), vel, "vx", 2, (-1.0, 1.0))
    assert c.tolist() == [0, 2] and o == 3
    c, o = hr.histogram(np.zeros((5, 3)), vel, "v2", 2, (0.0, 1.0))   # inf*inf = inf, NaN stays NaN: all outside
    assert c.tolist() == [1, 0] and o == 4


def test_the_min_catches_a_product_that_rounds_up_to_bins():
    rng = np.random.default_rng(5)
    found = []
    for _ in range(400):
        lo = rng.uniform(-1, 1)
        hi = lo + rng.uniform(1e-3, 1)
        bins = int(rng.integers(1, 1000))
        top = np.nextafter(hi, lo)
        if np.floor((top - lo) * hr.scale_of(bins, lo, hi)) >= bins:
            found.append((lo, hi, bins))
    assert len(found) >= 10, len(found)             # (about one triple in five)
    for lo, hi, bins in found + [(-0.7322673547034516, -0.18700837184614172, 111)]:
        top = np.nextafter(hi, lo)
        assert np.floor((top - lo) * hr.scale_of(bins, lo, hi)) == bins
        assert one(top, bins, lo, hi) == (True, bins - 1)
        c, o = hr.histogram(np.zeros((1, 3)), [[top, 0, 0]], "vx", bins, (lo, hi))
        assert o == 0 and c[bins - 1] == 1 and c.sum() == 1


def test_dead_slots_are_skipped_only_on_request():
    pos = np.array([[0.5, 0, 0], [-1.0, 0, 0], [0.25, 0, 0]])
    vel = np.array([[0.1, 0, 0], [0.1, 0, 0], [5.0, 0, 0]])
    c, o = hr.histogram(pos, vel, "vx", 2, (0.0, 1.0), dead_slots=True)
    assert c.tolist() == [1, 0] and o == 1
    c, o = hr.histogram(pos, vel, "vx", 2, (0.0, 1.0))
    assert c.tolist() == [2, 0] and o == 1


@pytest.mark.parametrize("axes,bins,ranges", [
    (("vx",), (0,), ((0, 1),)), (("vx", "vy"), (2048, 2049), ((0, 1), (0, 1))), (("vx", "vx"), (4, 4), ((0, 1), (0, 1))),
    (("w",), (4,), ((0, 1),)), (("x", "y", "z"), (2, 2, 2), ((0, 1),) * 3), (("vx",), (4,), ((1, 1),)), (("vx",), (4,), ((2, 1),)),
    (("vx",), (4,), ((np.nan, 1),)), (("vx",), (4,), ((0, np.inf),)), (("vx",), (4,), ((-1.7e308, 1.7e308),)),
    (("vx",), (4,), ((0, 5e-324),)),
])
def test_refused_requests(axes, bins, ranges):
    with pytest.raises(ValueError):
        hr.histogram(np.zeros((1, 3)), np.zeros((1, 3)), axes, bins, ranges)


def test_the_largest_request_is_accepted():
    c, o = hr.histogram(np.full((3, 3), 0.5), np.zeros((3, 3)), ("x", "vx"), (2048, 2048), ((0, 1), (-1, 1)))
    assert c.shape == (2048, 2048) and c[1024, 1024] == 3 and o == 0
