"""The numpy restatement of the series diagnostic's point rule (tests/series_reference.py) checked on its own, without the
library: a point on a node gets the node's record exactly, the weights add up to 2^42, a point and its periodic images get
the same weights, and a field linear in one coordinate is reproduced to rounding away from the periodic seam."""
import numpy as np
import pytest

import series_reference as sr

GRIDS = [(16, 16, 16), (12, 20, 24), (24, 10, 36), (7, 9, 11)]      # (at most 64 nodes per axis: the nodal identity's range in float32)
LENGTHS = [(0.016, 0.016, 0.016), (0.012, 0.02, 0.024), (1.0, 0.37, 2.9), (7e-3, 0.3, 11.0)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,L", list(zip(GRIDS, LENGTHS)))
@pytest.mark.parametrize("form", [0, 1])
def test_a_point_on_a_node_gets_the_node_record(dtype, shape, L, form):
    rng = np.random.default_rng(sum(shape) + form)
    nodes = shape[0] * shape[1] * shape[2]
    E = rng.normal(0, 1e4, (nodes, 4)).astype(dtype)
    B = rng.normal(0, 0.05, (nodes, 4)).astype(dtype)
    pts = sr.node_points(L, shape, form)
    idx, W, k = sr.weights(pts, L, shape, dtype)
    # all the weight is on the node itself: as the lower node of its own cell, or — where u * n lands just below the integer —
    # as the upper node of the cell before it, whose upper weights round to 16384
    full = W == sr.ONE
    assert (full.sum(axis=1) == 1).all() and not W[~full].any()
    assert np.array_equal(idx[full], np.arange(nodes))
    assert (((np.arange(nodes) // (shape[0] * shape[1]) - k) % shape[2]) <= 1).all()
    rows = sr.point_rows(pts, L, shape, E, B)
    assert rows[:, 0:4].tobytes() == E.astype(np.float64).tobytes()
    assert rows[:, 4:7].tobytes() == np.ascontiguousarray(B[:, :3].astype(np.float64)).tobytes()
    assert (rows[:, 7] == 1).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,L", list(zip(GRIDS, LENGTHS)))
def test_weights_add_up_and_wrap(dtype, shape, L):
    rng = np.random.default_rng(11)
    p = rng.random((4000, 3)) * L
    idx, W, k = sr.weights(p, L, shape, dtype)
    assert (W >= 0).all() and np.array_equal(W.sum(axis=1), np.full(len(p), sr.ONE))
    assert (idx >= 0).all() and (idx < shape[0] * shape[1] * shape[2]).all() and (k >= 0).all() and (k < shape[2]).all()
    for shift in (1.0, -3.0):
        idx2, W2, k2 = sr.weights(p + shift * np.array(L), L, shape, dtype)
        # (an image differs from the point by a rounding of the division: the cell and the 2^-14 weights only move where
        # the point lies within that rounding of a weight's step — none of these does)
        assert np.array_equal(idx, idx2) and np.array_equal(W, W2) and np.array_equal(k, k2)
    # the seam itself and what rounds onto it
    edge = np.array([[0.0, 0.0, 0.0], [L[0], L[1], L[2]], [-L[0], 2 * L[1], -0.0], [np.nextafter(L[0], 0), L[1] * (1 - 2.0 ** -60), -1e-300]])
    idx, W, k = sr.weights(edge, L, shape, dtype)
    assert np.array_equal(W.sum(axis=1), np.full(len(edge), sr.ONE))
    assert (idx[:3, 0] == 0).all() and (W[:3, 0] == sr.ONE).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_linear_field_is_reproduced(dtype, axis):
    shape, L = (12, 20, 24), (0.012, 0.02, 0.024)
    rng = np.random.default_rng(5 + axis)
    coord = [np.arange(shape[a], dtype=np.float64) * (L[a] / shape[a]) for a in range(3)]
    z, y, x = np.meshgrid(coord[2], coord[1], coord[0], indexing="ij")
    F = ((3.0 + 1e3 * (x, y, z)[axis]).ravel()[:, None] * np.ones(4)).astype(dtype)
    # away from the seam: cells 0 .. n - 2 along the axis, where the upper node is not the wrapped one
    p = rng.random((3000, 3)) * L
    p[:, axis] *= (shape[axis] - 1.001) / shape[axis]
    idx, W, _ = sr.weights(p, L, shape, dtype)
    got = sr.interpolate(F, idx, W)
    # the exact value of the rule: the two node values along the axis with the integer weights w0, w1 (the other axes'
    # weights add up to 16384 each), in extended precision
    i, w1 = sr.axis(sr.unit(p[:, axis], L[axis]).astype(dtype), shape[axis])
    line = (3.0 + 1e3 * coord[axis]).astype(dtype).astype(np.longdouble)
    want = ((16384 - w1).astype(np.longdouble) * line[i] + w1.astype(np.longdouble) * line[i + 1]) / np.longdouble(16384)
    err = np.abs(got.astype(np.longdouble) - want[:, None]).max()
    assert err <= 2 * np.finfo(np.float64).eps * np.abs(F.astype(np.float64)).max(), float(err)
    # ... and it is the linear function of the position to the weights' resolution (2^-14 of a cell; the state's rounding of u)
    true = 3.0 + 1e3 * p[:, axis]
    step = 1e3 * L[axis] / shape[axis]
    assert np.abs(got[:, 0] - true).max() <= step * (2.0 ** -15 + shape[axis] * 4 * np.finfo(dtype).eps) + 32 * np.finfo(dtype).eps     # (+ the field's own rounding, |F| < 32)


def test_columns_are_named():
    assert len(sr.POINT_COLUMNS) == len(sr.TRACER_COLUMNS) == 8
    assert sr.POINT_COLUMNS.index("present") == 7 and sr.TRACER_COLUMNS.index("found") == 6
