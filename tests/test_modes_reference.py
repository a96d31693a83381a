"""tests/modes_reference.py (the numpy restatement of the rule of fpic_modes_*) against numpy.fft.fftn(F) / N at the requested
bins, on the shapes the GPU tests use; its naive float64 evaluation against its long-double one within the derived bound;
the tables' two properties; the slab form adding up to the box.  No GPU, nothing of the library."""
import numpy as np
import pytest

import modes_reference as mr

SHAPES = [(12, 10, 9), (5, 6, 7), (2, 16, 3), (16, 16, 16)]


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_equals_fftn(shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(sum(shape))
    F = rng.normal(0, 1, (nz, ny, nx, 3))
    modes = mr.mode_list(shape, rng)
    got = mr.amplitudes(F, modes)
    tol = mr.tolerance(F)
    for q in range(3):
        full = np.fft.fftn(F[..., q]) / F[..., q].size            # axes (z, y, x)
        want = np.array([full[m[2] % nz, m[1] % ny, m[0] % nx] for m in modes])
        # fftn is one more order of the same float64 sum: it lies within the bound of the long-double reference
        assert np.abs(got[:, q].real.astype(np.float64) - want.real).max() <= tol[q]
        assert np.abs(got[:, q].imag.astype(np.float64) - want.imag).max() <= tol[q]
        assert np.abs(want).max() > 1e3 * tol[q]                  # (the comparison sees the values)
    # the mean is the (0, 0, 0) amplitude
    assert abs(complex(got[0, 0]) - F[..., 0].mean()) <= tol[0]


@pytest.mark.parametrize("shape", [(5, 6, 7), (2, 16, 3), (12, 10, 9)])
def test_naive_float64_is_far_inside_the_bound(shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(7 + nx)
    F = rng.normal(0, 1, (nz, ny, nx))
    modes = mr.mode_list(shape, rng, extra=6)
    ref, got = mr.amplitudes(F, modes), mr.naive(F, modes)
    err = max(np.abs(got.real - ref.real.astype(np.float64)).max(), np.abs(got.imag - ref.imag.astype(np.float64)).max())
    assert err <= 0.05 * mr.tolerance(F)
    # ... and a wrong sign, index or plane is many orders outside it
    wrong = mr.amplitudes(np.roll(F, 1, axis=0), modes)
    assert np.abs(wrong[3] - ref[3]) > 1e9 * mr.tolerance(F)       # mode (0, 0, 1)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 8, 9, 10, 12, 33, 256])
def test_table_properties(n):
    w = mr.table(n)
    for t in range(n):
        if (4 * t) % n == 0:
            assert tuple(w[t]) == [(1, 0), (0, -1), (-1, 0), (0, 1)][4 * t // n]
        if 0 < t and 2 * t != n:
            assert w[n - t, 0].tobytes() == w[t, 0].tobytes() and w[n - t, 1].tobytes() == (-w[t, 1]).tobytes()
    # every entry is the long-double value rounded once (numpy's own float64 exp(-2j pi t / n) is several times further off)
    assert np.abs(w.astype(np.longdouble) - mr.table(n, np.longdouble)).max() <= 2.0 ** -53
    assert np.abs(w[:, 0] + 1j * w[:, 1] - np.exp(-2j * np.pi * np.arange(n) / n)).max() < 2e-15


def test_slabs_add_up_and_negative_modes_are_conjugates():
    shape = (6, 5, 12)
    rng = np.random.default_rng(3)
    F = rng.normal(0, 1, (12, 5, 6, 2))
    modes = mr.mode_list(shape, rng)
    whole = mr.amplitudes(F, modes)
    parts = sum(mr.amplitudes_slab(F[k0:k0 + 4], modes, k0, 12) for k0 in (0, 4, 8))
    assert np.abs(parts - whole).max() < 1e-17
    neg = mr.amplitudes(F, -modes)
    assert np.abs(neg - np.conj(whole)).max() < 1e-17
    assert mr.reduce(-1, 7) == 6 and mr.reduce(-7, 7) == 0 and mr.reduce(-3, 6) == 3
