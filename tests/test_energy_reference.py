"""The reference of the energy diagnostics (tests/energy_reference.py) checked on its own, without a GPU: the vectorised
floor(d * 2^80) and its exact sums against the scalar routes (float.as_integer_ratio and fractions.Fraction) on doubles
chosen where a conversion goes wrong, and the conversion of the 128-bit sums to doubles on hand-made values."""
import math
from fractions import Fraction

import numpy as np
import pytest

import energy_reference as er


def awkward_doubles(rng, n=100000):
    """about n doubles: zeros of both signs, subnormals, exact multiples of 2^-80, both sides of 2^-70, 2^-17, 2^-16 and
    of the fixed-point bound 2^15 (and of sqrt(2^15), the bound of a component), values near -1e-20, which are floored
    wrongly when 2^64 + x is rounded, and a log-uniform spread over the whole range"""
    special = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072014e-308, 1e-310, -1e-310]
    for p in (-80, -79, -71, -70, -69, -65, -64, -63, -17, -16, -1, 0, 14):
        for k in ((1, 3, 2 ** 20 - 1) if p < -20 else (1, 3) if p < 14 else (1,)):
            special += [k * 2.0 ** p, -k * 2.0 ** p]
        x = 2.0 ** p
        for y in (np.nextafter(x, 0), np.nextafter(x, np.inf)):
            special += [float(y), -float(y)]
    below = float(np.nextafter(er.FIX_RANGE, 0))
    special += [below, -below, math.sqrt(below), -math.sqrt(below), 181.0, -181.0]
    special += [-1e-20, -1.0000000001e-20, 1e-20, -12288 * 2.0 ** -80, -12090 * 2.0 ** -80, -12089.5 * 2.0 ** -80]
    m = (n - len(special)) // 4
    multiples = rng.integers(-2 ** 62, 2 ** 62, m).astype(np.float64) * 2.0 ** -80       # exact multiples of 2^-80
    near = (rng.integers(-2 ** 20, 2 ** 20, m) * 2.0 ** -72) * (1 + rng.random(m) * 1e-3)
    thermal = rng.normal(0, 1e-5, m)
    logu = np.exp(rng.uniform(np.log(1e-320), np.log(3e4), m)) * rng.choice([-1.0, 1.0], m)
    out = np.concatenate([np.array(special, dtype=np.float64), multiples, near, thermal, logu])
    assert np.all(np.abs(out) < er.FIX_RANGE)
    return out


def test_fix_floor_agrees_with_exact_routes():
    d = awkward_doubles(np.random.default_rng(7))
    assert d.size > 99000
    vec = er.fix_floor(d)
    for x, got in zip(d.tolist(), vec):
        assert got == er.fix_floor_scalar(x), x
    # Fraction is slower: every special value and a sample of the rest
    for x in d[:200].tolist() + d[200::97].tolist():
        assert er.fix_floor_fraction(x) == er.fix_floor_scalar(x), x
    # the sums, grouped by shift in limbs, are the sums of the terms
    assert er.fix_sum(d) == sum(vec)
    for part in (d[:1], d[:7], d[5000:5001], d[-3:], d[:0]):
        assert er.fix_sum(part) == sum(er.fix_floor(part))


def test_fix_floor_known_values():
    assert er.fix_floor_scalar(0.0) == er.fix_floor_scalar(-0.0) == 0
    assert er.fix_floor_scalar(2.0 ** -80) == 1 and er.fix_floor_scalar(-2.0 ** -80) == -1
    assert er.fix_floor_scalar(2.0 ** -81) == 0 and er.fix_floor_scalar(-2.0 ** -81) == -1
    assert er.fix_floor_scalar(-5e-324) == -1 and er.fix_floor_scalar(5e-324) == 0
    assert er.fix_floor_scalar(-1e-20) == -12090          # (a rounded 2^64 + x makes it -12288)
    assert er.fix_floor_scalar(1.0) == 1 << 80 and er.fix_floor_scalar(-1.5) == -3 << 79
    # a component and its negation: their floors add to 0 for exact multiples of 2^-80, to -1 otherwise
    assert er.fix_floor_scalar(0.03) + er.fix_floor_scalar(-0.03) == 0
    assert er.fix_floor_scalar(1e-20) + er.fix_floor_scalar(-1e-20) == -1
    assert er.fix_floor(np.array([-1e-20, 2.0 ** -70, -2.0 ** -70, -2.0 ** -90])) == [-12090, 1024, -1024, -1]
    with pytest.raises(ValueError):
        er.fix_floor(np.array([np.nan]))
    with pytest.raises(ValueError):
        er.fix_sum(np.array([1.0, np.inf]))


def test_fix_sum_is_order_independent():
    rng = np.random.default_rng(3)
    d = rng.normal(0, 0.03, 300000) * np.exp(rng.uniform(-40, 0, 300000))
    s = er.fix_sum(d)
    assert er.fix_sum(d[::-1]) == s == er.fix_sum(rng.permutation(d))
    assert s == sum(er.fix_floor(d))
    # the exact sum lies within one unit per term below the real sum (a floor drops less than one unit)
    exact = sum(Fraction(x) for x in d[:2000].tolist()) * (1 << 80)
    s2 = er.fix_sum(d[:2000])
    assert exact - 2000 < s2 <= exact


def test_from_fix_is_correctly_rounded():
    u = 2.0 ** -80
    for s in (0, 1, -1, 12345, -12090, (1 << 53) - 1, -(1 << 53)):
        assert er.from_fix(s) == s * u
    # ties to even
    assert er.from_fix((1 << 53) + 1) == (1 << 53) * u
    assert er.from_fix((1 << 53) + 3) == ((1 << 53) + 4) * u
    assert er.from_fix(-(1 << 53) - 3) == -((1 << 53) + 4) * u
    # no double rounding: hi = 2^52 + 1, lo = 2^63 - 1 lies just below the tie between (2^52 + 1) 2^64 and (2^52 + 2) 2^64
    # (rounding lo first to 2^63 makes it a tie, which goes to the even neighbour, the wrong one)
    s = (((1 << 52) + 1) << 64) + (1 << 63) - 1
    assert er.from_fix(s) == float((1 << 52) + 1) * 2.0 ** 64 * u
    assert er.from_fix(-s) == -er.from_fix(s)
    assert er.from_fix(s + 2) == float((1 << 52) + 2) * 2.0 ** 64 * u
    # every value against Fraction (exact scale, nearest even)
    rng = np.random.default_rng(1)
    for _ in range(2000):
        s = int(rng.integers(-2 ** 62, 2 ** 62)) << int(rng.integers(0, 65))
        s += int(rng.integers(-2 ** 62, 2 ** 62))
        f = er.from_fix(s)
        exact = Fraction(s) * Fraction(1, 1 << 80)
        lo, hi = np.nextafter(f, -np.inf), np.nextafter(f, np.inf)
        assert abs(Fraction(f) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    # 128-bit wrap-around
    assert er.wrap128((1 << 128) - 1) == -1 and er.from_fix((1 << 128) - (1 << 70)) == -2.0 ** -10


def test_species_row_against_fraction():
    rng = np.random.default_rng(11)
    for dtype in (np.float32, np.float64):
        v = rng.normal(0, 0.03, (501, 3)).astype(dtype)
        v[::7] *= dtype(1e-13)
        row = er.species_row(v, 9.109e-31, 3.0)
        x = v.astype(np.float64)
        v2 = [((a * a + b * b) + c * c) for a, b, c in x.tolist()]
        sv2 = sum(math.floor(Fraction(t) * (1 << 80)) for t in v2)
        assert row["count"] == 501
        assert row["kinetic"] == 0.5 * 9.109e-31 * 3.0 * er.C * er.C * float(Fraction(sv2, 1 << 80))
        for a in range(3):
            sa = sum(math.floor(Fraction(t) * (1 << 80)) for t in x[:, a].tolist())
            assert row["momentum"][a] == 9.109e-31 * 3.0 * er.C * float(Fraction(sa, 1 << 80))
        assert row["speed_max"] == math.sqrt(max(v2))
    empty = er.species_row(np.zeros((0, 3), np.float32), 1.0, 1.0)
    assert empty["count"] == 0 and empty["kinetic"] == 0.0 and empty["speed_max"] == 0.0
    assert not np.any(empty["momentum"])


def test_square_sum_is_correctly_rounded():
    rng = np.random.default_rng(5)
    a = rng.normal(0, 1, (1000, 3)) * np.exp(rng.uniform(-20, 20, (1000, 1)))
    assert er.square_sum(a) == float(sum(Fraction(float(x)) for x in (a * a).ravel()))
