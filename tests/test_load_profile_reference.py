"""The numpy restatement of the profiled load's rule (tests/load_profile_reference.py) on its own, without the library: the
inverse of the cumulative mass is well defined on awkward tables (no NaN, no hit in an interval without mass, 0 <= f' < 1,
monotone in the word), a random load has the table's statistics and a lattice load is a quiet start on it, the thermal and
shear tables act as stated, and two species on one stream coincide.  The product is held to this reference bit for bit by
tests/test_load_profile_host.py (g++) and tests/test_gpu_load_profile.py (the kernels)."""
import numpy as np
import pytest

import load_profile_reference as pref
import load_reference as ref

L = (0.016, 0.016, 0.016)
N = 200000


def gaussian(nodes=1025, sigma=0.2):
    x = np.linspace(0.0, 1.0, nodes)
    return np.exp(-0.5 * ((x - 0.5) / sigma) ** 2)


# the tables the rule was designed on, and a triangle
TABLES = {
    "ramp_from_0": [0.0, 1.0],
    "ramp_to_0": [1.0, 0.0],
    "holes_middle_end": [1, 1, 0, 0, 0, 2, 0],
    "holes_both_ends": [0, 0, 1, 3, 0, 0],
    "gaussian_1025": gaussian(),
    "tiny_ends": [1e-300, 1, 1e-300],
    "triangle": [0.0, 1.0, 0.0],
}


def words(n=2000000):
    rng = np.random.default_rng(20)
    w = np.sort(np.concatenate([rng.integers(0, 1 << 32, n - 2, dtype=np.uint64), np.array([0, (1 << 32) - 1], dtype=np.uint64)]))
    assert w[0] == 0 and w[-1] == (1 << 32) - 1
    return w


WORDS = words()


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_inverse_is_well_defined(name):
    d = np.asarray(TABLES[name], dtype=np.float64)
    f = WORDS.astype(np.float64) * 2.0 ** -32
    fq, j, s = pref.warp(d, f)
    assert not np.isnan(fq).any() and not np.isnan(s).any()
    assert np.all(fq >= 0) and np.all(fq < 1) and np.all(s >= 0) and np.all(s <= 1)
    mass = 0.5 * (d[:-1] + d[1:])
    assert np.all(mass[j] > 0)                                        # never an interval without mass
    assert np.all(np.diff(fq) >= 0) and np.all(np.diff(j) >= 0)       # monotone in the word
    assert np.unique(j).size == np.count_nonzero(mass > 0)            # and every interval with mass is reached


def test_a_random_load_has_the_tables_statistics_and_a_lattice_load_is_quiet():
    d = gaussian()
    K = d.size - 1
    C = pref.cumulative(d)
    expect = N * np.diff(C) / C[K]
    i = np.arange(N)
    req = pref.request(L, density=(d, None, None), seed=0xFEED, stream=1)
    f, j = pref.fractions(req, i)
    counts = np.bincount(j[:, 0], minlength=K)
    assert np.array_equal(j[:, 1:], np.full((N, 2), -1)) and np.array_equal(f[:, 1:], ref.fractions(req, i)[:, 1:])
    assert np.array_equal(np.minimum((f[:, 0] * K).astype(np.int64), K - 1), j[:, 0])
    chi2, dof = float(((counts - expect) ** 2 / expect).sum()), K - 1
    print("chi^2 %.1f, dof %d, per dof %.3f" % (chi2, dof, chi2 / dof))
    assert abs(chi2 - dof) <= 5 * np.sqrt(2 * dof)
    # The Kronecker lattice.  The figure first proposed for it - every interval's count within 2 of its expectation + 1 - is
    # NOT met by the reference: the largest |count - expectation| measured over the 1024 intervals at 2e5 particles is 6.13
    # for this request (6.97, 7.10, 7.48 for three other seeds and streams; 157-183 intervals are off by more than 3).  That
    # is the discrepancy of the 1-D sequence (i mult_0 + shift) mod 2^32, which grows like log N, not a fault of the
    # inverse.  The bound is twice the measured figure, 12.25; a random load's largest deviation here is about 3.3 standard
    # deviations of a count of 195, i.e. 46, so the bound still tells a quiet start from a random one.
    lat = pref.request(L, density=(d, None, None), seed=0xFEED, stream=1, lattice=True)
    _, jl = pref.fractions(lat, i)
    off = np.abs(np.bincount(jl[:, 0], minlength=K) - expect)
    print("lattice: largest |count - expectation| %.3f; random: %.3f" % (off.max(), np.abs(counts - expect).max()))
    assert np.all(off <= 12.25)
    assert np.abs(counts - expect).max() > 2 * 12.25


def test_a_thermal_table_scales_the_spread():
    vth = 1e-3
    i = np.arange(N)
    req = pref.request(L, thermal=([1.0, 2.0], None, None), vth=vth, seed=99, stream=4)
    v = pref.velocities(req, i)
    _, _, f = pref.base(req, i)
    for k in range(10):
        inside = (f[:, 0] >= 0.1 * k) & (f[:, 0] < 0.1 * (k + 1))
        n, want = inside.sum(), vth * (1.0 + 0.1 * (k + 0.5))
        got = v[inside, 0].std()
        assert n > N // 20 and abs(got - want) <= 5 * want / np.sqrt(2 * n), (k, got, want)
    # y and z carry the same factor; without a table the plain rule's velocities
    assert np.array_equal(v, (vth * pref.lookup([1.0, 2.0], f[:, 0])[0])[:, None] * ref.normals(req, i) + 0.0)
    assert np.array_equal(pref.velocities(pref.request(L, vth=vth, seed=99, stream=4), i), ref.velocities(ref.request(L, vth=vth, seed=99, stream=4), i))


def test_a_shear_table_adds_to_the_drift_bit_for_bit():
    i = np.arange(4000)
    tab = np.array([-0.02, 0.03, 0.01, -0.05])
    d = [0.0, 1.0, 3.0]
    for lattice in (False, True):
        req = pref.request(L, density=(None, d, None), shear=dict(axis=1, component=2, values=tab), drift=(0.01, 0.0, -0.005), vth=0, seed=7, lattice=lattice)
        v = pref.velocities(req, i)
        f, _ = pref.fractions(req, i)
        g = f[:, 1] * 3.0
        k = np.minimum(g.astype(np.int64), 2)
        want = -0.005 + (tab[k] + (tab[k + 1] - tab[k]) * (g - k))
        assert v[:, 2].tobytes() == want.tobytes()
        assert np.all(v[:, 0] == 0.01) and np.all(v[:, 1] == 0.0) and not np.signbit(v[:, 1]).any()
        assert want.min() < -0.02 and want.max() > 0.0


def test_two_species_on_one_stream_coincide():
    i = np.arange(4000)
    d = (gaussian(65), [0, 0, 1, 3, 0, 0], [1.0, 0.0])
    a = pref.request(L, density=d, seed=31, stream=3, vth=0.01, mode=(1, 0, 0), xamp=(1e-4, 0, 0))
    b = pref.request(L, density=d, seed=31, stream=3, vth=0.01, mode=(1, 0, 0), xamp=(1e-4, 0, 0))
    c = pref.request(L, density=d, seed=31, stream=4, vth=0.01, mode=(1, 0, 0), xamp=(1e-4, 0, 0))
    for T in (np.float32, np.float64):
        assert pref.stored_positions(a, i, T).tobytes() == pref.stored_positions(b, i, T).tobytes()
        assert pref.stored_positions(a, i, T).tobytes() != pref.stored_positions(c, i, T).tobytes()
    assert pref.velocities(a, i).tobytes() == pref.velocities(b, i).tobytes()


def test_without_tables_the_reference_is_the_plain_one():
    i = np.arange(3000)
    kw = dict(seed=5, stream=2, drift=(0.01, 0, 0), vth=0.02, mode=(1, 2, 0), xamp=(1e-5, 0, 0), vamp=1e-3, paired=True, lo=0.001, hi=0.012)
    for T in (np.float32, np.float64):
        assert pref.stored_positions(pref.request(L, **kw), i, T).tobytes() == ref.stored_positions(ref.request(L, **kw), i, T).tobytes()
    assert pref.velocities(pref.request(L, **kw), i).tobytes() == ref.velocities(ref.request(L, **kw), i).tobytes()
