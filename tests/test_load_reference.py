"""The numpy restatement of the loader's rule (tests/load_reference.py) proved on the CPU: the generator against the Random123
known answers and the oracle library, the rounded parts against 50-digit values, the moments and the uniformity of a large
draw, the loaded mode's density amplitude, the pairing, and five wrong variants that the reference must tell apart from
itself.  The kernel is compared with this reference in tests/test_gpu_load.py.

Deviation of the reference's normals and sines from the 50-digit values over the 10^5 particles of load_exact.ulp_scene,
in float64 ulps of the value (measured here, asserted below REF_ULPS): normals 3.02, sine 1.66."""
import ctypes
import os

import numpy as np
import pytest

import load_exact as exact
import load_reference as ref
from helpers import ROOT

L = (1e-3, 2e-3, 1.5e-3)
# The reference's own deviation stays below this (tests/test_gpu_load.py adds it to the kernel's bound): libm's log, sin and
# cos within 1 ulp, sqrt within 1/2 (halving what the logarithm brought), the product pi r and the constant pi within 1 more,
# the final product within 1/2
REF_ULPS = 4.0


def test_known_answer_vectors():
    hexes = lambda *a: ["%08x" % int(w[0]) for w in ref.philox(*a)]
    assert hexes(0, 0, 0, 0, 0, 0) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = 0xFFFFFFFF
    assert hexes(ones, ones, ones, ones, ones, ones) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert hexes(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_agrees_with_the_oracle_library_on_random_counters():
    so = os.path.join(ROOT, "oracle", "libpic_oracle.so")
    if not os.path.exists(so):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(so)
    u32 = ctypes.c_uint32
    lib.orc_philox4x32_10.argtypes = [u32] * 6 + [ctypes.POINTER(u32 * 4)]
    lib.orc_philox4x32_10.restype = None
    rng = np.random.default_rng(20261019)
    args = rng.integers(0, 1 << 32, size=(10000, 6), dtype=np.uint64)
    mine = np.stack(ref.philox(*args.T), axis=1)
    out = (u32 * 4)()
    for k in range(args.shape[0]):
        lib.orc_philox4x32_10(*[int(v) for v in args[k]], ctypes.byref(out))
        assert list(out) == [int(v) for v in mine[k]], k


@pytest.fixture(scope="module")
def exact_values():
    req = exact.ulp_scene(L)
    i = np.arange(exact.ULP_PARTICLES)
    return req, i, exact.exact_normals_and_sines(req, i)


def test_normals_and_sines_against_fifty_digits(exact_values):
    req, i, (hi, lo) = exact_values
    _, theta = ref.base(req, i)
    got = np.concatenate([ref.normals(req, i), ref.sinpi(2.0 * (theta + req["vphase"]))[:, None]], axis=1)
    d = exact.ulps(got, hi, lo)
    print("reference against 50 digits, largest deviation in ulps: normals %.3f %.3f %.3f, sine %.3f" % tuple(d.max(axis=0)))
    assert d.max() < REF_ULPS
    assert np.abs(hi[:, :3]).max() < 6.76


def test_float_rounding_of_the_reference_is_that_of_the_exact_values(exact_values):
    # an fp32 handle stores the float rounding: the reference's float64 error moves it on a share of K 2^-29 of the values at
    # most; the GPU test's cap for values that are not bit-equal is 1e-4
    req, i, (hi, lo) = exact_values
    _, theta = ref.base(req, i)
    got = np.concatenate([ref.normals(req, i), ref.sinpi(2.0 * (theta + req["vphase"]))[:, None]], axis=1)
    # the float rounding of hi + lo: hi is within half a float64 ulp of the value, a float boundary lies 2^28 float64 ulps off
    near = hi.astype(np.float32)
    moved = got.astype(np.float32) != near
    assert moved.mean() <= 1e-4
    assert np.all(np.abs(got.astype(np.float32)[moved].astype(np.float64) - near[moved]) <= np.spacing(np.abs(near[moved])))


N = 1 << 20


def test_moments_of_the_velocities():
    drift, vth = np.array([0.01, -0.02, 0.0]), np.array([0.05, 0.02, 0.1])
    v = ref.velocities(ref.request(L, seed=11, stream=3, drift=drift, vth=vth), np.arange(N))
    for a in range(3):
        assert abs(v[:, a].mean() - drift[a]) <= 5 * vth[a] / np.sqrt(N)
        assert abs(v[:, a].var() - vth[a] ** 2) <= 5 * vth[a] ** 2 * np.sqrt(2.0 / N)     # var of s^2: 2 sigma^4 / n
    c = np.corrcoef(v.T)
    assert np.abs(c[np.triu_indices(3, 1)]).max() <= 5 / np.sqrt(N)


@pytest.mark.parametrize("lattice", [False, True])
def test_positions_are_uniform(lattice):
    lo, hi = np.array([0.1, 0.0, 0.25]) * L, np.array([0.9, 1.0, 0.75]) * L
    req = ref.request(L, seed=5, stream=1, lo=lo, hi=hi, lattice=lattice)
    p = ref.positions(req, np.arange(N))
    assert np.all(p >= req["lo_f"]) and np.all(p < req["lo_f"] + req["w_f"])
    for a in range(3):
        counts = np.bincount(np.minimum(((p[:, a] - req["lo_f"][a]) / req["w_f"][a] * 64).astype(int), 63), minlength=64)
        chi2 = ((counts - N / 64) ** 2 / (N / 64)).sum()
        # 63 degrees of freedom: mean 63, variance 126.  The lattice is more even than a random draw by construction (its
        # chi^2 is far BELOW the band), so for it only the upper edge is a statement about uniformity
        assert chi2 <= 63 + 5 * np.sqrt(126)
        if not lattice:
            assert chi2 >= 63 - 5 * np.sqrt(126)


def test_a_loaded_mode_has_the_density_amplitude():
    eps = 0.01
    i = np.arange(N)
    plain = ref.request(L, seed=9, lattice=True)
    req = ref.request(L, seed=9, lattice=True, mode=(2, 0, 0), xamp=(eps * L[0] / (2 * np.pi * 2), 0, 0))
    amp = lambda x: abs(np.exp(-2j * np.pi * 2 * x).mean())
    noise = amp(ref.positions(plain, i)[:, 0])
    # x = x0 + (eps / k) sin(k x0): the mean of exp(-i k x) over a uniform x0 is -J1(eps) = -(eps / 2) (1 - eps^2 / 8 + ...);
    # the lattice sum of a smooth integrand misses it by about what it leaves of the unperturbed one (`noise`, 1 / N at least)
    got = amp(ref.stored_positions(req, i, np.float64)[:, 0])
    assert noise < 1e-4 * eps
    assert abs(got - eps / 2) <= 4 * max(noise, 1.0 / N) + eps ** 3 / 16 * 1.01


def test_paired_halves_cancel_bit_for_bit():
    req = ref.request(L, seed=3, stream=2, vth=(0.05, 0.02, 0.1), paired=True)
    v = ref.velocities(req, np.arange(3, 3 + 4096))            # (starts odd: the pairs are (2k, 2k + 1), not neighbours of the range)
    assert np.all(v[1:-1:2] + v[2:-1:2] == 0) and np.all(v[1:-1:2] != 0)
    assert np.array_equal(ref.velocities(req, np.arange(1 << 12)).sum(axis=0), np.zeros(3))    # exact: the terms cancel in pairs in any order
    drifting = ref.velocities(dict(req, drift=np.array([0.01, 0, 0])), np.arange(8))
    assert np.all(drifting[0::2, 0] + drifting[1::2, 0] != 0)


def test_five_wrong_variants_differ_from_the_reference():
    i = np.arange(20000)
    sub = dict(lo=np.array([0.1, 0.0, 0.25]) * L, hi=np.array([0.9, 1.0, 0.75]) * L)
    far = lambda a, b: np.abs(a - b) > 1000 * np.spacing(np.abs(a))     # beyond any bound of a few ulps
    # 1. x and y words swapped: every particle's position
    req = ref.request(L, seed=1, **sub)
    assert (ref.positions(req, i) != ref.positions(req, i, "swapped_words")).any(axis=1).mean() > 0.99
    # 2. a fused multiply-add: x = 0.1 + f 0.8 is rounded twice by the rule, once by the fused form; they differ, by one ulp,
    #    where the product's rounding decides the sum's — more than a tenth of the particles (y has lo = 0: the sum is exact)
    j = i[:4000]
    a, b = ref.positions(req, j), ref.positions(req, j, "fma")
    assert 0.1 < (a[:, 0] != b[:, 0]).mean() < 0.5 and np.array_equal(a[:, 1], b[:, 1])
    assert np.all(np.abs(a - b) <= np.spacing(a))
    # 3. u1 = w 2^-32 without the half: every normal of the two radii moves by far more than an ulp
    req = ref.request(L, seed=1, vth=1.0)
    with np.errstate(invalid="ignore"):
        assert far(ref.velocities(req, i), ref.velocities(req, i, "no_half")).all(axis=1).mean() > 0.99
    # 4. the velocity's phase from the displaced position
    req = ref.request(L, seed=1, mode=(2, 1, -3), xamp=(1e-5, 0, 2e-5), vamp=(1e-3, 0, 0), vphase=0.1)
    assert far(ref.velocities(req, i)[:, 0], ref.velocities(req, i, "theta_displaced")[:, 0]).mean() > 0.99
    # 5. the cell plane by rounding: the upper half of every cell goes to the next plane
    z = ref.stored_positions(ref.request(L, seed=1), i, np.float32)[:, 2]
    share = (ref.plane(z, 16) != ref.plane(z, 16, "round_plane")).mean()
    assert 0.45 < share < 0.55
    assert ref.plane(z, 16).min() == 0 and ref.plane(z, 16).max() == 15
