"""The numpy restatement of the radial load's rule (tests/load_radial_reference.py) on its own, without the library: the
radius is monotone in the word, the halvings bracket the mass to the last bit, no particle falls in an interval without
mass, a random load has the table's statistics and a lattice load is a quiet start on it, the sphere's directions are
isotropic, the thermal and flow tables act as stated — and each of the reference's four deliberate mutations fails one of
these checks.  The product is held to this reference bit for bit by tests/test_load_radial_host.py (g++) and
tests/test_gpu_load_radial.py (the kernels)."""
import numpy as np
import pytest

import load_profile_reference as pref
import load_radial_reference as rref
import load_reference as ref

L = (0.016, 0.016, 0.016)
CENTER = (0.008, 0.008, 0.008)
R_MAX = 0.004
N = 200003
GEOMETRIES = ("sphere", "cylinder")
X = np.linspace(0.0, 1.0, 65)

# four tables of 65 nodes: a shell, a Gaussian, a hot core with a shell, and a flat one
TABLES = {
    "shell": np.where((X >= 0.6) & (X <= 0.9), 1.0, 0.0),
    "gaussian": np.exp(-0.5 * ((X - 0.5) / 0.15) ** 2),
    "core_and_shell": np.where(X < 0.3, 0.2, 0.0) + np.where((X >= 0.6) & (X <= 0.85), 1.0, 0.0),
    "flat": np.ones(65),
}
# tables with holes in the middle and at both ends, and nearly massless ends
AWKWARD = {
    "holes_middle_end": [1, 1, 0, 0, 0, 2, 0],
    "holes_both_ends": [0, 0, 1, 3, 0, 0],
    "tiny_ends": [1e-300, 1, 1e-300],
    "ramp_from_0": [0.0, 1.0],
    "ramp_to_0": [1.0, 0.0],
}


def interval_shares(geometry, d):
    """the share of the mass in each interval, from the antiderivatives taken between the nodes (not the reference's Horner form)"""
    d = np.asarray(d, dtype=np.float64)
    j, d0, D = np.arange(d.size - 1, dtype=np.float64), d[:-1], np.diff(d)
    p2, p3, p4 = (j + 1) ** 2 - j ** 2, (j + 1) ** 3 - j ** 3, (j + 1) ** 4 - j ** 4
    m = d0 * p3 / 3 + D * (p4 / 4 - j * p3 / 3) if geometry == "sphere" else d0 * p2 / 2 + D * (p3 / 3 - j * p2 / 2)
    return m / m.sum()


def words(n=400000):
    rng = np.random.default_rng(20)
    return np.sort(np.concatenate([rng.integers(0, 1 << 32, n - 2, dtype=np.uint64), np.array([0, (1 << 32) - 1], dtype=np.uint64)]))


WORDS = words()


def body(geometry, density, axis=0, **kw):
    return rref.request(L, geometry, CENTER, R_MAX, axis=axis, density=density, **kw)


# ---- the checks; `variant` runs them on a mutated reference
def check_the_radius(geometry, d, variant=None):
    d = np.asarray(d, dtype=np.float64)
    K = d.size - 1
    f = WORDS.astype(np.float64) * 2.0 ** -32
    rho, j, s = rref.radius(geometry, d, f, variant)
    assert not np.isnan(rho).any() and np.all(rho >= 0) and np.all(rho < 1) and np.all(s >= 0) and np.all(s < 1)
    assert np.all(np.diff(rho) >= 0) and np.all(np.diff(j) >= 0)                        # monotone in the word
    shares = interval_shares(geometry, d)
    assert np.all(shares[j] > 0)                                                         # never an interval without mass
    assert np.all(np.isin(np.flatnonzero(shares > 1e-3), j))                             # and every interval with mass to speak of (400 words) is reached
    # the halvings bracket r: M_j(s) <= r < M_j(s + 2^-52), the ends of [0, 1] excepted (lo and hi of the last halving: hi is
    # 1 or a place found above r, lo is 0 or a place found at or below it) ...
    C = rref.cumulative(geometry, d)
    a = rref.coefficients(geometry, d[j], d[j + 1], j)
    r = f * C[K] - C[j]
    at, above = rref.mass(geometry, a, s), rref.mass(geometry, a, s + 2.0 ** -52)
    assert np.all((at <= r) | (s == 0)) and np.all((above > r) | (s + 2.0 ** -52 == 1))
    # ... so |M_j(s) - r| is at most the mass of 2^-52 of the interval - its density at most max(d[j], d[j+1]), its weight at
    # most (j + 1)^2 or j + 1 - plus the rounding of the two evaluations: at most seven operations each, every one rounded
    # by half a last bit of a partial result that does not exceed M_j(1) <= C[K], so 2 x 3.5 last bits of C[K]
    inner = (s > 0) & (s + 2.0 ** -52 < 1)
    slice_mass = 2.0 ** -52 * np.maximum(d[j], d[j + 1]) * (j + 1.0) ** (2 if geometry == "sphere" else 1)
    assert np.all(np.abs(at - r)[inner] <= slice_mass[inner] + 7 * np.spacing(C[K]))
    return rho, j


def interval_counts(geometry, d, lattice, variant=None):
    req = body(geometry, d, seed=0xFEED, stream=1, lattice=lattice)
    return np.bincount(rref.parts(req, np.arange(N), variant)["j"], minlength=len(d) - 1)


def check_a_random_load(geometry, name, variant=None):
    share = interval_shares(geometry, TABLES[name])
    counts = interval_counts(geometry, TABLES[name], False, variant)
    assert np.all(counts[share == 0] == 0)
    sigma = np.sqrt(N * share * (1 - share))
    worst = (np.abs(counts - N * share)[share > 0] / sigma[share > 0]).max()
    print("%s %s random: largest deviation of an interval's count %.2f sigma" % (geometry, name, worst))
    assert worst <= 4.5
    return worst


def check_the_thermal_table(variant=None):
    # hot inside, cold outside, displaced by a quarter of the radius: the spread of a particle follows where it was BEFORE
    i = np.arange(20000)
    tab = [1.0, 1.0, 0.0, 0.0]
    req = body("sphere", None, thermal=tab, vth=1e-3, seed=12, stream=2, mode=(1, 0, 0), xamp=(0.25 * R_MAX, 0, 0))
    v, pt = rref.velocities(req, i, variant), rref.parts(req, i)
    want = (1e-3 * pref.lookup(tab, pt["rho"])[0])[:, None] * ref.normals(req, i) + 0.0
    assert np.array_equal(v, want)
    assert np.all(v[pt["rho"] >= 2.0 / 3.0] == 0) and np.count_nonzero(pt["rho"] >= 2.0 / 3.0) > 10000


def check_the_azimuthal_flow(variant=None):
    # a rigid rotation about each axis in turn: u_t = omega rho, so the velocity is omega a-hat x (the offset from the axis)
    i = np.arange(4000)
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        req = body("cylinder", TABLES["gaussian"], axis=axis, flow_azimuthal=[0.0, 0.02], vth=0, seed=3, stream=axis)
        v, pt = rref.velocities(req, i, variant), rref.parts(req, i)
        assert np.all(v[:, axis] == 0)
        assert np.array_equal(v[:, b], 0.0 + (0.02 * pt["rho"]) * -pt["dir"][:, c]) and np.array_equal(v[:, c], 0.0 + (0.02 * pt["rho"]) * pt["dir"][:, b])
        spin = pt["dir"][:, b] * v[:, c] - pt["dir"][:, c] * v[:, b]                 # (r-hat x v) along the axis: counter-clockwise
        assert np.all(spin >= 0) and np.allclose(spin, 0.02 * pt["rho"], rtol=1e-12, atol=0)


# ---- the tests
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", sorted(AWKWARD) + sorted(TABLES))
def test_the_radius_is_monotone_and_the_halvings_bracket_the_mass(geometry, name):
    check_the_radius(geometry, AWKWARD[name] if name in AWKWARD else TABLES[name])


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_holes_are_skipped(geometry):
    _, j = check_the_radius(geometry, AWKWARD["holes_middle_end"])
    assert set(j) == {0, 1, 4, 5}
    _, j = check_the_radius(geometry, AWKWARD["holes_both_ends"])
    assert set(j) == {1, 2, 3} and j[0] == 1 and j[-1] == 3
    _, j = check_the_radius(geometry, AWKWARD["tiny_ends"])
    assert set(j) == {0, 1}


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", sorted(TABLES))
def test_a_random_load_has_the_tables_interval_counts(geometry, name):
    """largest deviation met: 3.27 sigma (cylinder, flat)"""
    check_a_random_load(geometry, name)


def test_a_lattice_load_is_a_quiet_start():
    """The largest |count - expectation| of an interval over the four tables and both geometries, 200003 particles and 64
    intervals, measured on this reference: 7.31 (sphere: shell 7.31, Gaussian 5.26, core and shell 6.03, flat 5.52; cylinder:
    3.97, 4.21, 3.75, 4.55).  The bound is twice that, 14.62 - the margin the profiled load's test takes for the same quantity;
    a random load's deviations on the same tables are 170 to 320."""
    worst = 0.0
    for geometry in GEOMETRIES:
        for name in sorted(TABLES):
            expect = N * interval_shares(geometry, TABLES[name])
            off = np.abs(interval_counts(geometry, TABLES[name], True) - expect).max()
            print("%s %s lattice: largest |count - expectation| %.3f" % (geometry, name, off))
            worst = max(worst, off)
    assert worst <= 14.62


def test_the_spheres_directions_are_isotropic():
    i = np.arange(N)
    centroid = {}
    for lattice in (False, True):
        req = body("sphere", TABLES["core_and_shell"], seed=0xFEED, stream=1, lattice=lattice)
        p, _, pt = rref.base(req, i)
        if not lattice:
            # mu is uniform on [-1, 1): 32 bins, each count within 4.5 binomial sigma
            counts = np.bincount(np.minimum(((pt["mu"] + 1.0) * 16.0).astype(np.int64), 31), minlength=32)
            assert np.abs(counts - N / 32).max() <= 4.5 * np.sqrt(N / 32 * (1 - 1 / 32))
        assert np.allclose((pt["dir"] ** 2).sum(axis=1), 1.0, rtol=0, atol=2e-15) and np.array_equal(pt["dir"][:, 2], pt["mu"])   # (a dozen roundings of 1.1e-16)
        x = (p - req["c_f"]) / req["rl"]                                                    # offsets in units of r_max
        assert np.allclose(np.sqrt((x * x).sum(axis=1)), pt["rho"], rtol=0, atol=1e-13)
        centroid[lattice] = x.mean(axis=0)
        if not lattice:
            # a component of an isotropic offset has variance <rho^2> / 3
            sigma = np.sqrt((pt["rho"] ** 2).mean() / 3 / N)
            assert np.all(np.abs(centroid[lattice]) <= 4.5 * sigma), (centroid[lattice], sigma)
    print("centroid / r_max: random %s, lattice %s" % (centroid[False], centroid[True]))
    assert np.linalg.norm(centroid[True]) < np.linalg.norm(centroid[False])


def test_the_cylinder_turns_with_its_axis():
    i = np.arange(5000)
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        req = body("cylinder", TABLES["shell"], axis=axis, seed=8, stream=1, lo=0.002, hi=0.01)
        p, _, pt = rref.base(req, i)
        f = ref.fractions(req, i)
        assert np.array_equal(p[:, axis], ref.base(req, i)[0][:, axis])                    # the plain rule's own coordinate
        assert np.array_equal(pt["rho"], rref.radius("cylinder", TABLES["shell"], f[:, b])[0])
        assert np.array_equal(pt["dir"][:, b], ref.cospi(2.0 * f[:, c])) and np.array_equal(pt["dir"][:, c], ref.sinpi(2.0 * f[:, c])) and np.all(pt["dir"][:, axis] == 0)
        x = (p - req["c_f"]) / req["rl"]
        assert np.allclose(np.hypot(x[:, b], x[:, c]), pt["rho"], rtol=0, atol=1e-13) and pt["rho"].min() >= 0.59 and pt["rho"].max() <= 0.91


def test_a_thermal_table_is_read_at_the_undisplaced_radius():
    check_the_thermal_table()


def test_the_flows_add_to_the_drift():
    check_the_azimuthal_flow()
    i = np.arange(4000)
    u_r, u_a = np.array([0.0, -0.01, -0.03]), np.array([0.02, 0.0])
    req = body("sphere", None, flow_radial=u_r, drift=(0.001, 0.0, 0.0), vth=0, seed=5, lattice=True)
    v, pt = rref.velocities(req, i), rref.parts(req, i)
    inward = (v - np.array([0.001, 0.0, 0.0])) * pt["dir"]
    assert np.array_equal(v[:, 2], 0.0 + pref.lookup(u_r, pt["rho"])[0] * pt["mu"]) and np.all(inward.sum(axis=1) <= 0)  # an implosion
    req = body("cylinder", None, axis=1, flow_radial=u_r, flow_axial=u_a, drift=(0.0, 0.005, 0.0), vth=0, seed=5)
    v, pt = rref.velocities(req, i), rref.parts(req, i)
    assert np.array_equal(v[:, 1], 0.005 + pref.lookup(u_a, pt["rho"])[0])
    assert np.array_equal(v[:, 2], 0.0 + pref.lookup(u_r, pt["rho"])[0] * pt["dir"][:, 2]) and np.array_equal(v[:, 0], 0.0 + pref.lookup(u_r, pt["rho"])[0] * pt["dir"][:, 0])


def test_two_species_on_one_stream_coincide_and_a_body_across_the_boundary_wraps():
    i = np.arange(4000)
    kw = dict(density=TABLES["gaussian"], thermal=[1.0, 0.5], flow_radial=[0.0, -0.01], seed=31, vth=0.01, mode=(1, 0, 0), xamp=(1e-4, 0, 0))
    a, b, c = (rref.request(L, "sphere", (0.001, 0.008, 0.0155), R_MAX, stream=s, **kw) for s in (3, 3, 4))
    for T in (np.float32, np.float64):
        pa = rref.stored_positions(a, i, T)
        assert pa.tobytes() == rref.stored_positions(b, i, T).tobytes() and pa.tobytes() != rref.stored_positions(c, i, T).tobytes()
        assert np.all(pa >= 0) and np.all(pa < 1) and (pa[:, 0] > 0.75).any() and (pa[:, 2] < 0.25).any()
    assert rref.velocities(a, i).tobytes() == rref.velocities(b, i).tobytes()


def test_every_mutation_of_the_reference_fails_a_check():
    assert set(rref.VARIANTS) == {"weight_rho", "halvings_51", "thermal_displaced", "theta_hat_sign"}
    with pytest.raises(AssertionError):
        check_a_random_load("sphere", "gaussian", "weight_rho")
    with pytest.raises(AssertionError):
        check_the_radius("sphere", TABLES["gaussian"], "halvings_51")
    with pytest.raises(AssertionError):
        check_the_radius("cylinder", TABLES["flat"], "halvings_51")
    with pytest.raises(AssertionError):
        check_the_thermal_table("thermal_displaced")
    with pytest.raises(AssertionError):
        check_the_azimuthal_flow("theta_hat_sign")
