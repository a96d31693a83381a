"""The numpy definition of the fluid moment grids (tests/moments_reference.py) against what the header promises: the
exact-sum identities on random states in both dtypes, N equal to the oracle's charge deposit with Z = 1 bit for bit,
rejected particles, dead slots, and one-particle cases computed by hand (on a node, mid-cell, in the last cell of each
axis so that the wrap is exercised, a negative value)."""
import numpy as np
import pytest

import es3d_oracle as eo
import moments_reference as mr

ME, QE = 9.109e-31, -1.602e-19
DTYPES = [np.float32, np.float64]


def random_state(rng, n, dtype, sigma=0.05):
    pos = rng.random((n, 3)).astype(dtype)
    pos[pos >= 1] = 0                      # (a float32 rounding of a double just below 1)
    return pos, rng.normal(0, sigma, (n, 3)).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 10, 7), (2, 5, 3), (33, 2, 9)])
def test_exact_sum_identities(dtype, shape):
    rng = np.random.default_rng(sum(shape))
    n = 4000
    pos, vel = random_state(rng, n, dtype, sigma=3.0)
    vel[::50] *= 30                        # some beyond the limit
    vel[7, 1] = np.nan
    vel[9, 2] = -np.inf
    got, rej = mr.moments(pos, vel, shape)
    want, rej2 = mr.particle_sums(vel, 0x3FF)
    assert rej == rej2 and 2 < rej < n // 5
    assert int(got["N"].sum()) == mr.ONE * (n - rej) == want["N"]
    for name in mr.NAMES[1:]:
        assert int(got[name].sum()) == want[name], name
        assert got[name].shape == (shape[2], shape[1], shape[0]) and got[name].dtype == np.int64
    # second moments of the diagonal are never negative, per node either
    for name in ("SXX", "SYY", "SZZ"):
        assert (got[name] >= 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_n_is_the_oracles_deposit_with_unit_charge(dtype):
    rng = np.random.default_rng(11)
    n, shape, L = 5000, (12, 10, 8), (1.0, 2.0, 0.5)
    spec = dict(radius=L[0], length_y=L[1], height=L[2], nr=shape[0], ny=shape[1], nz=shape[2], dt=1e-10, nparticles=0, count=n,
                particle_mass=ME, particle_charge=-QE, geometry="cart3d", solver="poisson_fft", macro_weight=1.0)
    sim = eo.OracleES3D(spec, dtype)
    assert sim.charge_number(0) == 1
    pos = rng.random((n, 3)) * L
    pos[:8] = [[0, 0, 0], [1.0, 2.0, 0.5], [0.999999999, 0, 0], [1.0 - 1e-12, 1e-12, 0.25], [0.5, 1.0, 0.25],
               [1 / 12, 2 / 10, 0.5 / 8], [-0.25, 2.5, 1.0], [1e-30, 0, 0.4999999]]      # edges, node positions, outside the box
    sim.set(position=pos, velocity=rng.normal(0, 0.01, (n, 3)))
    sim.deposit()
    stored = np.stack([sim.species[0].x, sim.species[0].y, sim.species[0].z], axis=1)
    assert stored.dtype == dtype
    got, rej = mr.moments(stored, sim.velocities(0), shape, "n")
    assert rej == 0 and mr.ONE == eo.FIXED_ONE
    assert np.array_equal(got["N"].ravel(), np.asarray(sim.rho_fixed).ravel())
    # the cells are the oracle's too
    i, _ = mr.axis(stored[:, 0].copy(), shape[0]); j, _ = mr.axis(stored[:, 1].copy(), shape[1]); k, _ = mr.axis(stored[:, 2].copy(), shape[2])
    assert np.array_equal(i + shape[0] * (j + shape[1] * k), sim.cells(0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rejected_particles_add_to_nothing(dtype):
    top = np.nextafter(dtype(128), dtype(0))
    pos = np.full((8, 3), 0.3, dtype=dtype)
    vel = np.zeros((8, 3), dtype=dtype)
    vel[0, 0] = np.nan; vel[1, 1] = np.inf; vel[2, 2] = -np.inf; vel[3, 0] = 128; vel[4, 2] = -128; vel[5, 1] = 1e30
    vel[6] = [top, -top, top]             # the largest value below the limit: accepted
    vel[7] = [0.5, 0.25, -0.125]
    got, rej = mr.moments(pos, vel, (4, 4, 4))
    assert rej == 6
    only, rej2 = mr.moments(pos[6:], vel[6:], (4, 4, 4))
    assert rej2 == 0
    for name in mr.NAMES:
        assert np.array_equal(got[name], only[name]), name
    assert int(got["N"].sum()) == 2 * mr.ONE
    t = float(top)
    assert int(got["SXX"].sum()) == int(np.floor(t * t * 2.0 ** 32)) + (1 << 30) and int(np.floor(t * t * 2.0 ** 32)) < 1 << 46
    assert int(got["SXY"].sum()) == int(np.floor(-(t * t) * 2.0 ** 32)) + (1 << 29)
    # N alone obeys the same rule
    n_only, rej3 = mr.moments(pos, vel, (4, 4, 4), "n")
    assert rej3 == 6 and np.array_equal(n_only["N"], got["N"])


def test_dead_slots_are_skipped():
    pos = np.array([[0.1, 0.2, 0.3], [-1.0, 0.2, 0.3], [0.6, 0.7, 0.8]], dtype=np.float32)
    vel = np.array([[0.1, 0, 0], [np.nan, 0, 0], [0.2, 0, 0]], dtype=np.float32)
    got, rej = mr.moments(pos, vel, (4, 4, 4), dead_slots=True)
    assert rej == 0 and int(got["N"].sum()) == 2 * mr.ONE     # (the dead slot's NaN is not a rejected particle)


def one(pos, vel, shape, dtype=np.float64):
    got, rej = mr.moments(np.array([pos], dtype=dtype), np.array([vel], dtype=dtype), shape)
    assert rej == 0
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_particle_on_a_node(dtype):
    got = one([0.25, 0.5, 0.75], [0.5, -0.25, 2.0], (4, 4, 4), dtype)       # node (1, 2, 3): every upper weight 0
    for name, m in zip(mr.NAMES, (None, 0.5, -0.25, 2.0, 0.25, 0.0625, 4.0, -0.125, 1.0, -0.5)):
        want = np.zeros((4, 4, 4), dtype=np.int64)
        want[3, 2, 1] = mr.ONE if m is None else int(m * 2 ** 32)
        assert np.array_equal(got[name], want), name


def test_one_particle_mid_cell():
    got = one([0.125, 0.125, 0.125], [1.0, 0.0, -1.0], (4, 4, 4))           # the centre of cell (0, 0, 0): every weight 8192
    want = np.zeros((4, 4, 4), dtype=np.int64)
    want[0:2, 0:2, 0:2] = 8192 ** 3
    assert np.array_equal(got["N"], want)
    want[0:2, 0:2, 0:2] = 2 ** 32 // 8
    assert np.array_equal(got["FX"], want)
    assert not got["FY"].any()
    # m = -1: t = -2^32 halves exactly three times
    assert np.array_equal(got["FZ"], -want) and np.array_equal(got["SXZ"], -want) and np.array_equal(got["SZZ"], want)


def test_a_negative_value_that_does_not_divide_rounds_by_the_rule():
    # t = floor(-3 * 2^-32 * 2^32) = -3 at the cell's centre: along z upper = (8192 * -3 + 8192) >> 14 = -1, lower = -2;
    # -1 -> upper (−8192 + 8192) >> 14 = 0, lower −1; −2 -> upper (−16384 + 8192) >> 14 = −1, lower −1
    v = -3.0 / 2 ** 32
    got = one([0.125, 0.125, 0.125], [v, 0.0, 0.0], (4, 4, 4))
    f = got["FX"]
    assert int(f.sum()) == -3
    # z upper = -1: its y parts (lower -1, upper 0); the -1 along x: (lower -1, upper 0)
    assert f[1, 1, 0] == 0 and f[1, 1, 1] == 0 and f[1, 0, 0] == -1 and f[1, 0, 1] == 0
    # z lower = -2: y parts (lower -1, upper -1); each along x: (lower -1, upper 0)
    assert f[0, 0, 0] == -1 and f[0, 0, 1] == 0 and f[0, 1, 0] == -1 and f[0, 1, 1] == 0
    # a tiny negative value floors to -1, which stays whole on the lowest node
    got = one([0.125, 0.125, 0.125], [-1e-30, 0.0, 0.0], (4, 4, 4))
    assert int(got["FX"].sum()) == -1 and got["FX"][0, 0, 0] == -1 and int(got["SXX"].sum()) == 0


@pytest.mark.parametrize("last", [0, 1, 2])
def test_the_last_cell_of_an_axis_wraps(last):
    shape = (4, 5, 3)
    pos = [0.125 / 1, 0.1, 1.0 / 6]                   # cell (0, 0, 0), weights (8192, 8192, 8192)
    pos[last] = 1.0 - 0.5 / shape[last]                # the centre of the axis' last cell
    got = one(pos, [0.5, 0.5, 0.5], shape)
    n = got["N"]
    lo = [slice(0, 2), slice(0, 2), slice(0, 2)]
    idx = [[0, 1], [0, 1], [0, 1]]
    idx[last] = [shape[last] - 1, 0]                   # the upper node is node 0
    want = np.zeros((shape[2], shape[1], shape[0]), dtype=np.int64)
    for a in idx[0]:
        for b in idx[1]:
            for c in idx[2]:
                want[c, b, a] = 8192 ** 3
    assert np.array_equal(n, want), lo
    assert np.array_equal(got["FX"], want // 8192 ** 3 * (2 ** 31 // 8))
