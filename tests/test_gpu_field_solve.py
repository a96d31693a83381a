"""The field solve of the periodic box (spec.geometry = 'cart3d') against float64 references that share no code with the
library or the oracle: numpy's FFT applied to the library's OWN charge density (helpers.numpy_poisson), so that every case
tests the transform and not the deposit, and exact eigenmodes of the 3-point Laplacian (no FFT at all).

PARITY UNPINNED (the reference has no field solve; the definition is oracle/es3d_oracle_impl.h: es3d_poisson, es3d_gradient,
em_edge_gradient).  The cells are not cubes (a different length per axis), so that swapping per-axis quantities shows.
  A. one handle, the library's own FFT passes (csrc/fes_fft.hpp: power-of-two axes of 8 .. 512 nodes): each axis alone at
     every length beside axes of 8 and 16 nodes, and mixed grids; phi against numpy, E against central differences of the
     handle's own phi, E4[..., 3] bit-identical to phi;
  B. the rocFFT path (FPIC_POISSON_FFT=rocfft) on the same grids: within tolerance of numpy and of the own passes, and not
     bit-identical to them (the switch took effect);
  C. grids the own passes do not take (2, 3, 5, 6, 12, 24 and 1024 nodes on one axis): the rocFFT path against numpy;
  D. exact eigenmodes: one charge per charged node, on the node, rho = A c_x(i) c_y(j) c_z(k) with each factor 1, (-1)^i or
     a quarter wave; phi = rho / (eps0 K^2), and E = the central differences of that phi (0 along a Nyquist factor);
  E. the initial field of a full-EM handle: the forward differences of its phi, bit for bit;
  F. long boxes (70000 nodes on one axis): push, deposit and solve where the per-node sweeps have the most planes.
Bounds: phi within 2e-5 (fp32) / 1e-12 (fp64) of max |phi|, the eigenmodes within 1e-6 / 1e-12.  The worst ratio of every
family is printed at the end of the module (pytest -s).
"""
import numpy as np
import pytest

from helpers import EPS0, node_mode, numpy_poisson, same_bits

pytestmark = pytest.mark.gpu

ME, QE, MP = 9.109e-31, -1.602e-19, 1.67e-27
FIXED_ONE = 1 << 42                        # the charge grid's unit: one particle of charge number 1
L3 = (0.7, 1.3, 0.9)                       # box lengths (x, y, z): no two cell edges alike on the grids below
TOL = {"fp32": 2e-5, "fp64": 1e-12}        # phi against a float64 reference, relative to max |phi|
EIGEN_TOL = {"fp32": 1e-6, "fp64": 1e-12}
EPS = {"fp32": float(np.finfo(np.float32).eps), "fp64": float(np.finfo(np.float64).eps)}
WORST = {}                                 # family -> worst observed ratio


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


@pytest.fixture(scope="module")
def eo():
    import es3d_oracle
    return es3d_oracle


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    for family in sorted(WORST):
        print("worst ratio  %-26s %.3g" % (family, WORST[family]))


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)


def grid_id(shape):
    return "x".join(str(n) for n in shape)


def along(axis, n):
    """n nodes on one axis, 8 and 16 on the other two"""
    return ((n, 8, 16), (16, n, 8), (8, 16, n))[axis]


def own_fft_takes(shape):
    return all(8 <= n <= 512 and n & (n - 1) == 0 for n in shape)


def box_spec(shape, count, solver="poisson_fft", dt=1e-10, macro_weight=1e9, L=L3):
    return dict(radius=L[0], length_y=L[1], height=L[2], nr=shape[0], ny=shape[1], nz=shape[2], dt=dt, nparticles=0, count=count,
                particle_mass=ME, particle_charge=QE, geometry="cart3d", solver=solver, macro_weight=macro_weight)


def make_box(fp, monkeypatch, spec, precision, path):
    """path 'rocfft': FPIC_POISSON_FFT=rocfft while the handle is created (the library reads it there); 'default': the
    library's own choice (its own passes where they take the grid)"""
    if path == "rocfft":
        monkeypatch.setenv("FPIC_POISSON_FFT", "rocfft")
    else:
        monkeypatch.delenv("FPIC_POISSON_FFT", raising=False)
    try:
        return fp.makeCylindricalParticlePusher(spec, precision=precision)
    finally:
        monkeypatch.delenv("FPIC_POISSON_FFT", raising=False)


def lumpy_cloud(shape, count=20000, L=L3):
    """every wavelength from the box down to a few cells carries charge (as the 256^3 / 512^3 test's cloud)"""
    rng = np.random.default_rng(list(shape))
    centres = rng.random((40, 3))
    return (centres[rng.integers(0, 40, count)] + rng.normal(0, 0.03, (count, 3)) * rng.random((count, 1))) % 1.0 * np.asarray(L)


def fields(fp, sim, shape, e4=True):
    """rho (float64), phi (the handle's precision), E4 and the int64 charge grid, each [nz][ny][nx](...)"""
    grid = (shape[2], shape[1], shape[0])
    out = dict(rho=sim.readField(fp.F3_RHO, np.float64).reshape(grid), phi=sim.readField(fp.F3_PHI).reshape(grid),
               fixed=sim.readField(fp.F3_RHO_FIXED).reshape(grid))
    if e4:
        out["e4"] = sim.readField(fp.F3_E).reshape(grid + (4,))
    return out


def solve_cloud(fp, monkeypatch, shape, precision, path, pos):
    sim = make_box(fp, monkeypatch, box_spec(shape, len(pos)), precision, path)
    sim.set(position=pos, velocity=np.zeros_like(pos))
    sim.precalc()
    out = fields(fp, sim, shape)
    sim.destroy()
    return out


def check_phi(phi, want, tol, family, what):
    top = float(np.abs(want).max())
    assert top > 0, what
    ratio = float(np.abs(phi.astype(np.float64) - want).max()) / top
    note(family, ratio)
    assert ratio <= tol, "%s: max |phi - reference| / max |phi| = %.3g (bound %.0e)" % (what, ratio, tol)
    return top


def axes_of(phi, L):
    """(component, numpy axis, nodes, length) of x, y, z for a [nz][ny][nx] array"""
    nz, ny, nx = phi.shape[:3]
    return ((0, 2, nx, L[0]), (1, 1, ny, L[1]), (2, 0, nz, L[2]))


def check_central_e(e4, phi, eps, top, family, what, L=L3):
    """E = -grad phi by central differences of the handle's OWN phi with each axis's spacing (es3d_gradient), within the
    bound of the 256^3 / 512^3 test: the difference and the product are formed in T from phi in T, eps(T) |phi| n / (2 L)
    each; and the node record's fourth value is phi itself"""
    assert same_bits(e4[..., 3], phi), what + ": E4[..., 3] is not phi"
    p = phi.astype(np.float64)
    for comp, axis, n, length in axes_of(p, L):
        h = n / (2.0 * length)
        grad = (np.roll(p, 1, axis=axis) - np.roll(p, -1, axis=axis)) * h
        worst = float(np.abs(e4[..., comp].astype(np.float64) - grad).max())
        note(family + " E", worst / (top * h))
        bound = 4 * eps * top * h + 1e-6 * float(np.abs(grad).max())
        assert worst <= bound, "%s: E%s off the central difference of phi by %.3g of max |phi| / (2 d) (bound %.3g)" % (
            what, "xyz"[comp], worst / (top * h), bound / (top * h))


# ------------------------------------------------------------------------------------ A + B: power-of-two grids, both paths

OWN_GRIDS = [along(a, n) for a in range(3) for n in (8, 16, 32, 64, 128, 256, 512)] + \
            [(512, 256, 8), (8, 512, 512), (256, 8, 512), (512, 8, 8)]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", OWN_GRIDS, ids=grid_id)
def test_own_fft_and_rocfft_against_numpy(fp, monkeypatch, shape, precision):
    """A: one handle, the library's own passes — every axis alone at every length (twiddle table, logn, line and stride of
    the column passes, the k-space indices of the fused z sweep: a swap of per-axis quantities is invisible on a cube,
    not here), the 512-point columns of either precision and the half-width float tiles on a y or z axis alone, an 8-point
    axis beside 512-point ones.  B: the same charge solved again with rocFFT forced: both within tolerance of numpy and
    of each other, and not bit-identical (the paths form the transform and the factor 1 / K^2 differently)."""
    pos = lumpy_cloud(shape)
    tol, eps = TOL[precision], EPS[precision]
    what = "%s %s" % (grid_id(shape), precision)
    own = solve_cloud(fp, monkeypatch, shape, precision, "default", pos)
    assert int(own["fixed"].sum()) == len(pos) * FIXED_ONE
    want = numpy_poisson(own["rho"], L3)
    top = check_phi(own["phi"], want, tol, "A own " + precision, "own FFT " + what)
    check_central_e(own["e4"], own["phi"], eps, top, "A own " + precision, "own FFT " + what)

    roc = solve_cloud(fp, monkeypatch, shape, precision, "rocfft", pos)
    assert np.array_equal(roc["fixed"], own["fixed"]) and same_bits(roc["rho"], own["rho"]), what
    check_phi(roc["phi"], want, tol, "B rocfft " + precision, "rocFFT " + what)
    check_central_e(roc["e4"], roc["phi"], eps, top, "B rocfft " + precision, "rocFFT " + what)
    ratio = float(np.abs(own["phi"].astype(np.float64) - roc["phi"]).max()) / top
    note("B own-rocfft " + precision, ratio)
    assert ratio <= tol, "%s: max |phi(own) - phi(rocFFT)| / max |phi| = %.3g (bound %.0e)" % (what, ratio, tol)
    assert not same_bits(own["phi"], roc["phi"]), what + ": FPIC_POISSON_FFT=rocfft gave the own passes' phi bit for bit"


# ------------------------------------------------------------------------------------ C: grids the own passes do not take

ROCFFT_GRIDS = [along(a, n) for a in range(3) for n in (2, 3, 5, 6, 12, 24, 1024)]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", ROCFFT_GRIDS, ids=grid_id)
def test_rocfft_grids_against_numpy(fp, monkeypatch, shape, precision):
    """C: lengths that are no power of two, below the own passes' 8 or above their 512 on one axis: the library's own
    choice (rocFFT) against numpy, E against the central differences of its phi (an axis of two nodes: E = 0 there)"""
    assert not own_fft_takes(shape)
    pos = lumpy_cloud(shape)
    what = "%s %s" % (grid_id(shape), precision)
    got = solve_cloud(fp, monkeypatch, shape, precision, "default", pos)
    assert int(got["fixed"].sum()) == len(pos) * FIXED_ONE
    top = check_phi(got["phi"], numpy_poisson(got["rho"], L3), TOL[precision], "C rocfft " + precision, "rocFFT " + what)
    check_central_e(got["e4"], got["phi"], EPS[precision], top, "C rocfft " + precision, "rocFFT " + what)


# ------------------------------------------------------------------------------------ D: exact eigenmodes

# (x, y, z) factors: each Nyquist factor alone and together; the x-Nyquist value beside y and z rows that differ (the fp32
# x passes keep k = nx / 2 apart from the vector stores: a mix-up of the two rows of a pair shows only where they differ)
PATTERNS = [("nyq", "one", "one"), ("one", "nyq", "one"), ("one", "one", "nyq"), ("nyq", "nyq", "nyq"), ("nyq", "qs", "one"),
            ("nyq", "one", "qc"), ("qc", "nyq", "qs"), ("qs", "qc", "nyq"), ("qc", "qs", "qc")]
EIGEN_GRIDS = [(32, 8, 16), (16, 64, 8), (8, 16, 32), (12, 20, 24)]


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", EIGEN_GRIDS, ids=grid_id)
def test_exact_eigenmodes(fp, monkeypatch, shape, precision):
    """D: charges exactly on nodes — two species of opposite sign, one particle per charged node at the node's own
    coordinate i dx (es3d_axis rounds a coordinate within 2^-15 of a cell of a node wholly onto it) — make rho one
    eigenvector of the 3-point Laplacian.  The charge grid is exactly the pattern; phi = rho / (eps0 K^2) with K^2 the
    eigenvalue; E = the central differences of that phi (analytically 0 along a Nyquist factor).  Both paths where the own
    passes take the grid."""
    tol, eps = EIGEN_TOL[precision], EPS[precision]
    paths = ("default", "rocfft") if own_fft_takes(shape) else ("default",)
    for pattern in PATTERNS:
        ideal, K2, plus, minus = node_mode(shape, L3, pattern)
        assert len(plus) == len(minus) > 0
        for path in paths:
            what = "%s %s %s %s" % (grid_id(shape), precision, "/".join(pattern), path)
            sim = make_box(fp, monkeypatch, box_spec(shape, len(plus)), precision, path)
            assert sim.addSpecies(MP, -QE, len(minus)) == 1
            sim.set(position=plus, velocity=np.zeros_like(plus))
            sim.set(position=minus, velocity=np.zeros_like(minus), species=1)
            sim.precalc()
            got = fields(fp, sim, shape)
            sim.destroy()
            assert np.array_equal(got["fixed"], ideal.astype(np.int64) * FIXED_ONE), what + ": the charge grid is not the pattern"
            family = "D %s %s" % ("own" if path == "default" and own_fft_takes(shape) else "rocfft", precision)
            want = got["rho"] / (EPS0 * K2)
            top = check_phi(got["phi"], want, tol, family, what)
            assert same_bits(got["e4"][..., 3], got["phi"]), what
            for comp, axis, n, length in axes_of(want, L3):
                h = n / (2.0 * length)
                exact = (np.roll(want, 1, axis=axis) - np.roll(want, -1, axis=axis)) * h
                ratio = float(np.abs(got["e4"][..., comp].astype(np.float64) - exact).max()) / (top * h)
                note(family + " E", ratio)
                # phi within tol of max |phi| at both neighbours, and the difference and product rounded in T
                assert ratio <= 2 * tol + 4 * eps, "%s: E%s off the exact mode's by %.3g of max |phi| / (2 d) (bound %.3g)" % (
                    what, "xyz"[comp], ratio, 2 * tol + 4 * eps)


# ------------------------------------------------------------------------------------ E: the full-EM start

def cfl_dt(shape, L=L3, courant=0.5):
    return courant / (2.998e8 * np.sqrt(sum((shape[a] / L[a]) ** 2 for a in range(3))))


def check_edge_field(edge, phi, what, L=L3):
    """em_edge_gradient: E on the edge (c, c + 1) = (phi[c] - phi[c + 1]) * T(1 / d), one rounding each, bit for bit"""
    T = phi.dtype.type
    for comp, axis, n, length in axes_of(phi, L):
        want = (phi - np.roll(phi, -1, axis=axis)) * T(1.0 / (length / n))
        assert same_bits(edge[..., comp], want), "%s: edge E%s is not the forward difference of phi (worst %.3g)" % (
            what, "xyz"[comp], float(np.abs(edge[..., comp].astype(np.float64) - want).max()))
    assert not edge[..., 3].any(), what


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", [(32, 8, 16), (8, 64, 16), (16, 8, 128), (12, 10, 6)], ids=grid_id)
def test_full_em_start_is_the_forward_difference_of_phi(fp, monkeypatch, shape, precision):
    """E: a solver 'yee' handle starts from the Poisson field: F3_EDGE_E after precalc() holds the forward differences of
    the handle's phi (em_edge_gradient, oracle/es3d_oracle_impl.h), and that phi is numpy's solve of the handle's rho"""
    pos = lumpy_cloud(shape)
    what = "%s %s yee" % (grid_id(shape), precision)
    sim = make_box(fp, monkeypatch, box_spec(shape, len(pos), solver="yee", dt=cfl_dt(shape)), precision, "default")
    sim.set(position=pos, velocity=np.zeros_like(pos))
    sim.precalc()
    got = fields(fp, sim, shape, e4=False)
    edge = sim.readField(fp.F3_EDGE_E).reshape(got["phi"].shape + (4,))
    sim.destroy()
    family = "E %s %s" % ("own" if own_fft_takes(shape) else "rocfft", precision)
    check_phi(got["phi"], numpy_poisson(got["rho"], L3), TOL[precision], family, what)
    check_edge_field(edge, got["phi"], what)


# ------------------------------------------------------------------------------------ F: long boxes

LONG_BOXES = [(4, 4, 70000), (4, 70000, 4), (70000, 4, 4)]


def long_box_particles(shape, n, L):
    rng = np.random.default_rng(list(shape))
    pos = rng.random((n, 3)) * L
    # a fifth of them cross a cell or two per sub-step: the wrap and the out-of-window path along the long axis too
    vel = rng.normal(0, 0.01, (n, 3)) + rng.normal(0, 0.3, (n, 3)) * (rng.random((n, 1)) < 0.2)
    return rng, pos, vel


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", LONG_BOXES, ids=grid_id)
def test_long_box_in_a_given_field_against_the_oracle(fp, eo, shape, precision):
    """F, solver 'none': 70000 nodes on one axis (on z: 70000 planes of the per-node sweeps); particles, cells and the
    integer charge grid bit-identical to the oracle's in a given E, after precalc() and two step()s; total charge exact"""
    n = 20000
    L = tuple(1e-3 * s for s in shape)
    rng, pos, vel = long_box_particles(shape, n, L)
    spec = box_spec(shape, n, solver="none", dt=2e-11, macro_weight=2e4, L=L)
    dtype = np.float32 if precision == "fp32" else np.float64
    sim, ora = fp.makeCylindricalParticlePusher(spec, precision=precision), eo.OracleES3D(spec, dtype)
    E = rng.normal(0, 3e4, shape + (3,))
    for s in (sim, ora):
        s.set(position=pos, velocity=vel, E=E)
    sim.addB(0.3, -0.2, 0.9); ora.add_b(0.3, -0.2, 0.9)
    sim.precalc(); ora.precalc()
    assert np.array_equal(sim.readField(fp.F3_RHO_FIXED), ora.rho_fixed)
    for frame in range(2):
        sim.step(); ora.step()
        got = sim.getParticles()
        assert np.array_equal(sim.getCells(), ora.cells(0)), frame
        assert same_bits(got["position"], ora.positions(0)) and same_bits(got["velocity"], ora.velocities(0)), frame
        fixed = sim.readField(fp.F3_RHO_FIXED)
        assert np.array_equal(fixed, ora.rho_fixed), frame
        assert int(fixed.sum()) == n * FIXED_ONE, frame
    sim.destroy()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("shape", LONG_BOXES, ids=grid_id)
def test_long_box_solve_against_numpy(fp, shape, precision):
    """F, solver 'poisson_fft' (rocFFT: 70000 is no length of the own passes): after precalc() and after each of two
    step()s the total charge is exact, phi is numpy's solve of the handle's rho and E its central differences"""
    n = 20000
    L = tuple(1e-3 * s for s in shape)
    _, pos, vel = long_box_particles(shape, n, L)
    sim = fp.makeCylindricalParticlePusher(box_spec(shape, n, dt=2e-11, macro_weight=2e4, L=L), precision=precision)
    sim.set(position=pos, velocity=vel)
    sim.precalc()
    for frame in range(3):
        if frame:
            sim.step()
        got = fields(fp, sim, shape)
        what = "%s %s frame %d" % (grid_id(shape), precision, frame)
        assert int(got["fixed"].sum()) == n * FIXED_ONE, what
        top = check_phi(got["phi"], numpy_poisson(got["rho"], L), TOL[precision], "F rocfft " + precision, what)
        check_central_e(got["e4"], got["phi"], EPS[precision], top, "F rocfft " + precision, what, L=L)
    sim.destroy()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_long_full_em_box(fp, precision):
    """F, solver 'yee' on 8 x 8 x 70000 nodes: the start is the forward difference of numpy's phi; two step()s; the
    charge grid of the particles then (density()) holds the total charge exactly"""
    shape, n = (8, 8, 70000), 20000
    L = tuple(1e-3 * s for s in shape)
    _, pos, vel = long_box_particles(shape, n, L)
    sim = fp.makeCylindricalParticlePusher(box_spec(shape, n, solver="yee", dt=cfl_dt(shape, L), macro_weight=2e4, L=L),
                                           precision=precision)
    sim.set(position=pos, velocity=vel)
    sim.precalc()
    got = fields(fp, sim, shape, e4=False)
    what = "%s %s yee" % (grid_id(shape), precision)
    assert int(got["fixed"].sum()) == n * FIXED_ONE, what
    check_phi(got["phi"], numpy_poisson(got["rho"], L), TOL[precision], "F rocfft " + precision, what)
    check_edge_field(sim.readField(fp.F3_EDGE_E).reshape(got["phi"].shape + (4,)), got["phi"], what, L=L)
    for frame in range(2):
        sim.step()
        sim.density()
        assert int(sim.readField(fp.F3_RHO_FIXED).sum()) == n * FIXED_ONE, (what, frame)
        edge = sim.readField(fp.F3_EDGE_E)
        assert np.isfinite(edge).all(), (what, frame)
    sim.destroy()
