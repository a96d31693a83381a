"""CPU checks of what tests/test_gpu_decomposed_solve.py relies on (no GPU, no library):
  * the two closed forms of tests/decomposed_solve_reference.py against numpy's FFT solve, for every source and every
    charged plane the GPU module uses;
  * ROOM: the whole 3-D interface solve emulated on the host — numpy does the x / y transforms and the (0, 0) line, the
    host build of the arithmetic core (tests/native/tri_core_test.cpp, csrc/fes_tri.hpp) every other mode, in double and
    in float storage — on the grids of the GPU module's family A: the fp64 figure uses at most a tenth of the GPU bound;
  * SENSITIVITY: the GPU module's own check functions applied to deliberately wrong variants of an emulated decomposed
    result: each misses the check meant for it by at least 100 times its (loosest, fp32) bound.
"""
import os
import subprocess

import numpy as np
import pytest

import decomposed_solve_reference as dr
import test_gpu_decomposed_solve as gd
from helpers import EPS0, ROOT, node_mode, numpy_poisson

QE, W = gd.QE, 1e9


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("tri") / "tri_core_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split(),
                           os.path.join(ROOT, "tests", "native", "tri_core_test.cpp"), "-o", str(out)])
    return str(out)


# ------------------------------------------------------------------------------------ plane sets and the charge grid

def test_plane_sets():
    geo = dr.Slabs((16, 8, 16), gd.L3, 4, 2)
    assert list(geo.own(1)) == [4, 5, 6, 7] and list(geo.field(1)) == list(range(2, 11)) and list(geo.phi(1)) == list(range(1, 12))
    assert list(geo.received(1)) == [1, 2, 3, 8, 9, 10, 11]             # nzl = G + 2: the four from above are rank 2's whole slab
    assert list(geo.phi(0)) == [0, 1, 2, 3, 4, 5, 6, 7, 13, 14, 15] and list(geo.ghost_field(3)) == [0, 1, 2, 10, 11]
    assert list(geo.em_edge(0)) == [0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15] and len(geo.em_phi(0)) == 13
    two = dr.Slabs((8, 8, 8), gd.L3, 2, 1)                              # the 2 + 3 received planes overlap: plane 6 arrives twice
    assert list(two.phi(0)) == list(range(8)) and list(two.received(0)) == [4, 5, 6, 7] and two.owner(6) == 1
    flat = dr.Slabs((64, 8, 32), gd.FLAT, 4, 2)
    assert abs(flat.lam_min() - 1.5e-4) < 1e-5


def test_assemble_and_density():
    rng = np.random.default_rng(1)
    parts = [rng.integers(-9, 9, (8, 2, 3)) for _ in range(4)]
    whole = dr.assemble(parts, 2)
    for r in range(4):
        assert np.array_equal(whole[2 * r:2 * r + 2], parts[r][2 * r:2 * r + 2])
    fixed = np.zeros((8, 2, 3), np.int64)
    fixed[3, 1, 2] = 5 << 42
    rho = dr.rho64(fixed, QE, W, (3, 2, 8), (0.3, 0.2, 0.8))
    assert rho[3, 1, 2] == pytest.approx(5 * QE * W / 1e-3, rel=1e-15) and np.count_nonzero(rho) == 1


# ------------------------------------------------------------------------------------ the closed forms against numpy

@pytest.mark.parametrize("where", gd.B_PLANES)
@pytest.mark.parametrize("grid", gd.B_GRIDS + [(4, (16, 8, 32), 2)], ids=lambda g: gd.grid_id(g[1]))
def test_closed_forms_against_numpy(grid, where):
    world, shape, G = grid
    geo = dr.Slabs(shape, (0.7, 1.3, 0.9), world, G)
    k0 = gd.charged_plane(geo, where)
    rho0 = QE * W / float(np.prod(geo.d))
    for source in gd.B_SOURCES:
        rho, phi = dr.sheet_source(shape, geo.L, k0, rho0) if source == "sheet" else dr.plane_source(shape, geo.L, k0, source[0], source[1], rho0)
        _, pattern = gd.plane_species(geo, k0, source)
        assert np.array_equal(rho, pattern * rho0)
        want = numpy_poisson(rho, geo.L)
        ratio = np.abs(phi - want).max() / np.abs(want).max()
        assert ratio <= 1e-13, (source, k0, ratio)


def test_eigenmodes_against_numpy():
    shape = (16, 8, 16)
    for pattern in gd.C_PATTERNS:
        ideal, K2, plus, minus = node_mode(shape, gd.L3, pattern)
        want = numpy_poisson(ideal, gd.L3)
        assert np.abs(ideal / (EPS0 * K2) - want).max() <= 1e-13 * np.abs(want).max(), pattern
    assert ("qc", "one", "one") in gd.C_PATTERNS and all(p[2] != "one" for p in gd.C_PATTERNS[:-1]) and len(gd.C_PATTERNS) == 7


# ------------------------------------------------------------------------------------ the emulated interface solve

def deposit(pos, geo):
    """trilinear weights in 14 bits per axis: every particle adds exactly 2^42 to the int64 grid"""
    g = pos / np.asarray(geo.d)
    cell = np.floor(g).astype(np.int64)
    up = np.rint((g - cell) * (1 << 14)).astype(np.int64)
    fixed = np.zeros(geo.grid, np.int64)
    for corner in range(8):
        o = [(corner >> a) & 1 for a in range(3)]
        wgt = np.prod([up[:, a] if o[a] else (1 << 14) - up[:, a] for a in range(3)], axis=0)
        np.add.at(fixed, ((cell[:, 2] + o[2]) % geo.nz, (cell[:, 1] + o[1]) % geo.ny, (cell[:, 0] + o[0]) % geo.nx), wgt)
    return fixed


def spectrum(rho, geo, dz_for_lam=None):
    """f = rho_hat dz^2 / eps0 [nz][ny][nxh] after the x and y transforms, and lam = (k2x + k2y) dz^2 [ny][nxh]"""
    dz = geo.d[2]
    k2 = [(2.0 / geo.d[a] * np.sin(np.pi * np.arange(n) / geo.shape[a])) ** 2 for a, n in ((0, geo.nx // 2 + 1), (1, geo.ny))]
    lam = (k2[1][:, None] + k2[0][None, :]) * (dz if dz_for_lam is None else dz_for_lam) ** 2
    return np.fft.rfft2(rho, axes=(1, 2)) * (dz * dz / EPS0), lam


def zero_line(f):
    """the (0, 0) mode along z: mean dropped, by numpy's transform"""
    n = len(f)
    kz2 = (2 * np.sin(np.pi * np.arange(n) / n)) ** 2
    hat = np.fft.fft(f)
    hat[0], kz2[0] = 0, 1
    return np.fft.ifft(hat / kz2)


def finish(f, modes, geo, line=True):
    hat = np.concatenate([(zero_line(f[:, 0, 0]) if line else np.zeros(geo.nz, complex))[:, None], modes], axis=1).reshape(f.shape)
    return np.fft.irfft2(hat, s=(geo.ny, geo.nx), axes=(1, 2))


def solve_with_core(exe, tmp_path, rho, geo, storage):
    """every mode but (0, 0) through the host build of the core: P ranks of m planes, down sweep, exchange, up sweep"""
    f, lam = spectrum(rho, geo)
    nm = lam.size - 1
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(lam.ravel()[1:].astype("<f8").tobytes())
        fh.write(np.ascontiguousarray(f.reshape(geo.nz, -1)[:, 1:]).view(np.float64).astype("<f8").tobytes())
    subprocess.check_call([exe, str(geo.world), str(geo.nzl), str(nm), storage, str(src), str(dst)], timeout=120)
    return finish(f, np.fromfile(dst, dtype="<f8").view(np.complex128).reshape(geo.nz, nm), geo)


def substructured(f, lam, P, m, swap=False, wrong_neighbour=False):
    """the interface solve of fes_tri.hpp in dense numpy algebra, f [nz][modes], lam [modes]: per rank y = T^-1 f, the
    2 P-unknown interface system, phi = y + a v + b w.  swap: y_1 and y_m exchanged in the gather; wrong_neighbour: a rank
    takes a from the slab above and b from the slab below."""
    nm = lam.size
    T = (2.0 + lam)[:, None, None] * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1)
    Tinv = np.linalg.inv(T)
    v, w = Tinv[:, :, 0], Tinv[:, :, -1]
    alpha, beta = v[:, 0], v[:, -1]
    y = np.einsum("nij,npj->npi", Tinv, f.reshape(P, m, nm).transpose(2, 0, 1))
    y1, ym = y[:, :, 0], y[:, :, -1]
    if swap:
        y1, ym = ym, y1
    A = np.zeros((nm, 2 * P, 2 * P))
    for r in range(P):       # x_r - beta x_{r+1} - alpha z_{r-1} = y_1^r,  z_r - alpha x_{r+1} - beta z_{r-1} = y_m^r
        A[:, r, r] += 1; A[:, r, (r + 1) % P] -= beta; A[:, r, P + (r - 1) % P] -= alpha
        A[:, P + r, P + r] += 1; A[:, P + r, (r + 1) % P] -= alpha; A[:, P + r, P + (r - 1) % P] -= beta
    sol = np.linalg.solve(A.astype(complex), np.concatenate([y1, ym], axis=1)[:, :, None])[:, :, 0]
    x, z = sol[:, :P], sol[:, P:]
    a, b = (np.roll(z, -1, axis=1), np.roll(x, 1, axis=1)) if wrong_neighbour else (np.roll(z, 1, axis=1), np.roll(x, -1, axis=1))
    phi = y + a[:, :, None] * v[:, None, :] + b[:, :, None] * w[:, None, :]
    return phi.transpose(1, 2, 0).reshape(P * m, nm)


def solve_in_numpy(rho, geo, line=True, dz_for_lam=None, **wrong):
    f, lam = spectrum(rho, geo, dz_for_lam)
    return finish(f, substructured(f.reshape(geo.nz, -1)[:, 1:], lam.ravel()[1:], geo.world, geo.nzl, **wrong), geo, line)


def rank_views(phi, fixed, geo, shift=0, z_spacing=None):
    """what every rank holds after the exchange and the gradient: phi on its phi set (received planes are copies of the
    owner's; shift: taken that many planes too high), E4 = (central differences of its OWN phi, phi) on its field set"""
    views = []
    L = geo.L if z_spacing is None else (geo.L[0], geo.L[1], z_spacing * geo.nz)
    for r in range(geo.world):
        mine = np.zeros(geo.grid)
        mine[geo.own(r)] = phi[geo.own(r)]
        got = geo.received(r)
        mine[got] = phi[(got + shift) % geo.nz]
        e4 = np.zeros(geo.grid + (4,))
        planes = geo.field(r)
        e4[planes, ..., :3] = dr.central_e(mine, L)[planes]
        e4[planes, ..., 3] = mine[planes]
        views.append(dict(fixed=fixed, phi=mine, e4=e4))
    return views


def cloud_case(case):
    world, shape, G, modes, L = case
    geo = dr.Slabs(shape, L, world, G)
    fixed = deposit(gd.lumpy_cloud(shape, gd.N_CLOUD, L), geo)
    assert int(fixed.sum()) == gd.N_CLOUD * gd.FIXED_ONE
    return geo, fixed, gd.weight_for(L)


I_CASES = [c for c in gd.A_CASES if "I" in c[3]]


@pytest.mark.parametrize("case", I_CASES, ids=gd.case_id)
def test_room_under_the_gpu_bounds(exe, tmp_path, case, capsys):
    """the emulated interface solve against numpy on family A's grids: double storage within 0.1 of the fp64 bound of the
    GPU module; float storage (the core alone: the transforms stay double here) is printed beside the fp32 bound"""
    geo, fixed, weight = cloud_case(case)
    rho = dr.rho64(fixed, QE, weight, geo.shape, geo.L)
    want = numpy_poisson(rho, geo.L)
    top = np.abs(want).max()
    ratio = {s: float(np.abs(solve_with_core(exe, tmp_path, rho, geo, s) - want).max() / top) for s in ("double", "float")}
    ratio["numpy"] = float(np.abs(solve_in_numpy(rho, geo) - want).max() / top)
    bound = gd.phi_bound(geo, "I", "fp64")
    with capsys.disabled():
        print("\nroom %-16s lam_min %.2g  double %.2g (bound %.2g)  float %.2g (bound %.0e)  dense numpy %.2g" % (
            gd.case_id(case), geo.lam_min(), ratio["double"], bound, ratio["float"], gd.TOL["fp32"], ratio["numpy"]))
    assert ratio["double"] <= 0.1 * bound, ratio
    assert ratio["numpy"] <= 0.1 * bound, ratio
    # and a correct result passes every check of the GPU module
    views = rank_views(solve_with_core(exe, tmp_path, rho, geo, "double"), fixed, geo)
    gd.check_frame(views, geo, "I", "fp64", gd.N_CLOUD, "emulated", gd.case_id(case), macro_weight=weight)
    gd.WORST.pop("emulated", None); gd.WORST.pop("emulated E", None)


SENSITIVITY_CASES = [gd.A_CASES[3], gd.A_CASES[4]]      # four ranks with nzl = G + 2, and eight ranks


@pytest.mark.parametrize("case", SENSITIVITY_CASES, ids=gd.case_id)
def test_wrong_variants_miss_their_checks(case, capsys):
    """each wrong variant of the emulated decomposed result misses the check meant for it — check 2 (phi on the rank's
    planes, fp32 bound 2e-5) or check 5 (E against the rank's own phi, fp32 eps) — by at least 100 times the bound"""
    geo, fixed, weight = cloud_case(case)
    rho = dr.rho64(fixed, QE, weight, geo.shape, geo.L)
    want = numpy_poisson(rho, geo.L)
    top = float(np.abs(want).max())
    good = solve_in_numpy(rho, geo)
    tol, eps = gd.TOL["fp32"], gd.EPS["fp32"]
    assert gd.measure_phi(rank_views(good, fixed, geo), geo, want, top) <= 1e-12
    assert gd.measure_central_e(rank_views(good, fixed, geo), geo, gd.EPS["fp64"], top)[1] <= 1.0
    variants = {
        "received planes one too high": rank_views(good, fixed, geo, shift=1),
        "lam with dx^2 for dz^2": rank_views(solve_in_numpy(rho, geo, dz_for_lam=geo.d[0]), fixed, geo),
        "(0, 0) line left at zero": rank_views(solve_in_numpy(rho, geo, line=False), fixed, geo),
        "y_1 and y_m swapped": rank_views(solve_in_numpy(rho, geo, swap=True), fixed, geo),
        "a / b from the wrong neighbour": rank_views(solve_in_numpy(rho, geo, wrong_neighbour=True), fixed, geo),
    }
    lines = []
    for name, views in variants.items():
        factor = gd.measure_phi(views, geo, want, top) / tol
        lines.append("sensitivity %-16s %-32s check 2 missed by %.3g x bound" % (gd.case_id(case), name, factor))
        assert factor >= 100, (name, factor)
        with pytest.raises(AssertionError):
            gd.check_phi_sets(views, geo, want, tol, "emulated", name)
    views = rank_views(good, fixed, geo, z_spacing=geo.d[1])
    factor = gd.measure_central_e(views, geo, eps, top)[1]
    lines.append("sensitivity %-16s %-32s check 5 missed by %.3g x bound" % (gd.case_id(case), "1 / (2 dy) for 1 / (2 dz)", factor))
    assert factor >= 100, factor
    with pytest.raises(AssertionError):
        gd.check_rank_central_e(views, geo, eps, top, "emulated", "gradient")
    gd.WORST.pop("emulated", None); gd.WORST.pop("emulated E", None)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
