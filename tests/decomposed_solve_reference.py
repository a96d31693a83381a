"""Float64 references for the slab-decomposed Poisson solves (tests/test_gpu_decomposed_solve.py,
tests/test_decomposed_solve_reference.py).  Plain numpy: this module imports neither the oracle nor the library.

  * the global charge grid assembled from every rank's OWN planes, and the density the solve is handed,
        rho = fixed q W / (2^42 dV)                                        (float64),
    so that want = helpers.numpy_poisson(rho, L) is the potential every rank must hold on its planes;
  * two closed forms of the periodic 3-point-Laplacian problem that need no FFT at all (plane_source, sheet_source):
    both excite EVERY kz of one (kx, ky) line, i.e. every rank frequency of the interface system of fes_tri.hpp;
  * the plane sets of a rank (Slabs): what it owns, where it forms E, and what it must hold of phi after the X_PHI
    exchange of fes_domain.inc.hpp.
"""
import numpy as np

from helpers import EPS0, NODE_FACTORS, numpy_poisson

FIXED_ONE = 1 << 42          # the charge grid's unit: one particle of charge number 1


class Slabs:
    """z-slab decomposition of an (nx, ny, nz) grid into `world` slabs with G ghost planes.  Plane sets of rank r, all
    taken mod nz (sorted, without repetition: on a short grid the sets wrap onto themselves):
        own        [z0, z0 + nzl)                     the rank's slab
        field      [z0 - G, z0 + nzl + G + 1)         where E is formed (the nodes the rank's particles can touch)
        phi        [z0 - G - 1, z0 + nzl + G + 2)     what the rank must hold of phi (a plane's gradient reads both neighbours)
    A full-EM rank keeps H = G + 2 halo planes: it forms the edge field on [z0 - H, z0 + nzl + H) by FORWARD differences
    and so holds phi on [z0 - H, z0 + nzl + H + 1) (H planes received from below, H + 1 from above)."""

    def __init__(self, shape, L, world, G):
        self.shape, self.L, self.world, self.G = tuple(shape), tuple(L), world, G
        self.nx, self.ny, self.nz = self.shape
        assert self.nz % world == 0
        self.nzl = self.nz // world
        self.grid = (self.nz, self.ny, self.nx)
        self.d = tuple(L[a] / self.shape[a] for a in range(3))

    def _planes(self, first, count):
        return np.unique(np.arange(first, first + count) % self.nz)

    def z0(self, r):
        return r * self.nzl

    def own(self, r):
        return self._planes(self.z0(r), self.nzl)

    def field(self, r):
        return self._planes(self.z0(r) - self.G, self.nzl + 2 * self.G + 1)

    def phi(self, r):
        return self._planes(self.z0(r) - self.G - 1, self.nzl + 2 * self.G + 3)

    def em_edge(self, r):
        H = self.G + 2
        return self._planes(self.z0(r) - H, self.nzl + 2 * H)

    def em_phi(self, r):
        H = self.G + 2
        return self._planes(self.z0(r) - H, self.nzl + 2 * H + 1)

    def received(self, r, em=False):
        """planes of phi that arrive from a neighbour"""
        return np.setdiff1d(self.em_phi(r) if em else self.phi(r), self.own(r))

    def ghost_field(self, r):
        return np.setdiff1d(self.field(r), self.own(r))

    def owner(self, plane):
        return int(plane) // self.nzl

    def lam_min(self):
        """the smallest non-zero (k2x + k2y) dz^2 of the grid: the worst-conditioned mode of the interface solve"""
        k2 = [(2.0 / self.d[a] * np.sin(np.pi * np.arange(1, self.shape[a] // 2 + 1) / self.shape[a])) ** 2 for a in (0, 1)]
        return float(min(k2[0].min(), k2[1].min())) * self.d[2] ** 2


def assemble(ranks_fixed, nzl):
    """the global int64 charge grid [nz][ny][nx] from each rank's own planes of its [nz][ny][nx] read-back"""
    out = np.zeros_like(ranks_fixed[0])
    for r, fixed in enumerate(ranks_fixed):
        out[r * nzl:(r + 1) * nzl] = fixed[r * nzl:(r + 1) * nzl]
    return out


def rho64(fixed, charge, macro_weight, shape, L):
    """the charge density of the integer grid: fixed q W / (2^42 dV), float64"""
    dV = np.prod([L[a] / shape[a] for a in range(3)])
    return fixed.astype(np.float64) * (charge * macro_weight / (FIXED_ONE * dV))


def reference_phi(fixed, charge, macro_weight, shape, L):
    return numpy_poisson(rho64(fixed, charge, macro_weight, shape, L), L)


def k2_term(factor, n, length):
    return (2.0 * n / length * np.sin(np.pi * NODE_FACTORS[factor][1](n) / n)) ** 2


def plane_pattern(shape, fx, fy):
    """c_y(j) c_x(i) [ny][nx] of two NODE_FACTORS names"""
    return NODE_FACTORS[fy][0](shape[1])[:, None] * NODE_FACTORS[fx][0](shape[0])[None, :]


def plane_source(shape, L, k0, fx, fy, rho0=1.0):
    """Plane k0 carries rho0 c_y(j) c_x(i) (not both factors 'one'), every other plane is empty: one (kx, ky) mode with
    every kz.  Along z the potential obeys -phi[k-1] + (2 + lam) phi[k] - phi[k+1] = rho[k] dz^2 / eps0 with
    lam = (k2x + k2y) dz^2, whose periodic Green's function is a sum of the two decaying powers of
    r = 2 / (2 + lam + sqrt(lam (lam + 4))):
        phi[k] = rho[k0] dz^2 / eps0 (r^d + r^(nz - d)) / ((1 / r - r) (1 - r^nz)),  d = (k - k0) mod nz.
    Returns (rho, phi), each [nz][ny][nx]."""
    nx, ny, nz = shape
    dz = L[2] / nz
    lam = (k2_term(fx, nx, L[0]) + k2_term(fy, ny, L[1])) * dz * dz
    assert lam > 0
    r = 2.0 / (2.0 + lam + np.sqrt(lam * (lam + 4.0)))
    d = (np.arange(nz) - k0) % nz
    green = (r ** d + r ** (nz - d)) / ((1.0 / r - r) * (1.0 - r ** nz))
    pat = plane_pattern(shape, fx, fy) * rho0
    rho = np.zeros((nz, ny, nx))
    rho[k0] = pat
    return rho, green[:, None, None] * pat[None] * (dz * dz / EPS0)


def sheet_source(shape, L, k0, rho0=1.0):
    """Every node of plane k0 carries rho0: only the (0, 0) line, with every kz (its mean is dropped).
        phi[k] = rho0 dz^2 / eps0 (g - mean g),  g = d (d - nz) / (2 nz),  d = (k - k0) mod nz."""
    nx, ny, nz = shape
    dz = L[2] / nz
    d = ((np.arange(nz) - k0) % nz).astype(np.float64)
    g = d * (d - nz) / (2.0 * nz)
    rho = np.zeros((nz, ny, nx))
    rho[k0] = rho0
    return rho, np.broadcast_to(((g - g.mean()) * (rho0 * dz * dz / EPS0))[:, None, None], (nz, ny, nx)).copy()


def central_e(phi, L):
    """E = -grad phi by central differences, [nz][ny][nx][3] (es3d_gradient's definition)"""
    nz, ny, nx = phi.shape
    out = np.empty(phi.shape + (3,))
    for comp, axis, n, length in ((0, 2, nx, L[0]), (1, 1, ny, L[1]), (2, 0, nz, L[2])):
        out[..., comp] = (np.roll(phi, 1, axis=axis) - np.roll(phi, -1, axis=axis)) * (n / (2.0 * length))
    return out
