"""Scenes and stage checks shared by tests/test_em_reference.py (the CPU oracle under the reference) and
tests/test_gpu_em_reference.py (the kernels under the same reference, same scenes, same bounds).  A simulator is driven
through a small adapter (`OracleBox`, `DeviceBox`) that speaks value[i][j][k][3] arrays; every check takes the simulator's OWN
read-back state as its input and returns (error, bound) arrays, so that a caller can print the figures and assert.

Bounds (T = the simulator's precision, eps = its machine epsilon):
  S1  node centring      2 eps x mean |samples averaged|          (1 or 3 rounded additions and an exact scaling: <= 1.5 eps)
  S2  velocity           K eps (|v0|_inf + 2 |h/c| sum w |E_node|), K = 32 -- the longest dependency chain of the
                         definition has about 24 rounded operations: 8 fused adds of the gather, the scaling by h/c, the half
                         kick, t = hB and 1 + t^2 (3), the division and s (2), two cross products with their additions
                         (2 x 3), the second half kick; |t| <= 1 in every scene, so the rotation does not amplify
  S2  position           eps + (dt c / L) x (the velocity bound), in periodic distance
  S3  current            exact
  S4  lattice            8 eps x sum |terms|
"""
import numpy as np

import em_reference as ref

ME, QE = 9.109e-31, -1.602e-19
C = ref.SPEED_OF_LIGHT
K_PUSH = 32


def eps_of(T):
    return float(np.finfo(T).eps)


def cfl_dt(shape, L, frac):
    return frac / (C * np.sqrt(sum((shape[a] / L[a]) ** 2 for a in range(3))))


def box_spec(shape, L, count, dt, solver, macro_weight):
    return dict(radius=L[0], length_y=L[1], height=L[2], nr=shape[0], ny=shape[1], nz=shape[2], dt=dt, nparticles=0, count=count,
                particle_mass=ME, particle_charge=QE, geometry="cart3d", solver=solver, macro_weight=macro_weight)


def to_ijk(a, shape):
    """[nodes][4] with node index i + nx (j + ny k)  ->  [nx][ny][nz][3]"""
    return np.asarray(a).reshape(shape[2], shape[1], shape[0], -1)[..., :3].transpose(2, 1, 0, 3)


# ------------------------------------------------------------------------------------------------------------------ adapters
class OracleBox:
    """oracle/es3d_oracle.OracleES3D behind the adapter's names"""

    def __init__(self, eo, spec, T):
        self.o, self.T, self.shape = eo.OracleES3D(spec, T), T, (spec["nr"], spec["ny"], spec["nz"])

    def add_species(self, mass, charge, count):
        return self.o.add_species(mass, charge, count)

    def set_particles(self, s, position, velocity):
        self.o.set(position=position, velocity=velocity, species=s)

    def set_lattice(self, E, B):
        self.o.set_lattice(E=E, B=B)

    def set_node_E(self, E):
        self.o.set(E=E)

    def add_b(self, b):
        self.o.add_b(*b)

    def precalc(self):
        self.o.precalc()

    def substeps(self, n):
        for _ in range(n):
            self.o.substep()

    def particles(self, s):
        return self.o.positions(s).copy(), self.o.velocities(s).copy()

    def field(self, name):
        a = {"E": self.o.E4, "B_nodes": getattr(self.o, "B4n", None), "edge_E": getattr(self.o, "Ey", None),
             "face_B": getattr(self.o, "By", None)}[name]
        return to_ijk(a.reshape(-1, 4), self.shape).copy()

    def j_fixed(self):
        return self.o.J_fixed.reshape(-1, 3).copy()

    def close(self):
        pass


class DeviceBox:
    """fusionpic's box handle behind the adapter's names (public API only)"""

    def __init__(self, fp, spec, T):
        self.fp, self.T, self.shape = fp, T, (spec["nr"], spec["ny"], spec["nz"])
        self.s = fp.makeCylindricalParticlePusher(spec, precision="fp32" if T == np.float32 else "fp64")

    def add_species(self, mass, charge, count):
        return self.s.addSpecies(mass, charge, count)

    def set_particles(self, s, position, velocity):
        self.s.set(position=position, velocity=velocity, species=s)

    def set_lattice(self, E, B):
        self.s.set(edge_E=E, face_B=B)

    def set_node_E(self, E):
        self.s.set(E=E)

    def add_b(self, b):
        self.s.addB(*b)

    def precalc(self):
        self.s.precalc()

    def substeps(self, n):
        self.s.substeps(n)

    def particles(self, s):
        p = self.s.getParticles(species=s)
        return p["position"], p["velocity"]

    def field(self, name):
        which = {"E": self.fp.F3_E, "B_nodes": self.fp.F3_B_NODES, "edge_E": self.fp.F3_EDGE_E, "face_B": self.fp.F3_FACE_B}[name]
        return to_ijk(self.s.readField(which), self.shape).copy()

    def j_fixed(self):
        return self.s.readField(self.fp.F3_J_FIXED).copy()

    def close(self):
        self.s.destroy()


# -------------------------------------------------------------------------------------------------------------------- scenes
class Scene:
    """spec, box, and per species (mass, charge, Z, position [m], velocity [c])"""

    def __init__(self, shape, d, dt_frac, solver, macro_weight, species):
        self.shape, self.d = tuple(shape), tuple(d)
        self.L = tuple(shape[a] * d[a] for a in range(3))
        self.dt = cfl_dt(shape, self.L, dt_frac)
        self.species = species
        self.spec = box_spec(shape, self.L, 0, self.dt, solver, macro_weight)     # count: set with the species
        self.q0W = QE * macro_weight
        self.k = np.array([self.dt * C / self.L[a] for a in range(3)])
        self.E = self.B = self.node_E = self.b0 = None

    def h(self, s):
        return self.species[s][1] * self.dt / (2 * self.species[s][0])

    def build(self, make):
        """a simulator holding the scene; `make(spec)` returns an adapter"""
        sim = make(self.spec)
        for s, (mass, charge, _, pos, vel) in enumerate(self.species):
            if s:
                assert sim.add_species(mass, charge, len(pos)) == s
            sim.set_particles(s, pos, vel)
        if self.node_E is not None:
            sim.set_node_E(self.node_E)
        if self.b0 is not None:
            sim.add_b(self.b0)
        if self.E is not None:
            sim.set_lattice(self.E, self.B)
        else:
            sim.precalc()
        return sim


STAGE_CELL = (1e-3, 2e-3, 0.5e-3)       # non-cubic: 1.5 c along z moves 1.18 cells per sub-step at 0.9 of the CFL limit
STAGE_SHAPES = [(3, 3, 3), (8, 6, 10), (20, 16, 12)]


def _population(rng, n, L, d, sigma, k_fine):
    """n particles: uniform positions, N(0, sigma c) velocities; the first 12 move 1.5 c along the finest axis (z), half of
    them backwards; the next 6 sit on nodes, on faces and at L (1 - 1e-9)"""
    pos, vel = rng.random((n, 3)) * L, rng.normal(0, sigma, (n, 3))
    vel[:12] = rng.normal(0, 0.05, (12, 3))
    vel[:12, 2] = 1.5 * np.where(np.arange(12) % 2, -1.0, 1.0)
    Lx, Ly, Lz = L
    pos[12:18] = [[0, 0, 0], [d[0], 2 * d[1], d[2]], [d[0], 0.3 * Ly, 0.7 * Lz], [0.4 * Lx, 0.6 * Ly, 2 * d[2]],
                  [Lx * (1 - 1e-9), Ly * (1 - 1e-9), Lz * (1 - 1e-9)], [0.5 * Lx, Ly * (1 - 1e-9), 0]]
    assert (np.abs(vel) * k_fine).max() < 0.5, "a move of half the box or more has no nearest image"
    return pos, vel


def stage_scene(shape):
    """the scene of the stage checks S1 .. S4: two species in random lattice fields"""
    rng = np.random.default_rng(shape[0] * 10000 + shape[1] * 100 + shape[2])
    sc = Scene(shape, STAGE_CELL, 0.9, "yee", 1e6, [None])
    ne, ni = 3001, 600
    pe, ve = _population(rng, ne, sc.L, sc.d, 0.35, sc.k.max())
    pi, vi = _population(rng, ni, sc.L, sc.d, 0.05, sc.k.max())
    sc.species = [(ME, QE, 1, pe, ve), (1836 * ME, -2 * QE, -2, pi, vi)]
    sc.spec["count"] = ne
    sc.E, sc.B = rng.normal(0, 1e4, sc.shape + (3,)), rng.normal(0, 0.05, sc.shape + (3,))
    return sc


LONG_SHAPE = (4, 3, 70000)
LONG_BANDS = (32768, 65536, 70000)      # where a doubled 32-bit coordinate changes sign, where it wraps, the periodic seam


def long_scene(_=None):
    """S3 where an index can leave 32 bits: the stage scene on 70000 planes with the particles within a cell of the planes
    32768 and 65536 (a doubled fixed-point coordinate, 2^15 per cell, reaches 2^30 and 2^31 there) and of the periodic seam,
    a fifth of them anywhere; many cross these planes in the sub-step, some by more than a cell"""
    shape = LONG_SHAPE
    rng = np.random.default_rng(70000)
    sc = Scene(shape, STAGE_CELL, 0.9, "yee", 1e6, [None])
    species = []
    for n, sigma in ((2000, 0.35), (300, 0.05)):
        pos, vel = _population(rng, n, sc.L, sc.d, sigma, sc.k.max())
        band = rng.integers(0, len(LONG_BANDS) + 2, n)
        near = band < len(LONG_BANDS)
        near[12:18] = False                                     # (the positions on nodes, faces and at L (1 - 1e-9) stay)
        z = (np.array(LONG_BANDS)[np.minimum(band, len(LONG_BANDS) - 1)] + rng.uniform(-1, 1, n)) % shape[2]
        pos[near, 2] = z[near] * sc.d[2]
        species.append((pos, vel))
    sc.species = [(ME, QE, 1) + species[0], (1836 * ME, -2 * QE, -2) + species[1]]
    sc.spec["count"] = len(species[0][0])
    sc.E, sc.B = rng.normal(0, 1e4, shape + (3,)), rng.normal(0, 0.05, shape + (3,))
    return sc


def crossings(r, plane):
    """how many particles of the record cross the plane z = `plane` cells in the sub-step (the seam: plane = nz)"""
    sc, total = r.sc, 0
    for s in range(len(sc.species)):
        a = ref.fixed_coordinate(r.old[s][0], sc.shape, r.T)
        b = ref.nearest_image(a, ref.fixed_coordinate(r.new[s][0], sc.shape, r.T), sc.shape)
        za, zb = a[:, 2] - (plane % sc.shape[2]) * ref.S, b[:, 2] - (plane % sc.shape[2]) * ref.S
        if plane % sc.shape[2] == 0:                            # the seam: seen from either side
            box = sc.shape[2] * ref.S
            shift = np.where(za > box // 2, box, 0)
            za, zb = za - shift, zb - shift
        total += int(((za < 0) != (zb < 0)).sum())
    return total


def affine_scene():
    """K1: E and B affine in the lattice coordinate, each component sampled where the lattice holds it; 2000 electrons at
    rest in the cells 2 .. n-3 (the field is not periodic: nobody gathers across the seam).  Every sample is a multiple of
    2^-1 below 2^15 (E) resp. of 2^-11 below 2^4 (B): exact in float32, so the analytic field IS the uploaded one.
    |t| = h |B| is about 0.3."""
    shape = (10, 8, 12)
    rng = np.random.default_rng(101)
    sc = Scene(shape, (1e-3, 1e-3, 1e-3), 0.5, "yee", 1e-30, [None])
    n = 2000
    pos = (2 + rng.random((n, 3)) * (np.array(shape) - 4)) * sc.d
    sc.species = [(ME, QE, 1, pos, np.zeros((n, 3)))]
    sc.spec["count"] = n
    h = abs(sc.h(0))
    unit = 2.0 ** -11
    scale = 0.3 / h / np.sqrt(3) / unit                        # |B| of 0.3 / h in units of 2^-11 T, per component
    sc.E0, sc.GE = np.array([9000.0, -7000.0, 8000.0]), np.array([[300, -500, 200], [-400, 250, 350], [150, 450, -300]], dtype=np.float64)
    sc.B0 = np.round(np.array([1.0, -0.9, 1.1]) * scale) * unit
    sc.GB = np.round(np.array([[0.04, -0.03, 0.02], [-0.02, 0.05, 0.03], [0.03, 0.02, -0.04]]) * scale) * 2 * unit
    idx = np.stack(np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij"), axis=-1)
    sc.E, sc.B = np.empty(shape + (3,)), np.empty(shape + (3,))
    for m in range(3):
        on_edge = idx + 0.5 * np.eye(3)[m]                      # Ex at (i+1/2, j, k), ...
        on_face = idx + 0.5 * (1 - np.eye(3)[m])                # Bx at (i, j+1/2, k+1/2), ...
        sc.E[..., m] = sc.E0[m] + on_edge @ sc.GE[m]
        sc.B[..., m] = sc.B0[m] + on_face @ sc.GB[m]
    sc.analytic = lambda xi: (sc.E0 + xi @ sc.GE.T, sc.B0 + xi @ sc.GB.T)       # xi: lattice coordinate [N][3]
    return sc


def drift_scene(solver):
    """K2: uniform E perpendicular to B, |t| = h |B| = 0.4, drift 0.05 c; 500 electrons of sigma = 0.2 c on 6 x 5 x 7"""
    shape = (6, 5, 7)
    rng = np.random.default_rng(202)
    sc = Scene(shape, (1e-3, 1e-3, 1e-3), 0.5, solver, 1e-30, [None])
    n = 500
    sc.species = [(ME, QE, 1, rng.random((n, 3)) * sc.L, rng.normal(0, 0.2, (n, 3)))]
    sc.spec["count"] = n
    bhat = np.array([2.0, -1.0, 2.0]) / 3.0
    ehat = np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)             # perpendicular to bhat
    sc.Bu = bhat * 0.4 / abs(sc.h(0))
    sc.Eu = ehat * 0.05 * C * np.linalg.norm(sc.Bu)             # |E| / (|B| c) = 0.05
    if solver == "yee":
        sc.E, sc.B = np.broadcast_to(sc.Eu, shape + (3,)).copy(), np.broadcast_to(sc.Bu, shape + (3,)).copy()
    else:
        sc.node_E, sc.b0 = np.broadcast_to(sc.Eu, shape + (3,)).copy(), sc.Bu
    return sc


def drift_closed_form(sc, v0, N):
    """v_N = v_d + R^N (v_0 - v_d): v_d = E x B / (B^2 c), R the rotation about B/|B| by -2 atan(h |B|), h signed
    (Rodrigues' formula)."""
    h = sc.h(0)
    Bn = np.linalg.norm(sc.Bu)
    vd = np.cross(sc.Eu, sc.Bu) / (Bn ** 2 * C)
    ang = -2.0 * np.arctan(h * Bn) * N
    k = sc.Bu / Bn
    w = v0 - vd
    return vd + w * np.cos(ang) + np.cross(k, w) * np.sin(ang) + k * (w @ k)[:, None] * (1 - np.cos(ang)), vd


def es_scene(shape):
    """K3: the electrostatic push (solver 'none') in a random node field and a uniform B of |t| about 0.3; a third of the
    electrons cross a good part of a cell per sub-step, so that after the warm-up sub-steps some gather from outside their
    tile's window"""
    rng = np.random.default_rng(shape[0] * 7 + shape[2])
    sc = Scene(shape, (1e-3, 1e-3, 1e-3), 0.9, "none", 2e4, [None])
    n, ni = 4000, 600
    vel = rng.normal(0, 0.01, (n, 3)) + rng.normal(0, 0.4, (n, 3)) * (rng.random((n, 1)) < 0.3)
    sc.species = [(ME, QE, 1, rng.random((n, 3)) * sc.L, vel),
                  (1836 * ME, -2 * QE, -2, rng.random((ni, 3)) * sc.L, rng.normal(0, 0.05, (ni, 3)))]
    sc.spec["count"] = n
    sc.node_E = rng.normal(0, 3e4, sc.shape + (3,))
    sc.b0 = np.array([0.3, -0.2, 0.9]) / np.linalg.norm([0.3, -0.2, 0.9]) * 0.3 / abs(sc.h(0))
    return sc


# -------------------------------------------------------------------------------------------------------------------- record
class Record:
    """the read-backs around ONE sub-step"""


def record_substep(sim, sc, yee=True):
    r = Record()
    r.sc, r.T = sc, sim.T
    ns = len(sc.species)
    r.old = [sim.particles(s) for s in range(ns)]
    r.E_nodes = sim.field("E")
    if yee:
        r.edge_E, r.face_B, r.B_nodes = sim.field("edge_E"), sim.field("face_B"), sim.field("B_nodes")
    sim.substeps(1)
    r.new = [sim.particles(s) for s in range(ns)]
    if yee:
        r.J, r.edge_E1, r.face_B1 = sim.j_fixed(), sim.field("edge_E"), sim.field("face_B")
    for s in range(ns):
        assert r.old[s][0].dtype == np.dtype(r.T)
    return r


# -------------------------------------------------------------------------------------------------------------------- checks
def check_nodes(r, node_fields=ref.node_fields):
    """S1 -> (error, bound) of the node-centred E and B, concatenated"""
    En, Bn, Ea, Ba = node_fields(r.edge_E, r.face_B)
    eps = eps_of(r.T)
    err = np.concatenate([np.abs(r.E_nodes - En).ravel(), np.abs(r.B_nodes - Bn).ravel()])
    return err, 2 * eps * np.concatenate([Ea.ravel(), Ba.ravel()])


def reference_push(r, s, E_nodes, B, boris=ref.boris):
    """reference velocity and position of species s after the sub-step from its OLD read-back state, in the given node
    fields (B: a node array, or a uniform 3-vector)  ->  (v_ref, v_bound, u_ref, u_bound)"""
    sc = r.sc
    u0, v0 = r.old[s]
    i, w1 = ref.cells_and_weights(u0, sc.shape, r.T)
    E_p, E_abs = ref.gather(E_nodes, i, w1)
    B_p = ref.gather(B, i, w1)[0] if np.ndim(B) == 4 else np.asarray(B, np.float64)
    h = sc.h(s)
    assert (h * h * (np.atleast_2d(B_p) ** 2).sum(axis=1)).max() <= 1.0, "|t| <= 1 is what the bound assumes"
    v_ref, mag = boris(v0, E_p, B_p, h, C, E_abs=E_abs)
    eps = eps_of(r.T)
    v_bound = K_PUSH * eps * mag[:, None] * np.ones(3)
    u_ref, _ = ref.drift(u0, v_ref, sc.k)
    return v_ref, v_bound, u_ref, eps + sc.k * v_bound


def check_push(r, s, E_nodes=None, B=None, boris=ref.boris):
    """S2 -> (velocity error, bound, position error, bound) of species s"""
    E_nodes = r.E_nodes if E_nodes is None else E_nodes
    B = r.B_nodes if B is None else B
    v_ref, v_bound, u_ref, u_bound = reference_push(r, s, E_nodes, B, boris)
    u1, v1 = r.new[s]
    return np.abs(v1 - v_ref), v_bound, ref.periodic_distance(u1, u_ref), u_bound


def reference_current(r, **kw):
    """S3 -> (J_fixed of the device's own moves, first moment per axis)"""
    sc = r.sc
    J = np.zeros((int(np.prod(sc.shape)), 3), dtype=np.int64)
    moment = np.zeros(3, dtype=np.int64)
    for s, (_, _, Z, _, _) in enumerate(sc.species):
        a = ref.fixed_coordinate(r.old[s][0], sc.shape, r.T)
        b = ref.fixed_coordinate(r.new[s][0], sc.shape, r.T)
        J += ref.current_exact(a, b, sc.shape, Z, **kw)
        moment += ref.first_moment(a, b, sc.shape, Z)
    return J, moment


def continuity_of(r):
    """96 (rho_new - rho_old) + div J_fixed per node, rho the CIC charge of the read-back positions, J the simulator's"""
    sc = r.sc
    res = np.zeros(sc.shape, dtype=np.int64)
    for s, (_, _, Z, _, _) in enumerate(sc.species):
        a = ref.fixed_coordinate(r.old[s][0], sc.shape, r.T)
        b = ref.fixed_coordinate(r.new[s][0], sc.shape, r.T)
        res += 96 * (ref.cic_charge(b, sc.shape, Z) - ref.cic_charge(a, sc.shape, Z))
    return res + ref.divergence(r.J, sc.shape)


def check_lattice(r, sign=1):
    """S4 -> (error, bound) of the new edge E and face B, concatenated, from the pre-step lattice and the device's J_fixed"""
    sc = r.sc
    E1, B1, Ea, Ba = ref.yee_substep(r.edge_E, r.face_B, sign * r.J, sc.dt, sc.d, sc.q0W)
    eps = eps_of(r.T)
    err = np.concatenate([np.abs(r.edge_E1 - E1).ravel(), np.abs(r.face_B1 - B1).ravel()])
    return err, 8 * eps * np.concatenate([Ea.ravel(), Ba.ravel()])


def affine_reference(r, node_fields=None):
    """K1 -> (v_ref, bound): Boris in the ANALYTIC field at the quantised position (i + w1 / 2^14) d.  With `node_fields`
    (a deliberately wrong centring: the sensitivity control) the fields are gathered from ITS nodes instead."""
    sc = r.sc
    u0, v0 = r.old[0]
    i, w1 = ref.cells_and_weights(u0, sc.shape, r.T)
    E_p, B_p = sc.analytic(i + w1 / float(ref.WEIGHT_ONE))
    E_abs = ref.gather(np.abs(r.E_nodes), i, w1)[0]
    if node_fields is not None:
        En, Bn = node_fields(r.edge_E, r.face_B)[:2]
        E_p, B_p = ref.gather(En, i, w1)[0], ref.gather(Bn, i, w1)[0]
    v_ref, mag = ref.boris(v0, E_p, B_p, sc.h(0), C, E_abs=E_abs)
    return v_ref, K_PUSH * eps_of(r.T) * mag[:, None] * np.ones(3)


def check_affine(r):
    v_ref, bound = affine_reference(r)
    return np.abs(r.new[0][1] - v_ref), bound


def drift_run(make, solver, N=40):
    """K2 -> (error [N][3], bound, relative movement of the lattice fields)"""
    scene = drift_scene(solver)
    sim = scene.build(make)
    v0 = sim.particles(0)[1].astype(np.float64)
    sim.substeps(N)
    want, vd = drift_closed_form(scene, v0, N)
    err = np.abs(sim.particles(0)[1] - want)
    bound = 8 * N * eps_of(sim.T) * (np.abs(v0 - vd).max() + np.abs(vd).max())
    moved = 0.0
    if solver == "yee":
        moved = max(np.abs(sim.field("edge_E") - scene.Eu).max() / np.abs(scene.Eu).max(),
                    np.abs(sim.field("face_B") - scene.Bu).max() / np.abs(scene.Bu).max())
    sim.close()
    return err, np.full_like(err, bound), moved


def report(tag, err, bound):
    """prints the figure before anybody asserts: the largest error over its bound"""
    ratio = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
    print("%-40s max error %.3e  max error / bound %.4f" % (tag, float(err.max()), ratio))
    return ratio
