"""The slab-decomposed Poisson solves (fusion-sim_amd/csrc/fes_domain.inc.hpp: solve_distributed, dom_fields and the X_PHI
exchange; the three kernels of csrc/fes_tri.hpp; the transpose kernels) against float64 references that share no code
with the library or the oracle (tests/decomposed_solve_reference.py): numpy's FFT applied to the charge grid assembled from
the ranks' OWN planes, two closed forms without any FFT, and exact eigenmodes.  The ranks are in-process handles under
fusionpic.BoxGroup; one GPU runs every case.

Modes: R replicated (distributed_solve=False), T transposed spectrum (True), I interface solve ("interface").
On every rank of every case, after group.precalc() and again after one group.step() (check_frame):
  1. the charge grid assembled from the ranks' own planes sums to n 2^42 exactly (pattern cases: it IS the pattern);
  2. phi on the planes the rank must hold (own, G + 1 received below, G + 2 above) within TOL (2e-5 / 1e-12) of max |want|
     (I in fp64: max(1e-12, 100 eps (1 + 1 / lam_min)), the core's bar of tests/test_tri_core.py);
  3. a received plane of phi has the bits of its owner's phi;           4. E4[..., 3] has the bits of phi where E is formed;
  5. E there is the central difference of the rank's OWN phi (the bound of the one-handle module's check_central_e);
  6. E on a ghost plane has the bits of its owner's E;
  7. T with the library's own passes: phi on own planes has the bits of ONE undecomposed handle's;
  8. R, T and I of one case agree within TOL (after precalc(): the same charge grid, asserted);
  9. no particle is lost and, after the step, every id is held by exactly one rank.
Families: A a lumpy cloud on the smallest grids of every structural edge (nzl = G + 2, overlapping received planes,
nzs = nz - 1, nyl = 1, eight ranks, flat cells, three ranks on rocFFT, the switches FPIC_DOMAIN_OVERLAP / _COMPACT /
FPIC_POISSON_FFT); B the closed forms with the charged plane on the seam, on a slab's first and last plane, inside and on
nz - 1; C exact eigenmodes through the ranks; D the full-EM start on ranks.  The worst ratio of every family is printed
at the end of the module (pytest -s).  The check functions are plain numpy on read-backs: tests/test_decomposed_solve_reference.py
applies them to deliberately wrong results of a CPU emulation.
"""
import numpy as np
import pytest

import decomposed_solve_reference as dr
from helpers import node_mode, same_bits
from test_gpu_field_solve import (EIGEN_TOL, EPS, FIXED_ONE, L3, ME, MP, PATTERNS, QE, TOL, WORST, axes_of, box_spec, cfl_dt,
                                  check_phi, grid_id, lumpy_cloud, make_box, note, own_fft_takes)

pytestmark = pytest.mark.gpu

MODES = {"R": False, "T": True, "I": "interface"}
PRECISIONS = ["fp32", "fp64"]
FLAT = (0.064, 0.008, 0.004)                 # cells 1 x 1 x 0.125 mm: lam_min = 1.5e-4 on 64 nodes along x


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    for family in sorted(f for f in WORST if f.startswith("dec ")):
        print("worst ratio  %-34s %.3g" % (family, WORST.pop(family)))


# ------------------------------------------------------------------------------------ the checks (numpy on read-backs)
# A rank's view: dict(fixed=int64 [nz][ny][nx], phi=T [nz][ny][nx], e4=T [nz][ny][nx][4]) as readField() gives them: only
# the planes the rank holds mean anything, and no check reads another.

def phi_bound(geo, mode, precision):
    if mode == "I" and precision == "fp64":
        return max(TOL["fp64"], 100 * EPS["fp64"] * (1.0 + 1.0 / geo.lam_min()))
    return TOL[precision]


def measure_phi(views, geo, want, top, em=False):
    """check 2's figure: the worst |phi - want| / max |want| over every rank's phi set"""
    worst = 0.0
    for r, v in enumerate(views):
        planes = geo.em_phi(r) if em else geo.phi(r)
        worst = max(worst, float(np.abs(v["phi"][planes].astype(np.float64) - want[planes]).max()) / top)
    return worst


def check_phi_sets(views, geo, want, bound, family, what, em=False):
    top = float(np.abs(want).max())
    assert top > 0, what
    ratio = measure_phi(views, geo, want, top, em)
    note(family, ratio)
    assert ratio <= bound, "%s: max |phi - reference| / max |phi| on a rank's planes = %.3g (bound %.3g)" % (what, ratio, bound)
    return top


def check_copies(views, geo, what):
    """checks 3, 4 and 6: what a rank received or formed from received planes has the owner's bits"""
    for r, v in enumerate(views):
        for p in geo.received(r):
            assert same_bits(v["phi"][p], views[geo.owner(p)]["phi"][p]), "%s: rank %d's phi on plane %d is not rank %d's" % (what, r, p, geo.owner(p))
        planes = geo.field(r)
        assert same_bits(v["e4"][planes][..., 3], v["phi"][planes]), "%s: rank %d: E4[..., 3] is not phi" % (what, r)
        for p in geo.ghost_field(r):
            assert same_bits(v["e4"][p], views[geo.owner(p)]["e4"][p]), "%s: rank %d's E on ghost plane %d is not rank %d's" % (what, r, p, geo.owner(p))


def measure_central_e(views, geo, eps, top):
    """check 5's figures: per rank and component, E against the central differences of the rank's own phi on its field
    set (x and y within the plane, z from the two neighbouring held planes); returns the worst difference in units of
    max |phi| / (2 d), and the worst difference / bound with check_central_e's bound"""
    worst_ratio = worst_factor = 0.0
    for r, v in enumerate(views):
        planes = geo.field(r)
        p = v["phi"].astype(np.float64)
        for comp, axis, n, length in axes_of(p, geo.L):
            h = n / (2.0 * length)
            grad = ((np.roll(p, 1, axis=axis) - np.roll(p, -1, axis=axis)) * h)[planes]
            worst = float(np.abs(v["e4"][planes][..., comp].astype(np.float64) - grad).max())
            bound = 4 * eps * top * h + 1e-6 * float(np.abs(grad).max())
            worst_ratio, worst_factor = max(worst_ratio, worst / (top * h)), max(worst_factor, worst / bound)
    return worst_ratio, worst_factor


def check_rank_central_e(views, geo, eps, top, family, what):
    ratio, factor = measure_central_e(views, geo, eps, top)
    note(family + " E", ratio)
    assert factor <= 1.0, "%s: E off the central difference of the rank's own phi by %.3g of max |phi| / (2 d): %.3g times the bound" % (what, ratio, factor)


def measure_exact_e(views, geo, want, top):
    """E on every rank's field set against the central differences of a closed form, in units of max |phi| / (2 d)"""
    exact = dr.central_e(want, geo.L)
    worst = 0.0
    for r, v in enumerate(views):
        planes = geo.field(r)
        for comp in range(3):
            h = geo.shape[comp] / (2.0 * geo.L[comp])
            worst = max(worst, float(np.abs(v["e4"][planes][..., comp].astype(np.float64) - exact[planes][..., comp]).max()) / (top * h))
    return worst


def check_frame(views, geo, mode, precision, count, family, what, pattern=None, charge=QE, macro_weight=1e9):
    """checks 1 to 6 on one set of read-backs; returns (the assembled charge grid, the float64 reference, max |want|)"""
    fixed = dr.assemble([v["fixed"] for v in views], geo.nzl)
    if pattern is not None:
        assert np.array_equal(fixed, pattern.astype(np.int64) * FIXED_ONE), what + ": the assembled charge grid is not the pattern"
    else:
        assert int(fixed.sum()) == count * FIXED_ONE, what + ": the assembled charge grid does not hold the total charge"
    want = dr.reference_phi(fixed, charge, macro_weight, geo.shape, geo.L)
    bound = phi_bound(geo, mode, precision)
    top = check_phi(own_phi(views, geo), want, bound, family, what)              # every rank's own planes, as one grid
    assert check_phi_sets(views, geo, want, bound, family, what) == top
    check_copies(views, geo, what)
    check_rank_central_e(views, geo, EPS[precision], top, family, what)
    return fixed, want, top


# ------------------------------------------------------------------------------------ running a group of ranks

def thermal(n, seed):
    return np.random.default_rng(seed).normal(0, 0.02, (n, 3))


def slow_dt(geo):
    """0.02 c moves 0.03 of the shortest cell edge per sub-step (as test_slab_decomposed_poisson_solve: 1 mm cells, 5e-12 s)"""
    return 0.03 * min(geo.d) / (0.02 * 2.998e8)


def weight_for(L):
    """the macro weight of box_spec (1e9 in the 0.7 x 1.3 x 0.9 m box) at the same density"""
    return 1e9 * float(np.prod(L)) / float(np.prod(L3))


def owners(pos, geo):
    """the rank owning each particle's plane; a particle ON a node (within 2^-17 of a cell) belongs to the node's plane"""
    plane = np.floor(pos[:, 2] / geo.d[2] + 2.0 ** -17).astype(int) % geo.nz
    return plane // geo.nzl


def read_views(fp, ranks, geo, em=False):
    views = []
    for s in ranks:
        v = dict(fixed=s.readField(fp.F3_RHO_FIXED).reshape(geo.grid), phi=s.readField(fp.F3_PHI).reshape(geo.grid))
        if em:
            v["edge"] = s.readField(fp.F3_EDGE_E).reshape(geo.grid + (4,))
        else:
            v["e4"] = s.readField(fp.F3_E).reshape(geo.grid + (4,))
        views.append(v)
    return views


def run_ranks(fp, monkeypatch, geo, precision, mode, species, solver="poisson_fft", dt=None, path="default", env=(), step=True):
    """species: [(mass, charge, position, velocity)], the first one the electrons of box_spec.  Every rank is created and
    decomposed with the environment switches `env` set, gets the particles of its planes (ids contiguous per rank), and
    the group runs precalc() and (step) one step().  Returns the read-backs after each and the ids' completeness."""
    em = solver == "yee"
    dt = slow_dt(geo) if dt is None else dt
    spec = box_spec(geo.shape, len(species[0][2]), solver=solver, dt=dt, macro_weight=weight_for(geo.L), L=geo.L)
    parts = []
    for mass, charge, pos, vel in species:
        own = owners(pos, geo)
        order = np.argsort(own, kind="stable")
        parts.append((pos[order], vel[order], np.bincount(own, minlength=geo.world)))
    ranks = []
    for key, value in dict(env).items():
        monkeypatch.setenv(key, value)
    try:
        for r in range(geo.world):
            s = make_box(fp, monkeypatch, spec, precision, path)
            ranks.append(s)
            for sp in range(1, len(species)):
                assert s.addSpecies(species[sp][0], species[sp][1], len(species[sp][2])) == sp
            s.domainInit(r, geo.world, ghost_planes=geo.G, migrate_every=2, distributed_solve=MODES[mode])
    finally:
        for key in dict(env):
            monkeypatch.delenv(key, raising=False)
    for r, s in enumerate(ranks):
        for sp, (pos, vel, counts) in enumerate(parts):
            first = int(counts[:r].sum())
            if counts[r]:
                s.domainSet(pos[first:first + counts[r]], vel[first:first + counts[r]], first_id=first, species=sp)
    group = fp.BoxGroup(ranks)
    group.precalc()
    frames = [read_views(fp, ranks, geo, em)]
    if step:
        group.step()
        frames.append(read_views(fp, ranks, geo, em))
        for sp, (pos, _, _) in enumerate(parts):                                   # check 9
            ids = np.concatenate([s.domainGet(species=sp)["ids"] for s in ranks])
            assert np.array_equal(np.sort(ids), np.arange(len(pos))), "species %d: the ranks do not hold every id once" % sp
    assert all(s.domainStats()["lost"] == 0 for s in ranks)
    for s in ranks:
        s.destroy()
    return frames


def one_handle(fp, monkeypatch, geo, precision, species, solver="poisson_fft", dt=None, path="default", em=False):
    """the same charge on ONE undecomposed handle after precalc()"""
    dt = slow_dt(geo) if dt is None else dt
    sim = make_box(fp, monkeypatch, box_spec(geo.shape, len(species[0][2]), solver=solver, dt=dt, macro_weight=weight_for(geo.L), L=geo.L), precision, path)
    for sp, (mass, charge, pos, vel) in enumerate(species):
        if sp:
            assert sim.addSpecies(mass, charge, len(pos)) == sp
        sim.set(position=pos, velocity=vel, species=sp)
    sim.precalc()
    out = read_views(fp, [sim], geo, em)[0]
    sim.destroy()
    return out


def own_phi(views, geo):
    """phi [nz][ny][nx] from every rank's own planes"""
    out = np.empty_like(views[0]["phi"])
    for r, v in enumerate(views):
        out[geo.own(r)] = v["phi"][geo.own(r)]
    return out


def check_same_bits_as(views, other, geo, what):
    for r, (a, b) in enumerate(zip(views, other)):
        assert np.array_equal(a["fixed"][geo.own(r)], b["fixed"][geo.own(r)]), (what, r)
        assert same_bits(a["phi"][geo.phi(r)], b["phi"][geo.phi(r)]), "%s: rank %d: phi differs" % (what, r)
        assert same_bits(a["e4"][geo.field(r)], b["e4"][geo.field(r)]), "%s: rank %d: E differs" % (what, r)


# ------------------------------------------------------------------------------------ A: a lumpy cloud on every structural edge

# (world, shape, G, modes, L)
A_CASES = [
    (2, (8, 8, 8), 1, "RTI", L3),        # nzl = 4: each rank is both neighbours of the other, the 3 + 2 received planes of phi overlap; nzs = 11 >= nz
    (2, (8, 16, 16), 1, "TI", L3),       # compact with nzs = 15 = nz - 1: exactly one plane not held
    (2, (8, 16, 16), 3, "TI", L3),       # 2 G + 1 = 7 <= 8; nzs = 19: whole-grid arrays
    (4, (16, 8, 16), 2, "RTI", L3),      # nzl = G + 2: the planes from above are the neighbour's whole slab; nyl = 2
    (8, (8, 8, 32), 1, "TI", L3),        # nyl = 1; eight ranks = festri::kMaxRanks
    (8, (32, 16, 64), 3, "TI", L3),      # the general case, uneven cells
    (4, (64, 8, 32), 2, "TI", FLAT),     # flat cells: lam_min = 1.5e-4, the longest wave of a 512^3 cube
    (3, (12, 6, 12), 1, "RT", L3),       # the decomposed rocFFT branch; a world that is no power of two; nzl = 4, nyl = 2
]
N_CLOUD = 20000


def case_id(case):
    return "w%d-%s-G%d" % (case[0], grid_id(case[1]), case[2])


def cloud(geo):
    pos = lumpy_cloud(geo.shape, N_CLOUD, geo.L)
    return [(ME, QE, pos, thermal(len(pos), geo.world))]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", A_CASES, ids=case_id)
def test_lumpy_cloud_on_ranks(fp, monkeypatch, case, precision):
    """A: checks 1 to 9 in every mode the case names, after precalc() and after one step()"""
    world, shape, G, modes, L = case
    geo = dr.Slabs(shape, L, world, G)
    species = cloud(geo)
    weight = weight_for(L)
    start = {}
    for mode in modes:
        what = "%s %s %s" % (case_id(case), mode, precision)
        family = "dec A %s %s" % (mode, precision)
        frames = run_ranks(fp, monkeypatch, geo, precision, mode, species)
        for tag, views in zip(("precalc", "step"), frames):
            fixed, want, top = check_frame(views, geo, mode, precision, N_CLOUD, family, what + " " + tag, macro_weight=weight)
            if tag == "precalc":
                start[mode] = (fixed, own_phi(views, geo), top, views)
    first = modes[0]
    for mode in modes[1:]:                                                       # check 8
        assert np.array_equal(start[mode][0], start[first][0]), (case_id(case), mode)
        ratio = float(np.abs(start[mode][1].astype(np.float64) - start[first][1]).max()) / start[first][2]
        note("dec A %s-%s %s" % (first, mode, precision), ratio)
        bound = max(phi_bound(geo, m, precision) for m in (first, mode))
        assert ratio <= bound, "%s: %s and %s differ by %.3g of max |phi| (bound %.3g)" % (case_id(case), first, mode, ratio, bound)
    if own_fft_takes(shape):                                                     # check 7
        one = one_handle(fp, monkeypatch, geo, precision, species)
        assert np.array_equal(one["fixed"], start["T"][0])
        assert same_bits(start["T"][1], one["phi"]), "%s %s: the transposed solve's phi is not one handle's, bit for bit (worst %.3g of max |phi|)" % (
            case_id(case), precision, float(np.abs(start["T"][1].astype(np.float64) - one["phi"]).max()) / start["T"][2])
    if L is FLAT:
        # float storage of g and of (y_1, y_m) for the longest waves: the decomposed solves beside one handle's
        ratio = {m: float(np.abs(start[m][1].astype(np.float64) - dr.reference_phi(start[m][0], QE, weight, shape, L)).max()) / start[m][2] for m in modes}
        ratio["one"] = float(np.abs(one["phi"].astype(np.float64) - dr.reference_phi(one["fixed"], QE, weight, shape, L)).max()) / start["T"][2]
        print("flat cells %s: max |phi - numpy| / max |phi|  " % precision + "  ".join("%s %.3g" % kv for kv in sorted(ratio.items())))
        note("dec A flat one handle " + precision, ratio["one"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rocfft_forced_on_ranks(fp, monkeypatch, precision):
    """A: the decomposed rocFFT branch on a grid the own passes take (FPIC_POISSON_FFT=rocfft while the handles are created):
    every check of T, within TOL of the own-pass T, and NOT its bits (the switch took effect)"""
    geo = dr.Slabs((16, 8, 16), L3, 4, 2)
    species = cloud(geo)
    what = "w4-16x8x16-G2 T rocfft " + precision
    own = run_ranks(fp, monkeypatch, geo, precision, "T", species, step=False)[0]
    frames = run_ranks(fp, monkeypatch, geo, precision, "T", species, path="rocfft")
    for tag, views in zip(("precalc", "step"), frames):
        fixed, want, top = check_frame(views, geo, "T", precision, N_CLOUD, "dec A T rocfft " + precision, what + " " + tag)
    a, b = own_phi(own, geo), own_phi(frames[0], geo)
    top = float(np.abs(a).max())
    ratio = float(np.abs(a.astype(np.float64) - b).max()) / top
    note("dec A T own-rocfft " + precision, ratio)
    assert ratio <= TOL[precision], "%s: max |phi(own) - phi(rocFFT)| / max |phi| = %.3g" % (what, ratio)
    assert not same_bits(a, b), what + ": FPIC_POISSON_FFT=rocfft gave the own passes' phi bit for bit"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", ["T", "I"])
@pytest.mark.parametrize("switch", ["FPIC_DOMAIN_OVERLAP", "FPIC_DOMAIN_COMPACT"])
def test_switches_change_no_bit(fp, monkeypatch, switch, mode, precision):
    """A: FPIC_DOMAIN_OVERLAP=0 takes the non-split gradient (one launch over the slab and its ghost planes instead of
    three), FPIC_DOMAIN_COMPACT=0 keeps whole-grid arrays where the default keeps nzs = 13 of 16 planes: every check
    again, and phi and E on every plane a rank holds have the default's bits, after precalc() and after a step()"""
    geo = dr.Slabs((16, 8, 16), L3, 4, 2)
    species = cloud(geo)
    what = "w4-16x8x16-G2 %s %s %s=0" % (mode, precision, switch)
    default = run_ranks(fp, monkeypatch, geo, precision, mode, species)
    frames = run_ranks(fp, monkeypatch, geo, precision, mode, species, env={switch: "0"})
    for tag, views, ref in zip(("precalc", "step"), frames, default):
        check_frame(views, geo, mode, precision, N_CLOUD, "dec A %s %s" % (mode, precision), what + " " + tag)
        check_same_bits_as(views, ref, geo, what + " " + tag)


# ------------------------------------------------------------------------------------ B: closed forms, charges on nodes

B_GRIDS = [(4, (16, 8, 16), 2), (8, (16, 8, 32), 1)]
B_SOURCES = [("qc", "one"), ("nyq", "one"), ("one", "nyq"), ("qs", "qc"), "sheet"]
B_PLANES = ["seam", "first", "last", "interior", "top"]


def charged_plane(geo, where):
    """0 (the seam of the periodic box), the first plane of rank 1, the last plane of rank 1, a plane inside rank 2, nz - 1"""
    return {"seam": 0, "first": geo.nzl, "last": 2 * geo.nzl - 1, "interior": 2 * geo.nzl + geo.nzl // 2, "top": geo.nz - 1}[where]


def plane_species(geo, k0, source):
    """one particle per charged node of plane k0, ON the node: electrons on the nodes of value +1 and (the patterns) a
    positive species on those of value -1; returns (species, the pattern [nz][ny][nx], the closed form's phi for unit rho)"""
    pat = np.ones((geo.ny, geo.nx)) if source == "sheet" else dr.plane_pattern(geo.shape, *source)
    at = lambda ji: np.stack([ji[:, 1] * geo.d[0], ji[:, 0] * geo.d[1], np.full(len(ji), k0 * geo.d[2])], axis=1)
    plus, minus = at(np.argwhere(pat > 0)), at(np.argwhere(pat < 0))
    species = [(ME, QE, plus, np.zeros_like(plus))]
    if len(minus):
        species.append((MP, -QE, minus, np.zeros_like(minus)))
    pattern = np.zeros(geo.grid)
    pattern[k0] = pat
    return species, pattern


def closed_form(geo, k0, source, rho0):
    return dr.sheet_source(geo.shape, geo.L, k0, rho0)[1] if source == "sheet" else dr.plane_source(geo.shape, geo.L, k0, source[0], source[1], rho0)[1]


def check_exact(views, geo, want, precision, family, what):
    """phi against a closed form within EIGEN_TOL on every rank's planes, E against the closed form's central differences
    within 2 tol + 4 eps (phi within tol at both neighbours, the difference and the product rounded in T)"""
    tol, eps = EIGEN_TOL[precision], EPS[precision]
    top = check_phi_sets(views, geo, want, tol, family, what)
    ratio = measure_exact_e(views, geo, want, top)
    note(family + " E", ratio)
    assert ratio <= 2 * tol + 4 * eps, "%s: E off the closed form's by %.3g of max |phi| / (2 d) (bound %.3g)" % (what, ratio, 2 * tol + 4 * eps)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("where", B_PLANES)
@pytest.mark.parametrize("source", B_SOURCES, ids=lambda s: s if isinstance(s, str) else "-".join(s))
@pytest.mark.parametrize("grid", B_GRIDS, ids=lambda g: "w%d-%s-G%d" % (g[0], grid_id(g[1]), g[2]))
def test_closed_forms_on_ranks(fp, monkeypatch, grid, source, where, precision):
    """B: one charged plane — a single (kx, ky) mode with every kz, so every rank frequency of the interface system; the
    sheet is the (0, 0) line alone (mode I: tri_zero_line_kernel on a right-hand side that is one spike).  T and I against
    the closed form within EIGEN_TOL, then every check of check_frame, and after a step() those against numpy"""
    world, shape, G = grid
    geo = dr.Slabs(shape, L3, world, G)
    k0 = charged_plane(geo, where)
    species, pattern = plane_species(geo, k0, source)
    count = len(species[0][2]) - (len(species[1][2]) if len(species) > 1 else 0)
    want = closed_form(geo, k0, source, QE * 1e9 / float(np.prod(geo.d)))
    for mode in "TI":
        what = "w%d %s %s plane %d %s %s" % (world, grid_id(shape), source, k0, mode, precision)
        family = "dec B %s %s %s" % ("sheet" if source == "sheet" else "plane", mode, precision)
        frames = run_ranks(fp, monkeypatch, geo, precision, mode, species)
        check_frame(frames[0], geo, mode, precision, count, family + " numpy", what, pattern=pattern)
        check_exact(frames[0], geo, want, precision, family, what)
        check_frame(frames[1], geo, mode, precision, count, family + " numpy", what + " step")


# ------------------------------------------------------------------------------------ C: exact eigenmodes through the ranks

C_PATTERNS = [p for p in PATTERNS if p[2] != "one"] + [("qc", "one", "one")]     # (the last: constant along z, rank frequency 0 alone: det0)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("pattern", C_PATTERNS, ids="-".join)
def test_exact_eigenmodes_on_ranks(fp, monkeypatch, pattern, precision):
    """C: rho one eigenvector of the 3-point Laplacian (charges on nodes, as family D of the one-handle module), four
    ranks: phi = rho / (eps0 K^2) within EIGEN_TOL on every plane a rank holds"""
    geo = dr.Slabs((16, 8, 16), L3, 4, 2)
    ideal, K2, plus, minus = node_mode(geo.shape, L3, pattern)
    assert len(plus) == len(minus) > 0
    species = [(ME, QE, plus, np.zeros_like(plus)), (MP, -QE, minus, np.zeros_like(minus))]
    want = ideal * (QE * 1e9 / float(np.prod(geo.d))) / (dr.EPS0 * K2)
    for mode in "TI":
        what = "eigenmode %s %s %s" % ("/".join(pattern), mode, precision)
        family = "dec C %s %s" % (mode, precision)
        frames = run_ranks(fp, monkeypatch, geo, precision, mode, species)
        check_frame(frames[0], geo, mode, precision, 0, family + " numpy", what, pattern=ideal)
        check_exact(frames[0], geo, want, precision, family, what)
        check_frame(frames[1], geo, mode, precision, 0, family + " numpy", what + " step")


# ------------------------------------------------------------------------------------ D: the full-EM start on ranks

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("world,shape,G", [(4, (16, 8, 32), 2), (2, (16, 16, 64), 2)], ids=["w4-16x8x32-G2", "w2-16x16x64-G2"])
def test_full_em_start_on_ranks(fp, monkeypatch, world, shape, G, precision):
    """D: solver 'yee' ranks solve once, decomposed, for the initial field (nzl = 8 = 2 (G + 2) is the thinnest slab
    domain_init allows).  After precalc(): phi on the slab and the H / H + 1 received planes within TOL of numpy and a copy
    of the owner's; F3_EDGE_E on the slab and its H halo planes is the forward difference of the rank's OWN phi, bit for
    bit (check_edge_field of the one-handle module on those planes); own planes have one handle's F3_EDGE_E, bit for bit"""
    geo = dr.Slabs(shape, L3, world, G)
    pos = lumpy_cloud(shape, N_CLOUD, L3)
    species = [(ME, QE, pos, np.zeros_like(pos))]
    dt = cfl_dt(shape)
    one = one_handle(fp, monkeypatch, geo, precision, species, solver="yee", dt=dt, em=True)
    for mode in "TI":
        what = "w%d %s yee %s %s" % (world, grid_id(shape), mode, precision)
        views = run_ranks(fp, monkeypatch, geo, precision, mode, species, solver="yee", dt=dt, step=False)[0]
        fixed = dr.assemble([v["fixed"] for v in views], geo.nzl)
        assert int(fixed.sum()) == N_CLOUD * FIXED_ONE and np.array_equal(fixed, one["fixed"]), what
        want = dr.reference_phi(fixed, QE, 1e9, shape, L3)
        check_phi_sets(views, geo, want, phi_bound(geo, mode, precision), "dec D %s %s" % (mode, precision), what, em=True)
        for r, v in enumerate(views):
            for p in geo.received(r, em=True):
                assert same_bits(v["phi"][p], views[geo.owner(p)]["phi"][p]), "%s: rank %d's phi on plane %d is not rank %d's" % (what, r, p, geo.owner(p))
            T = v["phi"].dtype.type
            planes = geo.em_edge(r)
            for comp, axis, n, length in axes_of(v["phi"], L3):
                forward = ((v["phi"] - np.roll(v["phi"], -1, axis=axis)) * T(1.0 / (length / n)))[planes]
                assert same_bits(v["edge"][planes][..., comp], forward), "%s: rank %d: edge E%s is not the forward difference of its phi" % (what, r, "xyz"[comp])
            assert not v["edge"][planes][..., 3].any(), what
            if mode == "T":
                assert same_bits(v["edge"][geo.own(r)], one["edge"][geo.own(r)]), "%s: rank %d's edge E on its slab is not one handle's" % (what, r)
        if mode == "I":
            # another algorithm: both potentials are within their bounds of numpy's at either end of an edge, and the
            # difference and the product are rounded in T
            top = float(np.abs(want).max())
            for comp in range(3):
                worst = max(float(np.abs(v["edge"][geo.own(r)][..., comp].astype(np.float64) - one["edge"][geo.own(r)][..., comp]).max()) for r, v in enumerate(views))
                ratio = worst * geo.d[comp] / top
                note("dec D I-one edge E " + precision, ratio)
                bound = 2 * (phi_bound(geo, "I", precision) + TOL[precision]) + 4 * EPS[precision]
                assert ratio <= bound, "%s: edge E%s differs from one handle's by %.3g of max |phi| / d (bound %.3g)" % (what, "xyz"[comp], ratio, bound)
