"""The float64 / exact reference of the CART3D pushes (tests/em_reference.py) proven before it judges a kernel:
(a) against closed forms, (b) against the CPU oracle on the scenes and within the bounds of tests/test_gpu_em_reference.py
(the evidence that those bounds leave room for correct code), (c) sensitivity controls: deliberately wrong variants of the
REFERENCE must miss the unmodified one by at least 100 x the bound of the check that is meant to catch them."""
import numpy as np
import pytest

import em_reference as ref
import em_scenes as sc

PRECISIONS = [np.float32, np.float64]


@pytest.fixture(scope="module")
def eo():
    import es3d_oracle
    return es3d_oracle


# ---------------------------------------------------------------------------------------------- (a) closed forms
def test_boris_map_is_drift_plus_rotation():
    """uniform E perpendicular to B: v_N = v_d + R^N (v_0 - v_d), v_d = E x B / (B^2 c), R about B by -2 atan(h |B|);
    40 applications of boris() in float64 against the closed form, both signs of the charge"""
    scene = sc.drift_scene("yee")
    v0 = scene.species[0][4]
    for sign in (1, -1):
        scene.species[0] = (sc.ME, sign * sc.QE) + scene.species[0][2:]
        v = v0.copy()
        for _ in range(40):
            v, _ = ref.boris(v, scene.Eu[None, :], scene.Bu[None, :] * np.ones((len(v), 1)), scene.h(0), sc.C)
        want, vd = sc.drift_closed_form(scene, v0, 40)
        assert abs(np.linalg.norm(vd) - 0.05) < 1e-12
        assert np.abs(v - want).max() < 40 * 8 * 2.3e-16
        handle_wide, _ = ref.boris(v0, scene.Eu, scene.Bu, scene.h(0), sc.C)          # one t for everybody: the same map
        per_particle, _ = ref.boris(v0, scene.Eu, scene.Bu[None, :] * np.ones((len(v0), 1)), scene.h(0), sc.C)
        assert np.array_equal(handle_wide, per_particle)


def test_centring_and_gather_reproduce_an_affine_field():
    """affine E and B sampled where the Yee lattice holds each component: node_fields + gather give the analytic field at
    the quantised position, away from the seam, to float64 rounding"""
    scene = sc.affine_scene()
    En, Bn, Ea, Ba = ref.node_fields(scene.E, scene.B)
    u = (scene.species[0][3] / scene.L).astype(np.float32)
    i, w1 = ref.cells_and_weights(u, scene.shape, np.float32)
    assert i.min() >= 2 and (i.max(axis=0) <= np.array(scene.shape) - 3).all() and w1.min() >= 0 and w1.max() <= 1 << 14
    E_want, B_want = scene.analytic(i + w1 / 16384.0)
    E_got, E_abs = ref.gather(En, i, w1)
    B_got, B_abs = ref.gather(Bn, i, w1)
    assert np.abs(E_got - E_want).max() <= 16 * 2.3e-16 * E_abs.max()
    assert np.abs(B_got - B_want).max() <= 16 * 2.3e-16 * B_abs.max()
    assert (E_abs >= np.abs(E_got) * (1 - 1e-15)).all() and (Ea >= np.abs(En)).all() and (Ba >= np.abs(Bn)).all()


def test_cells_and_weights_edges():
    """the discrete part at its edges: a node, the last representable coordinate below 1 (u n rounds up to n: cell 0), the
    weight's round-half-up, both precisions"""
    for T in PRECISIONS:
        below_one = np.nextafter(T(1), T(0))
        u = np.array([0.0, 0.25, below_one, 0.5 + 2.0 ** -18, 0.5 + 2.0 ** -17], dtype=T)
        i, w1 = ref.cells_and_weights(u, 4, T)
        g = float(below_one) * 4
        want_last = (0, 0) if T(below_one * T(4)) == T(4) else (3, ((int((g - 3) * 32768) + 1) >> 1))
        assert (i[0], w1[0]) == (0, 0) and (i[1], w1[1]) == (1, 0) and (i[2], w1[2]) == want_last
        assert (i[3], w1[3]) == (2, 0) and (i[4], w1[4]) == (2, 1)          # f 2^15 = 0.5 -> 0; f 2^15 = 1 -> 1
        assert ref.fixed_coordinate(u, 4, T)[4] == 2 * (2 * 16384 + 1)


def random_moves(rng, shape, n, reach):
    a = rng.integers(0, np.array(shape) * ref.S // 2, (n, 3)) * 2
    b = (a + rng.integers(-reach, reach + 1, (n, 3)) * 2) % (np.array(shape) * ref.S)
    return a, b


@pytest.mark.parametrize("shape,reach", [((5, 4, 6), ref.S // 2 - 1), ((3, 5, 4), int(0.7 * ref.S)), ((7, 5, 6), int(1.2 * ref.S))])
def test_exact_current_int64_form_equals_the_fractions_and_the_first_moment(shape, reach):
    """300 random moves of up to 1, 1.4 and 2.4 cells per axis (always below half the box): the int64 form with the
    integral multiplied out equals Simpson's rule in fractions.Fraction edge for edge, no edge value is fractional, the four
    edges of a direction sum to 12 2^30 Z (b - a), and with the CIC charge of the same quantised positions
    96 (rho_new - rho_old) + div J = 0 at every node -- also for the moves that skip a cell, which is what the whole-cell
    steps of pieces() are for: cut once, such a move breaks continuity at its relay point."""
    rng = np.random.default_rng(sum(shape))
    a, b = random_moves(rng, shape, 300, reach)
    skip = (np.abs(ref.nearest_image(a, b, shape) // ref.S - a // ref.S) >= 2).any(axis=1)
    assert skip.any() == (reach > ref.S // 2)
    for Z in (1, -2):
        J = ref.current_exact(a, b, shape, Z)
        assert np.array_equal(J, ref.current_exact_fractions(a, b, shape, Z))
        assert np.array_equal(J.sum(axis=0), ref.first_moment(a, b, shape, Z))
        assert not ref.continuity_residual(J, a, b, shape, Z).any()
    if skip.any():
        cut_once = np.zeros_like(J)
        nb = ref.nearest_image(a, b, shape)
        r = ref.relay_point(a, nb)
        ref._segment(a, r, a // ref.S, shape, 1, cut_once, "simpson")
        ref._segment(r, nb, nb // ref.S, shape, 1, cut_once, "simpson")
        assert ref.continuity_residual(cut_once, a, b, shape, 1).any()
    one_cell = ref.current_exact(np.array([[2, 4, 6]]), np.array([[2 + ref.S, 4, 6]]), shape, 1)
    assert one_cell[:, 0].sum() == ref.J_UNIT and not one_cell[:, 1:].any()


def test_vacuum_wave_follows_the_yee_dispersion():
    """one transverse mode on a non-cubic lattice, 12 sub-steps of yee_substep with J = 0: E = E0 cos(omega t) with
    sin(omega dt / 2) = c dt sqrt(sum (sin(k d / 2) / d)^2), to float64 rounding"""
    shape, d, mode = (8, 6, 10), sc.STAGE_CELL, (1, 2, 3)
    L = [shape[a] * d[a] for a in range(3)]
    dt = sc.cfl_dt(shape, L, 0.9)
    idx = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    kk = [2 * np.pi * mode[a] / L[a] for a in range(3)]
    K = np.array([2 / d[a] * np.sin(kk[a] * d[a] / 2) for a in range(3)])
    e0 = np.cross(K, [0.3, -0.5, 0.8]); e0 = e0 / np.linalg.norm(e0) * 1e3
    E0 = np.stack([e0[a] * np.cos(sum(kk[b] * d[b] * (idx[b] + (0.5 if b == a else 0.0)) for b in range(3))) for a in range(3)], axis=-1)
    omega = 2 / dt * np.arcsin(sc.C * dt * np.sqrt(sum((np.sin(kk[a] * d[a] / 2) / d[a]) ** 2 for a in range(3))))
    E, B = E0, np.zeros_like(E0)
    J = np.zeros((int(np.prod(shape)), 3), dtype=np.int64)
    for n in range(1, 13):
        E, B, Ea, Ba = ref.yee_substep(E, B, J, dt, d, sc.QE)
        assert np.abs(E - E0 * np.cos(n * omega * dt)).max() <= 1e-10 * 1e3, n
    assert (Ea >= np.abs(E)).all() and (Ba >= np.abs(B)).all()


# ---------------------------------------------------------------------------------------------- (b) the CPU oracle
@pytest.fixture(scope="module")
def records(eo):
    """one sub-step of the CPU oracle per (scene, precision), recorded once and shared"""
    cache = {}

    def get(kind, T, arg=None):
        key = (kind, np.dtype(T).name, arg)
        if key not in cache:
            make = lambda spec: sc.OracleBox(eo, spec, T)
            if kind in ("stage", "long"):
                scene = sc.stage_scene(arg) if kind == "stage" else sc.long_scene()
                cache[key] = sc.record_substep(scene.build(make), scene)
            elif kind == "affine":
                scene = sc.affine_scene()
                cache[key] = sc.record_substep(scene.build(make), scene)
            elif kind == "es":
                scene = sc.es_scene(arg)
                sim = scene.build(make)
                sim.substeps(4)
                cache[key] = sc.record_substep(sim, scene, yee=False)
        return cache[key]
    return get


def within(tag, err, bound):
    ratio = sc.report(tag, err, bound)
    assert (err <= bound).all(), (tag, ratio)


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("shape", sc.STAGE_SHAPES)
def test_oracle_stages_within_the_bounds(records, T, shape):
    r = records("stage", T, shape)
    within("S1 node centring", *sc.check_nodes(r))
    for s in (0, 1):
        ve, vb, ue, ub = sc.check_push(r, s)
        within("S2 velocity, species %d" % s, ve, vb)
        within("S2 position, species %d" % s, ue, ub)
    J, moment = sc.reference_current(r)
    assert np.array_equal(r.J, J) and np.array_equal(r.J.sum(axis=0), moment)
    assert not sc.continuity_of(r).any()
    within("S4 lattice", *sc.check_lattice(r))


@pytest.mark.parametrize("T", PRECISIONS)
def test_oracle_current_where_a_coordinate_leaves_32_bits(records, T):
    """the scene of the GPU test of that name: it does cross the planes it is about, and the oracle's push and current
    are the reference's there"""
    r = records("long", T)
    for plane in sc.LONG_BANDS:
        assert sc.crossings(r, plane) >= 20, plane
    for s in (0, 1):
        ve, vb, ue, ub = sc.check_push(r, s)
        within("S2 velocity on 70000 planes, species %d" % s, ve, vb)
        within("S2 position on 70000 planes, species %d" % s, ue, ub)
    J, moment = sc.reference_current(r)
    assert np.array_equal(r.J, J) and np.array_equal(r.J.sum(axis=0), moment)
    assert not sc.continuity_of(r).any()


@pytest.mark.parametrize("T", PRECISIONS)
def test_oracle_gathers_the_fields_from_where_the_lattice_holds_them(records, T):
    within("K1 staggering", *sc.check_affine(records("affine", T)))


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("solver", ["yee", "none"])
def test_oracle_drift_and_gyration(eo, T, solver):
    err, bound, moved = sc.drift_run(lambda spec: sc.OracleBox(eo, spec, T), solver)
    within("K2 drift and gyration, " + solver, err, bound)
    assert moved < 1e-6


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("shape", [(12, 10, 6), (40, 24, 20)])
def test_oracle_electrostatic_push(records, T, shape):
    r = records("es", T, shape)
    for s in (0, 1):
        ve, vb, ue, ub = sc.check_push(r, s, B=r.sc.b0)
        within("K3 velocity, species %d" % s, ve, vb)
        within("K3 position, species %d" % s, ue, ub)


# ---------------------------------------------------------------------------------------------- (c) sensitivity controls
def b_as_if_on_the_edges(E_edge, B_face):
    """WRONG: B centred like E (two samples along the component's own axis)"""
    En, _, Ea, _ = ref.node_fields(E_edge, B_face)
    Bn, _, Ba, _ = ref.node_fields(B_face, B_face)
    return En, Bn, Ea, Ba


def ex_from_the_wrong_side(E_edge, B_face):
    """WRONG: node-centred Ex from the samples i and i+1 instead of i-1 and i"""
    En, Bn, Ea, Ba = ref.node_fields(E_edge, B_face)
    En = En.copy()
    En[..., 0] = 0.5 * (E_edge[..., 0] + np.roll(E_edge[..., 0], -1, axis=0))
    return En, Bn, Ea, Ba


def boris_2t(v, E_p, B_p, h, c, E_abs=None):
    """WRONG: s = 2 t"""
    t = h * np.broadcast_to(np.asarray(B_p, np.float64), v.shape)
    a = (h / c) * E_p
    vm = v + a
    return vm + np.cross(vm + np.cross(vm, t), 2.0 * t) + a, None


def missed_by(tag, wrong, right, bound):
    ratio = float((np.abs(wrong - right) / bound).max())
    print("%-50s misses by %.3g x the bound" % (tag, ratio))
    return ratio


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("variant", [b_as_if_on_the_edges, ex_from_the_wrong_side])
def test_a_wrong_centring_is_seen_by_s1_and_k1(records, T, variant):
    r = records("stage", T, (8, 6, 10))
    right, wrong = ref.node_fields(r.edge_E, r.face_B), variant(r.edge_E, r.face_B)
    bound = 2 * sc.eps_of(T) * np.concatenate([right[2].ravel(), right[3].ravel()])
    got = lambda f: np.concatenate([f[0].ravel(), f[1].ravel()])
    assert missed_by("S1 " + variant.__name__, got(wrong), got(right), bound) >= 100
    r = records("affine", T)
    v_right, bound = sc.affine_reference(r)
    v_wrong, _ = sc.affine_reference(r, node_fields=variant)
    assert missed_by("K1 " + variant.__name__, v_wrong, v_right, bound) >= 100


@pytest.mark.parametrize("T", PRECISIONS)
def test_a_rotation_by_2t_is_seen_by_k2_and_k3(records, T):
    """(the stage scene's |t| is 0.01: K2 at 0.4 and K3 at 0.3 are the checks meant to catch it)"""
    r = records("es", T, (12, 10, 6))
    right = sc.reference_push(r, 0, r.E_nodes, r.sc.b0)
    wrong = sc.reference_push(r, 0, r.E_nodes, r.sc.b0, boris=lambda *a, **k: (boris_2t(*a, **k)[0], ref.boris(*a, **k)[1]))
    assert missed_by("K3 rotation by 2t", wrong[0], right[0], right[1]) >= 100
    scene = sc.drift_scene("yee")
    v0 = scene.species[0][4]
    v = v0.copy()
    for _ in range(40):
        v = boris_2t(v, scene.Eu[None, :], scene.Bu, scene.h(0), sc.C)[0]
    want, vd = sc.drift_closed_form(scene, v0, 40)
    bound = 8 * 40 * sc.eps_of(T) * (np.abs(v0 - vd).max() + np.abs(vd).max())
    assert missed_by("K2 rotation by 2t", v, want, bound) >= 100


@pytest.mark.parametrize("shape", sc.STAGE_SHAPES)
@pytest.mark.parametrize("kw", [dict(relay=ref.relay_midpoint), dict(rule="midpoint")], ids=["relay at the midpoint", "cross term dropped"])
def test_a_wrong_current_is_seen_by_s3(records, shape, kw):
    """S3 is exact (bound 0): the wrong variants differ on most edges, by far more than 100 units; they keep the first
    moment -- and the relay variant the divergence too, which is why the continuity tests cannot see it"""
    r = records("stage", np.float32, shape)
    right, moment = sc.reference_current(r)
    wrong, _ = sc.reference_current(r, **kw)
    differ = np.abs(wrong - right)
    print("edges that differ: %d of %d, largest difference %.3g units of 96 2^42" % ((differ > 0).sum(), differ.size, differ.max() / ref.J_UNIT))
    assert (differ > 100).sum() >= differ.size // 2
    assert np.array_equal(wrong.sum(axis=0), moment)


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("shape", sc.STAGE_SHAPES)
def test_a_flipped_current_is_seen_by_s4(records, T, shape):
    r = records("stage", T, shape)
    sc_ = r.sc
    right = ref.yee_substep(r.edge_E, r.face_B, r.J, sc_.dt, sc_.d, sc_.q0W)
    wrong = ref.yee_substep(r.edge_E, r.face_B, -r.J, sc_.dt, sc_.d, sc_.q0W)
    assert missed_by("S4 J with the sign flipped", wrong[0], right[0], 8 * sc.eps_of(T) * right[2]) >= 100
