"""The CART3D push kernels under a reference that shares no code with them or with the oracle (tests/em_reference.py:
float64 and exact integers, written from the definition and the equations; proven on the CPU by tests/test_em_reference.py,
which also shows that each bound below leaves room for correct code and that a wrong convention misses it by >= 100 x).

Stage-wise checks of ONE substeps(1) through the public API -- every stage takes the device's own read-back state as its
input, so one stage's rounding cannot move another stage's integers -- and known answers on the device.  Scenes, adapters,
checks and the derivation of the bounds: tests/em_scenes.py.  K of the push bound is 32: the longest dependency chain of the
definition has about 24 rounded operations (8 fused adds of the gather, the scaling by h/c, the half kick, t = hB and
1 + t^2, the division and s, two cross products with their additions, the second half kick)."""
import numpy as np
import pytest

import em_scenes as sc

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float32, np.float64]


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


@pytest.fixture(scope="module")
def records(fp):
    """the read-backs around one sub-step on the device per (scene, precision, lattice form), recorded once and shared"""
    cache = {}

    def get(kind, T, arg=None, chain="1"):
        key = (kind, np.dtype(T).name, arg, chain)
        if key not in cache:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("FPIC_EM_CHAIN", chain)
                make = lambda spec: sc.DeviceBox(fp, spec, T)
                scene = {"stage": sc.stage_scene, "long": sc.long_scene, "affine": lambda _: sc.affine_scene(), "es": sc.es_scene}[kind](arg)
                sim = scene.build(make)
                if kind == "es":
                    sim.substeps(4)             # fast particles leave their tile's window before the sub-step under test
                cache[key] = sc.record_substep(sim, scene, yee=kind != "es")
                sim.close()
        return cache[key]
    return get


def within(tag, err, bound):
    ratio = sc.report(tag, err, bound)
    assert (err <= bound).all(), (tag, ratio)


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("shape", sc.STAGE_SHAPES)
def test_s1_node_centring(records, T, shape):
    """F3_E, F3_B_NODES = the mean of the 2 resp. 4 lattice samples around the node, within 2 eps x mean |samples|"""
    within("S1 node centring", *sc.check_nodes(records("stage", T, shape)))


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("shape", sc.STAGE_SHAPES)
def test_s2_push(records, T, shape):
    """new velocities = Boris in the fields gathered at the OLD read-back positions, within 32 eps (|v0|_inf +
    2 |h/c| sum w |E_node|); new positions within eps + (dt c / L) x that, in periodic distance; both species"""
    r = records("stage", T, shape)
    for s in (0, 1):
        ve, vb, ue, ub = sc.check_push(r, s)
        within("S2 velocity, species %d" % s, ve, vb)
        within("S2 position, species %d" % s, ue, ub)


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("shape", sc.STAGE_SHAPES)
def test_s3_current_is_the_exact_line_integral(records, T, shape):
    """F3_J_FIXED = the line integral of the device's own moves, edge for edge and exactly (the particles that move more than
    one cell included, some of which skip a cell); per axis its sum over the nodes is 12 2^30 sum Z (b - a); and with the CIC
    charge of the read-back positions 96 (rho_new - rho_old) + div J = 0 at every node"""
    r = records("stage", T, shape)
    J, moment = sc.reference_current(r)
    moved = max(np.abs(sc.ref.nearest_image(sc.ref.fixed_coordinate(r.old[s][0], shape, T), sc.ref.fixed_coordinate(r.new[s][0], shape, T),
                                            shape) - sc.ref.fixed_coordinate(r.old[s][0], shape, T)).max() for s in (0, 1)) / sc.ref.S
    print("longest move %.2f cells; edges that differ: %d" % (moved, (J != r.J).sum()))
    assert 1.0 < moved < 2.0
    assert np.array_equal(r.J, J)
    assert np.array_equal(r.J.sum(axis=0), moment)
    assert not sc.continuity_of(r).any()


@pytest.mark.parametrize("T", PRECISIONS)
def test_s3_current_where_a_coordinate_leaves_32_bits(records, T):
    """S3 on 4 x 3 x 70000 nodes with the particles about the planes 32768 and 65536, where a doubled fixed-point coordinate
    (2^15 per cell) reaches 2^30 and 2^31, and about the periodic seam; particles cross each of them.  The push (S2) of the
    same sub-step too: the moves are the device's own"""
    r = records("long", T)
    for plane in sc.LONG_BANDS:
        n = sc.crossings(r, plane)
        print("plane %d crossed by %d particles" % (plane, n))
        assert n >= 20
    for s in (0, 1):
        ve, vb, ue, ub = sc.check_push(r, s)
        within("S2 velocity on 70000 planes, species %d" % s, ve, vb)
        within("S2 position on 70000 planes, species %d" % s, ue, ub)
    J, moment = sc.reference_current(r)
    print("edges that differ: %d" % (J != r.J).sum())
    assert np.array_equal(r.J, J)
    assert np.array_equal(r.J.sum(axis=0), moment)
    assert not sc.continuity_of(r).any()


@pytest.mark.parametrize("chain", ["1", "0"], ids=["chained", "four sweeps"])
@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("shape", sc.STAGE_SHAPES)
def test_s4_lattice(records, T, shape, chain):
    """new F3_EDGE_E, F3_FACE_B = the three lattice sweeps applied to the pre-step read-back and the device's own J_fixed,
    within 8 eps x sum |terms|; the default chained lattice step and FPIC_EM_CHAIN=0"""
    within("S4 lattice", *sc.check_lattice(records("stage", T, shape, chain)))


@pytest.mark.parametrize("T", PRECISIONS)
def test_k1_fields_are_gathered_from_where_the_lattice_holds_them(records, T):
    """affine E and B, each component sampled on its own edge / face, |t| about 0.3, particles at rest: the new velocity is
    Boris in the ANALYTIC field at the quantised position, within the S2 bound (half a cell of offset in any component is
    thousands of bounds away)"""
    within("K1 staggering", *sc.check_affine(records("affine", T)))


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("solver", ["yee", "none"])
def test_k2_drift_and_gyration(fp, T, solver):
    """40 sub-steps in uniform E perpendicular to B, |t| = 0.4: v_N = v_d + R^N (v_0 - v_d) within 8 N eps (|v0 - v_d|_inf +
    |v_d|).  'yee': uniform lattice fields, which must not move (macro_weight 1e-30); 'none': set(E) and addB -- the
    electrostatic push kernel and its handle-wide t, s under the same answer"""
    err, bound, moved = sc.drift_run(lambda spec: sc.DeviceBox(fp, spec, T), solver)
    within("K2 drift and gyration, " + solver, err, bound)
    print("lattice moved by %.3g relative" % moved)
    assert moved < 1e-6


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("shape", [(12, 10, 6), (40, 24, 20)])
def test_k3_electrostatic_push(records, T, shape):
    """the S2 check of the electrostatic push (solver 'none') in a random node field and a uniform B of |t| = 0.3, after four
    warm-up sub-steps; (40, 24, 20) is several 16 x 16 x 8 tiles with particles outside their tile's window"""
    r = records("es", T, shape)
    for s in (0, 1):
        ve, vb, ue, ub = sc.check_push(r, s, B=r.sc.b0)
        within("K3 velocity, species %d" % s, ve, vb)
        within("K3 position, species %d" % s, ue, ub)
