"""tests/deposit_reference.py proved on the CPU: closed forms, the reference run over the CPU oracle on the scenes the device
is held to (tests/test_gpu_deposit_reference.py) within the bounds derived in the reference's docstring, and seven wrong
variants of the REFERENCE, each missing the check meant to catch it by at least 100 bounds.  Every figure is printed before
it is asserted (pytest -s)."""
import numpy as np
import pytest

import deposit_reference as dr
import deposit_scenes as ds

W = dr.W
STAMP = dr.load_stamp()
WORST = {}     # (stage, precision) -> largest error over bound met so far in this run


def note(fig, precision):
    for k, v in fig.items():
        WORST[(k, precision)] = max(WORST.get((k, precision), 0.0), float(v))
    print("    " + precision + "  " + "  ".join("%s %.3g" % kv for kv in sorted(fig.items())))


@pytest.fixture(scope="module")
def po():
    import pic_oracle
    return pic_oracle


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_one_particle_is_its_colour_times_the_stamp(precision):
    """one particle at angle theta with v = v_r e_r + v_theta e_theta: the sums hold 0.001 (v_r, v_theta, v_z, 1) in its cell
    and the moments are that times the stamp around the cell, cropped (the cell is 3 columns from the axis)"""
    T = dr.real(precision)
    nr, nz, th, r, z = 24, 16, 0.7, 3.4 / 24, 9.25 / 16
    vr, vt, vz = 3e-4, -2e-4, 5e-4
    pos = np.array([[r * np.cos(th), r * np.sin(th), z]]).astype(T)
    vel = np.array([[vr * np.cos(th) - vt * np.sin(th), vr * np.sin(th) + vt * np.cos(th), vz]]).astype(T)
    ref = dr.cell_sums(pos, vel, nr, nz, T)
    assert ref["count"].sum() == 1 and ref["count"][9 + 5, 3 + 5] == 1
    c = ref["colour"][9 + 5, 3 + 5].astype(np.float64)
    np.testing.assert_allclose(c, float(T(0.001)) * np.array([vr, vt, vz]), rtol=8 * dr.eps(T))
    sums = np.concatenate([ref["colour"], (ref["count"] * dr.milli(T))[..., None]], axis=2)
    m, _ = dr.stamp_moments(sums, nr, nz, STAMP)
    colour = np.append(ref["colour"][9 + 5, 3 + 5], dr.milli(T))
    want = np.zeros((nz, nr, 4), dtype=W)
    for dj in range(-5, 6):
        for di in range(-5, 6):
            if 0 <= 3 + di < nr and 0 <= 9 + dj < nz:
                want[9 + dj, 3 + di] = W(STAMP[5 - dj, di + 5]) * colour
    assert np.array_equal(m, want)
    assert (m[..., 3] > 0).sum() == (STAMP[:, 2:] > 0).sum() < (STAMP > 0).sum()    # columns -2 and -1 are cropped
    n = dr.normalise(m, nr, nz)
    i = 5
    np.testing.assert_allclose(float(n[9, i, 0]), 1000 * vr * 0.5 / ((i + 0.5) / nr), rtol=16 * dr.eps(T))
    np.testing.assert_allclose(float(n[9, 3, 3]), float(T(0.001)) * STAMP[5, 5] * 1000 * 0.5 / (3.5 / nr), rtol=1e-15)


def test_the_stamp_as_the_fixture_holds_it():
    assert STAMP[0, 0] == 0 and STAMP[5, 5] == STAMP.max() and np.array_equal(STAMP, STAMP[::-1, ::-1]) and np.array_equal(STAMP, STAMP.T)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_count_channel_sums_to_the_stamp_weight_inside_the_grid(precision):
    T = dr.real(precision)
    nr, nz = 31, 65
    spec, inp, _, _ = ds.edges(nr, nz, 4097, T)
    pos, vel = inp["position"].astype(T), inp["velocity"].astype(T)
    assert np.array_equal(pos, inp["position"], equal_nan=True)      # the scene's coordinates are values of T
    ref = dr.cell_sums(pos, vel, nr, nz, T)
    m, _ = dr.stamp_moments((ref["count"] * dr.milli(T))[..., None], nr, nz, STAMP)
    ic, jc, vis = dr.ideal_cells(pos, nr, nz, T)
    inside = W(0)
    for i, j in zip(ic[vis], jc[vis]):      # per particle: the part of its stamp that lies on the grid
        inside += STAMP[max(0, 5 + j - (nz - 1)):min(11, 5 + j + 1), max(0, 5 - i):min(11, nr + 5 - i)].astype(W).sum()
    assert vis.sum() == 4097 - 3 and abs(m.sum() - dr.milli(T) * inside) <= 1e-15 * float(m.sum())


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_cic_count_channel(precision):
    """particles at least half a cell inside: all four corners on the grid, the count channel sums to 0.001 n; a particle
    a quarter of a cell from the outer wall keeps 3/4 of its weight, one in the corner 9/16"""
    T = dr.real(precision)
    nr, nz, n = 70, 45, 500
    rng = np.random.default_rng(5)
    r = 0.5 / nr + rng.random(n) * (1 - 1.0 / nr)
    z = 0.5 / nz + rng.random(n) * (1 - 1.0 / nz)
    th = 2 * np.pi * rng.random(n)
    pos = np.stack([r * np.cos(th), r * np.sin(th), z], axis=1).astype(T)
    pos = pos[(dr.radius(pos, T) > 0.5 / nr + 1e-6) & (dr.radius(pos, T) < 1 - 0.5 / nr - 1e-6)]
    vel = rng.normal(0, 1e-3, size=pos.shape).astype(T)
    ref = dr.cic_sums(pos, vel, nr, nz, T)
    assert abs(ref["sums"][..., 3].sum() - dr.milli(T) * len(pos)) <= 1e-15 * len(pos)
    pos = np.array([[1 - 0.25 / nr, 0, 0.5], [1 - 0.25 / nr, 0, 1 - 0.25 / nz]]).astype(T)
    ref = dr.cic_sums(pos, np.zeros_like(pos), nr, nz, T)
    got = float(ref["sums"][..., 3].sum() / dr.milli(T))
    assert abs(got - (0.75 + 0.5625)) < 100 * dr.eps(T)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_hand_placed_edge_particles(precision):
    T = dr.real(precision)
    nr, nz = 64, 64
    pos, vel, names = ds.hand_placed(nr, nz, T)
    ic, jc, vis = dr.ideal_cells(pos, nr, nz, T)
    at = {n: (int(i), int(j), bool(v)) for n, i, j, v in zip(names, ic, jc, vis)}
    assert at["r = 1"] == (nr, 16, True)
    assert at["z = 1"] == (32, nz, True)
    assert at["r = 1 and z = 1"] == (nr, nz, True)
    assert at["r = 0"] == (0, 32, True)
    assert at["z = 0"] == (32, 0, True)
    assert at["r = k / nr"] == (32, 48, True)          # exactly on the edge between columns 31 and 32: the upper one
    assert at["just inside r = 1"] == (nr - 1, 32, True)
    assert not at["r > 1"][2] and not at["z < 0"][2] and not at["NaN"][2]
    ref = dr.cell_sums(pos, vel, nr, nz, T)
    assert ref["count"].sum() == 7 and ref["nan"].sum() == 1 and ref["nan"][32 + 5, 0 + 5]
    cell = ref["colour"][32 + 5, 5]
    assert np.isnan(cell[0]) and np.isnan(cell[1]) and cell[2] == dr.milli(T) * W(T(vel[0, 2]))
    sums = np.concatenate([ref["colour"], (ref["count"] * dr.milli(T))[..., None]], axis=2)
    m, _ = dr.stamp_moments(sums, nr, nz, STAMP)
    nan = np.isnan(m[..., 0])
    want = np.zeros((nz, nr), dtype=bool)
    want[27:38, 0:6] = True                              # the whole cropped footprint, zero-weight corners included
    assert np.array_equal(nan, want) and np.array_equal(np.isnan(m[..., 1]), want) and not np.isnan(m[..., 2:]).any()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_rasterised_cells_at_chosen_offsets(precision):
    """pixel centres keep their cell for every b; a point exactly on the edge between two pixels: its sprite's left edge lies
    on a pixel centre, which is inclusive, so the sprite starts one column lower than the ideal cell (and, y running
    downwards, on the same row); r = 0 has column -1"""
    T = dr.real(precision)
    nr, nz = 16, 8
    for bits in (1, 4, 8):
        pos = np.array([[(7 + 0.5) / nr, 0, (3 + 0.5) / nz], [7.0 / nr, 0, 3.0 / nz], [0, 0, 0.5 / nz], [1.0, 0, 1.0]]).astype(T)
        ic, jc, vis = dr.raster_cells(pos, nr, nz, bits, T)
        assert vis.all()
        assert (ic[0], jc[0]) == (7, 3)
        assert (ic[1], jc[1]) == (6, 3)
        assert (ic[2], jc[2]) == (-1, 0)
        assert (ic[3], jc[3]) == (nr - 1, nz)
        # a pixel is covered when its centre lies in the square: a centre up to 5 pixels outside still reaches the grid
        far = np.array([[1 + 4.7 / nr, 0, 0.5], [1 + 5.3 / nr, 0, 0.5], [0.5, 0, -5.3 / nz], [0.5, 0, 1 + 4.7 / nz], [0.5, 0, 1 + 5.3 / nz]]).astype(T)
        ic, jc, vis = dr.raster_cells(far, nr, nz, bits, T)
        assert list(vis) == [True, False, False, True, False] and ic[0] == nr + 4 and jc[3] == nz + 4


# ------------------------------------------------------------------ the reference over the CPU oracle
def oracle_frame(ora, T, precision, prev_avg, bits=0, cic=False):
    """every stage of one density() of the oracle against the reference: cells, moments, norm, avg"""
    nr, nz = ora.nr, ora.nz
    pos, vel = ora.positions().copy(), ora.velocities().copy()
    e = W(dr.eps(T))
    got = ora.moments.astype(np.float64).reshape(nz, nr, 4)
    if cic:
        fig = dr.measure_cic(got, dr.cic_sums(pos, vel, nr, nz, T), T)
    else:
        ic, jc, vis = dr.sprite_cells(pos, nr, nz, T, bits)
        if bits:
            oi, oj = ora.raster_cells()
            finite = oi != np.iinfo(np.int32).min
            assert not (vis & ~finite).any()
            assert np.array_equal(oi[vis], ic[vis]) and np.array_equal(oj[vis], jc[vis])
            out = finite & ~vis      # dropped by the reference: nothing of the sprite reaches the grid
            assert ((oi[out] + 5 < 0) | (oi[out] - 5 >= nr) | (oj[out] + 5 < 0) | (oj[out] - 5 >= nz)).all()
        else:
            assert np.array_equal(ora.deposit_cells(), np.where(vis, ic + (nr + 1) * jc, -1))
        ref = dr.cell_sums(pos, vel, nr, nz, T, bits)
        dr.assert_cell_population(ref["count"])
        cnt = (ref["count"].astype(W) * dr.milli(T))[..., None]
        want, _ = dr.stamp_moments(np.concatenate([ref["colour"], cnt], axis=2), nr, nz, STAMP)
        mag, _ = dr.stamp_moments(np.concatenate([ref["mag"], cnt], axis=2), nr, nz, STAMP)
        nf, _ = dr.stamp_moments(ref["count"].astype(W)[..., None], nr, nz, np.ones((11, 11)))
        bound = (np.asarray(dr.K_COLOUR, dtype=W) + 2 + nf) * e * mag + 123 * W(np.finfo(T).tiny)
        fig = dict(moments=dr.over_bound(got, want, bound), touched_wrong=int(((got[..., 3] > 0) != (want[..., 3] > 0)).sum()))
    fig.update(dr.measure_finish(ora.norm, ora.avg_A, ora.moments, prev_avg, nr, nz, T))
    note(fig, precision)
    dr.assert_figures(fig)


def run_oracle(po, scene, precision, frames, steps_per_frame=1, bits=0, cic=False, count=None):
    T = dr.real(precision)
    spec, inputs, entropy, rand = scene
    ora = po.OracleSim(spec, dtype=T, count=count, raster_bits=bits, shape="cic" if cic else "ref11")
    ora.set(**inputs)
    ora.set_random_state(entropy, rand)
    ora.precalc()
    for frame in range(frames + 1):
        if frame:
            ora.step(steps_per_frame)
        prev = ora.avg_A.copy()
        ora.density()
        oracle_frame(ora, T, precision, prev, bits, cic)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_oracle_routes_scene(po, precision):
    run_oracle(po, ds.routes(160, 0.02), precision, frames=6)


def test_oracle_several_items_per_tile_scene(po):
    run_oracle(po, ds.routes(400, 0.025), "fp32", frames=2, steps_per_frame=3)


def test_oracle_spill_scene(po):
    run_oracle(po, ds.spill(), "fp32", frames=1, steps_per_frame=20)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", ds.EDGE_GRIDS, ids=lambda g: "%dx%d" % g)
def test_oracle_edges(po, grid, precision):
    for count in ds.EDGE_COUNTS:
        run_oracle(po, ds.edges(grid[0], grid[1], count, dr.real(precision)), precision, frames=1, count=count)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("bits", [1, 4, 8])
def test_oracle_rasterised(po, bits, precision):
    scene = ds.raster(dr.real(precision))
    run_oracle(po, scene, precision, frames=1, bits=bits, count=len(scene[1]["position"]))


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_oracle_cic(po, precision):
    run_oracle(po, ds.cic(), precision, frames=5, cic=True)


def test_print_the_oracle_columns():
    """(runs last in this module: the table of DESIGN section 2)"""
    for stage in sorted({k for k, _ in WORST}):
        print("    %-18s fp32 %-10.3g fp64 %.3g" % (stage, WORST.get((stage, "fp32"), float("nan")), WORST.get((stage, "fp64"), float("nan"))))


# ------------------------------------------------------------------ wrong variants of the reference
@pytest.fixture(scope="module")
def variant_scene():
    T = np.float32
    nr, nz = 31, 65
    _, inp, _, _ = ds.edges(nr, nz, 4097, T)
    pos, vel = inp["position"].astype(T), inp["velocity"].astype(T)
    ref = dr.cell_sums(pos, vel, nr, nz, T)
    sums = dr.as_readback(ref, T)
    moments, _ = dr.stamp_moments(sums, nr, nz, STAMP)
    moments = moments.astype(T).astype(np.float64)
    norm = dr.normalise(moments, nr, nz).astype(T).astype(np.float64)
    prev = np.abs(np.random.default_rng(2).normal(0, 1, size=norm.shape)).astype(T).astype(np.float64)
    prev[np.isnan(norm)] = np.nan
    return dict(T=T, nr=nr, nz=nz, pos=pos, vel=vel, ref=ref, sums=sums, moments=moments, norm=norm, prev=prev)


def test_the_right_reference_passes_its_own_checks(variant_scene):
    s = variant_scene
    T, nr, nz = s["T"], s["nr"], s["nz"]
    fig = dr.measure_sums(s["sums"], s["ref"], T)
    fig.update(dr.measure_moments(s["moments"], s["sums"], nr, nz, STAMP, T))
    avg, _ = dr.average(s["norm"], s["prev"], T)
    fig.update(dr.measure_finish(s["norm"], avg.astype(T), s["moments"], s["prev"], nr, nz, T))
    cic = dr.cic_sums(s["pos"], s["vel"], nr, nz, T)
    fig.update(dr.measure_cic(cic["sums"].astype(T).astype(np.float64), cic, T))
    print("   ", fig)
    dr.assert_figures(fig)


@pytest.mark.parametrize("variant", ["flip_theta", "round", "clip_r1", "stamp_shift", "norm_without_half_over_x", "ratio_swapped", "cic_exchange"])
def test_wrong_variant_misses_by_100_bounds(variant_scene, variant):
    s = variant_scene
    T, nr, nz = s["T"], s["nr"], s["nz"]
    if variant in ("flip_theta", "round", "clip_r1"):
        wrong = dr.as_readback(dr.cell_sums(s["pos"], s["vel"], nr, nz, T, variant=variant), T)
        fig = dr.measure_sums(wrong, s["ref"], T)
        miss = fig["colour"]
        if variant != "flip_theta":          # the exact check misses too: whole particles in the wrong cell
            assert fig["count_cells_wrong"] >= (2 if variant == "clip_r1" else 100), fig
    elif variant == "stamp_shift":
        wrong, _ = dr.stamp_moments(s["sums"], nr, nz, STAMP, shift=(1, 0))
        fig = dr.measure_moments(wrong.astype(T), s["sums"], nr, nz, STAMP, T)
        miss = fig["moments"]
    elif variant == "norm_without_half_over_x":
        wrong = dr.normalise(s["moments"], nr, nz, half_over_x=False).astype(T)
        avg, _ = dr.average(wrong, s["prev"], T)
        fig = dr.measure_finish(wrong, avg.astype(T), s["moments"], s["prev"], nr, nz, T)
        miss = fig["norm"]
        assert fig["avg"] <= 1
    elif variant == "ratio_swapped":
        avg, _ = dr.average(s["norm"], s["prev"], T, swapped=True)
        fig = dr.measure_finish(s["norm"], avg.astype(T), s["moments"], s["prev"], nr, nz, T)
        miss = fig["avg"]
        assert fig["norm"] <= 1
    else:
        right = dr.cic_sums(s["pos"], s["vel"], nr, nz, T)
        wrong = dr.cic_sums(s["pos"], s["vel"], nr, nz, T, variant="exchange")
        fig = dr.measure_cic(wrong["sums"].astype(T).astype(np.float64), right, T)
        miss = fig["cic"]
    print("    %s misses by %.3g bounds  %s" % (variant, miss, fig))
    assert miss >= 100
