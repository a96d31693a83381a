"""The (r,z) deposit on the device against tests/deposit_reference.py, stage by stage, each stage from the device's own
read-back of the stage before: the per-cell sums (FPIC_BUF_CELL_SUMS, the buffer a multi-GPU run all-reduces) against the
particles getParticles() returns — the count exact as integers, the colour sums within the derived bound —, then moments,
norm and the running average from readGrid().  Bounds: the reference's docstring.  Scenes: tests/deposit_scenes.py; they
reach every route of a particle into the sums (fused in-place and re-binning launch, the outbox and its overflow, the
separate kernel, census-only fusion, the spill path, carried particles and tail lanes, the apron, rasterised sprites, 'cic',
fp64).  Every figure (largest error over bound per stage) is printed before it is asserted (pytest -s).

GPU figures of the run that wrote DESIGN section 2's table: see there."""
import os

import numpy as np
import pytest

import deposit_reference as dr
import deposit_scenes as ds

pytestmark = pytest.mark.gpu

STAMP = dr.load_stamp()
WORST = {}


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    return fusionpic


def read_sums(sim, T):
    import torch
    from fusionpic.multi import device_tensor_view
    ptr, nbytes = sim.deviceBuffer()
    view = device_tensor_view(ptr, nbytes, torch.device("cuda", 0), "f4" if T is np.float32 else "f8")
    return dr.split_sums(view.cpu().numpy().copy(), sim.nr, sim.nz)


def check_frame(fp, sim, precision, where, bits=0, cic=False):
    """one deposit() + densityFinish() of `sim`, every stage checked; returns (reference of stage 1, sums read-back)"""
    T = dr.real(precision)
    nr, nz = sim.nr, sim.nz
    prev = sim.readGrid(fp.READ_AVG)
    sim.deposit()
    sim.sync()
    sums = read_sums(sim, T)
    parts = sim.getParticles(rand=False, alive=False)
    if cic:
        ref = dr.cic_sums(parts["position"], parts["velocity"], nr, nz, T)
        grid = sums[dr.APRON:dr.APRON + nz, dr.APRON:dr.APRON + nr]
        fig = dr.measure_cic(grid, ref, T)
        fig["apron_cells_set"] = int(np.count_nonzero(sums)) - int(np.count_nonzero(grid))
        for_finish = grid
    else:
        ref = dr.cell_sums(parts["position"], parts["velocity"], nr, nz, T, bits)
        fig = dr.measure_sums(sums, ref, T)
        for_finish = sums
    sim.densityFinish()
    moments, norm, avg = (sim.readGrid(w) for w in (fp.READ_MOMENTS, fp.READ_NORM, fp.READ_AVG))
    fig.update(dr.measure_moments(moments, for_finish, nr, nz, STAMP, T, identity=cic))
    fig.update(dr.measure_finish(norm, avg, moments, prev, nr, nz, T))
    for k, v in fig.items():
        WORST[(k, precision)] = max(WORST.get((k, precision), 0.0), float(v))
    print("    %s %s  " % (where, precision) + "  ".join("%s %.3g" % kv for kv in sorted(fig.items())))
    assert fig.pop("apron_cells_set", 0) == 0
    dr.assert_figures(fig, where)
    return ref, sums


def start(fp, scene, precision, count=0, **kw):
    spec, inputs, entropy, rand = scene
    sim = fp.makeCylindricalParticlePusher(spec, precision=precision, count=count, **kw)
    sim.set(**inputs)
    sim.setRandomState(entropy, rand)
    sim.precalc()
    return sim


# ------------------------------------------------------------------ 1, 2: the routes of the re-binning push
@pytest.fixture(scope="module")
def routes_scene():
    return ds.routes(160, 0.02)


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("fuse", [True, False, "census"], ids=["fused", "separate", "census"])
def test_routes(fp, routes_scene, fuse, precision):
    """sort_interval = 1, six frames: the first binning with the separate kernel, then in-place and re-binning launches in
    turn.  fp32 fused: the sums come from the push (the separate kernel ran once, for frame 0) and the leavers of every
    re-binning go through the outbox; 'census': re-binning in the push, sums by the separate kernel; separate and fp64:
    the separate kernel every frame."""
    sim = start(fp, routes_scene, precision, sort_interval=1, fuse_deposit=fuse)
    check_frame(fp, sim, precision, "frame 0")
    for frame in range(1, 7):
        sim.step()
        check_frame(fp, sim, precision, "frame %d" % frame)
    st = sim.stats()
    sim.destroy()
    print("   ", {k: st[k] for k in ("sort_passes", "deposit_launches", "outbox_items", "outbox_full_items")})
    fused_sums = fuse is True and precision == "fp32"
    assert st["deposit_launches"] == (1 if fused_sums else 7)
    assert st["sort_passes"] == (7 if fuse is False else 4)       # the first binning + every deposit / + every second launch
    assert (st["outbox_items"] > 0) == (fuse is not False and precision == "fp32") and st["outbox_full_items"] == 0


def test_outbox_overflow(fp, routes_scene, monkeypatch):
    """2500 records: some items of every re-binning launch find no room and store their leavers directly"""
    monkeypatch.setenv("FPIC_TEST_OUTBOX_RECORDS", "2500")
    sim = start(fp, routes_scene, "fp32", sort_interval=1)
    check_frame(fp, sim, "fp32", "frame 0")
    for frame in range(1, 7):
        sim.step()
        check_frame(fp, sim, "fp32", "frame %d" % frame)
    st = sim.stats()
    sim.destroy()
    assert st["deposit_launches"] == 1 and st["outbox_items"] > 0 and st["outbox_full_items"] > 0, st


# ------------------------------------------------------------------ 3: several work items per tile, several pieces
def test_several_items_per_tile_and_several_pieces(fp):
    """160 000 particles on 96 x 72 (the fullest tile is cut into three work items, whose ends carry up to three particles of
    the next tile; tests/test_gpu_rebin_outbox.py shows the preconditions), sort_interval = 2: the launches of frames 3 and 6
    re-bin.  At most 1000 particles per cell: measure_sums asserts it."""
    sim = start(fp, ds.routes(400, 0.025), "fp32", sort_interval=2)
    check_frame(fp, sim, "fp32", "frame 0")
    for frame in range(1, 7):
        sim.step()
        check_frame(fp, sim, "fp32", "frame %d" % frame)
    st = sim.stats()
    sim.destroy()
    assert st["sort_passes"] == 3 and st["outbox_items"] > 0 and st["deposit_launches"] == 1, st


# ------------------------------------------------------------------ 4: the spill path
@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "separate"])
def test_spill_path(fp, fuse):
    """one binning, then 20 steps without another: particles that left their tile's halo go to global memory one by one"""
    sim = start(fp, ds.spill(), "fp32", sort_interval=1 << 30, fuse_deposit=fuse)
    check_frame(fp, sim, "fp32", "frame 0")
    sim.step(20)
    check_frame(fp, sim, "fp32", "after 20 steps")
    st = sim.stats()
    sim.destroy()
    assert st["sort_passes"] == 1 and st["deposit_spilled"] > 0, st


# ------------------------------------------------------------------ 5: edges and tails
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("grid", ds.EDGE_GRIDS, ids=lambda g: "%dx%d" % g)
def test_edges_and_tails(fp, grid, precision):
    """5, 4097 and 4098 particles (tail lanes of one and two particles; a lane holds four in fp32, two in fp64) with the
    hand-placed edge cases among them, the separate kernel (frame 0) and the push (frame 1).  The particle at r = 0 makes
    channels 0 and 1 of exactly its cell NaN in the sums and of exactly its cropped footprint in the moments: the NaN sets
    are compared inside measure_*, the reference's are pinned in tests/test_deposit_reference.py."""
    T = dr.real(precision)
    nr, nz = grid
    for count in ds.EDGE_COUNTS:
        sim = start(fp, ds.edges(nr, nz, count, T), precision, count=count)
        ref, sums = check_frame(fp, sim, precision, "%d particles, frame 0" % count)
        jc = int(0.5 * nz)
        nan = np.zeros(sums.shape[:2], dtype=bool)
        nan[jc + dr.APRON, 0 + dr.APRON] = True
        assert np.array_equal(np.isnan(sums[..., 0]), nan) and np.array_equal(np.isnan(sums[..., 1]), nan)
        assert not np.isnan(sums[..., 2:]).any()
        m = sim.readMoments(np.float64).reshape(nz, nr, 4)
        foot = np.zeros((nz, nr), dtype=bool)
        foot[max(0, jc - 5):jc + 6, 0:6] = True
        assert np.array_equal(np.isnan(m[..., 0]), foot) and np.array_equal(np.isnan(m[..., 1]), foot) and not np.isnan(m[..., 2:]).any()
        sim.step()
        check_frame(fp, sim, precision, "%d particles, frame 1" % count)
        sim.destroy()


# ------------------------------------------------------------------ 6: rasterised sprites
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("bits", [1, 4, 8])
def test_rasterised_sprites(fp, bits, fuse, precision):
    """sprite centres up to five cells outside every edge: the apron holds particles on all four sides"""
    T = dr.real(precision)
    scene = ds.raster(T)
    sim = start(fp, scene, precision, count=len(scene[1]["position"]), raster_subpixel_bits=bits, fuse_deposit=fuse)
    for frame in range(2):
        if frame:
            sim.step()
        ref, sums = check_frame(fp, sim, precision, "bits %d frame %d" % (bits, frame), bits=bits)
        c, a = ref["count"], dr.APRON
        sides = [c[:, :a].sum(), c[:, a + sim.nr + 1:].sum(), c[:a].sum(), c[a + sim.nz + 1:].sum()]
        assert min(sides) > 0, sides
    sim.destroy()


# ------------------------------------------------------------------ 7: shape 'cic'
@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_cic(fp, precision):
    sim = start(fp, ds.cic(), precision, shape="cic")
    check_frame(fp, sim, precision, "frame 0", cic=True)
    for frame in range(1, 6):
        sim.step()
        check_frame(fp, sim, precision, "frame %d" % frame, cic=True)
    sim.destroy()


# ------------------------------------------------------------------ 8: the picture is that of the state stored NOW
def test_picture_follows_every_change_of_the_state(fp, routes_scene, tmp_path):
    """after step(); density() the fused push has left the sums of its final state and deposit() may skip its pass.  Every way
    of changing the stored state afterwards must be followed by the picture of what getParticles() returns now; where the
    change moves the picture, the OLD sums miss the new reference by at least 100 bounds (so a skipped pass would show)."""
    T = np.float32
    spec, inputs, entropy, rand = routes_scene
    sim = start(fp, routes_scene, "fp32", sort_interval=2)
    sim.density()
    sim.step()
    _, old = check_frame(fp, sim, "fp32", "after step")

    def moved(ref, old, what):
        fig = dr.measure_sums(old, ref, T)
        print("    the old sums against the state after %s: %s" % (what, fig))
        assert fig["colour"] >= 100, (what, fig)

    sim.set(velocity=-2.0 * np.asarray(inputs["velocity"]))
    ref, old2 = check_frame(fp, sim, "fp32", "set(velocity)")
    moved(ref, old, "set(velocity)")

    pos2 = ds.uniform_plasma(sim.n, spec, seed=99, margin=0.2)[0]
    sim.step()
    sim.density()
    sim.set(position=pos2)
    ref, old3 = check_frame(fp, sim, "fp32", "set(position)")
    moved(ref, old2, "set(position)")
    assert dr.measure_sums(old2, ref, T)["count_cells_wrong"] > 100

    sim.step()
    sim.density()
    sim.sort()
    check_frame(fp, sim, "fp32", "sort()")

    sim.step()
    _, at_save = check_frame(fp, sim, "fp32", "before saveCheckpoint")
    path = os.path.join(str(tmp_path), "deposit.ckp")
    sim.saveCheckpoint(path)
    sim.step(3)
    _, later = check_frame(fp, sim, "fp32", "three steps on")
    sim.loadCheckpoint(path)
    ref, again = check_frame(fp, sim, "fp32", "loadCheckpoint, same handle")
    moved(ref, later, "loadCheckpoint")
    assert np.array_equal(dr.counts_of(again, T)[0], dr.counts_of(at_save, T)[0])

    fresh = start(fp, routes_scene, "fp32", sort_interval=2)
    fresh.density()
    fresh.step()
    fresh.density()
    fresh.loadCheckpoint(path)
    ref2, _ = check_frame(fp, fresh, "fp32", "loadCheckpoint, fresh handle")
    assert np.array_equal(ref2["count"], ref["count"])
    fresh.destroy()

    sim.step()
    sim.density()
    sim.setRandomState(rand=np.random.default_rng(4).random((sim.n, 4), dtype=np.float32))
    check_frame(fp, sim, "fp32", "setRandomState(rand)")
    sim.destroy()


def test_print_the_gpu_columns():
    """(runs last in this module: the GPU columns of the table of DESIGN section 2)"""
    for stage in sorted({k for k, _ in WORST}):
        print("    %-18s fp32 %-10.3g fp64 %.3g" % (stage, WORST.get((stage, "fp32"), float("nan")), WORST.get((stage, "fp64"), float("nan"))))
