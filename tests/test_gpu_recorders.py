"""The three recorders of the CART3D box — energy rows, series, modes — armed together on one handle: three periods on the one
sub-step counter, every ring wrapped, every drain in two runs of slots.  Each history is the newest rows of its ring, bit for
bit the values a twin handle takes at those sub-steps, with the count of the rows the ring overwrote; a second drain is empty;
disarming gives back every byte that arming took, except the energy reduction's resident buffers."""
import numpy as np
import pytest

import modes_reference as mr
from test_gpu_histogram import box_spec, em_dt

pytestmark = pytest.mark.gpu

# what the first energy reduction of a handle allocates and keeps (diag_buffers): the partial rows of 16 species x 2048
# workgroups x 11 words, 2 x 512 field partials, 16 x 6 + 2 combined sums (8 bytes each), and the row of fpic_energy_now
ENERGY_RESIDENT = 8 * (16 * 2048 * 11 + 2 * 512 + 16 * 6 + 2)
# what the first sub-step of this box allocates and keeps whether or not anything records: nothing (electrostatic); the two
# half-time B arrays of the chained lattice step, 2 x 512 nodes x 4 floats, and the push's 120 bytes of arguments (full EM)
STEPPING = {"poisson_fft": 0, "yee": 2 * 512 * 4 * 4 + 120}


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def small_box(fp, solver, shape=(8, 8, 8), n=64, seed=9):
    rng = np.random.default_rng(seed)
    L = tuple(1e-3 * s for s in shape)
    dt = em_dt(shape, L) if solver == "yee" else 5e-12
    spec = box_spec(shape, L, n, dt, solver=solver, macro_weight=1e15 * np.prod(L) / n)
    sim = fp.makeCylindricalParticlePusher(spec, precision="fp32")
    sim.set(position=rng.random((n, 3)) * L, velocity=rng.normal(0, 0.03, (n, 3)))
    sim.addB(0.0, 0.02, 0.05)
    return sim, L


@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
def test_three_recorders_wrap_on_one_counter(fp, solver):
    a, L = small_box(fp, solver)
    b, _ = small_box(fp, solver)
    pts = np.array([[0.3, 0.55, 0.8]]) * L
    ids = np.array([41, 5])
    modes = [(1, 0, 0), (-2, 3, 1)]
    a.precalc(); b.precalc()
    before, twin_before = a.stats()["bytes_grid_state"], b.stats()["bytes_grid_state"]
    a.recordEnergy(1, 3)
    a.recordSeries(2, 3, points=pts, tracers=ids)
    a.recordModes(3, 3, modes, mr.FIELDS)
    twin = {}
    for t in range(1, 14):
        a.substeps(1); b.substeps(1)
        twin[t] = (b._energy_row("global"), b.series(points=pts, tracers=ids), b._modes_rows(modes, mr.FIELDS, "global")[0])
    erows, edropped = a.energyHistory()
    hist, sdropped = a.seriesHistory()
    msub, mout, names, mdropped = a._modes_history_rows("global")
    print(solver, "energy", [int(r["substep"]) for r in erows], edropped, "series", hist["substep"].tolist(), sdropped,
          "modes", msub.tolist(), mdropped)
    assert [int(r["substep"]) for r in erows] == [11, 12, 13] and edropped == 10
    assert hist["substep"].tolist() == [8, 10, 12] and sdropped == 3
    assert msub.tolist() == [6, 9, 12] and mdropped == 1 and names == list(mr.FIELDS)
    assert hist["points"].shape == (3, 1, 8) and hist["tracers"].shape == (3, 2, 8) and mout.shape == (3, 2, len(mr.FIELDS), 2)
    for r, t in enumerate([11, 12, 13]):
        assert erows[r].tobytes() == twin[t][0].tobytes(), t
    for r, t in enumerate([8, 10, 12]):
        assert hist["points"][r].tobytes() == twin[t][1]["points"].tobytes(), t
        assert hist["tracers"][r].tobytes() == twin[t][1]["tracers"].tobytes(), t
    for r, t in enumerate([6, 9, 12]):
        assert mout[r].tobytes() == twin[t][2].tobytes(), t
    # (the rows differ from one another: a row in the wrong slot would show)
    assert erows[0].tobytes() != erows[1].tobytes() and not np.array_equal(hist["tracers"][0], hist["tracers"][2])
    assert not np.array_equal(mout[0], mout[2])
    # drained: nothing is pending, nothing dropped
    erows, edropped = a.energyHistory()
    hist, sdropped = a.seriesHistory()
    msub, mout, _, mdropped = a._modes_history_rows("global")
    assert (len(erows), edropped, len(hist["substep"]), sdropped, len(msub), mdropped) == (0, 0, 0, 0, 0, 0)
    a.recordEnergy(0); a.recordSeries(0); a.recordModes(0)
    after, twin_after = a.stats()["bytes_grid_state"], b.stats()["bytes_grid_state"]
    print(solver, "bytes_grid_state", before, after, after - before, "twin", twin_before, twin_after, twin_after - twin_before)
    assert after - before == ENERGY_RESIDENT + fp.ENERGY_DTYPE.itemsize + STEPPING[solver]
    assert twin_after - twin_before == after - before      # (the twin never recorded: its energy() calls hold the same buffers)
    a.destroy(); b.destroy()
