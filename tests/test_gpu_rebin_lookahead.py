"""The bins of the (r,z) push may look ahead: with a lookahead of k sub-steps a particle is filed in the tile of position +
k sub-steps of its velocity (clamped into the unit square) instead of the tile it is in (bin_slot, csrc/fpic_push.hpp), so
that over a binning period it strays from -k to period - k sub-steps from its bin instead of from 0 to the period.  The bins
decide where a particle is stored and which LDS windows serve it, never a result: every case asks for the oracle's bits
(assert_frame_equal of tests/test_gpu_rebin_outbox.py: particle state, alive flags, random state, read-back order, and the
deposit at the bar of tests/test_gpu_parity.py), wherever the prediction lands.

Scene and helpers are those of tests/test_gpu_rebin_outbox.py: fp32 unless stated, 96 x 72 cells, 160^2 particles, radius 0.5,
height 0.4, the frame sink as sink and source, random E and B unless stated."""
import numpy as np
import pytest

from helpers import frame_sink, make_spec, same_bits, uniform_plasma
from test_gpu_rebin_outbox import NR, NZ, TILE, assert_frame_equal, scene, start

pytestmark = pytest.mark.gpu

RTOL64 = 1e-6           # the fp64 deposit's bar in tests/test_gpu_parity.py
HALO = 8                # kTileHalo (csrc/fpic_internal.hpp): cells of the sums window around a tile
MAX_LOOKAHEAD = 64       # kMaxLookahead (csrc/fpic_api.hip): cap of the adaptive lookahead, sub-steps


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    return fusionpic


@pytest.fixture(scope="module")
def po():
    import pic_oracle
    return pic_oracle


def run_frames(sim, ora, frames, rand=True, every=1):
    """frames of step() + density() on both; the oracle's bits every `every`-th frame.  Returns sort_passes after each frame."""
    passes = []
    for frame in range(1, frames + 1):
        sim.step(); ora.step()
        sim.density(); ora.density()
        if frame % every == 0:
            assert_frame_equal(sim, ora, rand=rand)
        passes.append(sim.stats()["sort_passes"])
    return passes


@pytest.mark.parametrize("rng", ["reference", "counter"])
@pytest.mark.parametrize("look", [1, 4, 16])
def test_forced_lookahead_with_wrong_predictions(fp, po, rng, look):
    """a re-binning every second frame with a fixed lookahead, hot particles in random fields: the fields turn the
    velocities, the sink removes particles and re-injection puts them elsewhere, so many predictions are wrong"""
    spec, fields, entropy, rand = scene(160, v_th=0.02)
    sim, ora = start(fp, po, spec, fields, entropy, rand, rng=rng, sort_interval=2, bin_lookahead=look)
    passes = run_frames(sim, ora, 8, rand=rng == "reference")
    sim.destroy()
    assert passes[-1] >= 3


def test_forced_lookahead_fp64(fp, po):
    """double state (the re-binning launch stores every leaver directly: no outbox), lookahead 4"""
    spec, fields, entropy, rand = scene(160, v_th=0.02)
    sim = fp.makeCylindricalParticlePusher(spec, precision="fp64", sort_interval=2, bin_lookahead=4)
    ora = po.OracleSim(spec, dtype=np.float64)
    for s in (sim, ora):
        s.set(**fields)
    sim.setRandomState(entropy, rand); ora.set_random_state(entropy, rand)
    sim.precalc(); ora.precalc()
    sim.density(); ora.density()
    for frame in range(8):
        sim.step(); ora.step()
        sim.density(); ora.density()
        got = sim.getParticles(np.float64)   # (the random state is read back as float32: the double state's bits follow from it)
        assert np.array_equal(got["alive"], ora.alive())
        assert np.array_equal(sim.getCells(), ora.cells())
        assert same_bits(got["position"], ora.positions()) and same_bits(got["velocity"], ora.velocities())
        m, w = sim.readMoments(np.float64).reshape(-1, 4), ora.moments.astype(np.float64).reshape(-1, 4)
        np.testing.assert_allclose(m[:, 3], w[:, 3], rtol=RTOL64)
        for c in range(3):
            assert np.array_equal(np.isnan(m[:, c]), np.isnan(w[:, c]))
            assert np.nanmax(np.abs(m[:, c] - w[:, c])) <= RTOL64 * np.nanmax(np.abs(w[:, c]))
    st = sim.stats()
    sim.destroy()
    assert st["sort_passes"] >= 3


def test_lookahead_beyond_the_domain(fp, po):
    """10000 sub-steps ahead nearly every predicted position lies outside the unit square and is clamped onto an edge tile:
    a few bins hold almost everything, nearly every particle is served by the global path"""
    spec, fields, entropy, rand = scene(160, v_th=0.02)
    sim, ora = start(fp, po, spec, fields, entropy, rand, sort_interval=1, bin_lookahead=10000)
    passes = run_frames(sim, ora, 6)
    sim.destroy()
    assert passes[-1] >= 3


def test_census_against_count_pass_with_lookahead(fp, monkeypatch):
    """test_census_against_count_pass_with_the_outbox with a lookahead: the census of final states (the launch before) and
    the re-binning launch's own count pass (FPIC_TEST_COUNT_PASS; it then reads the velocities too) file every state alike.
    In this hot scene a key two frames ahead makes more than half the particles leavers: more than the outbox's n / 2
    records, and which items then find room is a race between workgroups (outbox_items came out as 17 and as 18 of 19 in two
    runs of one build).  The outbox is therefore given room for every particle, so that outbox_items is a function of the
    reservations alone, and no item may have gone without room."""
    monkeypatch.setenv("FPIC_TEST_OUTBOX_RECORDS", str(160 * 160))
    spec, fields, entropy, rand = scene(160, v_th=0.02)
    runs = []
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("FPIC_TEST_COUNT_PASS", "1")
        sim = fp.makeCylindricalParticlePusher(spec, sort_interval=2, bin_lookahead=4)
        sim.set(**fields)
        sim.setRandomState(entropy, rand)
        sim.precalc(); sim.density()
        for _ in range(6):
            sim.step(); sim.density()
        got = sim.getParticles()
        st = sim.stats()
        runs.append((got["position"], got["velocity"], got["rand"], got["alive"], sim.getCells(), st["sort_passes"], st["outbox_items"]))
        print("count pass" if forced else "census", "sort_passes", st["sort_passes"], "outbox_items", st["outbox_items"], "outbox_full_items", st["outbox_full_items"])
        assert st["outbox_full_items"] == 0
        sim.destroy()
    assert runs[0][5] >= 3 and runs[0][5] == runs[1][5]
    assert runs[0][6] > 0 and runs[0][6] == runs[1][6]
    for a, b in zip(runs[0][:5], runs[1][:5]):
        assert np.array_equal(a, b, equal_nan=True)


def cells_of(p):
    """sprite cell (ic, jc) of oracle positions, as the push forms it"""
    p = p.astype(np.float32)
    r, z = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]), p[:, 2]
    assert ((r >= 0) & (r <= 1) & (z >= 0) & (z <= 1)).all()
    return (r * np.float32(NR)).astype(np.int64), (z * np.float32(NZ)).astype(np.int64)


def outside_window(key, final, slack):
    """particles whose final cell lies outside the sums window (tile + HALO cells) of the tile of their key position; slack
    > 0 shrinks the window, slack < 0 widens it"""
    out = np.zeros(len(key[0]), dtype=bool)
    for k, f in zip(key, final):
        lo = (k // TILE) * TILE - HALO + slack
        out |= (f < lo) | (f > lo + TILE + 2 * HALO - 1 - 2 * slack)
    return out


def test_lookahead_keeps_a_drifting_beam_inside_its_windows(fp, po):
    """What the key is for.  No field, every particle the same velocity along +z (VZ: 2.1 cells per frame, chosen on the CPU
    oracle alone), away from the sink.  With sort_interval=4 the launches of frames 5 and 10 re-bin, by the states they load
    (those of frames 4 and 9); the bins of a re-binning launch serve the five launches after it: four in place, which
    record deposit_spilled, and the next re-binning launch, which records none (stats() then says 0 whatever happened).
    Keyed on the position, the final state of the in-place launches is 2 to 5 frames of drift (4.2 to 10.5 cells) ahead of
    its bin, 12.6 cells in the re-binning launch: beyond the 8-cell halo for particles near their tile's upper edge.  Keyed 4
    sub-steps (2 frames) ahead it is 0 to 6.3 cells ahead: inside.

    A work item owns the 4-particle vectors that BEGIN in its tile, so an item whose tile does not end on a multiple of 4
    carries up to three particles of the next tile in storage order, far from its windows whatever the key.  Every position
    is therefore used four times: whole quadruples change bins, every tile population is a multiple of 4."""
    FRAMES, VZ = 11, 0.0097
    spec = make_spec(NR, NZ, 160, radius=0.5, height=0.4)
    pos, _, entropy, rand = uniform_plasma(160 * 160 // 4, spec, seed=8, v_th=0.0, margin=0.36)
    pos[:, 2] -= 0.16 * spec["height"]     # z over cells 14 .. 35: the beam crosses the tile edge at cell 32 while it is watched
    pos, rand = np.repeat(pos, 4, axis=0), np.repeat(rand, 4, axis=0)
    vel = np.zeros_like(pos); vel[:, 2] = VZ
    zero = np.zeros((NR, NZ, 3))
    fields = dict(E=zero, B=zero, position=pos, velocity=vel, sink_mask=frame_sink(NR, NZ), source_pdf=frame_sink(NR, NZ))

    spilled, passes, cells = {}, {}, None
    for look in (4, -1):
        sim, ora = start(fp, po, spec, fields, entropy, rand, sort_interval=4, bin_lookahead=look)
        frames = [cells_of(ora.positions())]
        spilled[look], passes[look] = [], []
        for frame in range(1, FRAMES + 1):
            sim.step(); ora.step()
            sim.density(); ora.density()
            assert_frame_equal(sim, ora)
            st = sim.stats()
            spilled[look].append(st["deposit_spilled"]); passes[look].append(st["sort_passes"])
            assert ora.alive().all()                       # precondition: nothing reaches the sink
            frames.append(cells_of(ora.positions()))
        sim.destroy()
        cells = frames
    rebins = [f for f in range(2, FRAMES + 1) if passes[4][f - 1] > passes[4][f - 2]]
    assert rebins == [5, 10] and passes[4] == passes[-1]
    # preconditions, from the oracle's positions: the bins of the re-binning launch of frame s serve frames s+1 .. s+5.  Two
    # frames of drift ahead of the state that launch loads (frame s-1) is the oracle's state of frame s+1.
    after = [f for f in range(rebins[0] + 1, FRAMES + 1)]
    counted = [f for f in after if f not in rebins]         # in-place launches: the ones that record a count
    served_by = {f: max(s for s in rebins if s < f) for f in after}
    for f in counted:
        s = served_by[f]
        assert not outside_window(cells[s + 1], cells[f], slack=1).any(), f     # inside the halo with a cell to spare
    assert any(outside_window(cells[served_by[f] - 1], cells[f], slack=-1).any() for f in counted)  # outside by a cell or more
    print("deposit_spilled per frame, lookahead 4:", spilled[4], "off:", spilled[-1])
    for f in after:
        assert spilled[4][f - 1] == 0, (f, spilled[4])
    assert any(spilled[-1][f - 1] > 0 for f in counted), spilled[-1]


def test_adaptive_mode(fp, po):
    """sort_interval=0 with the default: the lookahead is half the sub-steps pushed on the bins being left plus the
    re-binning launch's own (at most 64), and the spill rule may not fire while the sub-steps pushed since a re-binning
    are no more than its lookahead.  Two sub-steps per frame: the re-binning launch of frame s_k looks ahead L_k =
    min(64, s_k - s_(k-1) + 2) sub-steps (s_0 = 1: the first binning files the uploaded state, frame 1 is the first launch
    on it), and the next one comes at a frame s with 2 (s - s_k) > L_k."""
    spec, fields, entropy, rand = scene(160, v_th=0.02, fields=False)
    passes = {}
    for look in (0, -1):
        sim, ora = start(fp, po, spec, fields, entropy, rand, sort_interval=0, bin_lookahead=look)
        passes[look] = run_frames(sim, ora, 24, every=4)
        sim.destroy()
    print("sort_passes per frame, adaptive:", passes[0], "off:", passes[-1])
    assert passes[0][-1] <= passes[-1][-1]
    rebins = [f for f in range(2, 25) if passes[0][f - 1] > passes[0][f - 2]]
    assert len(rebins) >= 2
    last = 1
    for s, nxt in zip(rebins, rebins[1:]):
        look = min(MAX_LOOKAHEAD, s - last + 2)
        assert 2 * (nxt - s) > look, (rebins, s, nxt, look)
        last = s


def test_off_is_the_parent(fp):
    """bin_lookahead=-1 against the default at a fixed sort_interval (which keeps the position key): the same particle
    order, cells, re-binning launches and outbox items"""
    spec, fields, entropy, rand = scene(160, v_th=0.02)
    runs = []
    for look in (-1, 0):
        sim = fp.makeCylindricalParticlePusher(spec, sort_interval=2, bin_lookahead=look)
        sim.set(**fields)
        sim.setRandomState(entropy, rand)
        sim.precalc(); sim.density()
        for _ in range(6):
            sim.step(); sim.density()
        got = sim.getParticles()
        st = sim.stats()
        runs.append((got["position"], got["velocity"], got["rand"], got["alive"], sim.getCells(), st["sort_passes"], st["outbox_items"]))
        sim.destroy()
    assert runs[0][5] >= 3 and runs[0][5:] == runs[1][5:]
    for a, b in zip(runs[0][:5], runs[1][:5]):
        assert np.array_equal(a, b, equal_nan=True)
