"""The re-binning launch of the (r,z) push delivers its leavers (particles whose tile changed since the last binning) through
an outbox: records written densely into one region per work item, read back by the same workgroup once its LDS windows are
dead, sorted by destination in LDS in pieces of 2048 and stored in runs (csrc/fpic_push.hpp).  Only the order inside a bin's
range may change, so every case asks for the oracle's bits: particle state, alive flags, random state and read-back order,
and the deposit at the bar of tests/test_gpu_parity.py.

Scene of every case: fp32, 96 x 72 cells (tiles of 32: the centre tiles have all eight neighbours, the edge tiles have
neighbour slots outside the grid), radius 0.5, height 0.4, the frame sink as sink and source, random E and B."""
import numpy as np
import pytest

from helpers import frame_sink, make_spec, same_bits, uniform_plasma

pytestmark = pytest.mark.gpu

RTOL32 = 1e-3            # the deposit's bar in tests/test_gpu_parity.py
NR, NZ = 96, 72
TILE = 32                # kTileSide (csrc/fpic_internal.hpp)
DEPOSIT_CHUNK = 16384    # kDepositChunk: particles of one work item
PIECE = 2048             # kOutboxPiece (csrc/fpic_push.hpp)


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    return fusionpic


@pytest.fixture(scope="module")
def po():
    import pic_oracle
    return pic_oracle


def scene(side, v_th, seed=8, margin=0.0, fields=True):
    spec = make_spec(NR, NZ, side, radius=0.5, height=0.4)
    rng = np.random.default_rng(7)
    B = rng.normal(0, 0.5, size=(NR, NZ, 3))
    B[..., 2] += 1.0
    E = rng.normal(0, 2e4, size=(NR, NZ, 3))
    if not fields:
        E, B = np.zeros_like(E), np.zeros_like(B)
    pos, vel, entropy, rand = uniform_plasma(side * side, spec, seed=seed, v_th=v_th, margin=margin)
    return spec, dict(E=E, B=B, position=pos, velocity=vel, sink_mask=frame_sink(NR, NZ), source_pdf=frame_sink(NR, NZ)), entropy, rand


def start(fp, po, spec, fields, entropy, rand, rng="reference", **kw):
    if rng == "counter":
        sim = fp.makeCylindricalParticlePusher(spec, rng=rng, seed=0x5EEDF051CAFE, **kw)
        ora = po.OracleSim(spec, dtype=np.float32, rng=rng, seed=0x5EEDF051CAFE)
    else:
        sim = fp.makeCylindricalParticlePusher(spec, **kw)
        ora = po.OracleSim(spec, dtype=np.float32)
    for s in (sim, ora):
        s.set(**fields)
    if rng == "reference":
        sim.setRandomState(entropy, rand); ora.set_random_state(entropy, rand)
    sim.precalc(); ora.precalc()
    sim.density(); ora.density()
    return sim, ora


def assert_particles_equal(sim, ora, rand=True):
    got = sim.getParticles()
    assert np.array_equal(got["alive"], ora.alive()), "alive flags differ"
    assert np.array_equal(sim.getCells(), ora.cells()), "NGP cell indices differ"
    assert same_bits(got["position"], ora.positions())
    assert same_bits(got["velocity"], ora.velocities())
    if rand:
        assert same_bits(got["rand"], ora.rand().astype(np.float32))


def assert_frame_equal(sim, ora, rand=True):
    assert_particles_equal(sim, ora, rand=rand)
    got = sim.readMoments(np.float64).reshape(-1, 4)
    want = ora.moments.astype(np.float64).reshape(-1, 4)
    np.testing.assert_allclose(got[:, 3], want[:, 3], rtol=RTOL32)
    for c in range(3):
        assert np.array_equal(np.isnan(got[:, c]), np.isnan(want[:, c]))
        assert np.nanmax(np.abs(got[:, c] - want[:, c])) <= RTOL32 * np.nanmax(np.abs(want[:, c]))


def oracle_tiles(ora):
    """the bin of every particle as the push files it: the tile of the cell its sprite falls in, -1 outside the unit square"""
    p = ora.positions().astype(np.float32)
    r, z = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]), p[:, 2]
    inside = (r >= 0) & (r <= 1) & (z >= 0) & (z <= 1)
    ic = (np.where(inside, r, 0) * np.float32(NR)).astype(np.int64)
    jc = (np.where(inside, z, 0) * np.float32(NZ)).astype(np.int64)
    return np.where(inside, ic // TILE + ((NR + TILE) // TILE) * (jc // TILE), -1)


def test_several_pieces_and_several_items_per_tile(fp, po):
    """160 000 hot particles, a re-binning every second frame: a quarter and more of the particles leave their tile between
    two binnings, the fullest tile is cut into three work items, and at least one item sends more leavers than two pieces
    hold.  The first binning files the uploaded state (frame 0); with sort_interval=2 the launches of frames 3 and 6 re-bin,
    by the states they load: those of frames 2 and 5.  (v_th = 0.025 was chosen on the CPU oracle alone so that the
    preconditions below hold for these pairs, and for any two frames two apart besides.)"""
    spec, fields, entropy, rand = scene(400, v_th=0.025)
    sim, ora = start(fp, po, spec, fields, entropy, rand, sort_interval=2)
    tiles = [oracle_tiles(ora)]
    for frame in range(6):
        sim.step(); ora.step()
        sim.density(); ora.density()
        assert_frame_equal(sim, ora)
        tiles.append(oracle_tiles(ora))
    st = sim.stats()
    sim.destroy()
    assert st["outbox_items"] > 0
    assert st["sort_passes"] == 3
    for j, k in [(0, 2), (2, 5)] + [(k - 2, k) for k in range(3, len(tiles))]:
        before, left = tiles[j], tiles[j] != tiles[k]
        assert left.mean() >= 0.25, (j, k, left.mean())
        ids, counts = np.unique(before, return_counts=True)
        assert counts.max() > DEPOSIT_CHUNK
        # a tile of c particles is ceil(c / DEPOSIT_CHUNK) items: one of them sends at least the mean of its leavers
        most = max(left[before == t].sum() / -(-c // DEPOSIT_CHUNK) for t, c in zip(ids, counts))
        assert most > 2 * PIECE, (j, k, most)


@pytest.mark.parametrize("rng", ["reference", "counter"])
def test_every_launch_rebins(fp, po, rng):
    """sort_interval=1: every density() asks for a re-binning, so every second launch is one (the launch after a re-binning
    has nothing to re-bin by), for both generator forms (records of three and of two 16-byte planes)"""
    spec, fields, entropy, rand = scene(160, v_th=0.02)
    sim, ora = start(fp, po, spec, fields, entropy, rand, rng=rng, sort_interval=1)
    for frame in range(8):
        sim.step(); ora.step()
        sim.density(); ora.density()
        assert_frame_equal(sim, ora, rand=rng == "reference")
    st = sim.stats()
    sim.destroy()
    assert st["sort_passes"] >= 4 and st["outbox_items"] > 0 and st["outbox_full_items"] == 0


def test_outbox_too_small_for_some_items(fp, po, monkeypatch):
    """2500 records: on the CPU oracle no item of this scene (one per tile) has more than 2458 leavers between two frames
    two apart, and all items together have at least 6000, so in every re-binning launch the first reservation fits and a
    later one does not.  An item that finds no room stores all its leavers directly; the bits are those of the case above."""
    monkeypatch.setenv("FPIC_TEST_OUTBOX_RECORDS", "2500")
    spec, fields, entropy, rand = scene(160, v_th=0.02)
    sim, ora = start(fp, po, spec, fields, entropy, rand, sort_interval=1)
    for frame in range(8):
        sim.step(); ora.step()
        sim.density(); ora.density()
        assert_frame_equal(sim, ora)
    st = sim.stats()
    sim.destroy()
    assert st["outbox_items"] > 0 and st["outbox_full_items"] > 0, st


def test_census_against_count_pass_with_the_outbox(fp, monkeypatch):
    """the scene of test_rebinning_launch_reserves_the_same_ranges_with_and_without_the_census (tests/test_gpu_parity.py):
    the outbox's reservation is the census total less the own slot, whether the census came from the launch before or from
    the launch's own count pass (FPIC_TEST_COUNT_PASS)"""
    spec, fields, entropy, rand = scene(160, v_th=0.02)
    runs = []
    for forced in (False, True):
        if forced:
            monkeypatch.setenv("FPIC_TEST_COUNT_PASS", "1")
        sim = fp.makeCylindricalParticlePusher(spec, sort_interval=2)
        sim.set(**fields)
        sim.setRandomState(entropy, rand)
        sim.precalc(); sim.density()
        for _ in range(6):
            sim.step(); sim.density()
        got = sim.getParticles()
        st = sim.stats()
        runs.append((got["position"], got["velocity"], got["rand"], got["alive"], sim.getCells(), st["sort_passes"], st["outbox_items"]))
        sim.destroy()
    assert runs[0][5] >= 3 and runs[0][5] == runs[1][5]
    assert runs[0][6] > 0 and runs[0][6] == runs[1][6]
    for a, b in zip(runs[0][:5], runs[1][:5]):
        assert np.array_equal(a, b, equal_nan=True)


def test_no_leavers_at_all(fp, po):
    """cold particles away from the sink in no field: nothing moves, two re-binning launches leave the state as it was.  A
    work item owns the 4-particle vectors that BEGIN in its tile, so an item whose tile does not end on a multiple of 4 carries
    up to three particles of the next tile and sends them through the outbox; every other item has no leaver and may not
    reserve, write or read a record.  Which items those are follows from the tile populations alone."""
    spec, fields, entropy, rand = scene(160, v_th=0.0, margin=0.05, fields=False)
    sim, ora = start(fp, po, spec, fields, entropy, rand, sort_interval=1)
    first = sim.getParticles()
    ids, counts = np.unique(oracle_tiles(ora), return_counts=True)
    assert ids.min() >= 0 and counts.max() <= DEPOSIT_CHUNK    # one work item per tile, nothing clipped
    carrying = int((np.cumsum(counts) % 4 != 0).sum())
    assert 0 < carrying < len(ids)                             # items of both kinds
    for frame in range(5):   # (with sort_interval=1 every second launch re-bins: those of frames 2 and 4)
        sim.step(); ora.step()
        sim.density(); ora.density()
        assert_frame_equal(sim, ora)
    st, last = sim.stats(), sim.getParticles()
    sim.destroy()
    assert st["sort_passes"] == 3    # the first binning + two re-binning launches
    assert st["outbox_items"] == 2 * carrying and st["outbox_full_items"] == 0
    assert same_bits(first["position"], last["position"]) and same_bits(first["velocity"], last["velocity"])
    assert np.array_equal(first["alive"], last["alive"])
