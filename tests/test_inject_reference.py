"""The numpy rule of the particle sources (tests/inject_reference.py) and the scenes (tests/inject_scenes.py) on the CPU:
hand-made cases of the sequence numbers and the tallies, the volume kind as the loader's rule itself, the statistics and the
reach of the flux kind, and the conditions the GPU tests rely on."""
import math

import numpy as np
import pytest

import inject_reference as ir
import inject_scenes as sc
import load_reference as lr


def test_sequence_numbers_by_hand():
    assert list(ir.sequence(10, 3)) == [10, 11, 12]
    assert list(ir.sequence(10, 3, k=2)) == [16, 17, 18]
    assert list(ir.sequence(10, 3, k=2, epoch=5)) == [31, 32, 33]
    assert ir.sequence(1, (1 << 31) - 1, k=1)[-1] == (1 << 32) - 2          # first + count = 2^32 - 1: the loader's bound, met exactly
    assert ir.sequence(2, (1 << 31) - 1, k=1) is None and ir.sequence(0, 1, epoch=1 << 32) is None
    assert ir.fits(5, 8, 5, 3) and not ir.fits(5, 8, 5, 4) and not ir.fits(0, 1 << 40, (1 << 32) - 3, 3) and ir.fits(0, 1 << 40, (1 << 32) - 4, 3)


def test_volume_is_the_loaders_rule():
    for kw in sc.VOLUME:
        req, want = ir.request(sc.L, sc.DT, **kw), lr.request(sc.L, **kw)
        j = ir.sequence(sc.N, 257, k=3)
        for T in (np.float32, np.float64):
            p, v = ir.stored(req, j, T)
            assert p.tobytes() == lr.stored_positions(want, j, T).tobytes() and v.tobytes() == lr.stored_velocities(want, j, T).tobytes()


def test_tally_by_hand():
    req = ir.request((1.0, 1.0, 1.0), 1e-9, vth=0.0, drift=(0.5, -0.25, 0.0))
    got = ir.application(req, ir.sequence(0, 3), np.float32, mass=2.0, charge=-3.0, weight=4.0)
    assert got["injected"] == 3 and got["energy_fixed"] == 3 * 5 * (1 << 76) and got["momentum_fixed"] == [3 << 79, -(3 << 78), 0]
    assert got["charge"] == -36.0 and got["momentum"][0] == 2.0 * 4.0 * ir.C * 1.5 and got["energy"] == 0.5 * 2.0 * 4.0 * ir.C * ir.C * (15 / 16)
    both = ir.add_results([got, got])
    assert both["applications"] == 2 and both["injected"] == 6 and both["momentum_fixed"][1] == -(3 << 79)


def test_flux_by_hand():
    """one particle, every operation spelled out"""
    L, dt = (2.0, 4.0, 8.0), 1e-9
    kw = dict(axis=1, side=-1, plane=1.0, seed=3, stream=4, vth=(0.1, 0.2, 0.3), drift=(0.01, 0.0, 0.02), lo=(0.5, 0.0, 0.0), hi=(1.5, 4.0, 8.0))
    req = ir.request(L, dt, kind="flux", **kw)
    j = np.array([41], dtype=np.uint64)
    f = lr.fractions(req, j)[0]
    r1, c, s, r3, _ = (x[0] for x in lr.normal_parts(req, j))
    vy = -(0.2 * r3)
    want_v = [0.01 + 0.1 * (r1 * c), vy, 0.02 + 0.3 * (r1 * s)]
    want_p = [0.5 / 2.0 + f[0] * (1.0 / 2.0), 1.0 / 4.0 + (vy * ((dt * ir.C) / 4.0)) * f[1], 0.0 + f[2] * 1.0]
    p, v = ir.states(req, j)
    assert list(p[0]) == want_p and list(v[0]) == want_v and vy < 0


@pytest.mark.parametrize("kw", sc.FLUX)
def test_flux_statistics_and_reach(kw):
    req = ir.request(sc.L, sc.DT, kind="flux", **kw)
    n = 100000
    j = ir.sequence(1000, n)
    s = ir.normal_speed(req, j)
    # the flux-weighted half-Maxwellian: a Rayleigh deviate, mean sqrt(pi/2), variance 2 - pi/2
    assert abs(s.mean() - math.sqrt(math.pi / 2)) <= 4 * math.sqrt((2 - math.pi / 2) / n)
    assert np.all(s > 0) and s.max() <= 6.76
    p, v = ir.states(req, j)
    ax, vth = req["axis"], req["vth"][req["axis"]]
    assert np.all(v[:, ax] * req["side"] > 0)
    assert abs(np.abs(v[:, ax]).mean() - vth * math.sqrt(math.pi / 2)) <= 4 * vth * math.sqrt((2 - math.pi / 2) / n)
    reach = vth * 6.76 * sc.DT * ir.C / sc.L[ax]
    d = (p[:, ax] - req["plane_f"]) * req["side"]
    assert np.all(d >= 0) and np.all(d <= reach) and d.max() > 0.1 * reach / 6.76
    # the tangential components are the loader's first two normals: independent of the normal speed
    for t, col in ((req["t1"], 0), (req["t2"], 1)):
        assert np.array_equal(v[:, t], req["drift"][t] + req["vth"][t] * lr.normals(req, j)[:, col])
        assert abs(np.corrcoef(np.abs(v[:, t] - req["drift"][t]), s)[0, 1]) < 4 / math.sqrt(n)
        lo, w = req["lo_f"][t], req["w_f"][t]
        assert np.all(p[:, t] >= lo) and np.all(p[:, t] <= lo + w)


def test_scenes_meet_their_conditions():
    assert sc.THREADS % 64 == 0 and sc.GROUP == 4 and sc.CHUNK == sc.THREADS * sc.GROUP and sc.STRIDE == sc.BLOCKS * sc.CHUNK
    assert sc.N % sc.GROUP != 0                     # the new slots start inside a lane's vector
    for s in sc.SCENES:
        assert 0 < s["count"] and s["n"] + s["count"] <= s["capacity"]
        req = ir.request(sc.L, sc.DT, kind=s["kind"], **{k: s[k] for k in ("axis", "side", "plane") if k in s}, **sc.load_request(s))
        p, v = ir.stored(req, ir.sequence(s["first"], s["count"]), np.float32)
        assert np.all(p >= 0) and np.all(p < 1) and np.all(np.isfinite(v))
    counts = sc.boundary_counts()
    head = (-sc.N) % sc.GROUP
    for edge in (head, sc.GROUP, sc.CHUNK - sc.N % sc.CHUNK, sc.STRIDE - sc.N % sc.STRIDE):
        assert {edge - 1, edge, edge + 1} - {0} <= set(counts)
    assert 1 in counts and all(c > 0 for c in counts)
    # straddles: the range ends one short of, on and one past a vector, a workgroup's turn and the grid's turn
    ends = {(sc.N + c) % sc.GROUP for c in counts}
    assert ends == {0, 1, 2, 3}
    assert any((sc.N + c) % sc.CHUNK == 0 for c in counts) and any((sc.N + c) % sc.STRIDE == 0 for c in counts)


def test_the_fast_tally_is_the_exact_one():
    import remove_reference as rr
    rng = np.random.default_rng(3)
    v = rng.normal(0, 0.05, (3000, 3))
    v[:40] *= 1e-9                       # terms below 2^-27: the floor of a right shift, negative ones included
    v[40:50] = 0.0
    v[50] = (100.0, -140.0, 30.0)        # near the top of the range
    v[51] = (-2.0 ** -70, 2.0 ** -81, -2.0 ** -90)
    for T in (np.float32, np.float64):
        want, nan = rr.tally(v.astype(T), np.ones(len(v), dtype=bool))
        assert not any(nan) and ir.tally_fast(v.astype(T)) == want
