"""The numpy restatement of the ionisation rule (tests/ionize_reference.py) proved on the CPU: hand-made cases, the energy
the two electrons share, the share word's mean, the statistics of a cold beam, the threshold case, the order of the ranks —
and, on the reference alone, the CONDITIONS of every scene tests/test_gpu_ionize.py compares exactly (tests/ionize_scenes.py):
no candidate's acceptance within 1e-9 x_max of its threshold, no candidate's g within 1e-9 of an end of the table or of
g_threshold, events where events are meant, one scene with none and one with exactly one."""
import math

import numpy as np
import pytest

import gas_reference as gref
import ionize_reference as ref
import ionize_scenes as sc
from test_gas_reference import DT, G_HI, G_LO, L, TABLE, density_for, scene


def test_the_words_are_this_operators_own():
    req = ref.request(L, **sc.SCENES["whole"])
    ids = np.arange(1000)
    mine = ref.words(req, ids, 0)
    gas = gref.words(req, ids, 0)                 # the same seed, stream and epoch under the gas operator's tag
    assert ref.TAG == 0x1051E0 and gref.TAG == 0x6A500
    assert not any(np.array_equal(a, b) for a, b in zip(mine, gas))
    for b in (1, 2):
        assert not np.array_equal(ref.words(req, ids, b)[0], mine[0])


def hand_request(**kw):
    """a cold gas at rest, a flat table that covers every speed up to 0.5 c, P_max = 1: everybody is a candidate"""
    base = dict(g_threshold=0.1, density=1e32, tau=DT, sigma=np.full(2, 3e-19), g_lo=0.1, g_hi=0.5, drift=0.0, vth=0.0, seed=7, stream=1, epoch=2)
    base.update(kw)
    return ref.request(L, **base)


def test_hand_made_cases():
    req = hand_request()
    assert req["K"] == 1 << 32 and req["thr"] == 0.1
    ids = np.arange(8)
    pos = np.full((8, 3), 0.5)
    v = np.zeros((8, 3))
    v[:, 0] = [0.05, 0.1, 0.3, 0.5, 0.6, 0.2, 0.2, np.nan]
    out = ref.apply(req, ids, pos, v)
    assert out["candidate"].all()
    assert out["below"].tolist() == [True] + [False] * 7                        # g < g_lo
    assert out["above"].tolist() == [False, False, False, True, True, False, False, True]   # g >= g_hi, and a NaN
    assert np.array_equal(out["g"][:7], np.abs(v[:7, 0])) and np.all(out["vb"] == 0.0)
    # the acceptance: x / x_max = g / g_hi against u = (w1 + 0.5) 2^-32
    u = (ref.words(req, ids, 0)[1].astype(np.float64) + 0.5) * 2.0 ** -32
    live = ~out["below"] & ~out["above"]
    assert np.array_equal(out["event"], live & (u * req["x_max"] < np.minimum((req["column"] * 3e-19) * out["g"], req["x_max"])))
    # the outcome of particle 2, by hand
    r = (int(ref.words(req, [2], 2)[0][0]) + 0.5) * 2.0 ** -32
    gp2 = 0.3 * 0.3 - 0.1 * 0.1
    assert out["gp2"][2] == gp2 and out["g1"][2] == math.sqrt(r * gp2) and out["g2"][2] == math.sqrt(gp2 - r * gp2)
    n1 = ref.nhat(ref.words(req, [2], 0)[2], ref.words(req, [2], 0)[3])[0]
    assert np.array_equal(out["v1"][2], 0.0 + out["g1"][2] * n1)
    assert abs(float(n1 @ n1) - 1.0) < 1e-15
    # a window: a projectile outside is no candidate whatever its word
    req = hand_request(lo=(0.0, 0.0, 0.0), hi=(L[0] / 2, L[1], L[2]))
    pos2 = np.full((8, 3), 0.25)
    pos2[::2, 0] = 0.5                                          # on hi_f: outside
    assert np.array_equal(ref.apply(req, ids, pos2, v)["candidate"], np.arange(8) % 2 == 1)


def test_the_electrons_share_the_energy_above_the_threshold():
    """per event |v' - vb|^2 + |vs - vb|^2 = g^2 - g_threshold^2 within a few spacings"""
    for name in ("window", "dense"):
        n = 100003 if name == "window" else 4101
        req, out = sc.reference(name, n)
        ev = out["event"]
        assert ev.sum() > 400
        a = ((out["v1"] - out["vb"]) ** 2).sum(axis=1)[ev] + ((out["vs"] - out["vb"]) ** 2).sum(axis=1)[ev]
        want = (out["g"] ** 2 - req["thr"] ** 2)[ev]
        # the roots, the unit vectors (|nhat|^2 = 1 within 2 ulps), the differences against vb of the size of the velocities
        scale = np.maximum(want, (np.abs(out["vb"]).max(axis=1) ** 2)[ev])
        assert np.all(np.abs(a - want) <= 32 * np.spacing(scale)), float((np.abs(a - want) / np.spacing(scale)).max())
        assert np.all(out["gp2"][ev] >= 0) and np.all(out["g1"][ev] >= 0) and np.all(out["g2"][ev] >= 0)


def test_the_share_word_is_uniform():
    req = ref.request(L, **sc.SCENES["whole"])
    r = ref.share(req, np.arange(100000))
    assert 0 < r.min() and r.max() < 1
    assert abs(r.mean() - 0.5) <= 4 * math.sqrt(1.0 / 12.0 / len(r))


def test_cold_beam_event_count_is_binomial():
    """a cold beam of speed g in a cold gas at rest: every projectile has the event probability (K 2^-32) sigma(g) g column / x_max"""
    n, g = 200000, 0.12
    kw = dict(g_threshold=0.04, density=density_for(0.3 * 2.0 ** 32, TABLE, G_LO, G_HI), tau=DT, sigma=TABLE, g_lo=G_LO, g_hi=G_HI, drift=0.0, vth=0.0, seed=99, stream=4, epoch=11)
    req = ref.request(L, **kw)
    v = np.zeros((n, 3))
    v[:, 2] = g
    out = ref.apply(req, np.arange(n), np.full((n, 3), 0.5), v)
    import fusion_reference as uref
    x = (req["column"] * float(uref.sigma_at(req["table"], np.array([g]))[0])) * g
    p = (req["K"] * 2.0 ** -32) * (x / req["x_max"])
    m = int(out["event"].sum())
    assert 0.01 < p < 0.5 and abs(m - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (m, n * p)
    assert np.all(out["g"] == g)


def test_an_event_at_the_threshold_leaves_both_electrons_at_rest_in_the_gas_frame():
    req = hand_request(g_threshold=0.1, g_lo=0.1, drift=(0.01, 0.0, -0.02))
    n = 64
    v = np.tile(np.array([0.01, 0.1, -0.02]), (n, 1))          # d = (0, 0.1, 0) exactly: g == g_lo == g_threshold
    out = ref.apply(req, np.arange(n), np.full((n, 3), 0.5), v)
    ev = out["event"]
    assert np.all(out["g"] == 0.1) and not out["below"].any() and ev.any()
    assert np.all(out["gp2"][ev] == 0) and np.all(out["g1"][ev] == 0) and np.all(out["g2"][ev] == 0)
    assert np.array_equal(out["v1"][ev], out["vb"][ev]) and np.array_equal(out["vs"][ev], out["vb"][ev])


def test_the_rank_order_is_a_sort_by_primary_id():
    rng = np.random.default_rng(5)
    ids = rng.permutation(5000)[:3000] * 7 + 3               # thinned, shuffled ids
    event = rng.random(3000) < 0.3
    rank = ref.ranks(ids, event)
    assert np.all(rank[~event] == -1)
    by_id = sorted(int(i) for i in ids[event])
    assert [by_id[r] for r in rank[event]] == [int(i) for i in ids[event]]
    # an application places the new rows by rank, with the primary's stored position
    frac, vel = scene(4101)
    req = ref.request(L, **sc.DENSE)
    perm = rng.permutation(4101)
    app = ref.application(req, np.arange(4101)[perm], frac[perm].astype(np.float32), vel[perm].astype(np.float32), 10, 20, 30, 40)
    m = app["m"]
    assert m == int(app["event"].sum()) > 1000
    assert np.array_equal(app["electron"]["slot"], 10 + np.arange(m)) and np.array_equal(app["electron"]["id"], 20 + np.arange(m))
    assert np.array_equal(app["ion"]["slot"], 30 + np.arange(m)) and np.array_equal(app["ion"]["id"], 40 + np.arange(m))
    primaries = np.sort(np.arange(4101)[perm][app["event"]])
    assert np.array_equal(app["electron"]["position"], frac[primaries].astype(np.float32))
    # ... and does not depend on the order of the slots
    same = ref.application(req, np.arange(4101), frac.astype(np.float32), vel.astype(np.float32), 10, 20, 30, 40)
    for who in ("electron", "ion"):
        for key in ("position", "velocity", "id", "slot"):
            assert np.array_equal(app[who][key], same[who][key])
    assert app["primary"] == same["primary"] and app["electron_gain"] == same["electron_gain"] and app["ion_gain"] == same["ion_gain"]


def test_the_fit_rule():
    assert ref.fits(10, 15, 10, 5) and not ref.fits(10, 14, 10, 5)
    assert ref.fits(10, 1 << 33, ref.ID_END - 5, 5) and not ref.fits(10, 1 << 33, ref.ID_END - 4, 5)


# ---- the conditions of the scenes the GPU test compares exactly
@pytest.mark.parametrize("name", sorted(sc.SCENES) + sorted(sc.SPARSE))
def test_conditions_of_the_exact_scenes(name):
    sizes = [n for s, n in sc.exact_cases() if s == name]
    assert sizes
    for n in sizes:
        req, out = sc.reference(name, n)
        assert ref.margins_hold(req, out), (name, n)


def test_conditions_of_the_threshold_scenes():
    lo, hi = sc.compact_range()
    for name, kw in sc.THRESHOLD_SCENES.items():
        req, out = sc.reference(name, sc.THRESHOLD_N)
        assert ref.margins_hold(req, out), name
        assert out["event"].sum() >= 5, name
        k = int(name.split()[1])
        assert (lo <= req["K"] <= hi) == (k in (1, 2, 3)), (name, req["K"])
    assert 0.375 < sc.window_first_max() < 0.5625


def test_the_scenes_have_the_events_they_are_meant_to_have():
    for name, n in [(s, n) for s, n in sc.exact_cases() if n >= 100003 and s in sc.SCENES]:
        assert sc.reference(name, n)[1]["event"].sum() > 400, (name, n)
    got = [int(sc.reference("dense", n)[1]["event"].sum()) for n in sc.DENSE_SIZES]
    # past a lane's vector, a wave, a workgroup of the generation pass, the queue — each below the next boundary
    for m, lo, hi in zip(got, sc.EVENT_BOUNDS, sc.EVENT_BOUNDS[1:] + [1 << 30]):
        assert lo < m <= hi, (got, sc.EVENT_BOUNDS)
    assert sc.DENSE_SIZES[-1] > sc.SCAN_CHUNK and all(n % 32 for n in sc.DENSE_SIZES)      # more than one chunk of the scan; ragged id spans
    none, one = sc.reference("no event", sc.SPARSE_N)[1], sc.reference("one event", sc.SPARSE_N)[1]
    assert none["event"].sum() == 0 and none["candidate"].sum() > 0
    assert one["event"].sum() == 1
    assert sc.reference("at threshold", 100003)[0]["thr"] == sc.reference("at threshold", 100003)[0]["table"]["g_lo"]
