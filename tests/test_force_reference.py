"""The numpy restatement of the rule of the prescribed external forces (tests/force_reference.py) proved on the CPU: its
closed-form cases, and — on the reference alone — the conditions the scenes of tests/test_gpu_force.py must meet, so that
the GPU comparison reaches every path of the kernel: particles on either side of the window and exactly on its faces, groups
of four slots of which one to three are inside, the first and the last interval of every taper table, and sub-steps before,
on, between and after the nodes of the envelope.  The scenes are defined here and imported by the GPU test.

Positions are multiples of 2^-20 of a box whose edges are powers of two, so a handle of either precision stores exactly the
fractions the reference is given."""
import math

import numpy as np
import pytest

import energy_reference as eref
import force_reference as ref

ME, MP, QE = 9.109e-31, 1.6726e-27, 1.602e-19
SHAPE = (8, 8, 8)
L = (2.0 ** -7, 2.0 ** -7, 2.0 ** -7)          # metres: L / 4 and 3 L / 4 are exact, and so are the fractions 1/4 and 3/4
DT = 5e-12
SPECIES = [dict(mass=ME, charge=-QE), dict(mass=2 * MP, charge=2 * QE)]
GRID = 2.0 ** -20
N_SMALL = 4099

WINDOW = dict(lo=(L[0] / 4, 0.0, 0.0), hi=(3 * L[0] / 4, L[1], 3 * L[2] / 4))
# (stored fractions) 0: on lo_f, counted; 1: on hi_f, not counted; 2: on hi_f of z, not counted; 3: on lo_f of z, counted;
# 4, 5: the first and the last interval of the x table; 6, 7: of the z table
PLANTED = np.array([[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [0.5, 0.5, 0.75], [0.5, 0.5, 0.0],
                    [0.25 + GRID, 0.5, 0.25], [0.75 - GRID, 0.5, 0.25], [0.5, 0.5, GRID], [0.5, 0.5, 0.75 - GRID]])


def dyadic_table(nodes, seed):
    """nodes that are multiples of 1/16 in [0, 2]"""
    return np.random.default_rng(seed).integers(0, 33, nodes).astype(np.float64) / 16.0


def smooth_table(nodes, seed):
    x = np.linspace(0.0, 1.0, nodes)
    rng = np.random.default_rng(seed)
    return 0.25 + np.sin(math.pi * x) ** 2 + 0.1 * rng.random(nodes)


TAPER_DYADIC = (dyadic_table(1025, 1), dyadic_table(2, 2), dyadic_table(1025, 3))
TAPER_SMOOTH = (smooth_table(1025, 4), np.array([0.5, 1.5]), smooth_table(1025, 5))
ONE_PLAIN = [dict(amp=(2.0e6, -1.0e6, 0.5e6))]
FOUR_WAVES = [dict(amp=(1.5e6, 0.0, -0.7e6), mode=(1, 0, 0), nu=0.013, phase=0.1),
              dict(amp=(0.0, 2.0e6, 0.3e6), mode=(0, 2, -1), nu=-0.27, phase=0.0),
              dict(amp=(0.4e6, 0.4e6, 0.4e6), mode=(3, 1, 2), nu=0.0, phase=0.625),
              dict(amp=(-1.0e6, 0.2e6, 0.0), mode=(-2, 0, 5), nu=1.75, phase=-0.3)]
ENVELOPE = dict(start=5, stop=13, values=[0.0, 1.0, 0.5, 2.0, 0.25])    # nodes at s = 5, 7, 9, 11, 13
ENVELOPE_EPOCH = 2                                                       # s = sub-step + 2: active for the sub-steps 3 .. 11
ENVELOPE_SUBSTEPS = 13

_scene = {}


def scene(n, seed=1):
    """stored fractions [n][3] (multiples of 2^-20 in [0, 1), the planted particles first) and velocities [n][3] (units of
    c, exact in float32), computed once per (n, seed) and never changed"""
    key = (n, seed)
    if key not in _scene:
        rng = np.random.default_rng(seed)
        frac = rng.integers(0, 1 << 20, (n, 3)).astype(np.float64) * GRID
        frac[:len(PLANTED)] = PLANTED
        vel = rng.normal(0.0, 0.05, (n, 3)).astype(np.float32).astype(np.float64)
        frac.setflags(write=False)
        vel.setflags(write=False)
        _scene[key] = (frac, vel)
    return _scene[key]


def request(species, waves, **kw):
    sp = SPECIES[species]
    return ref.request(L, DT, sp["charge"], sp["mass"], waves, **kw)


# ---- the closed-form cases
def test_a_uniform_field_adds_kq_amp():
    frac, vel = scene(N_SMALL)
    for species in (0, 1):
        for kind in (ref.FIELD, ref.ACCEL):
            req = request(species, ONE_PLAIN, kind=kind)
            sp = SPECIES[species]
            kq = DT / ref.C if kind == ref.ACCEL else (sp["charge"] * DT) / (sp["mass"] * ref.C)
            out = ref.kicked(req, 7, frac, vel)
            assert out["inside"].all() and out["active"]
            assert np.array_equal(out["v"], vel + kq * np.array(ONE_PLAIN[0]["amp"])[None, :])
    assert request(0, ONE_PLAIN)["kq"] != request(1, ONE_PLAIN)["kq"]
    assert request(0, ONE_PLAIN, kind=ref.ACCEL)["kq"] == request(1, ONE_PLAIN, kind=ref.ACCEL)["kq"]


def test_quarter_and_half_waves():
    req = ref.request((1.0, 1.0, 1.0), 1.0, ref.C, 1.0, [dict(amp=(1.0, 0.0, 0.0), mode=(1, 0, 2), nu=0.25, phase=0.125)])
    p = np.array([[0.125, 0.7, 0.125], [0.375, 0.1, 0.125], [0.125, 0.1, 0.0]])
    v = np.full((3, 3), 0.5)
    assert ref.tfrac(req, 1) == [0.25] and req["kq"] == 1.0
    out = ref.kicked(req, 1, p, v)
    assert list(out["v"][:, 0]) == [0.5, -0.5, 1.5] and np.all(out["v"][:, 1:] == 0.5)
    assert list(out["c"][:, 0]) == [0.0, -1.0, 1.0]


def test_tfrac_activity_and_the_envelope():
    w = lambda nu: ref.request(L, DT, 1.0, 1.0, [dict(amp=1.0, nu=nu)])
    assert ref.tfrac(w(0.25), 3) == [0.75] and ref.tfrac(w(0.5), (1 << 40) + 1) == [0.5] and ref.tfrac(w(-0.25), 1) == [0.75]
    assert ref.tfrac(w(0.125), (1 << 52) + 3) == [0.375] and ref.tfrac(w(1.0), (1 << 64) - 1) == [0.0]
    req = ref.request(L, DT, 1.0, 1.0, [dict(amp=1.0, nu=0.25)], epoch=(1 << 64) - 2)            # s wraps: count 5 is s = 3
    assert ref.s_of(req, 5) == 3 and ref.tfrac(req, 5) == [0.75]
    req = ref.request(L, DT, 1.0, 1.0, [dict(amp=1.0)], envelope=dict(start=3, stop=11, values=[0.0, 1.0, 0.5, 2.0, -1.0]))
    assert [ref.active(req, s) for s in (2, 3, 11, 12)] == [False, True, True, False]
    assert [ref.envelope_value(req, s) for s in (3, 4, 5, 6, 7, 9, 10, 11)] == [0.0, 0.5, 1.0, 0.75, 0.5, 2.0, 0.5, -1.0]
    frac, vel = scene(64)
    off = ref.kicked(req, 2, frac, vel)
    assert not off["active"] and not off["inside"].any() and np.array_equal(off["v"], vel)
    assert np.array_equal(ref.kicked(req, 3, frac, vel)["v"], vel)                               # the node 0 of the table is zero: a kick of zero
    assert ref.kicked(req, 3, frac, vel)["inside"].all()


def test_lookup_at_zero_on_a_node_and_in_the_last_interval():
    tab = np.array([1.0, 3.0, 2.0, 6.0, 4.0])
    val, j = ref.lookup(tab, np.array([0.0, 0.25, 0.5, 0.75, 0.875, 1.0, 0.125]))
    assert list(val) == [1.0, 3.0, 2.0, 6.0, 5.0, 4.0, 2.0] and list(j) == [0, 1, 2, 3, 3, 3, 0]
    big = np.arange(1025) * 0.5
    val, j = ref.lookup(big, np.array([1023.5 / 1024]))
    assert val[0] == 511.75 and j[0] == 1023
    # the taper is (tx ty) tz over the window's fractions
    req = ref.request((1.0, 1.0, 1.0), 1.0, 1.0, 1.0, [dict(amp=1.0)], lo=(0.25, 0, 0), hi=(0.75, 1, 1), taper=(tab, None, [-2.0, 2.0]))
    t, js = ref.taper_value(req, np.array([[0.25 + 0.5 * 0.875, 0.3, 0.75], [0.25, 0.9, 0.0]]))
    assert list(t) == [5.0, -2.0] and list(js[0]) == [3, 0] and js[1] is None


def test_tallies_are_the_exact_integers():
    frac, vel = scene(257)
    req = request(0, FOUR_WAVES, taper=TAPER_SMOOTH, **WINDOW)
    for dtype in (np.float32, np.float64):
        before = vel.astype(dtype)
        after, k = ref.stored(req, 4, frac, before)
        t = ref.tallies(before, after, k["inside"])
        ins = np.flatnonzero(k["inside"])
        work = sum(eref.fix_floor_scalar(eref.v_squared(after[i:i + 1])[0]) - eref.fix_floor_scalar(eref.v_squared(before[i:i + 1])[0]) for i in ins)
        imp = [sum(eref.fix_floor_fraction(float(after[i, a])) - eref.fix_floor_fraction(float(before[i, a])) for i in ins) for a in range(3)]
        assert t == dict(kicked=len(ins), work_fixed=work, impulse_fixed=imp) and 0 < len(ins) < 257
        assert after.dtype == dtype and np.array_equal(after[~k["inside"]], before[~k["inside"]]) and (after[k["inside"]] != before[k["inside"]]).any(axis=1).all()
        d = ref.derived(t, ME, 1e9)
        assert d["work"] == 0.5 * ME * 1e9 * ref.C * ref.C * (float(work) * 2.0 ** -80) and d["impulse"][2] == ME * 1e9 * ref.C * (float(imp[2]) * 2.0 ** -80)
    assert ref.add_tallies(t, ref.ZERO) == t


# ---- what the GPU scenes must meet
@pytest.mark.parametrize("n", [N_SMALL, 70001])
def test_the_window_scene_reaches_every_path(n):
    frac, vel = scene(n)
    assert frac.min() >= 0 and frac.max() < 1 and np.array_equal(frac, frac.astype(np.float32).astype(np.float64))
    req = request(0, FOUR_WAVES, taper=TAPER_SMOOTH, **WINDOW)
    assert list(req["lo_f"]) == [0.25, 0.0, 0.0] and list(req["hi_f"]) == [0.75, 1.0, 0.75] and list(req["w"]) == [0.5, 1.0, 0.75]
    out = ref.kicked(req, 4, frac, vel)
    ins = out["inside"]
    assert 0.25 <= ins.mean() <= 0.75
    groups = ins[:n - n % 4].reshape(-1, 4).sum(axis=1)
    assert set(groups) == {0, 1, 2, 3, 4}                                   # groups of four slots with none, some and all inside
    assert n % 4 != 0                                                       # and a ragged last group
    assert list(ins[:8]) == [True, False, False, True, True, True, True, True]
    assert list(frac[0]) == [0.25, 0.5, 0.5] and list(frac[1]) == [0.75, 0.5, 0.5] and frac[2, 2] == 0.75 and frac[3, 2] == 0.0
    for a in (0, 1, 2):
        K = len(TAPER_SMOOTH[a]) - 1
        js = out["taper_j"][a][ins]
        assert js.min() == 0 and js.max() == K - 1, a                       # the first and the last interval hold a particle
    assert {len(t) for t in TAPER_SMOOTH} == {2, 1025} == {len(t) for t in TAPER_DYADIC}
    assert all(np.array_equal(t * 16, np.round(t * 16)) for t in TAPER_DYADIC)
    assert np.abs(out["d"][ins]).max() > 1e-4 and np.isfinite(out["v"]).all()


def test_the_envelope_scene_has_every_kind_of_substep():
    req = request(0, ONE_PLAIN, envelope=ENVELOPE, epoch=ENVELOPE_EPOCH)
    kinds = set()
    for k in range(1, ENVELOPE_SUBSTEPS + 1):
        s = ref.s_of(req, k)
        if s < ENVELOPE["start"]:
            kinds.add("before")
        elif s > ENVELOPE["stop"]:
            kinds.add("after")
        else:
            g = (s - ENVELOPE["start"]) * (len(ENVELOPE["values"]) - 1) / (ENVELOPE["stop"] - ENVELOPE["start"])
            kinds.add("node" if g == int(g) else "between")
        assert ref.active(req, k) == (3 <= k <= 11)
    assert kinds == {"before", "node", "between", "after"}
    assert [ref.envelope_value(req, k) for k in (3, 4, 5, 11)] == [0.0, 0.5, 1.0, 0.25]
