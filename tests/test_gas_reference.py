"""The numpy restatement of the rule of the windowed background collisions (tests/gas_reference.py) proved on the CPU: the
interval-wise candidate bound, the statistics of a cold beam, the scene properties — and, on the reference alone, the margins
of every scene tests/test_gpu_gas.py compares exactly, so that the GPU comparison of the decisions leaves no case out: no
candidate's acceptance lies within 1e-9 x_max of its threshold and no candidate's g within 1e-9 of an end of the table, far
outside what the device's rounded functions (the normals, cospi, sinpi: a few ulps) can move.  The scenes are defined here and
imported by the GPU test; reference() computes each once and never changes it.

Positions are multiples of 2^-20 of a box whose edges are powers of two and velocities are exact in float32, so a handle of
either precision stores exactly what the reference is given."""
import math
import os
import re

import numpy as np
import pytest

import gas_reference as ref
from helpers import ROOT

ME, QE = 9.109e-31, 1.602e-19
SHAPE = (16, 16, 16)
L = (2.0 ** -6, 2.0 ** -6, 2.0 ** -6)          # metres: the eighths of an edge are exact, and so are their fractions
DT = 5e-12
GRID = 2.0 ** -20
SIZES = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 100003]

# 0.75 x 1 x 0.5 = 0.375 of the box, dyadic edges; WIDE: 0.75 x 1 x 0.75 = 0.5625 (the other side of kGasWindowFirstMax)
WINDOW = dict(lo=(L[0] / 8, 0.0, L[2] / 4), hi=(7 * L[0] / 8, L[1], 3 * L[2] / 4))
WINDOW_WIDE = dict(lo=(L[0] / 8, 0.0, 0.0), hi=(7 * L[0] / 8, L[1], 3 * L[2] / 4))
# (stored fractions) 0: on lo_f of x, inside; 1: on hi_f of x, outside; 2: on hi_f of z, outside; 3: on lo_f of z, inside;
# 4, 5: the first and the last interval of the x taper; 6, 7: of the z taper
PLANTED = np.array([[0.125, 0.5, 0.5], [0.875, 0.5, 0.5], [0.5, 0.5, 0.75], [0.5, 0.5, 0.25],
                    [0.125 + GRID, 0.5, 0.5], [0.875 - GRID, 0.5, 0.5], [0.5, 0.5, 0.25 + GRID], [0.5, 0.5, 0.75 - GRID]])
BACKGROUND = dict(drift=(0.01, 0.0, -0.02), vth=(0.05, 0.02, 0.1))


def taper_table(nodes, seed):
    x = np.linspace(0.0, 1.0, nodes)
    return np.clip(0.15 + 0.8 * np.sin(math.pi * x) ** 2 + 0.05 * np.random.default_rng(seed).random(nodes), 0.0, 1.0)


TAPERS = (taper_table(1025, 4), None, taper_table(9, 5))


def power_law_with_resonance(n, g_lo, g_hi):
    g = np.linspace(g_lo, g_hi, n)
    return 2.0e-19 * (g_lo / g) ** 1.5 + 6.0e-19 * np.exp(-0.5 * ((g - 0.12) / 0.004) ** 2)


G_LO, G_HI = 0.05, 0.25
TABLE = power_law_with_resonance(96, G_LO, G_HI)
TABLE.setflags(write=False)


def density_for(K, sigma, g_lo, g_hi, tau=DT):
    """the density at which a request has (within a few units) the candidate word bound K"""
    x = -math.log1p(-K * 2.0 ** -32)
    return x / (ref.C * tau * ref.bound(sigma, g_lo, g_hi))


def gas(kind, K, seed, stream=0, epoch=0, sigma=TABLE, g_lo=G_LO, g_hi=G_HI, **kw):
    """the keywords of a request, as both the wrapper and the reference take them"""
    out = dict(density=density_for(K, sigma, g_lo, g_hi), tau=DT, sigma=sigma, g_lo=g_lo, g_hi=g_hi, seed=seed, stream=stream, epoch=epoch, **BACKGROUND)
    if kind == "elastic":
        out["mass_ratio"] = 2.0
    out.update(kw)
    return out


def compact_range():
    """kGasCompactMin, kGasCompactMax of the kernel header: the K between which the queue serves a request"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_gas_kernels.hpp")).read()
    m = re.search(r"kGasCompactMin\s*=\s*1ull\s*<<\s*(\d+)\s*,\s*kGasCompactMax\s*=\s*1ull\s*<<\s*(\d+)\s*;", text)
    return 1 << int(m.group(1)), 1 << int(m.group(2))


def window_first_max():
    """kGasWindowFirstMax of the kernel header: the share of the box's volume below which the window is tested first"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_gas_kernels.hpp")).read()
    return float(re.search(r"constexpr\s+double\s+kGasWindowFirstMax\s*=\s*([0-9.eE+-]+)\s*;", text).group(1))


P30 = 0.3 * 2.0 ** 32
# the scenes of the exact comparison: name -> (kind, keywords).  The first two: test 1 (every size, sorted and unsorted).
SCENES = {
    "exchange": ("exchange", gas("exchange", P30, 0x6A5000123456789, stream=5, epoch=3, taper=TAPERS, **WINDOW)),
    "elastic": ("elastic", gas("elastic", P30, 0x6A5000123456790, stream=6, epoch=4, taper=TAPERS, **WINDOW)),
}


def threshold_scenes():
    """requests on either side of every threshold the host chooses a form by (test 4): K just below, just above and between
    the two ends of the queue's range, in a window on either side of kGasWindowFirstMax and on the whole box"""
    lo, hi = compact_range()
    out = {}
    for k, (target, inside) in enumerate(((lo * 0.999, False), (lo * 1.001, True), ((lo * hi) ** 0.5, True), (hi * 0.999, True), (hi * 1.001, False))):
        for w, (name, window) in enumerate((("narrow", WINDOW), ("wide", WINDOW_WIDE), ("whole", {}))):
            kind = "exchange" if (k + w) % 2 == 0 else "elastic"
            out["K %d %s" % (k, name)] = (kind, gas(kind, target, 0xBADC0DE + 16 * k + w, stream=8, epoch=1, taper=TAPERS if w != 1 else (None, None, None), **window), inside)
    return out


THRESHOLD_SCENES = threshold_scenes()
_scene, _reference = {}, {}


def scene(n, seed=1):
    """stored fractions [n][3] (multiples of 2^-20 in [0, 1), the planted particles first) and velocities [n][3] (units of
    c, exact in float32), computed once per (n, seed) and never changed"""
    key = (n, seed)
    if key not in _scene:
        rng = np.random.default_rng(seed)
        frac = rng.integers(0, 1 << 20, (n, 3)).astype(np.float64) * GRID
        frac[:len(PLANTED)] = PLANTED[:n]
        vel = rng.normal(0.0, 0.05, (n, 3)).astype(np.float32).astype(np.float64)
        frac.setflags(write=False)
        vel.setflags(write=False)
        _scene[key] = (frac, vel)
    return _scene[key]


def code(kind):
    return dict(exchange=ref.EXCHANGE, elastic=ref.ELASTIC)[kind]


def reference(name, n):
    """(request, what the reference gives for scene(n)) of a scene of SCENES or THRESHOLD_SCENES: computed once, shared, unchanged"""
    key = (name, n)
    if key not in _reference:
        kind, kw = (SCENES.get(name) or THRESHOLD_SCENES[name])[:2]
        req = ref.request(L, code(kind), **kw)
        frac, vel = scene(n)
        _reference[key] = (req, ref.apply(req, np.arange(n), frac, vel))
    return _reference[key]


def margins_hold(req, out):
    c = out["candidate"]
    tab = req["table"]
    near_accept = np.abs(out["ux"] - out["x"])[c & out["live"]] < 1e-9 * req["x_max"]
    near_end = (np.abs(out["g"] - tab["g_lo"])[c] < 1e-9) | (np.abs(out["g"] - tab["g_hi"])[c] < 1e-9)
    return not near_accept.any() and not near_end.any()


# ---- the interval-wise bound
def bound_tables():
    g_lo, g_hi = 0.01, 0.4
    flat = np.full(17, 3.0e-19)
    falling = 5.0e-19 * (g_lo / np.linspace(g_lo, g_hi, 300)) ** 2
    resonance = 1e-22 + 8.0e-19 * np.exp(-0.5 * ((np.linspace(g_lo, g_hi, 4096) - 0.05) / 0.0005) ** 2)
    zeros = np.where((np.arange(40) // 5) % 2 == 0, 0.0, 4.0e-19)          # whole intervals of zeros between plateaus
    return dict(flat=flat, falling=falling, resonance=resonance, zeros=zeros), g_lo, g_hi


@pytest.mark.parametrize("name", ["flat", "falling", "resonance", "zeros"])
def test_the_interval_bound_holds(name):
    tables, g_lo, g_hi = bound_tables()
    S = tables[name]
    req = ref.request(L, ref.EXCHANGE, density=1e21, tau=1e-9, sigma=S, g_lo=g_lo, g_hi=g_hi)
    rng = np.random.default_rng(11)
    g = np.concatenate([rng.uniform(g_lo, g_hi, 99000), g_lo + (g_hi - g_lo) * (rng.integers(0, len(S) - 1, 998) + 1.0 - 2.0 ** -30) / (len(S) - 1), [g_lo, np.nextafter(g_hi, 0)]])
    g = g[(g >= g_lo) & (g < g_hi)]
    assert len(g) >= 99990
    for rho in (1.0, 0.37):
        x = ((req["column"] * rho) * ref.uref.sigma_at(req["table"], g)) * g          # not held to x_max
        assert np.all(x <= req["x_max"]), (name, rho, (x / req["x_max"]).max())
    # the bound is the interval-wise one: a resonance does not pay for its peak at every speed, a flat table pays g_hi
    if name == "resonance":
        assert req["x_max"] < 0.2 * req["column"] * S.max() * g_hi
    if name == "flat":
        assert req["x_max"] == req["column"] * (S[0] * g_hi)
    if name == "zeros":
        k = np.flatnonzero((S[:-1] == 0) & (S[1:] == 0))
        dg = (g_hi - g_lo) / (len(S) - 1)
        inside = g_lo + (k + 0.5) * dg
        assert len(k) > 8 and np.all(ref.uref.sigma_at(req["table"], inside) == 0)


# ---- the margins of the GPU test's scenes
def big_n():
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_gas_kernels.hpp")).read()
    get = lambda name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    return get("kGasBlocks") * get("kGasThreads") * 4 + 1027


@pytest.mark.parametrize("name", sorted(SCENES))
def test_margins_of_the_exact_scenes(name):
    for n in SIZES + [big_n()]:
        req, out = reference(name, n)
        assert margins_hold(req, out), (name, n)
        assert abs(req["K"] - P30) < 4
    req, out = reference(name, 100003)
    c = ref.counts(out)
    # every path is reached: outside and inside, candidates that are below, above, refused and accepted
    assert 0 < c["below"] and 0 < c["above"] and 0 < c["collided"] < c["candidates"] - c["below"] - c["above"] and c["candidates"] < out["inside"].sum() < 100003
    assert list(out["inside"][:8]) == [True, False, False, True, True, True, True, True]
    j = ref.fref.taper_value(req["window"], scene(100003)[0][:8])[1]
    assert (j[0][4], j[0][5], j[2][6], j[2][7]) == (0, 1023, 0, 7)
    groups = out["candidate"][:100000].reshape(-1, 4).sum(axis=1)
    assert set(np.unique(groups)) >= {0, 1, 2, 3}


def test_margins_of_the_threshold_scenes():
    lo, hi = compact_range()
    assert 0 < lo < hi < 1 << 32 and 0.375 < window_first_max() < 0.5625
    seen = set()
    for name, (kind, kw, inside) in THRESHOLD_SCENES.items():
        for n in SIZES:
            req, out = reference(name, n)
            assert margins_hold(req, out), (name, n)
        assert (lo <= req["K"] <= hi) == inside, name
        vol = float(np.prod(req["window"]["w"]))
        seen.add((inside, vol < window_first_max(), bool(np.all(req["window"]["w"] == 1.0))))
        assert ref.counts(out)["candidates"] > 0
    assert len(seen) == 6 and {s[0] for s in seen} == {True, False}


# ---- the statistics of a cold beam
def test_cold_beam_count():
    n = 400000
    S = power_law_with_resonance(64, 0.05, 0.25)
    kw = dict(density=density_for(0.5 * 2.0 ** 32, S, 0.05, 0.25), tau=DT, sigma=S, g_lo=0.05, g_hi=0.25, drift=(0.0, 0.0, 0.0), vth=0.0, seed=2026, stream=1, epoch=9)
    req = ref.request(L, ref.EXCHANGE, **kw)
    v = np.tile(np.array([[0.06, -0.08, 0.0]]), (n, 1))                      # g = 0.1 for everybody
    frac = np.random.default_rng(3).random((n, 3))
    out = ref.apply(req, np.arange(n), frac, v)
    g = out["g"]
    assert np.all(g == g[0]) and abs(g[0] - 0.1) < 1e-15 and out["inside"].all()
    x = float(out["x"][0])
    p = req["K"] * 2.0 ** -32 * x / req["x_max"]
    hits = int(out["collided"].sum())
    assert 0.01 < p < 0.5 and abs(hits - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (hits, n * p)
    assert np.all(out["v"][out["collided"]] == 0.0)                        # a cold background at rest: exchange stops the particle


# ---- scene properties
def test_a_taper_of_ones_equals_no_taper():
    n = 20000
    frac, vel = scene(n)
    ones = (np.ones(1025), np.ones(2), np.ones(9))
    for kind in ("exchange", "elastic"):
        kw = gas(kind, P30, 99, stream=2, epoch=1, **WINDOW)
        a = ref.apply(ref.request(L, code(kind), **kw), np.arange(n), frac, vel)
        b = ref.apply(ref.request(L, code(kind), **dict(kw, taper=ones)), np.arange(n), frac, vel)
        assert a["v"].tobytes() == b["v"].tobytes() and np.array_equal(a["collided"], b["collided"]) and a["collided"].sum() > 100
        assert a["x"].tobytes() == b["x"].tobytes()


def test_an_interval_of_zeros_gets_no_collision():
    n = 50000
    frac, vel = scene(n)
    S = TABLE.copy()
    S[20:41] = 0.0                                                          # the intervals 20 .. 39 are zero throughout
    req = ref.request(L, ref.EXCHANGE, **gas("exchange", 0.9 * 2.0 ** 32, 5, sigma=S))
    out = ref.apply(req, np.arange(n), frac, vel)
    dg = (G_HI - G_LO) / (len(S) - 1)
    dead = (out["g"] >= G_LO + 20 * dg + 1e-12) & (out["g"] < G_LO + 40 * dg - 1e-12)
    assert (dead & out["candidate"]).sum() > 1000 and not (dead & out["collided"]).any() and out["collided"].sum() > 1000
    # an all-zero table: K = 0, nobody is a candidate
    req = ref.request(L, ref.EXCHANGE, **dict(gas("exchange", P30, 5), sigma=np.zeros(8)))
    assert req["K"] == 0 and not ref.apply(req, np.arange(100), frac[:100], vel[:100])["candidate"].any()
    assert ref.request(L, ref.EXCHANGE, **dict(gas("exchange", P30, 5), density=0.0))["K"] == 0


def test_lo_is_inside_and_hi_is_outside():
    kw = gas("exchange", 2.0 ** 32 - 1, 7, **WINDOW)
    req = ref.request(L, ref.EXCHANGE, **dict(kw, density=1e30))              # P_max = 1: every particle inside is a candidate
    assert req["K"] == 1 << 32
    out = ref.apply(req, np.arange(8), PLANTED, np.zeros((8, 3)))
    assert list(out["candidate"]) == [True, False, False, True, True, True, True, True]
    assert list(req["window"]["lo_f"]) == [0.125, 0.0, 0.25] and list(req["window"]["hi_f"]) == [0.875, 1.0, 0.75]


def test_words_are_the_loaders_generator_at_a_tag_of_its_own():
    import collide_reference as cref
    import fusion_reference as uref
    assert ref.TAG == 0x6A500 and len({ref.TAG, ref.TAG + 1, cref.TAG, cref.TAG + 1, 0xC0120, uref.TAG, 0x10AD}) == 7
    req = ref.request(L, ref.EXCHANGE, **gas("exchange", P30, cref.SEED))
    ours = ref.words(req, np.arange(64), 0)
    theirs = cref.words(cref.request(cref.EXCHANGE, nu_tau=1.0, seed=cref.SEED), np.arange(64), 0)
    assert not any(np.array_equal(a, b) for a, b in zip(ours, theirs))
