"""The fusion yield tally (fpic_fusion*) on a machine WITHOUT a GPU: the header declares the entry points and libfusionpic.so
exports them, the ctypes mirrors have the C layout, the rule (fusion-sim_amd/csrc/fes_fusion_core.hpp) passes its g++ test and
agrees bit for bit with the integers of the numpy restatement (tests/fusion_reference.py) on random pairs — both also as a
stand-alone program under AddressSanitizer and UBSan —, the restatement has the pair sets, the table's edges and the fixed
point by hand, the Python wrapper builds the request, sigma_table samples a callable, a call without a handle fails cleanly,
and the restatement alone reproduces the reactivity <sigma v> of two Maxwellians.  The tally itself is checked on the GPU
(tests/test_gpu_fusion.py).

Reactivity, measured here (test_reactivity_of_two_maxwellians prints it): 8 cells of about 2000 deuterons and 2000 tritons at
10 keV with sigma(E) = (A / E) exp(-B / sqrt(E)), B = 34.38 keV^1/2, a table of 4096 points over 0.2 .. 300 keV.  Over 8
seeds the unlike tally is 0.9973 +- 0.0038 of the numpy quadrature of <sigma v>, the like tally 0.9975 +- 0.0097 of
half the quadrature (a cell has 1000 like pairs where it has 2000 unlike ones); halving n moves the tallies by 1.5e-6 of
themselves, the floors lose below 1e-10.  The tolerance is three of those standard errors plus that interpolation error plus
the floor's bound (one unit per pair), all computed in the test."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fusion_reference as ref
from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "fusionpic.h")
LIB = os.path.join(ROOT, "fusion-sim_amd", "lib", "libfusionpic.so")
NATIVE = os.path.join(ROOT, "tests", "native", "fusion_core_test.cpp")
SPEC = r"fpic_handle\s*\*\s*h\s*,\s*const\s+fpic_fusion_spec\s*\*\s*spec\s*,\s*"
ENTRIES = {
    "fpic_fusion": SPEC + r"fpic_fusion_result\s*\*\s*out\s*,\s*int64_t\s*\*\s*grid",
    "fpic_fusion_register": SPEC + r"int\s+every\s*,\s*int\s*\*\s*index",
    "fpic_fusion_stats": r"fpic_handle\s*\*\s*h\s*,\s*int\s+index\s*,\s*int\s+scope\s*,\s*fpic_fusion_result\s*\*\s*out",
    "fpic_fusion_grid": r"fpic_handle\s*\*\s*h\s*,\s*int\s+index\s*,\s*int64_t\s*\*\s*grid\s*,\s*int\s+reset",
    "fpic_fusion_clear": r"fpic_handle\s*\*\s*h",
}
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def fp():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import fusionpic
    return fusionpic


def test_fusion_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    for name, args in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)" % (name, args), text), name
        assert hasattr(lib, name) and name in fp.ABI_FUNCTIONS
    for name, value in (("MAX_OPS", 4), ("TABLE_MAX", 4096)):
        assert re.search(r"#define\s+FPIC_FUSION_%s\s+%d\b" % (name, value), text) and getattr(fp, "FUSION_" + name) == value
    assert ref.CELL_MAX == fp.PAIR_CELL_MAX and ref.TAG != 0xC0120


def test_the_tally_keeps_two_workgroups_on_a_cu():
    """the run's LDS of the pair pass plus one 64-bit word per cell of a chunk stays within 64 KiB"""
    pair = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_pair_kernels.hpp")).read()
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_fusion_kernels.hpp")).read()
    get = lambda name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, pair).group(1))
    assert re.search(r"kFusionLdsBytes\s*=\s*kPairChunk\s*\*\s*sizeof\(unsigned long long\)\s*\+\s*kPairLdsBytes", text)
    assert 8 * get("kPairChunk") + (3 * 4 + 2) * 2 * get("kPairCellMax") + 4 * (2 * (get("kPairChunk") + 1) + 2) <= 64 * 1024
    assert "pair_collide_kernel" not in re.sub(r"//.*", "", text)            # a kernel of its own


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("%s %zu\n", #m, offsetof(fpic_fusion_spec, m));
#define R(m) printf("result.%s %zu\n", #m, offsetof(fpic_fusion_result, m));
int main(void) {
    printf("sizeof %zu\n", sizeof(fpic_fusion_spec));
    printf("result.sizeof %zu\n", sizeof(fpic_fusion_result));
    F(species_a) F(species_b) F(seed) F(stream) F(epoch) F(tau) F(g_lo) F(g_hi) F(n) F(reserved_i) F(sigma) F(reserved)
    R(applications) R(pairs) R(below) R(above) R(cells) R(overfull_cells) R(overfull_particles) R(yield_hi) R(yield_lo) R(unit_exponent) R(reserved)
    return 0;
}
'''


def test_ctypes_mirrors_match_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(fp.FusionSpec)
    assert int(got.pop("result.sizeof")) == ctypes.sizeof(fp.FusionResult)
    result = {k[7:]: v for k, v in got.items() if k.startswith("result.")}
    spec = {k: v for k, v in got.items() if not k.startswith("result.")}
    for mirror, offsets in ((fp.FusionSpec, spec), (fp.FusionResult, result)):
        assert len(offsets) == len(mirror._fields_)
        for name, off in offsets.items():
            assert int(off) == getattr(mirror, name).offset, name


# ---- the header under g++
_built = {}


def native(tmp_path_factory, flags):
    key = tuple(flags)
    if key not in _built:
        exe = tmp_path_factory.mktemp("fusion_native") / "fusion_core_test"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, NATIVE, "-o", str(exe)])
        _built[key] = str(exe)
    return _built[key]


def run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0, out.stdout.decode()[-2000:] + out.stderr.decode()[-2000:]
    return out.stdout.decode()


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "sanitizers"])
def test_fusion_host_core(tmp_path_factory, flags):
    # its own program with its own main: under the sanitizers their runtime is linked into it, nothing is preloaded anywhere
    extra = os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split() if flags == ["-O2"] else []
    assert run(native(tmp_path_factory, flags + extra)).strip() == "ok"


def random_pairs(seed, m, g_lo, g_hi):
    """N_L and velocities whose relative speeds cover the table, both outsides, the nodes' neighbourhood and rest"""
    rng = np.random.default_rng(seed)
    n_l = rng.choice([1.0, 1.5, 2.0, 7.0, 64.0, 380.5, 1024.0, 2047.0, 2048.0], size=m)
    vp = rng.normal(0, 0.01, (m, 3))
    speed = rng.uniform(0.5 * g_lo, 1.1 * g_hi, m)
    axis = rng.normal(0, 1, (m, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    vo = vp + speed[:, None] * axis
    vo[:8] = vp[:8]                                                      # at rest
    vo[8:16] = vp[8:16] + np.array([g_hi, 0, 0])
    vo[16:24] = vp[16:24] + np.array([0, g_lo, 0])
    # stored values are T: half of the pairs carry float32 values
    vo[::2] = vo[::2].astype(np.float32)
    vp[::2] = vp[::2].astype(np.float32)
    return n_l, vo, vp


TABLES = [
    dict(sigma=lambda g: 1e-28 * (1 + np.sin(40 * g) ** 2), n=97, g_lo=0.0078125, g_hi=0.03125, tau=1e-9, W=1e10, dV=1.0),
    dict(sigma=lambda g: 3e-29 * np.exp(-0.01 / np.maximum(g, 1e-9)), n=4096, g_lo=0.0, g_hi=0.0301, tau=2.5e-11, W=3.7e12, dV=2.7e-11),
    dict(sigma=lambda g: np.where(g > 0.012, 5e-30, 0.0), n=2, g_lo=0.001, g_hi=0.05, tau=1.0, W=1.0, dV=1e-30),
]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "sanitizers"])
@pytest.mark.parametrize("case", range(len(TABLES)))
def test_the_header_equals_the_reference_bit_for_bit(tmp_path_factory, tmp_path, flags, case):
    t = TABLES[case]
    g = t["g_lo"] + np.arange(t["n"]) * ((t["g_hi"] - t["g_lo"]) / (t["n"] - 1))
    S = np.asarray(t["sigma"](g), dtype=np.float64)
    req = ref.request(S, t["g_lo"], t["g_hi"], t["tau"], t["W"], t["dV"])
    m = 4000
    n_l, vo, vp = random_pairs(100 + case, m, t["g_lo"], t["g_hi"])
    q, what, _ = ref.tally(req, n_l, vo, vp)
    assert (what == 0).sum() > m // 2 and ((what == 1).sum() > 8 or t["g_lo"] == 0) and (what == 2).sum() > 8 and max(q) > 2 ** 30
    hexes = lambda row: " ".join(float(x).hex() for x in row)
    lines = ["%d %s" % (t["n"], hexes([t["g_lo"], t["g_hi"], t["tau"], t["W"], t["dV"]]))] + [float(x).hex() for x in S] + [str(m)]
    lines += [hexes([n_l[k], *vo[k], *vp[k]]) for k in range(m)]
    path = tmp_path / "pairs.txt"
    path.write_text("\n".join(lines) + "\n")
    out = run(native(tmp_path_factory, flags), str(path)).splitlines()
    assert out[0] == "e %d" % req["e"]
    got = [tuple(int(x) for x in line.split()) for line in out[1:]]
    assert got == list(zip(what.tolist(), q))


# ---- the restatement by hand
def test_pair_sets_and_weights_by_hand():
    want = {0: [], 1: [], 2: [(0, 1, 2.0)], 3: [(0, 1, 1.5), (1, 2, 1.5), (2, 0, 1.5)], 4: [(0, 1, 4.0), (2, 3, 4.0)],
            5: [(0, 1, 2.5), (1, 2, 2.5), (2, 0, 2.5), (3, 4, 5.0)], 6: [(0, 1, 6.0), (2, 3, 6.0), (4, 5, 6.0)],
            7: [(0, 1, 3.5), (1, 2, 3.5), (2, 0, 3.5), (3, 4, 7.0), (5, 6, 7.0)]}
    for n, table in want.items():
        assert ref.pairing_like(n) == table
        assert sum(nl for _, _, nl in table) == (n * n / 2.0 if n >= 2 else 0)
    for n in (63, 64, 65, 129, 1025, 2047, 2048):
        assert sum(nl for _, _, nl in ref.pairing_like(n)) == n * n / 2.0
    assert ref.pairing_unlike(1, 1) == [(0, 0, 1.0)]
    assert ref.pairing_unlike(3, 2) == [(0, 0, 2.0), (1, 1, 2.0), (2, 0, 2.0)]
    assert ref.pairing_unlike(5, 2) == [(0, 0, 2.0), (1, 1, 2.0), (2, 0, 2.0), (3, 1, 2.0), (4, 0, 2.0)]
    assert ref.pairing_unlike(3, 0) == []
    for na, nb in ((1, 1), (3, 2), (2, 5), (130, 7)):
        assert sum(nl for _, _, nl in ref.pairing_unlike(max(na, nb), min(na, nb))) == na * nb
    # through schedule(): the `many` species owns the pairs whichever side it is, a tie goes to species a
    req = ref.request([1e-28, 1e-28], 0.0, 1.0, 1e-9, 1.0, 1.0)
    for na, nb in ((1, 1), (3, 2), (2, 5)):
        plan = ref.schedule(req, np.zeros(na, dtype=np.int64), np.arange(na), np.zeros(nb, dtype=np.int64), np.arange(nb))
        assert plan["n_l"].sum() == na * nb and len(plan["owner"]) == max(na, nb) and plan["cells"] == 1
        assert np.all((plan["owner"] >= na) == (nb > na)) and np.all((plan["partner"] >= na) == (nb <= na))
        assert sorted(set(plan["partner"].tolist())) == (list(range(na, na + nb)) if nb <= na else list(range(na)))


def test_interpolation_at_the_edges():
    S = [1e-28, 2e-28, 4e-28, 3e-28]
    req = ref.request(S, 0.0078125, 0.03125, 1e-9, 1e10, 1.0)
    assert req["inv_dg"] == 128.0

    def one(g, request=req, nl=7.0):
        q, what, _ = ref.tally(request, [nl], np.array([[g, 0.0, 0.0]]), np.zeros((1, 3)))
        return q[0], int(what[0])

    assert one(0.0078125)[1] == 0 and one(0.0078125)[0] > 0                                  # g == g_lo is inside
    assert one(np.nextafter(0.0078125, 0))[1] == 1 and one(0.0) == (0, 1)
    assert one(0.03125) == (0, 2) and one(1.0) == (0, 2)                                      # g == g_hi is above
    last = np.nextafter(0.03125, 0)
    assert one(last)[1] == 0 and 3e-28 < ref.sigma_at(req, np.array([last]))[0] < 3e-28 * (1 + 1e-12)   # the last interval
    assert ref.sigma_at(req, np.array([0.0078125, 0.015625, 0.0234375])).tolist() == [1e-28, 2e-28, 4e-28]   # a node reads the node
    assert ref.sigma_at(req, np.array([0.01171875]))[0] == 1e-28 + 0.5 * (2e-28 - 1e-28)
    y = ((((1e10 * 1e10) * 7.0) * 1e-9) / 1.0) * (2e-28 * (0.015625 * 2.998e8))
    assert one(0.015625)[0] == int(np.floor(np.ldexp(y, -req["e"])))
    zero = ref.request(S, 0.0, 0.03125, 1e-9, 1e10, 1.0)
    assert one(0.0, zero, 2048.0) == (0, 0)                                                   # g = 0 with g_lo = 0: inside, yields 0


def test_the_fixed_point():
    assert [ref.exponent(x) for x in (0.0, 1.0, 0.75, 2.0 ** 40, np.nextafter(1.0, 0), 1e-7, 5e-324)] == [0, -39, -40, 1, -40, -63, ref.EXPONENT_MIN]
    for W in (1e10, 1.1e10, 1.4142e10, 3.3e7, 1e-3):
        for top in (4e-28, 3.999e-28, 5.1e-28):
            S = [1e-28, 2e-28, 3e-28, top]
            req = ref.request(S, 0.0078125, 0.03125, 1e-9, W, 1.0)
            bound = ref.y_bound(W, 1e-9, 1.0, top, 0.03125)
            assert 2.0 ** (req["e"] + 39) <= bound < 2.0 ** (req["e"] + 40)
            q, what, _ = ref.tally(req, [2048.0], np.array([[np.nextafter(0.03125, 0), 0.0, 0.0]]), np.zeros((1, 3)))
            assert what[0] == 0 and 2 ** 38 <= q[0] < 2 ** 40                                 # q < 2^40 at the bound
    # the two words join to the Python-integer sum
    rng = np.random.default_rng(5)
    n = 3000
    v = rng.normal(0, 0.01, (n, 3)).astype(np.float32)
    req = ref.request([1e-28, 2e-28, 4e-28, 3e-28], 0.0, 0.05, 1e-9, 1e10, 1.0, like=True)
    out = ref.apply(req, 2, rng.integers(0, 2, n), np.arange(n), v)
    assert out["reactions_exact"] == sum(out["q"]) == int(out["grid"][0]) + int(out["grid"][1]) > 2 ** 40
    assert out["yield_lo"] < 2 ** 32 and (out["yield_hi"] << 32) + out["yield_lo"] == out["reactions_exact"] and out["yield_hi"] > 0
    zero = ref.apply(ref.request([0.0, 0.0], 0.0, 0.05, 1e-9, 1e10, 1.0, like=True), 2, rng.integers(0, 2, n), np.arange(n), v)
    assert zero["unit_exponent"] == 0 and not zero["grid"].any() and all(zero[k] == 0 for k in ("pairs", "below", "above", "cells", "reactions_exact"))


# ---- the wrapper
def test_wrapper_builds_the_request(fp):
    s = fp._fusion_spec(2e-9, sigma=[1e-28, 2e-28, 3e-28], g_lo=0, g_hi=0.03)
    assert (s.species_a, s.species_b, s.seed, s.stream, s.epoch, s.tau, s.g_lo, s.g_hi, s.n, s.reserved_i) == (0, 0, fp.FUSION_SEED, 0, 0, 2e-9, 0.0, 0.03, 3, 0)
    assert [s.sigma[k] for k in range(3)] == [1e-28, 2e-28, 3e-28] and not any(s.reserved)
    s = fp._fusion_spec(2e-9, 1, 0, sigma=np.ones(4096, dtype=np.float32), g_lo=0.001, g_hi=0.5, tau=1e-8, seed=(1 << 64) - 1, stream=(1 << 32) - 1, epoch=(1 << 32) - 1)
    assert (s.species_a, s.species_b, s.seed, s.stream, s.epoch, s.tau, s.n, s.sigma[4095]) == (1, 0, (1 << 64) - 1, (1 << 32) - 1, (1 << 32) - 1, 1e-8, 4096, 1.0)
    assert fp._fusion_spec(2e-9, 2, sigma=[0, 1], g_lo=0, g_hi=1).species_b == 2         # b None: a with itself
    good = dict(sigma=[1e-28, 2e-28], g_lo=0.0, g_hi=0.03)
    for bad, prop in ((dict(a=1 << 31), ".species_a"), (dict(a=0.5), ".species_a"), (dict(b="x"), ".species_b"), (dict(seed=-1), ".seed"), (dict(seed=1 << 64), ".seed"),
                      (dict(stream=1 << 32), ".stream"), (dict(epoch=-1), ".epoch"), (dict(tau="x"), ".tau"), (dict(g_lo=None), ".g_lo"), (dict(g_hi="x"), ".g_hi"),
                      (dict(sigma=None), ".sigma"), (dict(sigma="x"), ".sigma"), (dict(sigma=[[1, 2], [3, 4]]), ".sigma"), (dict(sigma=[1.0]), ".n"),
                      (dict(sigma=np.zeros(4097)), ".n")):
        with pytest.raises(fp.FusionPicError) as e:
            fp._fusion_spec(2e-9, **dict(good, **bad))
        assert prop + " <- " in str(e.value), (bad, str(e.value))
    r = fp.FusionResult(3, 10, 1, 2, 4, 0, 0, 5, 7, -60, 0)
    got = fp._fusion_counts(r)
    assert got["reactions_exact"] == (5 << 32) + 7 and got["reactions"] == ((5 << 32) + 7) * 2.0 ** -60 and got["unit_exponent"] == -60 and got["pairs"] == 10


def test_sigma_table(fp):
    md, mt, kev = 3.3435837724e-27, 5.0073567446e-27, 1.602176634e-16
    gamow = lambda e: 1e-24 / e * np.exp(-34.38 / np.sqrt(e))
    S, g_lo, g_hi = fp.sigma_table(gamow, md, mt, 1.0, 1000.0)
    mab = md * mt / (md + mt)
    assert len(S) == 4096 and abs(g_hi / g_lo - np.sqrt(1000.0)) < 1e-12
    assert abs(0.5 * mab * (g_lo * 2.998e8) ** 2 / kev - 1.0) < 1e-12 and abs(0.5 * mab * (g_hi * 2.998e8) ** 2 / kev - 1000.0) < 1e-9
    g = g_lo + np.arange(4096) * ((g_hi - g_lo) / 4095)
    assert np.allclose(S, gamow(0.5 * mab * (g * 2.998e8) ** 2 / kev), rtol=1e-12, atol=0) and S[0] > 0
    # uniform in g resolves the low end: linear interpolation at the first mid-point is within 1 %
    mid = 0.5 * (g[0] + g[1])
    assert abs(0.5 * (S[0] + S[1]) / gamow(0.5 * mab * (mid * 2.998e8) ** 2 / kev) - 1) < 0.01
    S2, lo2, hi2 = fp.sigma_table(lambda e: np.full_like(e, 2e-28), md, md, 0.0, 10.0, n=2)
    assert S2.tolist() == [2e-28, 2e-28] and lo2 == 0.0 and hi2 > 0
    for bad in (dict(mass_a=0.0), dict(mass_b=-1.0), dict(e_lo_keV=-1.0), dict(e_hi_keV=1.0), dict(n=1), dict(n=4097), dict(n=2.5),
                dict(sigma_of_keV=lambda e: -gamow(e)), dict(sigma_of_keV=lambda e: np.full_like(e, np.inf)), dict(sigma_of_keV=lambda e: 1.0)):
        kw = dict(dict(sigma_of_keV=gamow, mass_a=md, mass_b=mt, e_lo_keV=1.0, e_hi_keV=1000.0), **bad)
        with pytest.raises(fp.FusionPicError, match=" <- "):
            fp.sigma_table(**kw)


def test_fusion_without_a_handle(fp):
    lib = fp.load_library()
    s = fp._fusion_spec(2e-9, sigma=[1e-28, 2e-28], g_lo=0.0, g_hi=0.03)
    out = fp.FusionResult(7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 0)
    index = ctypes.c_int(77)
    grid = (ctypes.c_int64 * 4)(5, 5, 5, 5)
    assert lib.fpic_fusion(None, ctypes.byref(s), ctypes.byref(out), grid) == -1
    assert b"null handle" in lib.fpic_last_error(None) and out.pairs == 7 and list(grid) == [5, 5, 5, 5]
    assert lib.fpic_fusion_register(None, ctypes.byref(s), 1, ctypes.byref(index)) == -1 and index.value == 77
    assert lib.fpic_fusion_stats(None, 0, 0, ctypes.byref(out)) == -1 and out.applications == 7
    assert lib.fpic_fusion_grid(None, 0, grid, 1) == -1 and list(grid) == [5, 5, 5, 5]
    assert lib.fpic_fusion_clear(None) == -1
    assert b"null handle" in lib.fpic_last_error(None)


# ---- reactivity, with the restatement alone
MD, MT, KEV = 3.3435837724e-27, 5.0073567446e-27, 1.602176634e-16
KT_KEV, GAMOW_A, GAMOW_B = 10.0, 1e-24, 34.38


def gamow_of_g(g, mab):
    e = np.maximum(0.5 * mab * (g * ref.C) ** 2 / KEV, 1e-300)
    return GAMOW_A / e * np.exp(-GAMOW_B / np.sqrt(e))


def quadrature(s, mab):
    """<sigma v> (m^3/s) over the relative-speed Maxwellian whose components have the standard deviation s (units of c)"""
    g = np.linspace(0.0, 12.0 * s, 400001)[1:]
    f = np.sqrt(2.0 / np.pi) * g * g / s ** 3 * np.exp(-g * g / (2.0 * s * s))
    y = gamow_of_g(g, mab) * (g * ref.C) * f
    return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(g)) + 0.5 * y[0] * g[0])


def reactivity_ratio(seed, like, n_table):
    """the tally of 8 cells of about 2000 per species over W^2 tau / dV sum(Na Nb) <sigma v> (like: sum(N^2) <sigma v> / 2)"""
    rng = np.random.default_rng(seed)
    vth_d, vth_t = (np.sqrt(KT_KEV * KEV / m) / ref.C for m in (MD, MT))
    mb, vth_b = (MD, vth_d) if like else (MT, vth_t)
    mab = MD * mb / (MD + mb)
    s = np.sqrt(vth_d ** 2 + vth_b ** 2)
    e_lo, e_hi = 0.2, 300.0
    g_lo, g_hi = (np.sqrt(2.0 * e * KEV / mab) / ref.C for e in (e_lo, e_hi))
    S = gamow_of_g(g_lo + np.arange(n_table) * ((g_hi - g_lo) / (n_table - 1)), mab)
    W, tau, dV = 1e12, 1e-9, 1e-9
    req = ref.request(S, g_lo, g_hi, tau, W, dV, seed=seed, like=like)
    na, nb = rng.integers(1900, 2049, 8), rng.integers(1900, 2049, 8)
    cell_a, cell_b = np.repeat(np.arange(8), na), np.repeat(np.arange(8), nb)
    va, vb = rng.normal(0, vth_d, (len(cell_a), 3)), rng.normal(0, vth_b, (len(cell_b), 3))
    if like:
        out = ref.apply(req, 8, cell_a, np.arange(len(cell_a)), va)
        weight, expect = float((na * na).sum()) / 2.0, quadrature(s, mab)
    else:
        out = ref.apply(req, 8, cell_a, np.arange(len(cell_a)), va, cell_b, np.arange(len(cell_b)), vb)
        weight, expect = float((na * nb).sum()), quadrature(s, mab)
    assert out["weights"] == weight and out["overfull_cells"] == 0 and out["pairs"] > 0.99 * (out["pairs"] + out["below"] + out["above"])
    scale = ((W * W) * tau) / dV
    floor_share = len(out["q"]) / max(out["reactions_exact"], 1)           # the floors lose less than one unit per pair
    return out["reactions_exact"] * 2.0 ** out["unit_exponent"] / (scale * weight * expect), floor_share


@pytest.mark.parametrize("like", [False, True], ids=["unlike", "like"])
def test_reactivity_of_two_maxwellians(like):
    seeds = range(301, 309)
    got = [reactivity_ratio(seed, like, 4096) for seed in seeds]
    ratios = np.array([r for r, _ in got])
    mean, sem = float(ratios.mean()), float(ratios.std(ddof=1) / np.sqrt(len(ratios)))
    halved = abs(reactivity_ratio(301, like, 2048)[0] - ratios[0])          # the table's interpolation error: halving n
    floors = max(f for _, f in got)
    print("%s: tally / quadrature %.4f +- %.4f over %d seeds; halving n moves it by %.2g; the floors lose below %.2g" %
          ("like" if like else "unlike", mean, sem, len(ratios), halved, floors))
    assert sem < 0.02                                                       # (a measurement, not the check: 16000 pairs per seed)
    assert abs(mean - 1.0) <= 3.0 * sem + halved + floors
