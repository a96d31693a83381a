"""The windowed background collisions (fpic_gas*) on a machine WITHOUT a GPU: the header declares the four entry points and
libfusionpic.so exports them, the ctypes mirrors have the C layout, the rule and the checks of a request
(fusion-sim_amd/csrc/fes_gas_core.hpp) pass their g++ test and give, bit for bit, what the numpy reference
(tests/gas_reference.py) gives on cases whose rounded functions do not enter (vth = 0 and EXCHANGE: the decisions, the stored
velocity and the tallies are all exact) — also as a stand-alone program under AddressSanitizer and UBSan —, the launch shape
and the host's thresholds are named constants, the Python wrapper builds the request and refuses what the structure cannot
carry, and a call without a handle fails cleanly.  The collisions themselves are checked on the GPU (tests/test_gpu_gas.py)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gas_reference as ref
from helpers import ROOT
from test_gas_reference import DT, G_HI, G_LO, L, TABLE, TAPERS, WINDOW, density_for, scene

HEADER = os.path.join(ROOT, "include", "fusionpic.h")
LIB = os.path.join(ROOT, "fusion-sim_amd", "lib", "libfusionpic.so")
NATIVE = os.path.join(ROOT, "tests", "native", "gas_core_test.cpp")
KERNELS = os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_gas_kernels.hpp")
ENTRIES = {
    "fpic_gas": r"fpic_handle\s*\*\s*h\s*,\s*const\s+fpic_gas_spec\s*\*\s*spec\s*,\s*fpic_gas_result\s*\*\s*out",
    "fpic_gas_register": r"fpic_handle\s*\*\s*h\s*,\s*const\s+fpic_gas_spec\s*\*\s*spec\s*,\s*int\s+every\s*,\s*int\s*\*\s*index",
    "fpic_gas_stats": r"fpic_handle\s*\*\s*h\s*,\s*int\s+index\s*,\s*int\s+scope\s*,\s*fpic_gas_result\s*\*\s*out",
    "fpic_gas_clear": r"fpic_handle\s*\*\s*h",
}


@pytest.fixture(scope="module")
def fp():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import fusionpic
    return fusionpic


def test_gas_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    for name, args in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)" % (name, args), text), name
        assert hasattr(lib, name) and name in fp.ABI_FUNCTIONS
    for name, value in (("EXCHANGE", 0), ("ELASTIC", 1), ("MAX_OPS", 8), ("TABLE_MAX", 4096), ("TAPER_MAX", 1025)):
        assert re.search(r"#define\s+FPIC_GAS_%s\s+%d\b" % (name, value), text) and getattr(fp, "GAS_" + name) == value
    assert (ref.EXCHANGE, ref.ELASTIC, ref.MAX_OPS, ref.TABLE_MAX, ref.TAPER_MAX) == (0, 1, 8, 4096, 1025)
    assert re.search(r"#define\s+FPIC_ABI_VERSION\s+2\b", text)


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("%s %zu\n", #m, offsetof(fpic_gas_spec, m));
#define R(m) printf("result.%s %zu\n", #m, offsetof(fpic_gas_result, m));
int main(void) {
    printf("sizeof %zu\n", sizeof(fpic_gas_spec));
    printf("result.sizeof %zu\n", sizeof(fpic_gas_result));
    F(species) F(kind) F(seed) F(stream) F(epoch) F(density) F(tau) F(g_lo) F(g_hi) F(n) F(reserved_i) F(sigma) F(drift) F(vth) F(mass_ratio) F(lo) F(hi)
    F(taper_n) F(reserved_u) F(taper) F(reserved)
    R(applications) R(candidates) R(collided) R(below) R(above) R(energy_fixed) R(momentum_fixed) R(energy) R(momentum)
    return 0;
}
'''


def test_ctypes_mirrors_match_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for prefix, mirror in (("result.", fp.GasResult), ("", fp.GasSpec)):
        mine = {k[len(prefix):]: int(v) for k, v in got.items() if k.startswith(prefix) and (prefix or "." not in k)}
        assert mine.pop("sizeof") == ctypes.sizeof(mirror), prefix
        assert len(mine) == len(mirror._fields_), prefix
        for name, off in mine.items():
            assert off == getattr(mirror, name).offset, prefix + name


# ---- the cases of the g++ program and what the reference gives for them: vth = 0 and EXCHANGE, so the partner is the drift,
# g one square root, and the host's log, sin and cos enter nothing that is compared
def cases():
    frac, vel = scene(3001)
    drift = (0.01, 0.0, -0.02)
    base = dict(tau=DT, sigma=TABLE, g_lo=G_LO, g_hi=G_HI, drift=drift, vth=0.0, stream=3, epoch=9)
    at = lambda p: density_for(p * 2.0 ** 32, TABLE, G_LO, G_HI)
    flat = np.full(2, 3.0e-19)
    zeros = TABLE.copy()
    zeros[30:50] = 0.0
    fast = vel * 3000.0                                                     # |v|^2 >= 2^15 for most, and one |vy| >= 2^15 itself
    fast[5] = (0.0, -40000.0, 0.0)
    return [
        (np.float32, dict(base, density=at(0.3), seed=11), 0, frac, vel),
        (np.float64, dict(base, density=at(0.3), seed=12, **WINDOW), 5, frac, vel),
        (np.float32, dict(base, density=at(0.9), seed=13, taper=TAPERS, **WINDOW), 1 << 31, frac, vel),
        (np.float64, dict(base, density=at(0.9), seed=14, taper=(None, TAPERS[2], None)), 0, frac, vel),
        (np.float32, dict(base, density=at(0.99), seed=15, sigma=zeros, taper=TAPERS, **WINDOW), 0, frac, vel),
        (np.float64, dict(base, density=1e30, seed=16, sigma=flat, g_lo=0.0, g_hi=0.15), 0, frac, vel),     # P_max = 1: K = 2^32
        (np.float32, dict(base, density=0.0, seed=17), 0, frac[:64], vel[:64]),                           # K = 0
        (np.float64, dict(base, density=1e30, seed=18, sigma=flat, g_lo=0.0, g_hi=1e5, drift=(0.0, 0.0, 0.0), **WINDOW), 7, frac, fast),   # terms outside the range: the bits
    ]


def words128(v):
    v &= (1 << 128) - 1
    return [v & 0xFFFFFFFFFFFFFFFF, v >> 64]


def cases_and_expectations():
    blob, want = [], []
    all_cases = cases()
    for dtype, kw, first, frac, vel in all_cases:
        req = ref.request(L, ref.EXCHANGE, **kw)
        lo, hi = kw.get("lo", (0.0, 0.0, 0.0)), kw.get("hi", L)
        taper = kw.get("taper", (None, None, None))
        S = np.asarray(kw["sigma"], dtype=np.float64)
        n = len(frac)
        blob.append(struct.pack("<iiiiQII", ref.EXCHANGE, len(S), int(dtype == np.float64), 0, kw["seed"], kw["stream"], kw["epoch"]))
        blob.append(np.array([kw["density"], kw["tau"], kw["g_lo"], kw["g_hi"], *req["drift"], *req["vth"], 0.0, *L, *lo, *hi], dtype=np.float64).tobytes())
        blob.append(struct.pack("<4I", *[0 if t is None else len(t) for t in taper], 0))
        blob.append(S.tobytes())
        blob += [np.asarray(t, dtype=np.float64).tobytes() for t in taper if t is not None]
        blob.append(struct.pack("<II", n, first))
        stored_v = vel.astype(dtype)
        blob.append(np.concatenate([frac, stored_v.astype(np.float64)], axis=1).tobytes())
        ids = np.arange(n, dtype=np.uint64) + first
        out = ref.stored(req, ids, frac, stored_v)
        what = out["collided"] * 1 + out["below"] * 2 + out["above"] * 4
        rows = np.empty((n, 5), dtype=np.uint64)
        rows[:, 0], rows[:, 1] = out["candidate"], what
        rows[:, 2:] = out["v"].astype(np.float64).view(np.uint64)
        finite = np.abs(stored_v.astype(np.float64)) < 2.0 ** 15
        sq = lambda v: (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        b64, a64 = stored_v.astype(np.float64), out["v"].astype(np.float64)
        hit = out["collided"]
        ok_e = hit & (sq(b64) < 2.0 ** 15) & (sq(a64) < 2.0 ** 15)
        t = ref.tallies(stored_v, out["v"], ok_e)
        sums, bits = [t["energy_fixed"]], int((hit & ~ok_e).any())
        for a in range(3):
            ok = hit & finite[:, a] & (np.abs(a64[:, a]) < 2.0 ** 15)
            sums.append(ref.tallies(stored_v, out["v"], ok)["momentum_fixed"][a])
            bits |= int((hit & ~ok).any()) << (1 + a)
        c = ref.counts(out)
        tail = [c["candidates"], c["below"], c["above"], c["collided"]] + [w for s in sums for w in words128(s)] + [bits]
        head = np.array([req["column"], req["x_max"]], dtype=np.float64).view(np.uint64)
        want.append(np.concatenate([head, [np.uint64(req["K"])], rows.ravel(), np.array(tail, dtype=np.uint64)]))
    return struct.pack("<I", len(all_cases)) + b"".join(blob), np.concatenate(want), all_cases


def _native(tmp_path, name, flags):
    exe, cases_file, out = tmp_path / name, tmp_path / (name + ".in"), tmp_path / (name + ".out")
    blob, want, all_cases = cases_and_expectations()
    cases_file.write_bytes(blob)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, NATIVE, "-o", str(exe)])
    run = subprocess.run([str(exe), str(cases_file), str(out)], capture_output=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0 and run.stdout.decode().strip() == "ok", run.stdout.decode() + run.stderr.decode()
    got = np.frombuffer(out.read_bytes(), dtype=np.uint64)
    assert got.size == want.size
    differ = np.flatnonzero(got != want)
    assert differ.size == 0, (differ.size, differ[:5], got[differ[:5]], want[differ[:5]])
    # the cases cover what they are meant to: both precisions, the whole box and the window, tapers, zero intervals, K = 2^32
    # and K = 0, every outcome, and a term outside the fixed-point range
    sizes = [3 + 5 * len(c[3]) + 13 for c in all_cases]
    ends = np.cumsum(sizes)
    tails = [got[e - 13:e] for e in ends]
    assert all(t[0] > 0 and t[3] > 0 for t in tails[:6]) and tails[1][1] > 0 and tails[5][2] > 0 and tails[0][3] < tails[0][0]
    assert got[ends[4] + 2] == 1 << 32 and tails[5][0] == len(all_cases[5][3])
    assert got[ends[5] + 2] == 0 and not tails[6].any()
    assert tails[7][12] == 0x5 and tails[7][3] > 0 and not any(t[12] for t in tails[:7])
    assert tails[1][0] < tails[0][0]                                      # the window keeps candidates out
    first_rows = got[ends[0] + 3:ends[0] + 3 + 5 * 4].reshape(4, 5)
    assert not first_rows[1, 0] and not first_rows[2, 0]                  # on hi_f: outside


def test_gas_host_core(tmp_path):
    _native(tmp_path, "gas_core_test", ["-O2", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split()])


def test_gas_host_core_under_sanitizers(tmp_path):
    # its own program with its own main: the sanitizers' runtime is linked into it, nothing is preloaded anywhere
    _native(tmp_path, "gas_core_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def test_the_launch_shape_and_the_thresholds_are_named_constants_of_the_kernel_header():
    text = open(KERNELS).read()
    blocks = re.search(r"constexpr\s+int\s+kGasBlocks\s*=\s*(\d+)\s*;", text)
    threads = re.search(r"constexpr\s+int\s+kGasThreads\s*=\s*(\d+)\s*;", text)
    assert blocks and threads
    assert int(threads.group(1)) == 256 and int(blocks.group(1)) == 2048          # collide_kernel's shape
    assert re.search(r"constexpr\s+double\s+kGasWindowFirstMax\s*=", text)
    assert re.search(r"kGasCompactMin\s*=\s*1ull\s*<<\s*\d+\s*,\s*kGasCompactMax\s*=\s*1ull\s*<<\s*\d+\s*;", text)
    assert "<<<" not in text and re.search(r"<<<grid, kGasThreads, 0,", open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_gas.inc.hpp")).read())


def test_wrapper_builds_the_request(fp):
    box = [0.008, 0.016, 0.004]
    s, keep = fp._gas_spec(2e-9, box, "exchange", density=1e20, sigma=[1e-19, 2e-19], g_lo=0.0, g_hi=0.5)
    assert (s.species, s.kind, s.seed, s.stream, s.epoch, s.n, s.reserved_i, s.reserved_u) == (0, fp.GAS_EXCHANGE, fp.GAS_SEED, 0, 0, 2, 0, 0)
    assert (s.density, s.tau, s.g_lo, s.g_hi, s.mass_ratio) == (1e20, 2e-9, 0.0, 0.5, 0.0) and [s.sigma[0], s.sigma[1]] == [1e-19, 2e-19]
    assert list(s.lo) == [0, 0, 0] and list(s.hi) == box and list(s.drift) == [0, 0, 0] and list(s.vth) == [0, 0, 0]
    assert list(s.taper_n) == [0, 0, 0] and not any(bool(p) for p in s.taper) and not any(s.reserved) and len(keep) == 1
    s, keep = fp._gas_spec(2e-9, box, "elastic", species=1, density=3.0, tau=7.0, sigma=np.arange(5, dtype=np.float32), g_lo=0.1, g_hi=0.2, drift=(1, 2, 3), vth=0.5,
                           lo=(0.001, 0, 0), hi=0.004, taper=(None, [0, 1, 0.5], np.ones(4)), seed=(1 << 64) - 1, stream=7, epoch=(1 << 32) - 1)
    assert (s.species, s.kind, s.seed, s.stream, s.epoch, s.n) == (1, fp.GAS_ELASTIC, (1 << 64) - 1, 7, (1 << 32) - 1, 5)
    assert (s.density, s.tau, s.g_lo, s.g_hi) == (3.0, 7.0, 0.1, 0.2) and s.mass_ratio == float("inf") and [s.sigma[k] for k in range(5)] == [0, 1, 2, 3, 4]
    assert list(s.drift) == [1, 2, 3] and list(s.vth) == [0.5] * 3 and list(s.lo) == [0.001, 0, 0] and list(s.hi) == [0.004] * 3
    assert list(s.taper_n) == [0, 3, 4] and not bool(s.taper[0]) and [s.taper[1][k] for k in range(3)] == [0, 1, 0.5] and s.taper[2][3] == 1.0 and len(keep) == 3
    assert fp._gas_spec(2e-9, box, 7, density=1, sigma=[1], g_lo=0, g_hi=1)[0].kind == 7            # (the library refuses it, and the one-entry table)
    assert fp._gas_spec(2e-9, box, "elastic", density=1, sigma=[1, 1], g_lo=0, g_hi=1, mass_ratio=2.5)[0].mass_ratio == 2.5
    good = dict(density=1e20, sigma=[1e-19, 2e-19], g_lo=0.0, g_hi=0.5)
    for bad, prop in ((dict(kind="relax"), ".kind"), (dict(kind=1.5), ".kind"), (dict(species=1 << 31), ".species"), (dict(epoch=-1), ".epoch"), (dict(epoch=1 << 32), ".epoch"),
                      (dict(seed=1 << 64), ".seed"), (dict(stream=-1), ".stream"), (dict(density=None), ".density"), (dict(density="x"), ".density"), (dict(tau=[1]), ".tau"),
                      (dict(sigma=None), ".sigma"), (dict(sigma=5.0), ".sigma"), (dict(sigma=[[1, 2], [3, 4]]), ".sigma"), (dict(sigma="ab"), ".sigma"),
                      (dict(g_lo=None), ".g_lo"), (dict(g_hi="x"), ".g_hi"), (dict(drift=(0, 1)), ".drift"), (dict(vth="ab"), ".vth"), (dict(mass_ratio="m"), ".mass_ratio"),
                      (dict(lo=(0, 1)), ".lo"), (dict(hi="ab"), ".hi"), (dict(taper=[None, None]), ".taper"), (dict(taper=(None, 5.0, None)), ".taper"),
                      (dict(taper=(None, [[1, 2], [3, 4]], None)), ".taper")):
        kw = dict(good, **bad)
        kind = kw.pop("kind", "exchange")
        with pytest.raises(fp.FusionPicError) as e:
            fp._gas_spec(2e-9, box, kind, **kw)
        assert prop + " <- " in str(e.value), (bad, str(e.value))


def test_group_sums_form_the_doubles_from_the_summed_words(fp):
    a = dict(applications=3, candidates=9, collided=5, below=1, above=2, energy_fixed=(1 << 70) + 1, momentum_fixed=[-7, 1 << 64, 0], energy=1.0, momentum=[1.0, 2.0, 0.0])
    b = dict(applications=3, candidates=4, collided=2, below=0, above=1, energy_fixed=-(1 << 70), momentum_fixed=[7, 1 << 11, -3], energy=2.0, momentum=[1.0, float("nan"), 0.0])
    out = fp._gas_sum([a, b], 2.0, 3.0)
    ke, pm = 0.5 * 2.0 * 3.0 * ref.C * ref.C, 2.0 * 3.0 * ref.C
    assert (out["applications"], out["candidates"], out["collided"], out["below"], out["above"]) == (3, 13, 7, 1, 3)
    assert out["energy_fixed"] == 1 and out["momentum_fixed"] == [0, (1 << 64) + (1 << 11), -3]
    assert out["energy"] == ke * 2.0 ** -80 and out["momentum"][0] == 0.0 and out["momentum"][1] != out["momentum"][1] and out["momentum"][2] == pm * -3 * 2.0 ** -80
    assert ref.derived(dict(energy_fixed=1, momentum_fixed=[0, 0, -3]), 2.0, 3.0) == dict(energy=ke * 2.0 ** -80, momentum=[0.0, 0.0, pm * -3 * 2.0 ** -80])
    assert set(out) == set(a)


def test_gas_without_a_handle(fp):
    lib = fp.load_library()
    s, keep = fp._gas_spec(2e-9, [1.0, 1.0, 1.0], "exchange", density=1e20, sigma=[1e-19, 2e-19], g_lo=0.0, g_hi=0.5)
    out = fp.GasResult(7, 7)
    index = ctypes.c_int(77)
    assert lib.fpic_gas(None, ctypes.byref(s), ctypes.byref(out)) == -1
    assert b"null handle" in lib.fpic_last_error(None) and out.candidates == 7
    assert lib.fpic_gas_register(None, ctypes.byref(s), 1, ctypes.byref(index)) == -1 and index.value == 77
    assert lib.fpic_gas_stats(None, 0, 0, ctypes.byref(out)) == -1 and out.applications == 7
    assert lib.fpic_gas_clear(None) == -1
    assert b"null handle" in lib.fpic_last_error(None)
