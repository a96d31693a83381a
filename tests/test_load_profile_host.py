"""The profiled load (fpic_load_profile) on a machine WITHOUT a GPU: the header declares the entry point and libfusionpic.so
exports it, the ctypes mirror of the profile has the C layout, the rule and the checks of a profile
(fusion-sim_amd/csrc/fes_load_profile_core.hpp) pass their g++ test and give, bit for bit, what the numpy reference
(tests/load_profile_reference.py) gives — also as a stand-alone program under AddressSanitizer and UBSan —, the Python
wrapper builds the profile and refuses what the structure cannot carry, and a call without a handle fails cleanly.  The
populations themselves are checked on the GPU (tests/test_gpu_load_profile.py)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import load_profile_reference as pref
from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "fusionpic.h")
LIB = os.path.join(ROOT, "fusion-sim_amd", "lib", "libfusionpic.so")
NATIVE = os.path.join(ROOT, "tests", "native", "load_profile_core_test.cpp")
M = 4000


@pytest.fixture(scope="module")
def fp():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import fusionpic
    return fusionpic


def test_load_profile_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+fpic_load_profile\s*\(\s*fpic_handle\s*\*\s*h\s*,\s*const\s+fpic_load_spec\s*\*\s*spec\s*,\s*const\s+struct\s+fpic_load_profile\s*\*\s*profile\s*,"
                     r"\s*uint64_t\s*\*\s*loaded\s*\)", text)
    assert hasattr(ctypes.CDLL(LIB), "fpic_load_profile") and "fpic_load_profile" in fp.ABI_FUNCTIONS
    assert re.search(r"#define\s+FPIC_LOAD_TABLE_MAX\s+1025\b", text) and fp.LOAD_TABLE_MAX == 1025
    assert re.search(r"#define\s+FPIC_ABI_VERSION\s+2\b", text)


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("%s %zu\n", #m, offsetof(struct fpic_load_profile, m));
int main(void) {
    printf("sizeof %zu\n", sizeof(struct fpic_load_profile));
    F(density_n) F(thermal_n) F(shear_n) F(shear_axis) F(shear_component) F(reserved) F(density) F(thermal) F(shear)
    return 0;
}
'''


def test_ctypes_mirror_matches_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(fp.LoadProfile)
    assert len(got) == len(fp.LoadProfile._fields_)
    for name, off in got.items():
        assert int(off) == getattr(fp.LoadProfile, name).offset, name


# ---- the cases of the g++ program and what the reference gives for them
def gaussian(nodes):
    x = np.linspace(0.0, 1.0, nodes)
    return np.exp(-0.5 * ((x - 0.5) / 0.15) ** 2)


DENSITIES = [[1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [0.0, 1.0, 0.0], [2.0, 0.5, 3.0], gaussian(1025), [1, 1, 0, 0, 0, 2, 0], [0, 0, 1, 3, 0, 0], [1e-300, 1, 1e-300],
             [3.0, 0.0, 0.0, 0.0], np.concatenate([np.zeros(400), gaussian(225), np.zeros(400)])]
TABLES = [[1.0, 2.0], [0.5, 0.0, 4.0], np.cos(np.linspace(0, 7, 1025)), [-0.02, 0.03, 0.01, -0.05]]
L = (0.016, 0.012, 0.008)
FULL = [   # (lattice, seed, stream, lo, hi, drift, density, thermal, shear)
    (0, 0xC0FFEE0123456789, 5, (0.0016, 0.0, 0.002), (0.0144, 0.012, 0.006), (0.01, 0.0, -0.02), (None, None, [0.0, 1.0, 0.0]), (None, None, None), None),
    (1, 77, 2, (0.0, 0.0, 0.0), L, (0.0, 0.0, 0.0), ([1.0, 3.0], gaussian(1025), None), ([1.0, 2.0], None, None), dict(axis=1, component=0, values=[-0.02, 0.03, 0.01, -0.05])),
    (0, 31, 3, (0.001, 0.002, 0.003), (0.015, 0.011, 0.0075), (0.0, 0.003, 0.0), ([0, 0, 1, 3, 0, 0], [1, 1, 0, 0, 0, 2, 0], gaussian(1025)),
     ([0.5, 0.0, 4.0], np.cos(np.linspace(0, 7, 1025)) ** 2, [2.0, 1.0]), dict(axis=2, component=2, values=np.sin(np.linspace(0, 9, 1025)) * 0.1)),
]


def words():
    rng = np.random.default_rng(3)
    return np.concatenate([np.array([0, (1 << 32) - 1, 1, 1 << 31], dtype=np.uint32), rng.integers(0, 1 << 32, M - 4, dtype=np.uint32)])


def indices():
    rng = np.random.default_rng(4)
    return np.concatenate([np.array([0, 1, (1 << 32) - 1], dtype=np.uint32), rng.integers(0, 1 << 32, M - 3, dtype=np.uint32)])


def cases_and_expectations():
    blob, want = [struct.pack("<I", len(DENSITIES) + len(TABLES) + len(FULL))], []
    w = words()
    for d in DENSITIES:
        d = np.asarray(d, dtype=np.float64)
        blob += [struct.pack("<III", 1, d.size, M), d.tobytes(), w.tobytes()]
        fq, j, s = pref.warp(d, w.astype(np.float64) * 2.0 ** -32)
        want.append(np.stack([fq, j.astype(np.float64), s], axis=1).ravel())
    fr = np.concatenate([np.array([0.0, 1.0 - 2.0 ** -53, 0.5, 2.0 ** -60]), np.random.default_rng(5).random(M - 4)])
    for t in TABLES:
        t = np.asarray(t, dtype=np.float64)
        blob += [struct.pack("<III", 2, t.size, M), t.tobytes(), fr.tobytes()]
        v, j, s = pref.lookup(t, fr)
        want.append(np.stack([v, j.astype(np.float64), s], axis=1).ravel())
    idx = indices()
    for lattice, seed, stream, lo, hi, drift, density, thermal, shear in FULL:
        tabs = [np.zeros(0) if t is None else np.asarray(t, dtype=np.float64) for t in list(density) + list(thermal)] + \
               [np.zeros(0) if shear is None else np.asarray(shear["values"], dtype=np.float64)]
        where = (0, 0) if shear is None else (shear["axis"], shear["component"])
        blob += [struct.pack("<IIQI", 3, lattice, seed, stream), np.array(list(L) + list(lo) + list(hi) + list(drift), dtype=np.float64).tobytes(),
                 struct.pack("<7I2i", *[t.size for t in tabs], *where)] + [t.tobytes() for t in tabs] + [struct.pack("<I", M), idx.tobytes()]
        req = pref.request(L, density=density, thermal=thermal, shear=shear, seed=seed, stream=stream, lo=lo, hi=hi, drift=drift, vth=0, lattice=bool(lattice))
        p, _, f = pref.base(req, idx)
        want.append(np.concatenate([p, f, pref.velocities(req, idx)], axis=1).ravel())
    return b"".join(blob), np.concatenate(want)


def _native(tmp_path, name, flags):
    exe, cases, out = tmp_path / name, tmp_path / (name + ".in"), tmp_path / (name + ".out")
    blob, want = cases_and_expectations()
    cases.write_bytes(blob)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, NATIVE, "-o", str(exe)])
    run = subprocess.run([str(exe), str(cases), str(out)], capture_output=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0 and run.stdout.decode().strip() == "ok", run.stdout.decode() + run.stderr.decode()
    got = np.frombuffer(out.read_bytes(), dtype=np.float64)
    assert got.size == want.size == 3 * M * (len(DENSITIES) + len(TABLES)) + 9 * M * len(FULL)
    differ = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert differ.size == 0, (differ.size, differ[:5], got[differ[:5]], want[differ[:5]])
    # the cases cover what they are meant to: tables of 2, 3 and 1025 nodes, intervals without mass at the start, in the
    # middle and at the end, the words 0 and 2^32 - 1
    assert {2, 3, 1025} <= {len(d) for d in DENSITIES} and {2, 3, 1025} <= {len(t) for t in TABLES}
    w = words()
    assert w[0] == 0 and w[1] == (1 << 32) - 1
    first = want[:3 * M * len(DENSITIES)].reshape(len(DENSITIES), M, 3)
    assert np.all(first[:, :, 0] >= 0) and np.all(first[:, :, 0] < 1)
    assert first[7, 0, 1] == 1 and first[7, 1, 1] == 3 and first[6, 1, 1] == 5 and first[10, 0, 1] == 399 and first[10, 1, 1] == 624     # the holes at either end are skipped
    assert not np.isin(first[6, :, 1], (2, 3)).any() and set(first[6, :, 1]) == {0.0, 1.0, 4.0, 5.0}                                        # and the one in the middle


def test_load_profile_host_core(tmp_path):
    _native(tmp_path, "load_profile_core_test", ["-O2", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split()])


def test_load_profile_host_core_under_sanitizers(tmp_path):
    # its own program with its own main: the sanitizers' runtime is linked into it, nothing is preloaded anywhere
    _native(tmp_path, "load_profile_core_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def test_wrapper_builds_the_profile(fp):
    assert fp._load_profile() is None
    p = fp._load_profile(density=[None] * 3)
    assert list(p.density_n) + list(p.thermal_n) + [p.shear_n, p.shear_axis, p.shear_component] + list(p.reserved) == [0] * 11
    assert not any(bool(x) for x in list(p.density) + list(p.thermal)) and not bool(p.shear)
    p = fp._load_profile(density=(None, [1, 2, 3], None), thermal=([1.0, 2.0], None, np.arange(5, dtype=np.float32)), shear=dict(axis=2, component=1, values=(0.1, 0.2)))
    assert list(p.density_n) == [0, 3, 0] and list(p.thermal_n) == [2, 0, 5] and (p.shear_n, p.shear_axis, p.shear_component) == (2, 2, 1)
    assert [p.density[1][k] for k in range(3)] == [1.0, 2.0, 3.0] and [p.thermal[2][k] for k in range(5)] == [0, 1, 2, 3, 4] and p.shear[1] == 0.2
    assert not bool(p.density[0]) and not bool(p.thermal[1])
    for bad, prop in ((dict(density=[None, None]), ".density"), (dict(density="abc"), ".density"), (dict(density=[None, None, "x"]), ".density"), (dict(thermal=5), ".thermal"),
                      (dict(thermal=[None, [[1, 2], [3, 4]], None]), ".thermal"), (dict(shear=[1, 2]), ".shear"), (dict(shear=dict(axis=0, values=[1, 2])), ".shear"),
                      (dict(shear=dict(axis=0.5, component=0, values=[1, 2])), ".shear_axis"), (dict(shear=dict(axis=0, component=True, values=[1, 2])), ".shear_component"),
                      (dict(shear=dict(axis=0, component=0, values=None)), ".shear")):
        with pytest.raises(fp.FusionPicError) as e:
            fp._load_profile(**bad)
        assert prop + " <- " in str(e.value), (bad, str(e.value))


def test_load_profile_without_a_handle(fp):
    lib = fp.load_library()
    s = fp._load_spec([1.0, 1.0, 1.0], count=4)
    p = fp._load_profile(density=([1.0, 2.0], None, None))
    loaded = ctypes.c_uint64(77)
    assert lib.fpic_load_profile(None, ctypes.byref(s), ctypes.byref(p), ctypes.byref(loaded)) == -1
    assert b"null handle" in lib.fpic_last_error(None) and loaded.value == 77
