"""The particle selection (fpic_select) on a machine WITHOUT a GPU: the header declares the entry point and libfusionpic.so
exports it, fusionpic.ABI_FUNCTIONS lists it, the ctypes mirror of fpic_select_spec has the C layout, the rule and the checks
of a request (fusion-sim_amd/csrc/fes_select_core.hpp) pass their g++ test, the launch shape is a pair of named constants of
the kernel header, the Python wrapper refuses what the structure cannot carry, and a call without a handle fails cleanly.
The selections themselves are checked on the GPU (tests/test_gpu_select.py)."""
import ctypes
import math
import os
import re
import subprocess

import pytest

from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "fusionpic.h")
LIB = os.path.join(ROOT, "fusion-sim_amd", "lib", "libfusionpic.so")


@pytest.fixture(scope="module")
def fp():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import fusionpic
    return fusionpic


def test_select_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+fpic_select\s*\(", text)
    assert hasattr(ctypes.CDLL(LIB), "fpic_select")
    assert "fpic_select" in fp.ABI_FUNCTIONS
    assert re.search(r"#define\s+FPIC_SELECT_MAX_TERMS\s+7\b", text) and fp.SELECT_MAX_TERMS == 7
    assert re.search(r"#define\s+FPIC_SELECT_MAX_ROWS\s+\(1u << 24\)", text) and fp.SELECT_MAX_ROWS == 1 << 24
    assert re.search(r"#define\s+FPIC_ABI_VERSION\s+2\b", text)


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("%s %zu\n", #m, offsetof(fpic_select_spec, m));
int main(void) {
    printf("sizeof %zu\n", sizeof(fpic_select_spec));
    F(species) F(nterms) F(axis) F(lo) F(hi) F(id_mod) F(id_rem) F(reserved)
    return 0;
}
'''


def test_ctypes_mirror_matches_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(fp.SelectSpec)
    assert len(got) == len(fp.SelectSpec._fields_)
    for name, off in got.items():
        assert int(off) == getattr(fp.SelectSpec, name).offset, name


def test_select_host_core(tmp_path):
    exe = tmp_path / "select_core_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split(),
                           os.path.join(ROOT, "tests", "native", "select_core_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stdout.decode()


def test_the_launch_shape_is_named_constants_of_the_kernel_header():
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_select_kernels.hpp")).read()
    blocks = re.search(r"constexpr\s+int\s+kSelectBlocks\s*=\s*(\d+)\s*;", text)
    threads = re.search(r"constexpr\s+int\s+kSelectThreads\s*=\s*(\d+)\s*;", text)
    assert blocks and threads
    assert int(threads.group(1)) % 64 == 0 and 64 <= int(threads.group(1)) <= 1024 and int(blocks.group(1)) >= 256
    assert "select_kernel<T, NA, true><<<kSelectBlocks, kSelectThreads" in open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_select.inc.hpp")).read()


def test_wrapper_builds_the_request(fp):
    s = fp._select_spec({"x": (0.25, 0.5), "v2": (1e-4, None), "vy": (None, 0.0)}, 1, (1000, 7))
    assert (s.species, s.nterms, list(s.axis)[:3], s.id_mod, s.id_rem) == (1, 3, [0, 6, 4], 1000, 7)
    assert list(s.lo)[:3] == [0.25, 1e-4, -math.inf] and list(s.hi)[:3] == [0.5, math.inf, 0.0]
    assert not any(s.reserved) and not any(list(s.axis)[3:]) and not any(list(s.lo)[3:]) and not any(list(s.hi)[3:])
    for empty in (None, {}):
        s = fp._select_spec(empty, 0, None)
        assert (s.species, s.nterms, s.id_mod, s.id_rem) == (0, 0, 0, 0)
    s = fp._select_spec({k: (-1, 1) for k in ("x", "y", "z", "vx", "vy", "vz", "v2")}, 0, None)
    assert s.nterms == 7 and sorted(s.axis)[1:] == [0, 1, 2, 3, 4, 5, 6]
    for bad, prop in ((dict(where={"w": (0, 1)}), ".axis"), (dict(where={"x": 3}), ".range"), (dict(where={"x": (0, 1, 2)}), ".range"),
                      (dict(where={"x": ("a", 1)}), ".range"), (dict(where=None, every=7), ".every"), (dict(where=None, every=(7,)), ".every"),
                      (dict(where=None, every=(7.5, 1)), ".every"), (dict(where=None, every=(-1, 0)), ".every"),
                      (dict(where=None, every=(1 << 32, 0)), ".every"), (dict(where=None, every=(True, 0)), ".every")):
        with pytest.raises(fp.FusionPicError) as e:
            fp._select_spec(bad["where"], 0, bad.get("every"))
        assert prop + " <- " in str(e.value), (bad, str(e.value))


def test_select_without_a_handle(fp):
    lib = fp.load_library()
    s = fp._select_spec({"vx": (0, 1)}, 0, None)
    matched = ctypes.c_uint64()
    assert lib.fpic_select(None, ctypes.byref(s), fp.DIAG_LOCAL, 0, None, None, None, fp.F32, ctypes.byref(matched)) == -1
    assert b"null handle" in lib.fpic_last_error(None)
