"""The modes diagnostic (fpic_modes_*) on a machine WITHOUT a GPU: the header declares the entry points and libfusionpic.so
exports them, fusionpic.ABI_FUNCTIONS lists them, the ctypes mirror has the C layout, the host rules
(fusion-sim_amd/csrc/fes_modes_core.hpp: the checks and their messages, the index reduction, the twiddle tables' two
properties, the launch shape, the ranks' sum) pass their g++ test, the library's tables are the Python restatement's bit for
bit, the Python wrapper builds a request, and a call without a handle fails cleanly.  The amplitudes themselves are checked
on the GPU (tests/test_gpu_modes.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import modes_reference as mr
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


def test_modes_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    for name in ("fpic_modes_now", "fpic_modes_record", "fpic_modes_history"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in fp.ABI_FUNCTIONS, name
    m = re.search(r"#define\s+FPIC_MODES_MAX\s+(\d+)u", text)
    assert m and int(m.group(1)) == fp.MODES_MAX == 256
    for b, name in enumerate(fp.MODE_FIELDS):
        assert re.search(r"#define\s+FPIC_MODE_%s\s+\(1u << %d\)" % (name.upper(), b), text), name
    assert re.search(r"#define\s+FPIC_ABI_VERSION\s+2\b", text)       # the ABI only grows
    assert fp.MODE_FIELDS == mr.FIELDS


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("%s %zu\n", #m, offsetof(fpic_modes_spec, m));
int main(void) {
    printf("sizeof %zu\n", sizeof(fpic_modes_spec));
    F(nmodes) F(mask) F(modes) F(reserved)
    return 0;
}
'''


def test_ctypes_mirror_matches_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(fp.ModesSpec) == 48
    for name, off in got.items():
        assert int(off) == getattr(fp.ModesSpec, name).offset, name


@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("modes") / "modes_core_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split(),
                           os.path.join(ROOT, "tests", "native", "modes_core_test.cpp"), "-o", str(exe)])
    return str(exe)


def test_modes_host_core(core_exe):
    out = subprocess.run([core_exe], capture_output=True, timeout=300)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stdout.decode()


@pytest.mark.parametrize("n", [2, 3, 6, 7, 8, 10, 12, 33, 256, 300])
def test_library_tables_are_the_restatement(core_exe, n):
    """n odd, n = 2, n no multiple of 4, powers of two: the table the library uploads, bit for bit"""
    lines = subprocess.check_output([core_exe, str(n)], timeout=60).decode().split()
    got = np.array([float.fromhex(v) for v in lines]).reshape(n, 2)
    assert got.tobytes() == mr.table(n).tobytes()


def test_wrapper_builds_the_request(fp):
    s, names, keep = fp._modes_spec([[1, 0, 0], [0, -2, 3]], ("phi", "ex", "rho"))
    assert (s.nmodes, s.mask) == (2, 0x89) and names == ["ex", "phi", "rho"]          # ascending bit order
    m = np.ctypeslib.as_array(ctypes.cast(s.modes, ctypes.POINTER(ctypes.c_int32)), (6,))
    assert m.tolist() == [1, 0, 0, 0, -2, 3]
    s, names, keep = fp._modes_spec(np.zeros((300, 3), dtype=np.int64), "ey")         # (over the limit: the library's refusal)
    assert (s.nmodes, s.mask) == (300, 2)
    s, names, keep = fp._modes_spec(None, ())                                         # (empty: the library's refusal)
    assert (s.nmodes, s.mask) == (0, 0) and not s.modes
    for bad in (dict(modes=[[1, 2]]), dict(modes=[1, 2, 3]), dict(modes=[[0.5, 0, 0]]), dict(modes=[[1 << 31, 0, 0]]),
                dict(modes=[[0, 0, 0]], fields=("ex", "jx"))):
        with pytest.raises(fp.FusionPicError) as e:
            fp._modes_spec(bad["modes"], bad.get("fields", ("ex",)))
        assert e.value.code == -1 and " <- " in str(e.value), bad
    rows = np.arange(2 * 3 * 2 * 2, dtype=np.float64).reshape(2, 3, 2, 2)
    d = fp._modes_dict(rows, ["ex", "rho"])
    assert d["ex"].shape == (2, 3) and d["rho"][1, 2] == complex(rows[1, 2, 1, 0], rows[1, 2, 1, 1])
    a, b = np.array([[1e16, 1.0]]), np.array([[1.0, 1e16]])
    assert fp._modes_sum([a, b, -a]).tolist() == [[(1e16 + 1.0) - 1e16, (1.0 + 1e16) - 1.0]]   # left to right, from member 0 on


def test_modes_without_a_handle(fp):
    lib = fp.load_library()
    s = fp.ModesSpec()
    n = ctypes.c_uint64()
    assert lib.fpic_modes_now(None, ctypes.byref(s), fp.DIAG_LOCAL, None) == -1
    assert b"null handle" in lib.fpic_last_error(None)
    assert lib.fpic_modes_record(None, ctypes.byref(s), 1, 8) == -1
    assert lib.fpic_modes_history(None, fp.DIAG_LOCAL, None, None, 0, ctypes.byref(n), None) == -1
