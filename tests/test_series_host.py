"""The series diagnostic (fpic_series_*) on a machine WITHOUT a GPU: the header declares the entry points and
libfusionpic.so exports them, fusionpic.ABI_FUNCTIONS lists them, the ctypes mirror has the C layout, the host rules
(fusion-sim_amd/csrc/fes_series_core.hpp: request checks, the tracers' sorted tables and filter, the selection by flag) pass
their g++ test, the Python wrapper builds a request and selects among a group's members as the library does among ranks, and
a call without a handle fails cleanly.  The rows themselves are checked on the GPU (tests/test_gpu_series.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import series_reference as sr
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


def test_series_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    for name in ("fpic_series_now", "fpic_series_record", "fpic_series_history"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in fp.ABI_FUNCTIONS, name
    m = re.search(r"#define\s+FPIC_SERIES_MAX_POINTS\s+(\d+)u", text)
    assert m and int(m.group(1)) == fp.SERIES_MAX_POINTS == 4096
    m = re.search(r"#define\s+FPIC_SERIES_MAX_TRACERS\s+(\d+)u", text)
    assert m and int(m.group(1)) == fp.SERIES_MAX_TRACERS == 65536
    assert re.search(r"#define\s+FPIC_ABI_VERSION\s+2\b", text)       # the ABI only grows
    assert fp.SERIES_POINT_COLUMNS == sr.POINT_COLUMNS and fp.SERIES_TRACER_COLUMNS == sr.TRACER_COLUMNS


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("%s %zu\n", #m, offsetof(fpic_series_spec, m));
int main(void) {
    printf("sizeof %zu\n", sizeof(fpic_series_spec));
    F(npoints) F(ntracers) F(points) F(tracer_species) F(tracer_id) F(reserved)
    return 0;
}
'''


def test_ctypes_mirror_matches_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(fp.SeriesSpec) == 64
    for name, off in got.items():
        assert int(off) == getattr(fp.SeriesSpec, name).offset, name


def test_series_host_core(tmp_path):
    exe = tmp_path / "series_core_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split(),
                           os.path.join(ROOT, "tests", "native", "series_core_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stdout.decode()


def test_wrapper_builds_the_request(fp):
    s, keep = fp._series_spec(np.array([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]), [7, 3, 9], 1)
    assert (s.npoints, s.ntracers) == (2, 3)
    ids = np.ctypeslib.as_array(ctypes.cast(s.tracer_id, ctypes.POINTER(ctypes.c_uint32)), (3,))
    sp = np.ctypeslib.as_array(ctypes.cast(s.tracer_species, ctypes.POINTER(ctypes.c_int32)), (3,))
    pts = np.ctypeslib.as_array(ctypes.cast(s.points, ctypes.POINTER(ctypes.c_double)), (6,))
    assert ids.tolist() == [7, 3, 9] and sp.tolist() == [1, 1, 1] and pts.tolist() == [0, 1, 2, 3, 4, 5]
    s, keep = fp._series_spec(None, np.array([4, 5], dtype=np.uint32), [0, 2])
    assert (s.npoints, s.ntracers) == (0, 2) and not s.points
    assert np.ctypeslib.as_array(ctypes.cast(s.tracer_species, ctypes.POINTER(ctypes.c_int32)), (2,)).tolist() == [0, 2]
    s, keep = fp._series_spec(None, None, 0)
    assert (s.npoints, s.ntracers) == (0, 0)                              # (the library refuses it: both lists empty)
    s, keep = fp._series_spec(np.zeros((5000, 3)), np.arange(70000), 0)   # (over the limits: the library's refusal, not the wrapper's)
    assert (s.npoints, s.ntracers) == (5000, 70000)
    for bad in (dict(points=np.zeros((2, 2))), dict(points=np.zeros(3)), dict(tracers=[1.5]), dict(tracers=[-1]), dict(tracers=[1 << 32]),
                dict(tracers=[[1, 2]]), dict(tracers=[1, 2], species=[0]), dict(tracers=[1], species=0.5)):
        with pytest.raises(fp.FusionPicError) as e:
            fp._series_spec(bad.get("points"), bad.get("tracers"), bad.get("species", 0))
        assert e.value.code == -1 and " <- " in str(e.value), bad


def test_selection_among_members(fp):
    a, b, c = np.zeros((2, 3, 8)), np.zeros((2, 3, 8)), np.zeros((2, 3, 8))
    a[0, 0] = [-0.0, 1, 2, 3, 4, 5, 1, 0]
    b[0, 1] = [9, 8, 7, 6, 5, 4, 1, 0]
    c[1, 0] = [np.nan, 0, 0, 0, 0, 0, 1, 0]
    b[1, 2, 0] = 5.0                                                       # values without a flag are nobody's
    out, owner = fp._series_select([a, b, c], 6)
    assert owner.tolist() == [[0, 1, -1], [2, -1, -1]]
    assert out[0, 0].tobytes() == a[0, 0].tobytes() and out[0, 1].tobytes() == b[0, 1].tobytes() and out[1, 0].tobytes() == c[1, 0].tobytes()
    assert not out[0, 2].any() and not out[1, 1:].any()
    c[0, 1, 6] = 1.0                                                       # two members flag one entry: reported
    with pytest.raises(fp.FusionPicError, match="two members"):
        fp._series_select([a, b, c], 6)
    out, owner = fp._series_select([np.zeros((0, 4, 8))] * 2, 7)            # no rows: nothing to select
    assert out.shape == (0, 4, 8) and owner.shape == (0, 4)


def test_series_without_a_handle(fp):
    lib = fp.load_library()
    s = fp.SeriesSpec()
    n = ctypes.c_uint64()
    assert lib.fpic_series_now(None, ctypes.byref(s), fp.DIAG_LOCAL, None, None) == -1
    assert b"null handle" in lib.fpic_last_error(None)
    assert lib.fpic_series_record(None, ctypes.byref(s), 1, 8) == -1
    assert lib.fpic_series_history(None, fp.DIAG_LOCAL, None, None, None, 0, ctypes.byref(n), None) == -1
