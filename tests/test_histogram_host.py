"""The phase-space histograms (fpic_histogram) on a machine WITHOUT a GPU: the header declares the entry point and
libfusionpic.so exports it, fusionpic.ABI_FUNCTIONS lists it, the ctypes mirror of fpic_hist_spec has the C layout, the bin
rule and the checks of a request (fusion-sim_amd/csrc/fes_hist_core.hpp) pass their g++ test, the Python wrapper refuses
what the structure cannot carry, and a call without a handle fails cleanly.  The counts themselves are checked on the GPU
(tests/test_gpu_histogram.py)."""
import ctypes
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


def test_histogram_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+fpic_histogram\s*\(", text)
    assert hasattr(ctypes.CDLL(LIB), "fpic_histogram")
    assert "fpic_histogram" in fp.ABI_FUNCTIONS
    assert re.search(r"#define\s+FPIC_HIST_MAX_BINS\s+\(1u << 22\)", text) and fp.HIST_MAX_BINS == 1 << 22
    for name, code in fp.HIST_AXES.items():
        assert re.search(r"#define\s+FPIC_AXIS_%s\s+%d\b" % (name.upper(), code), text), name
    assert len(fp.HIST_AXES) == 7


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("%s %zu\n", #m, offsetof(fpic_hist_spec, m));
int main(void) {
    printf("sizeof %zu\n", sizeof(fpic_hist_spec));
    F(species) F(naxes) F(axis) F(bins) F(lo) F(hi) F(reserved)
    return 0;
}
'''


def test_ctypes_mirror_matches_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(fp.HistSpec)
    for name, off in got.items():
        assert int(off) == getattr(fp.HistSpec, name).offset, name


def test_hist_host_core(tmp_path):
    exe = tmp_path / "hist_core_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split(),
                           os.path.join(ROOT, "tests", "native", "hist_core_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stdout.decode()


def test_the_lds_limit_is_a_named_constant_of_the_kernel_header():
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_hist_kernels.hpp")).read()
    m = re.search(r"constexpr\s+uint32_t\s+kHistLdsBins\s*=\s*(\d+)\s*;", text)
    assert m and 1 <= int(m.group(1)) * 4 <= 160 * 1024      # uint32 bins within a CU's LDS


def test_wrapper_builds_the_request(fp):
    s, shape, rg = fp._hist_spec("vx", 1024, (-0.1, 0.1), 1)
    assert (s.species, s.naxes, s.axis[0], s.bins[0], s.lo[0], s.hi[0]) == (1, 1, 3, 1024, -0.1, 0.1) and shape == (1024,)
    assert not any(s.reserved)
    s, shape, rg = fp._hist_spec(("z", "v2"), (8, 5), ((0, 1), (0, 0.01)), 0)
    assert (s.naxes, list(s.axis), list(s.bins), list(s.lo), list(s.hi)) == (2, [2, 6], [8, 5], [0.0, 0.0], [1.0, 0.01]) and shape == (8, 5)
    s, shape, rg = fp._hist_spec(("x", "vx"), 16, ((0, 1), (-1, 1)), 0)
    assert list(s.bins) == [16, 16]
    res = fp._hist_result(None, 0, (4,), rg[:1])
    assert res["edges"][0].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    for bad, prop in ((dict(axes="w", bins=4, range=(0, 1)), ".axis"), (dict(axes=("x", "y", "z"), bins=4, range=((0, 1),) * 3), ".naxes"),
                      (dict(axes=(), bins=4, range=()), ".naxes"), (dict(axes="x", bins=(4, 4), range=(0, 1)), ".bins"),
                      (dict(axes="x", bins=2.5, range=(0, 1)), ".bins"), (dict(axes="x", bins=1 << 40, range=(0, 1)), ".bins"),
                      (dict(axes=("x", "vx"), bins=4, range=(0, 1)), ".range")):
        with pytest.raises(fp.FusionPicError) as e:
            fp._hist_spec(species=0, **bad)
        assert prop + " <- " in str(e.value), (bad, str(e.value))


def test_histogram_without_a_handle(fp):
    lib = fp.load_library()
    s, _, _ = fp._hist_spec("vx", 4, (0, 1), 0)
    counts, outside = (ctypes.c_uint64 * 4)(), ctypes.c_uint64()
    assert lib.fpic_histogram(None, ctypes.byref(s), fp.DIAG_LOCAL, counts, ctypes.byref(outside)) == -1
    assert b"null handle" in lib.fpic_last_error(None)
