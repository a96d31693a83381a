"""The fluid moment grids (fpic_moments) on a machine WITHOUT a GPU: the header declares the entry point and
libfusionpic.so exports it, fusionpic.ABI_FUNCTIONS lists it, the ctypes mirrors have the C layout, the rule and the checks
of a request (fusion-sim_amd/csrc/fes_mom_core.hpp) pass their g++ test — the split against a 128-bit restatement —, the
Python wrapper names its masks as the header does, and a call without a handle fails cleanly.  The grids themselves are
checked on the GPU (tests/test_gpu_moments.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import moments_reference as mr
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


def test_moments_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+fpic_moments\s*\(", text)
    assert hasattr(ctypes.CDLL(LIB), "fpic_moments")
    assert "fpic_moments" in fp.ABI_FUNCTIONS
    for bit, name in enumerate(fp.MOMENT_NAMES):
        assert re.search(r"#define\s+FPIC_MOM_%s\s+\(1u << %d\)" % (name, bit), text), name
    assert fp.MOMENT_NAMES == mr.NAMES and len(fp.MOMENT_NAMES) == 10
    for name, key in (("ORDER0", "n"), ("ORDER1", "order1"), ("ORDER2", "order2")):
        m = re.search(r"#define\s+FPIC_MOM_%s\s+0x([0-9A-Fa-f]+)u" % name, text)
        assert m and int(m.group(1), 16) == fp.MOMENT_SETS[key] == mr.SETS[key]
    assert re.search(r"#define\s+FPIC_ABI_VERSION\s+2\b", text)       # the ABI only grows
    assert fp.MOM_ONE == mr.ONE == 1 << 42 and fp.MOM_SCALE == mr.SCALE == 1 << 32


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("spec.%s %zu\n", #m, offsetof(fpic_moments_spec, m));
#define G(m) printf("info.%s %zu\n", #m, offsetof(fpic_moments_info, m));
int main(void) {
    printf("sizeof.spec %zu\nsizeof.info %zu\n", sizeof(fpic_moments_spec), sizeof(fpic_moments_info));
    F(species) F(mask) F(reserved)
    G(rejected) G(spilled) G(reserved)
    return 0;
}
'''


def test_ctypes_mirrors_match_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got.pop("sizeof.spec")) == ctypes.sizeof(fp.MomentsSpec) == 40
    assert int(got.pop("sizeof.info")) == ctypes.sizeof(fp.MomentsInfo) == 32
    for name, off in got.items():
        kind, field = name.split(".")
        assert int(off) == getattr(fp.MomentsSpec if kind == "spec" else fp.MomentsInfo, field).offset, name


def test_mom_host_core(tmp_path):
    exe = tmp_path / "mom_core_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split(),
                           os.path.join(ROOT, "tests", "native", "mom_core_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stdout.decode()


def test_the_sweep_size_follows_a_named_budget_of_the_kernel_header():
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_mom_kernels.hpp")).read()
    m = re.search(r"constexpr\s+size_t\s+kMomLdsBudget\s*=\s*(\d+)\s*\*\s*1024\s*;", text)
    assert m and 17 * 17 * 9 * 8 + 16 <= int(m.group(1)) * 1024 <= 160 * 1024     # one 16 x 16 x 8 tile's window fits; within a CU's LDS


def test_wrapper_builds_the_mask(fp):
    assert fp._moments_mask("n") == 1 and fp._moments_mask("order1") == 0xF and fp._moments_mask("order2") == 0x3FF
    assert fp._moments_mask(["SYZ", "N"]) == 0x201 and fp._moments_mask(("FX",)) == 2
    assert fp._moments_mask([]) == 0                                   # (the library refuses it: .mask)
    for bad in ("order3", ["N", "W"], ["n"]):
        with pytest.raises(fp.FusionPicError) as e:
            fp._moments_mask(bad)
        assert ".which <- " in str(e.value)
    grids = np.arange(3 * 2 * 2 * 2, dtype=np.int64).reshape(3, 2, 2, 2)
    res = fp._moments_result(0x111, grids, 5, 7)
    assert sorted(res) == ["N", "SXX", "SXZ", "rejected", "spilled"] and res["rejected"] == 5 and res["spilled"] == 7
    assert res["N"] is not None and np.array_equal(res["SXX"], grids[1]) and np.array_equal(res["SXZ"], grids[2])


def test_moments_without_a_handle(fp):
    lib = fp.load_library()
    s = fp.MomentsSpec()
    s.mask = 1
    out, info = (ctypes.c_int64 * 8)(), fp.MomentsInfo()
    assert lib.fpic_moments(None, ctypes.byref(s), fp.DIAG_LOCAL, out, ctypes.byref(info)) == -1
    assert b"null handle" in lib.fpic_last_error(None)
