"""The absorbing particle sinks (fpic_remove*, fpic_renumber) on a machine WITHOUT a GPU: the header declares the five entry
points and libfusionpic.so exports them, fusionpic.ABI_FUNCTIONS lists them, the ABI version is still 2, the ctypes mirrors
of fpic_remove_spec and fpic_remove_result have the C layout, the rule and the checks of a request
(fusion-sim_amd/csrc/fes_remove_core.hpp) pass their g++ test, the launch shape is named constants of the kernel header, the
Python wrapper refuses what the structure cannot carry, and a call without a handle fails cleanly.  The removals themselves
are checked on the GPU (tests/test_gpu_remove.py)."""
import ctypes
import math
import os
import re
import subprocess

import pytest

from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "fusionpic.h")
LIB = os.path.join(ROOT, "fusion-sim_amd", "lib", "libfusionpic.so")
NAMES = ("fpic_remove", "fpic_remove_register", "fpic_remove_stats", "fpic_remove_clear", "fpic_renumber")


@pytest.fixture(scope="module")
def fp():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import fusionpic
    return fusionpic


def test_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in fp.ABI_FUNCTIONS, name
    assert re.search(r"#define\s+FPIC_REMOVE_OUTSIDE\s+1u\b", text) and fp.REMOVE_OUTSIDE == 1
    assert re.search(r"#define\s+FPIC_REMOVE_MAX_OPS\s+8\b", text) and fp.REMOVE_MAX_OPS == 8
    assert re.search(r"#define\s+FPIC_ABI_VERSION\s+2\b", text)


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("spec.%s %zu\n", #m, offsetof(fpic_remove_spec, m));
#define G(m) printf("result.%s %zu\n", #m, offsetof(fpic_remove_result, m));
int main(void) {
    printf("spec.sizeof %zu\n", sizeof(fpic_remove_spec));
    printf("result.sizeof %zu\n", sizeof(fpic_remove_result));
    F(species) F(nterms) F(axis) F(lo) F(hi) F(id_mod) F(id_rem) F(flags) F(reserved_u) F(reserved)
    G(applications) G(scanned) G(removed) G(energy_fixed) G(momentum_fixed) G(energy) G(momentum) G(charge)
    return 0;
}
'''


def test_ctypes_mirrors_match_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for prefix, mirror in (("spec", fp.RemoveSpec), ("result", fp.RemoveResult)):
        mine = {k.split(".", 1)[1]: int(v) for k, v in got.items() if k.startswith(prefix + ".")}
        assert mine.pop("sizeof") == ctypes.sizeof(mirror)
        assert len(mine) == len(mirror._fields_)
        for name, off in mine.items():
            assert off == getattr(mirror, name).offset, (prefix, name)
    # the predicate's fields lie where fpic_select_spec has them
    for name in ("species", "nterms", "axis", "lo", "hi", "id_mod", "id_rem"):
        assert getattr(fp.RemoveSpec, name).offset == getattr(fp.SelectSpec, name).offset


def test_remove_host_core(tmp_path):
    exe = tmp_path / "remove_core_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split(),
                           os.path.join(ROOT, "tests", "native", "remove_core_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, timeout=60)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stdout.decode()


def test_the_launch_shape_is_named_constants_of_the_kernel_header():
    import remove_scenes as rs
    assert rs.THREADS % 64 == 0 and 64 <= rs.THREADS <= 1024 and rs.BLOCKS >= 256
    assert rs.CHUNK % (64 * 2 * 4) == 0      # whole turns of two 16-byte vectors per lane, in either precision
    host = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_remove.inc.hpp")).read()
    assert "kRemoveBlocks" in host and "kRemoveChunk" in host and "load_scan_kernel<<<1, 1024" in host
    scan = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_load_kernels.hpp")).read()
    assert re.search(r"at \+= %d\b" % rs.SCAN_TURN, scan)      # the scan's turn is what the boundary cases assume


def test_wrapper_builds_the_request(fp):
    s = fp._remove_spec({"x": (0.25, 0.5), "v2": (1e-4, None), "vy": (None, 0.0)}, 1, (1000, 7), True)
    assert (s.species, s.nterms, list(s.axis)[:3], s.id_mod, s.id_rem, s.flags, s.reserved_u) == (1, 3, [0, 6, 4], 1000, 7, fp.REMOVE_OUTSIDE, 0)
    assert list(s.lo)[:3] == [0.25, 1e-4, -math.inf] and list(s.hi)[:3] == [0.5, math.inf, 0.0]
    assert not any(s.reserved) and not any(list(s.axis)[3:]) and not any(list(s.lo)[3:]) and not any(list(s.hi)[3:])
    s = fp._remove_spec(None, 0, None, False)
    assert (s.species, s.nterms, s.id_mod, s.id_rem, s.flags) == (0, 0, 0, 0, 0)
    for bad, prop in ((dict(where={"w": (0, 1)}), ".axis"), (dict(where={"x": 3}), ".range"), (dict(every=7), ".every"), (dict(every=(True, 0)), ".every"),
                      (dict(outside=1), ".outside"), (dict(outside=None), ".outside")):
        with pytest.raises(fp.FusionPicError) as e:
            fp._remove_spec(bad.get("where"), 0, bad.get("every"), bad.get("outside", False))
        assert prop + " <- " in str(e.value), (bad, str(e.value))


def test_without_a_handle(fp):
    lib = fp.load_library()
    s, out, n, index = fp._remove_spec({"vx": (0, 1)}, 0, None, False), fp.RemoveResult(), ctypes.c_uint64(), ctypes.c_int()
    calls = [lambda: lib.fpic_remove(None, ctypes.byref(s), ctypes.byref(out)), lambda: lib.fpic_remove_register(None, ctypes.byref(s), 1, ctypes.byref(index)),
             lambda: lib.fpic_remove_stats(None, 0, fp.DIAG_LOCAL, ctypes.byref(out)), lambda: lib.fpic_remove_clear(None),
             lambda: lib.fpic_renumber(None, 0, ctypes.byref(n))]
    for call in calls:
        assert call() == -1
        assert b"null handle" in lib.fpic_last_error(None)


def test_the_group_refuses_by_name(fp):
    group = fp.BoxGroup.__new__(fp.BoxGroup)
    for call in (group.remove, lambda: group.removeEvery(1), lambda: group.removeStats(0), group.clearRemovals, group.renumber):
        with pytest.raises(fp.FusionPicError) as e:
            call()
        assert e.value.code == -5 and "undecomposed" in str(e.value)
