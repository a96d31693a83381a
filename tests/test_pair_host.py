"""The binary collision operator (fpic_pair*) on a machine WITHOUT a GPU: the header declares the entry points and
libfusionpic.so exports them, fusionpic.ABI_FUNCTIONS lists them, the ctypes mirrors have the C layout, the rule and the
checks of a request (fusion-sim_amd/csrc/fes_pair_core.hpp) pass their g++ test — also as a stand-alone program under
AddressSanitizer and UBSan —, the Python wrapper builds the request and refuses what the structure cannot carry, and a call
without a handle fails cleanly.  The collisions themselves are checked on the GPU (tests/test_gpu_pair.py)."""
import ctypes
import os
import re
import subprocess

import pytest

from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "fusionpic.h")
LIB = os.path.join(ROOT, "fusion-sim_amd", "lib", "libfusionpic.so")
NATIVE = os.path.join(ROOT, "tests", "native", "pair_core_test.cpp")
ENTRIES = {
    "fpic_pair": r"fpic_handle\s*\*\s*h\s*,\s*const\s+fpic_pair_spec\s*\*\s*spec\s*,\s*fpic_pair_result\s*\*\s*out",
    "fpic_pair_register": r"fpic_handle\s*\*\s*h\s*,\s*const\s+fpic_pair_spec\s*\*\s*spec\s*,\s*int\s+every\s*,\s*int\s*\*\s*index",
    "fpic_pair_stats": r"fpic_handle\s*\*\s*h\s*,\s*int\s+index\s*,\s*int\s+scope\s*,\s*fpic_pair_result\s*\*\s*out",
    "fpic_pair_clear": r"fpic_handle\s*\*\s*h",
}


@pytest.fixture(scope="module")
def fp():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import fusionpic
    return fusionpic


def test_pair_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    for name, args in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)" % (name, args), text), name
        assert hasattr(lib, name) and name in fp.ABI_FUNCTIONS
    for name, value in (("MAX_OPS", 8), ("CELL_MAX", 2048)):
        assert re.search(r"#define\s+FPIC_PAIR_%s\s+%d\b" % (name, value), text) and getattr(fp, "PAIR_" + name) == value


def test_the_cap_and_the_launch_shape_are_named_constants_of_the_kernel_header():
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_pair_kernels.hpp")).read()
    get = lambda name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    assert get("kPairCellMax") >= 2048 and get("kPairThreads") == 256 and get("kPairChunk") == 64 and get("kPairRankMax") == 64
    assert re.search(r"kPairEntries\s*=\s*2\s*\*\s*kPairCellMax", text)           # two full species of a cell fit a run
    # the run's LDS: three words and 16 bits per entry and the tables, within the 64 KiB that leave two workgroups on a CU
    assert (3 * 4 + 2) * 2 * get("kPairCellMax") + 4 * (2 * (get("kPairChunk") + 1) + 2) <= 64 * 1024


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("%s %zu\n", #m, offsetof(fpic_pair_spec, m));
#define R(m) printf("result.%s %zu\n", #m, offsetof(fpic_pair_result, m));
int main(void) {
    printf("sizeof %zu\n", sizeof(fpic_pair_spec));
    printf("result.sizeof %zu\n", sizeof(fpic_pair_result));
    F(species_a) F(species_b) F(seed) F(stream) F(epoch) F(log_lambda) F(tau) F(reserved)
    R(applications) R(pairs) R(strong) R(cells) R(overfull_cells) R(overfull_particles)
    return 0;
}
'''


def test_ctypes_mirrors_match_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(fp.PairSpec)
    assert int(got.pop("result.sizeof")) == ctypes.sizeof(fp.PairResult)
    result = {k[7:]: v for k, v in got.items() if k.startswith("result.")}
    spec = {k: v for k, v in got.items() if not k.startswith("result.")}
    for mirror, offsets in ((fp.PairSpec, spec), (fp.PairResult, result)):
        assert len(offsets) == len(mirror._fields_)
        for name, off in offsets.items():
            assert int(off) == getattr(mirror, name).offset, name


def _native(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, NATIVE, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, timeout=60, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stdout.decode() + out.stderr.decode()


def test_pair_host_core(tmp_path):
    _native(tmp_path, "pair_core_test", ["-O2", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split()])


def test_pair_host_core_under_sanitizers(tmp_path):
    # its own program with its own main: the sanitizers' runtime is linked into it, nothing is preloaded anywhere
    _native(tmp_path, "pair_core_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def test_wrapper_builds_the_request(fp):
    s = fp._pair_spec(2e-9, log_lambda=10)
    assert (s.species_a, s.species_b, s.seed, s.stream, s.epoch, s.log_lambda, s.tau) == (0, 0, fp.PAIR_SEED, 0, 0, 10.0, 2e-9)
    assert not any(s.reserved)
    s = fp._pair_spec(2e-9, 1, 0, log_lambda=12.5, tau=1e-8, seed=(1 << 64) - 1, stream=(1 << 32) - 1, epoch=(1 << 32) - 1)
    assert (s.species_a, s.species_b, s.seed, s.stream, s.epoch, s.log_lambda, s.tau) == (1, 0, (1 << 64) - 1, (1 << 32) - 1, (1 << 32) - 1, 12.5, 1e-8)
    assert fp._pair_spec(2e-9, 2, log_lambda=1).species_b == 2                      # b None: a with itself
    for bad, prop in ((dict(a=1 << 31), ".species_a"), (dict(a=0.5), ".species_a"), (dict(b=-(1 << 31) - 1), ".species_b"), (dict(b="x"), ".species_b"),
                      (dict(seed=-1), ".seed"), (dict(seed=1 << 64), ".seed"), (dict(stream=1 << 32), ".stream"), (dict(epoch=-1), ".epoch"),
                      (dict(epoch=0.5), ".epoch"), (dict(log_lambda="x"), ".log_lambda"), (dict(log_lambda=None), ".log_lambda"), (dict(tau="x"), ".tau"),
                      (dict(tau=[1, 2]), ".tau")):
        with pytest.raises(fp.FusionPicError) as e:
            fp._pair_spec(2e-9, **dict(dict(log_lambda=10.0), **bad))
        assert prop + " <- " in str(e.value), (bad, str(e.value))


def test_pair_without_a_handle(fp):
    lib = fp.load_library()
    s = fp._pair_spec(2e-9, log_lambda=10.0)
    out = fp.PairResult(7, 7, 7, 7, 7, 7)
    index = ctypes.c_int(77)
    assert lib.fpic_pair(None, ctypes.byref(s), ctypes.byref(out)) == -1
    assert b"null handle" in lib.fpic_last_error(None) and out.pairs == 7
    assert lib.fpic_pair_register(None, ctypes.byref(s), 1, ctypes.byref(index)) == -1 and index.value == 77
    assert lib.fpic_pair_stats(None, 0, 0, ctypes.byref(out)) == -1 and out.applications == 7
    assert lib.fpic_pair_clear(None) == -1
    assert b"null handle" in lib.fpic_last_error(None)
