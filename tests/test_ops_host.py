"""What the registered operators of the box share (fusion-sim_amd/csrc/fes_ops_core.hpp) on a machine WITHOUT a GPU: the
registration and index checks of all eight families pass their g++ test — also as a stand-alone program under
AddressSanitizer and UBSan —, the families' limits are the header's and the wrapper's, and no family keeps a copy of the
checks.  The rows and the hook are checked on the GPU (tests/test_gpu_ops_rows.py and the sequences modules)."""
import glob
import os
import re
import subprocess

from helpers import ROOT

HEADER = os.path.join(ROOT, "include", "fusionpic.h")
CSRC = os.path.join(ROOT, "fusion-sim_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native", "ops_core_test.cpp")
FAMILIES = ("FORCE", "COLLIDE", "GAS", "PAIR", "FUSION", "FUSION_SPECTRUM", "REMOVE", "INJECT")      # the hook's order


def _native(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *flags, NATIVE, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, timeout=60, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", out.stdout.decode() + out.stderr.decode()


def test_ops_host_core(tmp_path):
    _native(tmp_path, "ops_core_test", ["-O2", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split()])


def test_ops_host_core_under_sanitizers(tmp_path):
    # its own program with its own main: the sanitizers' runtime is linked into it, nothing is preloaded anywhere
    _native(tmp_path, "ops_core_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def test_the_table_holds_the_headers_limits_in_the_hooks_order():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    core = open(os.path.join(CSRC, "fes_ops_core.hpp")).read()
    rows = re.findall(r"\{ FPIC_(\w+)_MAX_OPS, \".spec <- FPIC_(\w+)_MAX_OPS \((\d+)\) (\w+) are registered already\", \".index <- no such registered (\w+)\" \}", core)
    assert [r[0] for r in rows] == list(FAMILIES) and all(r[0] == r[1] for r in rows)
    for name, _, count, plural, noun in rows:
        assert re.search(r"#define\s+FPIC_%s_MAX_OPS\s+%s\b" % (name, count), header), name
        assert plural == noun + "s"
    enum = re.search(r"enum Family \{([^}]*)\}", core).group(1)
    assert [x.strip() for x in enum.split(",")] == ["kForce", "kCollide", "kGas", "kPair", "kFusion", "kFspec", "kRemove", "kInject", "kFamilies"]


def test_no_family_keeps_a_copy_of_the_checks_or_moves_a_tally_row_itself():
    for path in sorted(glob.glob(os.path.join(CSRC, "fes_*_core.hpp"))):
        if os.path.basename(path) != "fes_ops_core.hpp":
            assert not re.search(r"\bcheck_(register|index)\b", open(path).read()), path
    for name in ("collide", "force", "gas", "pair", "fusion", "fusion_spectrum", "remove", "inject"):
        text = open(os.path.join(CSRC, "fes_%s.inc.hpp" % name)).read()
        assert not re.search(r"fes\w+::check_(register|index)\b", text), name
        assert not re.search(r"hipMem(set|cpy)Async\([^;]*(\brow\(|Words\b)", text), name      # (a row is zeroed and fetched by OpRows)
