"""The electron-impact ionisation (fpic_ionize*) on a machine WITHOUT a GPU: the header declares the four entry points and
libfusionpic.so exports them, the ABI version stays 2, the ctypes mirrors have the C layout, the rule and the checks of a
request (fusion-sim_amd/csrc/fes_ionize_core.hpp) pass their g++ test — every refusal by its message, the threshold, the
species rules and the fit rule on both sides of every bound — and give, bit for bit, what the numpy reference
(tests/ionize_reference.py) gives on cases whose rounded functions do not enter (vth = 0: the decisions, the ranks, the ids,
the ions' velocities, the copied positions and the counts are all exact) — also as a stand-alone program under
AddressSanitizer and UBSan —, the family keeps its own messages beside the shared table, the launch shape is a named
constant, the Python wrapper builds the request, and a call without a handle fails cleanly.  The passes themselves are
checked on the GPU (tests/test_gpu_ionize.py)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ionize_reference as ref
import ionize_scenes as sc
from helpers import ROOT
from test_gas_reference import DT, G_HI, G_LO, L, TABLE, TAPERS, WINDOW, density_for, scene

HEADER = os.path.join(ROOT, "include", "fusionpic.h")
LIB = os.path.join(ROOT, "fusion-sim_amd", "lib", "libfusionpic.so")
NATIVE = os.path.join(ROOT, "tests", "native", "ionize_core_test.cpp")
CSRC = os.path.join(ROOT, "fusion-sim_amd", "csrc")
ENTRIES = {
    "fpic_ionize": r"fpic_handle\s*\*\s*h\s*,\s*const\s+fpic_ionize_spec\s*\*\s*spec\s*,\s*fpic_ionize_result\s*\*\s*out",
    "fpic_ionize_register": r"fpic_handle\s*\*\s*h\s*,\s*const\s+fpic_ionize_spec\s*\*\s*spec\s*,\s*int\s+every\s*,\s*int\s*\*\s*index",
    "fpic_ionize_stats": r"fpic_handle\s*\*\s*h\s*,\s*int\s+index\s*,\s*int\s+scope\s*,\s*fpic_ionize_result\s*\*\s*out",
    "fpic_ionize_clear": r"fpic_handle\s*\*\s*h",
}


@pytest.fixture(scope="module")
def fp():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import fusionpic
    return fusionpic


def test_ionize_declared_exported_and_listed(fp):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(LIB)
    for name, args in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)" % (name, args), text), name
        assert hasattr(lib, name) and name in fp.ABI_FUNCTIONS
    assert re.search(r"#define\s+FPIC_IONIZE_MAX_OPS\s+8\b", text) and fp.IONIZE_MAX_OPS == ref.MAX_OPS == 8
    assert re.search(r"#define\s+FPIC_ABI_VERSION\s+2\b", text) and lib.fpic_abi_version() == 2


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "fusionpic.h"
#define F(m) printf("%s %zu\n", #m, offsetof(fpic_ionize_spec, m));
#define G(m) printf("gain.%s %zu\n", #m, offsetof(fpic_ionize_gain, m));
#define R(m) printf("result.%s %zu\n", #m, offsetof(fpic_ionize_result, m));
int main(void) {
    printf("sizeof %zu\n", sizeof(fpic_ionize_spec));
    printf("gain.sizeof %zu\n", sizeof(fpic_ionize_gain));
    printf("result.sizeof %zu\n", sizeof(fpic_ionize_result));
    F(species) F(electron) F(ion) F(reserved_i) F(seed) F(stream) F(epoch) F(density) F(tau) F(g_lo) F(g_hi) F(g_threshold) F(n) F(reserved_n) F(sigma) F(drift) F(vth)
    F(lo) F(hi) F(taper_n) F(reserved_u) F(taper) F(reserved)
    G(energy_fixed) G(momentum_fixed) G(energy) G(momentum) G(charge)
    R(applications) R(candidates) R(below) R(above) R(ionised) R(primary) R(electron) R(ion)
    return 0;
}
'''


def test_ctypes_mirrors_match_the_c_layout(fp, tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for prefix, mirror in (("result.", fp.IonizeResult), ("gain.", fp.IonizeGain), ("", fp.IonizeSpec)):
        mine = {k[len(prefix):]: int(v) for k, v in got.items() if k.startswith(prefix) and (prefix or "." not in k)}
        assert mine.pop("sizeof") == ctypes.sizeof(mirror), prefix
        assert len(mine) == len(mirror._fields_), prefix
        for name, off in mine.items():
            assert off == getattr(mirror, name).offset, prefix + name


# ---- the cases of the g++ program and what the reference gives for them: vth = 0, so the partner is the drift, g one square
# root, and the host's log, sin and cos enter nothing that is compared
def cases():
    frac, vel = scene(3001)
    drift = (0.01, 0.0, -0.02)
    base = dict(tau=DT, sigma=TABLE, g_lo=G_LO, g_hi=G_HI, g_threshold=0.04, drift=drift, vth=0.0, stream=3, epoch=9)
    at = lambda p: density_for(p * 2.0 ** 32, TABLE, G_LO, G_HI)
    flat = np.full(2, 3.0e-19)
    rng = np.random.default_rng(17)
    ids = np.arange(3001, dtype=np.uint32)
    thinned = np.sort(rng.permutation(9000)[:3001]).astype(np.uint32)        # a thinned species: ids below a span of 9001, not a multiple of 32
    shuffled = rng.permutation(3001).astype(np.uint32)                       # a binned species: the slots are not in id order
    # (dtype, keywords, ids, id span, n_e, span_e, n_i, span_i, fractions, velocities)
    return [
        (np.float32, dict(base, density=at(0.3), seed=11), ids, 3001, 3001, 3001, 10, 10, frac, vel),
        (np.float64, dict(base, density=at(0.3), seed=12, **WINDOW), thinned, 9001, 3001, 9001, 0, 77, frac, vel),
        (np.float32, dict(base, density=at(0.9), seed=13, taper=TAPERS, **WINDOW), shuffled, 3001, 5, 5, 7, 9, frac, vel),
        (np.float64, dict(base, density=1e30, seed=16, sigma=flat, g_lo=0.04, g_hi=0.15), shuffled, 3001, 1, 1, 2, 2, frac, vel),   # P_max = 1: K = 2^32
        (np.float32, dict(base, density=1e30, seed=18, sigma=flat, g_lo=0.04, g_hi=0.5, g_threshold=0.04), ids[:64] + (1 << 20), (1 << 20) + 64, 1, (1 << 32) - 1 - 64, 2, 2, frac[:64], vel[:64]),
        (np.float64, dict(base, density=0.0, seed=17), ids[:64], 64, 64, 64, 0, 0, frac[:64], vel[:64]),               # K = 0
    ]


def cases_and_expectations():
    blob, want, all_cases = [], [], cases()
    for dtype, kw, ids, span, n_e, span_e, n_i, span_i, frac, vel in all_cases:
        req = ref.request(L, **kw)
        lo, hi = kw.get("lo", (0.0, 0.0, 0.0)), kw.get("hi", L)
        taper = kw.get("taper", (None, None, None))
        S = np.asarray(kw["sigma"], dtype=np.float64)
        n = len(frac)
        blob.append(struct.pack("<iiQII", len(S), int(dtype == np.float64), kw["seed"], kw["stream"], kw["epoch"]))
        blob.append(np.array([kw["density"], kw["tau"], kw["g_lo"], kw["g_hi"], kw["g_threshold"], *req["drift"], *L, *lo, *hi], dtype=np.float64).tobytes())
        blob.append(struct.pack("<4I", *[0 if t is None else len(t) for t in taper], 0))
        blob.append(S.tobytes())
        blob += [np.asarray(t, dtype=np.float64).tobytes() for t in taper if t is not None]
        blob.append(struct.pack("<5QI", n_e, span_e, n_i, span_i, span, n))
        blob.append(np.asarray(ids, dtype=np.uint32).tobytes())
        stored_v = vel.astype(dtype)
        blob.append(np.concatenate([frac, stored_v.astype(np.float64)], axis=1).tobytes())
        app = ref.application(req, ids, frac.astype(dtype), stored_v, n_e, span_e, n_i, span_i)
        what = app["event"] * 1 + app["below"] * 2 + app["above"] * 4
        rows = np.stack([app["candidate"].astype(np.uint64), what.astype(np.uint64), (app["rank"] + 1).astype(np.uint64)], axis=1)
        c = ref.counts(app)
        m = app["m"]
        new = np.empty((m, 10), dtype=np.uint64)
        new[:, 0], new[:, 1], new[:, 2], new[:, 3] = app["electron"]["slot"], app["electron"]["id"], app["ion"]["slot"], app["ion"]["id"]
        new[:, 4:7] = app["electron"]["position"].astype(np.float64).view(np.uint64)
        new[:, 7:10] = app["ion"]["velocity"].astype(np.float64).view(np.uint64)
        assert np.array_equal(app["ion"]["position"], app["electron"]["position"])
        if m:
            assert np.array_equal(app["ion"]["velocity"], np.tile(np.array(kw["drift"]).astype(dtype), (m, 1)))     # the ion's velocity is the drift
        head = np.array([req["column"], req["x_max"]], dtype=np.float64).view(np.uint64)
        tail = np.array([c["candidates"], c["below"], c["above"], c["ionised"]], dtype=np.uint64)
        want.append(np.concatenate([head, [np.uint64(req["K"])], rows.ravel(), tail, new.ravel()]))
    return struct.pack("<I", len(all_cases)) + b"".join(blob), want, all_cases


def _native(tmp_path, name, flags):
    exe, cases_file, out = tmp_path / name, tmp_path / (name + ".in"), tmp_path / (name + ".out")
    blob, want, all_cases = cases_and_expectations()
    cases_file.write_bytes(blob)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, NATIVE, "-o", str(exe)])
    run = subprocess.run([str(exe), str(cases_file), str(out)], capture_output=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0 and run.stdout.decode().strip() == "ok", run.stdout.decode() + run.stderr.decode()
    got = np.frombuffer(out.read_bytes(), dtype=np.uint64)
    whole = np.concatenate(want)
    assert got.size == whole.size
    differ = np.flatnonzero(got != whole)
    assert differ.size == 0, (differ.size, differ[:5], got[differ[:5]], whole[differ[:5]])
    # the cases cover what they are meant to: both precisions, the whole box and the window, tapers, thinned and shuffled ids,
    # K = 2^32 and K = 0, every outcome, events in all but the last
    tails = [w[3 + 3 * len(c[8]):3 + 3 * len(c[8]) + 4] for w, c in zip(want, all_cases)]
    assert all(t[0] > 0 and t[1] > 0 and t[3] > 0 for t in tails[:5]) and tails[3][2] > 0 and not tails[5].any()
    assert want[3][2] == 1 << 32 and tails[3][0] == 3001 and want[5][2] == 0
    assert tails[1][0] < tails[0][0]                                      # the window keeps candidates out


def test_ionize_host_core(tmp_path):
    _native(tmp_path, "ionize_core_test", ["-O2", *os.environ.get("FPIC_NATIVE_CXXFLAGS", "").split()])


def test_ionize_host_core_under_sanitizers(tmp_path):
    # its own program with its own main: the sanitizers' runtime is linked into it, nothing is preloaded anywhere
    _native(tmp_path, "ionize_core_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def test_the_family_keeps_its_own_messages_and_the_shared_table_its_eight():
    core = open(os.path.join(CSRC, "fes_ops_core.hpp")).read()
    assert "IONIZE" not in core and "kIonize" not in core
    inc = open(os.path.join(CSRC, "fes_ionize.inc.hpp")).read()
    m = re.search(r"\{ FPIC_IONIZE_MAX_OPS, \".spec <- FPIC_IONIZE_MAX_OPS \((\d+)\) (\w+) are registered already\", \".index <- no such registered (\w+)\" \}", inc)
    assert m and m.group(1) == "8" and m.group(2) == "ionisers" and m.group(3) == "ioniser"
    assert not re.search(r"\bcheck_(register|index)\b", open(os.path.join(CSRC, "fes_ionize_core.hpp")).read())
    assert not re.search(r"fes\w+::check_(register|index)\b", inc)
    assert not re.search(r"hipMem(set|cpy)Async\([^;]*(\brow\(|Words\b)", inc)      # (a row is zeroed and fetched by OpRows)
    state = open(os.path.join(CSRC, "fes_state.inc.hpp")).read()
    families = re.search(r"#define FES_OP_FAMILIES\(X\) (.*)", state).group(1).split()
    assert families[-1] == "X(ionize)" and families[-2] == "X(inject)" and "OpFamily<IonizeOp> ionize;" in state      # the ionisers run last


def test_the_launch_shapes_are_named_constants_of_the_kernel_header():
    text = open(os.path.join(CSRC, "fes_ionize_kernels.hpp")).read()
    assert sc.THREADS == 256 and sc.BLOCKS == 2048 and sc.GAS_THREADS == 256 and sc.GAS_BLOCKS == 2048 and sc.SCAN_CHUNK == 2048
    assert "<<<" not in text and "asm" not in text
    inc = open(os.path.join(CSRC, "fes_ionize.inc.hpp")).read()
    assert re.search(r"<<<grid, kGasThreads, 0,", inc) and re.search(r"<<<ggrid, kIonizeThreads, 0,", inc)


def test_wrapper_builds_the_request(fp):
    box = [0.008, 0.016, 0.004]
    s, keep = fp._ionize_spec(2e-9, box, ion=1, g_threshold=0.01, density=1e20, sigma=[1e-19, 2e-19], g_lo=0.02, g_hi=0.5)
    assert (s.species, s.electron, s.ion, s.seed, s.stream, s.epoch, s.n, s.reserved_i, s.reserved_n, s.reserved_u) == (0, 0, 1, fp.IONIZE_SEED, 0, 0, 2, 0, 0, 0)
    assert (s.density, s.tau, s.g_lo, s.g_hi, s.g_threshold) == (1e20, 2e-9, 0.02, 0.5, 0.01) and [s.sigma[0], s.sigma[1]] == [1e-19, 2e-19]
    assert list(s.lo) == [0, 0, 0] and list(s.hi) == box and list(s.drift) == [0, 0, 0] and list(s.vth) == [0, 0, 0]
    assert list(s.taper_n) == [0, 0, 0] and not any(bool(p) for p in s.taper) and not any(s.reserved) and len(keep) == 1
    s, keep = fp._ionize_spec(2e-9, box, species=1, electron=2, ion=0, g_threshold=0.1, density=3.0, tau=7.0, sigma=np.arange(5, dtype=np.float32), g_lo=0.1, g_hi=0.2,
                              drift=(1, 2, 3), vth=0.5, lo=(0.001, 0, 0), hi=0.004, taper=(None, [0, 1, 0.5], np.ones(4)), seed=(1 << 64) - 1, stream=7, epoch=(1 << 32) - 1)
    assert (s.species, s.electron, s.ion, s.seed, s.stream, s.epoch, s.n) == (1, 2, 0, (1 << 64) - 1, 7, (1 << 32) - 1, 5)
    assert (s.density, s.tau, s.g_lo, s.g_hi, s.g_threshold) == (3.0, 7.0, 0.1, 0.2, 0.1) and [s.sigma[k] for k in range(5)] == [0, 1, 2, 3, 4]
    assert list(s.drift) == [1, 2, 3] and list(s.vth) == [0.5] * 3 and list(s.lo) == [0.001, 0, 0] and list(s.hi) == [0.004] * 3
    assert list(s.taper_n) == [0, 3, 4] and not bool(s.taper[0]) and [s.taper[1][k] for k in range(3)] == [0, 1, 0.5] and s.taper[2][3] == 1.0 and len(keep) == 3
    good = dict(ion=1, g_threshold=0.01, density=1e20, sigma=[1e-19, 2e-19], g_lo=0.02, g_hi=0.5)
    for bad, prop in ((dict(ion=None), ".ion"), (dict(ion=1.5), ".ion"), (dict(electron="e"), ".electron"), (dict(species=1 << 31), ".species"), (dict(g_threshold=None), ".g_threshold"),
                      (dict(g_threshold="x"), ".g_threshold"), (dict(epoch=-1), ".epoch"), (dict(seed=1 << 64), ".seed"), (dict(density=None), ".density"), (dict(sigma=None), ".sigma"),
                      (dict(g_lo=None), ".g_lo"), (dict(drift=(0, 1)), ".drift"), (dict(taper=[None, None]), ".taper")):
        with pytest.raises(fp.FusionPicError) as e:
            fp._ionize_spec(2e-9, box, **dict(good, **bad))
        assert prop + " <- " in str(e.value), (bad, str(e.value))
    for name in ("ionize", "ionizeEvery", "ionizeStats", "clearIonization"):
        assert callable(getattr(fp.CylindricalParticlePusher, name)) and callable(getattr(fp.BoxGroup, name))


def test_the_group_refuses_by_name(fp):
    g = fp.BoxGroup.__new__(fp.BoxGroup)
    for name, call in (("ionize", lambda: g.ionize(ion=1)), ("ionizeEvery", lambda: g.ionizeEvery(1, ion=1)), ("ionizeStats", lambda: g.ionizeStats(0)),
                       ("clearIonization", lambda: g.clearIonization())):
        with pytest.raises(fp.FusionPicError, match=name + " needs an undecomposed handle") as e:
            call()
        assert e.value.code == -5


def test_ionize_without_a_handle(fp):
    lib = fp.load_library()
    s, keep = fp._ionize_spec(2e-9, [1.0, 1.0, 1.0], ion=1, g_threshold=0.0, density=1e20, sigma=[1e-19, 2e-19], g_lo=0.0, g_hi=0.5)
    out = fp.IonizeResult(7, 7)
    index = ctypes.c_int(77)
    assert lib.fpic_ionize(None, ctypes.byref(s), ctypes.byref(out)) == -1
    assert b"null handle" in lib.fpic_last_error(None) and out.candidates == 7
    assert lib.fpic_ionize_register(None, ctypes.byref(s), 1, ctypes.byref(index)) == -1 and index.value == 77
    assert lib.fpic_ionize_stats(None, 0, 0, ctypes.byref(out)) == -1 and out.applications == 7
    assert lib.fpic_ionize_clear(None) == -1
    assert b"null handle" in lib.fpic_last_error(None)
