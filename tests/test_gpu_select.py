"""The particle selection of the CART3D box, filtered and compacted on the GPU (fpic_select): every id, position and velocity
against tests/select_reference.py applied to what getParticles / domainGet return — ids equal, values bit-equal — in fp32
and fp64, electrostatic and full EM; the loop boundaries of the pass, everything and nothing matching, the id rule, the cast
to another dtype, the histogram's counts, the call changing nothing, decomposed groups after migrations, the
communicator's GLOBAL scope over the stand-in RCCL, the Node host, and the refusals."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import select_reference as ref
from helpers import ROOT
from test_gpu_histogram import DTYPE, LANES, ME, MP, PRECISIONS, QE, SIGMA, box_spec, group_of, plain_box, two_species_box

pytestmark = pytest.mark.gpu


def kernel_constants():
    """kSelectBlocks and kSelectThreads of the kernel header, so that a new launch grid moves the cases"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_select_kernels.hpp")).read()
    get = lambda name: int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    return get("kSelectBlocks"), get("kSelectThreads")


BLOCKS, THREADS = kernel_constants()


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def stored_of(sim, species=0):
    """(ids, pos, vel) of an undecomposed handle: the id is the caller's index"""
    p = sim.getParticles(species=species)
    return np.arange(len(p["position"]), dtype=np.uint32), p["position"], p["velocity"]


def live_of(sims, species=0):
    """(ids, pos, vel) of the live slots of the members of a decomposition (domainGet returns dead ones too: x < 0)"""
    parts = [s.domainGet(species=species) for s in sims]
    ids = np.concatenate([p["ids"] for p in parts])
    pos = np.concatenate([p["position"] for p in parts])
    vel = np.concatenate([p["velocity"] for p in parts])
    live = ~(pos[:, 0] < 0)
    return ids[live], pos[live], vel[live]


def same(got, want, what=""):
    assert got["matched"] == want["matched"], (what, got["matched"], want["matched"])
    if want["ids"] is None:
        assert got["ids"] is None and got["position"] is None and got["velocity"] is None, what
        return
    assert got["ids"].dtype == np.uint32 and np.array_equal(got["ids"], want["ids"]), what
    for k in ("position", "velocity"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (what, k)


def check(sim, where=None, every=None, species=0, stored=None, dtype=None, capacity=None):
    """select() and count() of one handle against the reference over its read-back, exactly"""
    st = stored if stored is not None else stored_of(sim, species)
    want = ref.select(*st, where, every, capacity=capacity, dtype=dtype)
    got = sim.select(where, species=species, every=every, dtype=dtype, capacity=capacity)
    same(got, want, (where, every, species))
    assert sim.count(where, species=species, every=every) == want["matched"]
    return got


TERMS = {"x": (0.25, 0.6), "y": (None, 0.3), "z": (0.7, None), "vx": (-SIGMA, 0.5 * SIGMA), "vy": (0.01, None), "vz": (None, -0.02),
         "v2": (SIGMA ** 2, None)}
SEVEN = {"x": (0.1, 0.95), "y": (0.05, None), "z": (None, 0.9), "vx": (-2 * SIGMA, 2 * SIGMA), "vy": (-SIGMA, None), "vz": (None, 1.5 * SIGMA),
         "v2": (0.25 * SIGMA ** 2, 9 * SIGMA ** 2)}
ION_TERMS = {"x": (0.5, None), "vx": (0.0, None), "v2": (None, 3e-6), "z": (0.125, 0.875)}


# ---- each axis code alone, three terms, seven terms, on a two-species box as loaded and after a re-binning has permuted the slots
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_axis_alone_then_three_and_seven_terms(fp, precision, solver):
    sim, spec, _ = two_species_box(fp, precision, solver)
    n, ni = 20000, 8000
    for stage in ("loaded", "stepped"):
        if stage == "stepped":
            sim.precalc()
            sim.substeps(10)
        el, io = stored_of(sim, 0), stored_of(sim, 1)
        for name, bounds in TERMS.items():
            got = check(sim, {name: bounds}, stored=el)
            assert 0 < got["matched"] < n, (stage, name)
        for name, bounds in ION_TERMS.items():
            got = check(sim, {name: bounds}, species=1, stored=io)
            assert 0 < got["matched"] < ni, (stage, name)
        got = check(sim, {k: TERMS[k] for k in ("x", "vy", "v2")}, stored=el)
        assert 0 < got["matched"] < n
        got = check(sim, SEVEN, stored=el)
        assert 0 < got["matched"] < n
        assert check(sim, dict(reversed(list(SEVEN.items()))), stored=el)["matched"] == got["matched"]       # the terms' order does not matter
        assert check(sim, None, stored=el)["matched"] == n and check(sim, {}, species=1, stored=io)["matched"] == ni
    sim.destroy()


# ---- the loop boundaries of the pass: before any binning slot = index, so the planted slots are the planted ids
def loop_counts(lanes):
    S = BLOCKS * THREADS * lanes            # one grid stride in slots
    return S, sorted({1, lanes - 1, lanes, lanes + 1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 5})


@pytest.mark.parametrize("precision", PRECISIONS)
def test_loop_boundaries_of_the_pass(fp, precision):
    T, lanes = DTYPE[precision], LANES[precision]
    S, counts = loop_counts(lanes)
    sim, L = plain_box(fp, precision, counts[0])
    for n in counts[1:]:
        sim.addSpecies(MP, -QE, n)
    planted = {}
    for s, n in enumerate(counts):
        vel = np.zeros((n, 3), dtype=T)
        vel[:, 0] = 0.5                                                    # outside the window
        planted[s] = sorted({k for k in (0, lanes - 1, S - 1, S, 2 * S - 1, 2 * S, n - 1) if 0 <= k < n})
        vel[planted[s], 0] = 0.0
        pos = np.full((n, 3), 0.5, dtype=T) * np.array(L, dtype=T)
        sim.set(position=pos, velocity=vel, species=s)
        del pos, vel
    for s, n in enumerate(counts):
        st = stored_of(sim, s)
        assert len(st[0]) == n
        got = check(sim, {"vx": (-0.1, 0.1)}, species=s, stored=st)                                  # the delivering pass and the count query
        assert got["ids"].tolist() == planted[s], (n, got["ids"].tolist())
        got = check(sim, {"vx": (-0.1, 0.1), "v2": (None, 0.01), "x": (0.25, 0.75)}, species=s, stored=st, every=(1, 0))
        assert got["ids"].tolist() == planted[s]
        got = check(sim, {"vx": (None, None)}, species=s, stored=st, every=(n + 1, n - 1))           # the id stream: only the last slot's id passes
        assert got["ids"].tolist() == [n - 1]
        got = check(sim, None, species=s, stored=st, every=(S, S - 1))                                # ... and the last slot of every grid stride
        assert got["ids"].tolist() == list(range(S - 1, n, S))
        assert sim.count(None, species=s) == n and sim.count({"vx": (0.25, None)}, species=s) == n - len(planted[s])
        del st
    assert -(-max(counts) // lanes) > 3 * BLOCKS * THREADS
    sim.destroy()


def raw_select(fp, sim, where, capacity, rows, sentinel, every=None, species=0):
    """fpic_select straight into caller arrays of `rows` rows filled with sentinels -> (ids, pos, vel, matched)"""
    T = DTYPE["fp32" if sim.precision == fp.F32 else "fp64"]
    ids = np.full(rows, 0xDEADBEEF, dtype=np.uint32)
    pos, vel = np.full((rows, 3), sentinel, dtype=T), np.full((rows, 3), sentinel, dtype=T)
    matched = ctypes.c_uint64()
    s = fp._select_spec(where, species, every)
    sim._check(sim._lib.fpic_select(sim._h, ctypes.byref(s), fp.DIAG_LOCAL, capacity, ids.ctypes.data, pos.ctypes.data, vel.ctypes.data, sim.precision,
                                    ctypes.byref(matched)))
    return ids, pos, vel, int(matched.value)


# ---- everything matches: every wave allocates rows in every iteration
@pytest.mark.parametrize("precision", PRECISIONS)
def test_everything_matches(fp, precision):
    n = 1 << 18
    sim, L = plain_box(fp, precision, n)
    rng = np.random.default_rng(4)
    sim.set(position=rng.random((n, 3)) * L, velocity=rng.normal(0, SIGMA, (n, 3)))
    st = stored_of(sim)
    for where in (None, {"vx": (None, None), "x": (0.0, 1.0), "v2": (0.0, None)}):
        assert sim.count(where) == n
        want = ref.select(*st, where)
        ids, pos, vel, m = raw_select(fp, sim, where, n, n, -7.0)                                    # capacity == matched: all rows
        assert m == n and np.array_equal(ids, want["ids"]) and pos.tobytes() == want["position"].tobytes() and vel.tobytes() == want["velocity"].tobytes()
        ids, pos, vel, m = raw_select(fp, sim, where, n - 1, n, -7.0)                                # capacity == matched - 1: nothing
        assert m == n and (ids == 0xDEADBEEF).all() and (pos == -7.0).all() and (vel == -7.0).all()
    extra = 1000
    ids, pos, vel, m = raw_select(fp, sim, None, n + extra, n + extra, -7.0)                          # rows past matched stay
    assert m == n and np.array_equal(ids[:n], st[0]) and pos[:n].tobytes() == st[1].tobytes() and vel[:n].tobytes() == st[2].tobytes()
    assert (ids[n:] == 0xDEADBEEF).all() and (pos[n:] == -7.0).all() and (vel[n:] == -7.0).all()
    same(sim.select(None), ref.select(*st, None))
    same(sim.select(None, capacity=n - 1), ref.select(*st, None, capacity=n - 1))
    # a NULL output is skipped, the others are written
    s = fp._select_spec(None, 0, None)
    only = np.zeros(n, dtype=np.uint32)
    matched = ctypes.c_uint64()
    sim._check(sim._lib.fpic_select(sim._h, ctypes.byref(s), fp.DIAG_LOCAL, n, only.ctypes.data, None, None, sim.precision, ctypes.byref(matched)))
    assert matched.value == n and np.array_equal(only, st[0])
    sim.destroy()


# ---- nothing matches; a cold beam on a bound; values that are not finite
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nothing_matches_cold_beam_and_values_that_are_not_finite(fp, precision):
    n = 100003
    sim, L = plain_box(fp, precision, n)
    rng = np.random.default_rng(8)
    vel = np.tile(np.array([[0.0125, -0.5, 0.25]]), (n, 1))
    sim.set(position=rng.random((n, 3)) * L, velocity=vel)
    st = stored_of(sim)
    got = check(sim, {"vx": (0.1, 0.2)}, stored=st)
    assert got["matched"] == 0 and got["ids"].shape == (0,) and got["position"].shape == (0, 3)
    ids, pos, velo, m = raw_select(fp, sim, {"vx": (0.1, 0.2)}, 16, 16, -7.0)
    assert m == 0 and (ids == 0xDEADBEEF).all() and (pos == -7.0).all() and (velo == -7.0).all()
    assert check(sim, {"vx": (0.0125, 0.1)}, stored=st)["matched"] == n                              # every value on lo: in
    assert check(sim, {"vx": (-0.1, 0.0125)}, stored=st)["matched"] == 0                             # every value on hi: out
    assert check(sim, {"vy": (-0.5, None), "vz": (None, 0.25)}, stored=st)["matched"] == 0
    assert check(sim, {"v2": (None, 1.0)}, stored=st)["matched"] == n
    vel = rng.normal(0, SIGMA, (n, 3))
    vel[5::97, 0] = np.nan
    vel[11::89, 0] = np.inf
    vel[13::83, 0] = -np.inf
    vel[17::101, 2] = np.nan
    sim.set(velocity=vel)
    st = stored_of(sim)
    finite_x = int(np.isfinite(st[2][:, 0]).sum())
    assert n - finite_x > 2000
    assert check(sim, {"vx": (-1.0, 1.0)}, stored=st)["matched"] == finite_x
    assert check(sim, {"vx": (None, None)}, stored=st)["matched"] == finite_x + int(np.isneginf(st[2][:, 0]).sum())
    assert check(sim, {"vx": (None, 0.0)}, stored=st)["matched"] > int(np.isneginf(st[2][:, 0]).sum()) > 0
    assert check(sim, {"v2": (0.0, None)}, stored=st)["matched"] == int(np.isfinite(st[2][:, [0, 2]]).all(axis=1).sum())
    got = check(sim, None, stored=st)                                                                 # no term: the NaNs come back as they are
    assert got["matched"] == n and np.isnan(got["velocity"][:, 0]).sum() == np.isnan(st[2][:, 0]).sum()
    sim.destroy()


# ---- the id rule: the same particles at every time
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_id_rule(fp, precision, solver):
    sim, spec, _ = two_species_box(fp, precision, solver, shape=(16, 16, 16), n=20000, ni=3000, seed=11)
    sim.precalc()
    seen = []
    for stage in ("loaded", "sorted", "stepped"):
        if stage == "sorted":
            sim.sort()
        if stage == "stepped":
            sim.substeps(10)
        st = stored_of(sim)
        got = check(sim, None, every=(7, 3), stored=st)
        assert got["ids"].tolist() == list(range(3, 20000, 7))
        seen.append(got)
        check(sim, {"vx": (0.0, None), "z": (0.1, 0.9)}, every=(7, 3), stored=st)
        check(sim, {"v2": (None, SIGMA ** 2)}, every=(1000, 0), stored=st)
        check(sim, None, every=(3000, 2999), species=1)
        assert check(sim, None, every=(1, 0), stored=st)["matched"] == check(sim, None, every=(0, 5), stored=st)["matched"] == 20000
    assert seen[0]["position"].tobytes() == seen[1]["position"].tobytes() and seen[0]["velocity"].tobytes() == seen[1]["velocity"].tobytes()   # sort() moves slots, not particles
    assert seen[2]["velocity"].tobytes() != seen[1]["velocity"].tobytes()
    sim.destroy()


# ---- a dtype other than the handle's precision: the C cast of the stored values
@pytest.mark.parametrize("precision", PRECISIONS)
def test_dtype_other_than_the_handles(fp, precision):
    n = 30000
    sim, L = plain_box(fp, precision, n)
    rng = np.random.default_rng(15)
    vel = rng.normal(0, SIGMA, (n, 3))
    vel[::1001, 1] = 1e300 if precision == "fp64" else 3e38          # fp64 -> float: inf
    vel[7::1001, 2] = 1e-300 if precision == "fp64" else 1e-45       # fp64 -> float: 0
    sim.set(position=rng.random((n, 3)) * L, velocity=vel)
    st = stored_of(sim)
    other = np.float32 if precision == "fp64" else np.float64
    for dt in (other, DTYPE[precision]):
        got = check(sim, {"x": (0.2, 0.8)}, stored=st, dtype=dt)
        assert got["position"].dtype == dt and got["matched"] > 1000
        check(sim, None, stored=st, dtype=dt, every=(3, 1))
    sim.destroy()


# ---- the histogram's counts
@pytest.mark.parametrize("precision", PRECISIONS)
def test_counts_equal_the_histograms(fp, precision):
    sim, spec, _ = two_species_box(fp, precision, "poisson_fft", shape=(16, 16, 16), n=20000, ni=3000, seed=6)
    sim.precalc()
    sim.substeps(6)
    for axis, (lo, hi) in (("vx", (-0.5 * SIGMA, SIGMA)), ("x", (0.25, 0.5)), ("v2", (0.0, SIGMA ** 2)), ("vz", (-1.0, 1.0))):
        h = sim.histogram(axis, 1, (lo, hi))
        assert sim.count({axis: (lo, hi)}) == int(h["counts"][0])
        assert int(h["counts"][0]) + h["outside"] == sim.count(None) == 20000
    h = sim.histogram("vx", 64, (-3 * SIGMA, 3 * SIGMA), species=1)
    assert int(h["counts"].sum()) + h["outside"] == sim.count(None, species=1) == 3000
    assert int(h["counts"].sum()) == sim.count({"vx": (-3 * SIGMA, 3 * SIGMA)}, species=1)
    sim.destroy()


# ---- the call changes nothing, and needs no precalc()
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_call_changes_nothing(fp, precision, solver):
    sim, spec, _ = two_species_box(fp, precision, solver, shape=(16, 16, 16), n=8000, ni=4000, seed=5)
    check(sim, {"vx": (0.0, None)})                           # before precalc()
    sim.precalc()
    sim.substeps(9)
    before = [sim.getParticles(species=s) for s in range(2)]
    row = sim._energy_row("global").tobytes()
    a = sim.select({"x": (0.1, 0.9), "v2": (None, 4 * SIGMA ** 2)})
    sim.select(None, species=1, every=(5, 1))
    sim.count({"vz": (0.0, None)})
    b = sim.select({"x": (0.1, 0.9), "v2": (None, 4 * SIGMA ** 2)}, scope="local")
    for k in ("ids", "position", "velocity"):
        assert a[k].tobytes() == b[k].tobytes()
    after = [sim.getParticles(species=s) for s in range(2)]
    for s in range(2):
        for k in ("position", "velocity"):
            assert before[s][k].tobytes() == after[s][k].tobytes(), (s, k)
    assert sim._energy_row("global").tobytes() == row
    twin, _, _ = two_species_box(fp, precision, solver, shape=(16, 16, 16), n=8000, ni=4000, seed=5)
    twin.precalc()
    twin.substeps(10)
    sim.substeps(1)
    for s in range(2):
        for k in ("position", "velocity"):
            assert sim.getParticles(species=s)[k].tobytes() == twin.getParticles(species=s)[k].tobytes()
    assert sim.readField(fp.F3_E).tobytes() == twin.readField(fp.F3_E).tobytes()
    sim.destroy(); twin.destroy()


# ---- decomposition: members of an in-process group, with dead slots and tail arrivals, against the reference over their union
GROUP_REQUESTS = [(None, None), ({"vx": (-0.05, 0.02)}, None), ({"z": (0.4, 0.6)}, None), ({"x": (0.25, None), "vz": (None, 0.0), "v2": (None, 0.02)}, None),
                  (None, (7, 3)), ({"z": (None, 0.5), "vy": (0.0, None)}, (3, 0)), ({"vx": (5.0, None)}, None)]


@pytest.mark.parametrize("world,dist,every,em,precision", [(2, 0, 1, False, "fp32"), (2, 1, 1, False, "fp64"), (4, 0, 2, False, "fp32"),
                                                           (4, 1, 2, False, "fp64"), (2, 0, 2, True, "fp32")])
def test_decomposed_group(fp, world, dist, every, em, precision):
    import decomp_scene as ds
    sc = ds.build(fp, dict(world=world, shape=(16, 16, 32), ghost=2, every=every, em=em, distributed_solve=dist, precision=precision,
                           n=20000, seed=world + dist))
    g = group_of(fp, sc)
    for frame in range(3):
        g.step()
        st = live_of(g.sims)
        lives = [live_of([m]) for m in g.sims]
        assert len(st[0]) == sc["n"] == g.count()
        for where, ev in GROUP_REQUESTS:
            got = g.select(where, every=ev)
            same(got, ref.select(*st, where, ev), (frame, where, ev))
            assert sum(got["matched_members"]) == got["matched"] == g.count(where, every=ev)
            members = [m.select(where, every=ev, scope="local") for m in g.sims]
            assert [m["matched"] for m in members] == got["matched_members"]
            allids = np.concatenate([m["ids"] for m in members])
            assert len(np.unique(allids)) == len(allids)                                              # no id from two members
            for r in range(world):                                                                     # each member against its own live slots
                same(members[r], ref.select(*lives[r], where, ev), (frame, where, ev, r))
        small = g.select(None, capacity=sc["n"] - 1)
        assert small["ids"] is None and small["matched"] == sc["n"]
        same(g.select({"vx": (0.0, None)}, dtype=np.float64), ref.select(*st, {"vx": (0.0, None)}, dtype=np.float64))
    dead = sum(int((s.domainGet()["position"][:, 0] < 0).sum()) for s in g.sims)
    print("world", world, "dist", dist, "dead slots held at the end", dead)
    assert sum(s.domainStats()["migrated"] for s in g.sims) > 0
    with pytest.raises(fp.FusionPicError, match="in-process group"):
        g.sims[0].select(None, scope="global")
    for s in g.sims:
        s.destroy()


# ---- the communicator: ranks as threads of one process over the stand-in RCCL (tests/fake_rccl)
COMM_DRIVER = r'''
import hashlib, json, os, sys, threading
sys.path.insert(0, os.path.join(sys.argv[1], "fusion-sim_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import fusionpic as fp
import decomp_scene as ds
import select_reference as ref
import test_gpu_select as ts
import test_gpu_histogram as th
sc = ds.build(fp, json.loads(sys.argv[2]))
requests = json.loads(sys.argv[3])
world = sc["world"]
uid = fp.commUniqueId()
out, err = [None] * world, [None] * world
def digest(r):
    if r["ids"] is None:
        return [r["matched"], None]
    return [r["matched"], hashlib.sha256(r["ids"].tobytes() + r["position"].tobytes() + r["velocity"].tobytes()).hexdigest()]
def rank_main(r):
    try:
        s = fp.makeCylindricalParticlePusher(dict(sc["spec"], count=3 * sc["n"]), precision=sc["precision"])
        s.commInit(uid, r, world)
        s.domainInit(r, world, ghost_planes=sc["G"], migrate_every=sc["every"], distributed_solve=sc["dist_solve"])
        first = int(sc["counts"][:r].sum())
        s.domainSet(sc["pos"][first:first + sc["counts"][r]], sc["vel"][first:first + sc["counts"][r]], first_id=first)
        s.precalc()
        for _ in range(sc["frames"]):
            s.step()
        res = []
        for where, ev, cap in requests:
            g = s.select(where, every=ev, capacity=cap, scope="global")
            l = s.select(where, every=ev, scope="local")
            res.append((digest(g), s.count(where, every=ev, scope="global"), l["matched"]))
        out[r] = (res, s.domainStats()["migrated"])
        s.destroy()
    except Exception as e:
        err[r] = repr(e)
threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
for t in threads: t.start()
for t in threads: t.join()
if any(err):
    print(json.dumps({"error": err})); sys.exit(0)
g = th.group_of(fp, sc)
for _ in range(sc["frames"]):
    g.step()
st = ts.live_of(g.sims)
grp = []
for where, ev, cap in requests:
    h = g.select(where, every=ev, capacity=cap)
    want = ref.select(*st, where, ev, capacity=cap)
    ok = h["matched"] == want["matched"] and ((h["ids"] is None) == (want["ids"] is None))
    if ok and h["ids"] is not None:
        ok = all(h[k].tobytes() == want[k].tobytes() for k in ("ids", "position", "velocity"))
    grp.append((digest(h), bool(ok)))
print(json.dumps({"ranks": out, "group": grp}))
'''


@pytest.mark.parametrize("world,shape", [(2, (16, 16, 32)), (3, (12, 16, 18))])
def test_communicator_global_equals_the_groups_merge(fp, world, shape):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "fake_rccl")])
    env = dict(os.environ, FPIC_RCCL_LIBRARY=os.path.join(ROOT, "tests", "fake_rccl", "libfakerccl.so"))
    n = 80000      # (a rank holds more rows than one chunk of the gather: 2^15)
    case = dict(world=world, shape=shape, ghost=2 if world == 2 else 1, every=2 if world == 2 else 1, em=False, distributed_solve=0,
                precision="fp32", n=n, seed=8, frames=3)
    requests = [(None, None, None), ({"vx": (-0.05, 0.02)}, None, None), ({"z": (0.4, 0.6), "v2": (None, 0.02)}, (7, 3), None),
                ({"vx": (5.0, None)}, None, None), ({"z": (None, 0.25)}, None, None),              # (rows of the first rank alone)
                (None, None, n - 1), ({"vx": (0.0, None)}, None, 100), (None, (2, 1), n), (None, None, 0)]   # matched > capacity on every rank; room to spare; the count alone
    raw = subprocess.check_output([sys.executable, "-c", COMM_DRIVER, ROOT, json.dumps(case), json.dumps(requests)], env=env, timeout=600)
    res = json.loads(raw.decode().strip().splitlines()[-1])
    assert "error" not in res, res
    ranks = res["ranks"]
    assert sum(r[1] for r in ranks) > 0                                   # particles migrated
    for i, (want, ok) in enumerate(res["group"]):
        assert ok, requests[i]                                            # the group's merge is the reference's
        for r in range(world):
            got, counted, _ = ranks[r][0][i]
            assert got == want and counted == want[0], (requests[i], r)   # every rank: the group's merge, bit for bit
        assert sum(ranks[r][0][i][2] for r in range(world)) == want[0]    # the LOCAL selections hold every row once
    assert res["group"][0][0][0] == n and res["group"][5][0] == [n, None] and res["group"][6][0][1] is None and res["group"][7][0][1] is not None


def test_select_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    rng = np.random.default_rng(2)
    n, shape, L = 4000, (16, 16, 16), (0.016, 0.016, 0.016)
    spec = box_spec(shape, L, n, 5e-12, macro_weight=1e15 * np.prod(L) / n)
    pos, vel = rng.random((n, 3)) * L, rng.normal(0, 2e-3, (n, 3))
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, p=pos.tolist(), v=vel.tolist())))
    script = r"""
const fs = require('fs');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.set({position: inp.p, velocity: inp.v});
sim.precalc();
sim.step(3);
const hex = (a) => a === null ? null : Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('hex');
const pack = (r) => ({ids: r.ids === null ? null : Array.from(r.ids), position: hex(r.position), velocity: hex(r.velocity), matched: r.matched,
  types: r.ids === null ? null : [r.ids.constructor.name, r.position.constructor.name, r.velocity.constructor.name]});
const a = sim.select({where: {vx: [-0.001, 0.002], z: [0.25, null]}, species: 0});
const b = sim.select({where: {v2: [null, 4e-6]}, every: [7, 3], dtype: 'fp64'}, 'local');
const c = sim.select({where: {}, capacity: 10});
const d = sim.select({capacity: 0});
const e = sim.select({where: {x: [0.5, 0.75]}, capacity: 4000});
const errors = [];
for (const bad of [{where: {w: [0, 1]}}, {where: {vx: [1, 0]}}, {where: {vx: 3}}, {where: {vx: [0, 1]}, species: 3}, {every: [7, 7]}, {every: [7]},
                   {capacity: -2}, {capacity: 1 << 25}, {where: {vx: [NaN, 1]}}, {dtype: 'fp16'}, {where: [1, 2]}, 7]) {
  try { sim.select(bad); errors.push(null); } catch (err) { errors.push(String(err.message)); }
}
console.log(JSON.stringify({a: pack(a), b: pack(b), c: pack(c), d: pack(d), e: pack(e), errors: errors}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    sim = fp.makeCylindricalParticlePusher(spec)
    sim.set(position=pos, velocity=vel)
    sim.precalc()
    sim.step(3)
    st = stored_of(sim)
    a = check(sim, {"vx": (-0.001, 0.002), "z": (0.25, None)}, stored=st)
    b = check(sim, {"v2": (None, 4e-6)}, every=(7, 3), dtype=np.float64, stored=st)
    e = check(sim, {"x": (0.5, 0.75)}, stored=st)
    for name, want, types in (("a", a, ["Uint32Array", "Float32Array", "Float32Array"]), ("b", b, ["Uint32Array", "Float64Array", "Float64Array"]),
                              ("e", e, ["Uint32Array", "Float32Array", "Float32Array"])):
        got = out[name]
        assert got["matched"] == want["matched"] > 0 and got["ids"] == want["ids"].tolist() and got["types"] == types, name
        assert got["position"] == want["position"].tobytes().hex() and got["velocity"] == want["velocity"].tobytes().hex(), name
    assert out["c"] == dict(ids=None, position=None, velocity=None, matched=n, types=None)
    assert out["d"] == dict(ids=None, position=None, velocity=None, matched=n, types=None)
    assert all(err is not None for err in out["errors"]), out["errors"]
    sim.destroy()


# ---- refusals
def test_refusals_name_the_property(fp):
    sim, spec, _ = two_species_box(fp, "fp32", "poisson_fft", shape=(16, 16, 16), n=2000, ni=500)
    lib = sim._lib

    def raw(**kw):
        """a request written straight into the structure: what the Python wrapper would refuse itself"""
        s = fp.SelectSpec()
        s.species, s.nterms = kw.get("species", 0), kw.get("nterms", 1)
        for t in range(8):
            s.axis[t] = kw.get("axis", (3, 0, 0, 0, 0, 0, 0, 0))[t]
            s.lo[t] = kw.get("lo", (-1.0, 0, 0, 0, 0, 0, 0, 0))[t]
            s.hi[t] = kw.get("hi", (1.0, 0, 0, 0, 0, 0, 0, 0))[t]
        s.id_mod, s.id_rem = kw.get("id_mod", 0), kw.get("id_rem", 0)
        for k, v in enumerate(kw.get("reserved", (0, 0, 0, 0))):
            s.reserved[k] = v
        cap = kw.get("capacity", 4096)
        ids = np.zeros(4096, dtype=np.uint32)
        pos = np.zeros((4096, 3), dtype=np.float64)
        matched = ctypes.c_uint64()
        out = (ids.ctypes.data, pos.ctypes.data, None) if kw.get("outputs", True) else (None, None, None)
        sim._check(lib.fpic_select(sim._h, ctypes.byref(s), kw.get("scope", 0), cap, *out, kw.get("dtype", fp.F32), ctypes.byref(matched)))
        return int(matched.value)

    two = dict(nterms=2, axis=(3, 0, 0, 0, 0, 0, 0, 0), lo=(-1.0, 0.0, 0, 0, 0, 0, 0, 0), hi=(1.0, 1.0, 0, 0, 0, 0, 0, 0))
    assert raw() == 2000 and raw(species=1) == 500 and raw(nterms=0, lo=(0,) * 8, hi=(0,) * 8, axis=(0,) * 8) == 2000
    assert raw(**dict(two, axis=(3, 0) + (0,) * 6)) == 2000 and raw(lo=(-np.inf,) + (0,) * 7, hi=(np.inf,) + (0,) * 7) == 2000
    assert raw(capacity=0, outputs=False) == 2000 and raw(id_mod=1, id_rem=5) == 2000 and raw(capacity=1 << 24) == 2000
    for kw, prop in ((dict(nterms=-1), ".nterms"), (dict(nterms=8), ".nterms"), (dict(species=2), ".species"), (dict(species=-1), ".species"),
                     (dict(axis=(7,) + (0,) * 7), ".axis"), (dict(axis=(-1,) + (0,) * 7), ".axis"), (dict(two, axis=(3, 3) + (0,) * 6), ".axis"),
                     (dict(lo=(np.nan,) + (0,) * 7), ".range"), (dict(hi=(np.nan,) + (0,) * 7), ".range"), (dict(lo=(1.0,) + (0,) * 7), ".range"),
                     (dict(lo=(2.0,) + (0,) * 7), ".range"), (dict(lo=(np.inf,) + (0,) * 7, hi=(np.inf,) + (0,) * 7), ".range"),
                     (dict(id_mod=7, id_rem=7), ".id_rem"), (dict(id_mod=2, id_rem=9), ".id_rem"), (dict(reserved=(0, 1, 0, 0)), ".reserved"),
                     (dict(axis=(3, 1) + (0,) * 6), ".axis"), (dict(hi=(1.0, 0, 0, 0, 0, 0, 0, 2.0)), ".axis"),
                     (dict(capacity=(1 << 24) + 1), ".capacity"), (dict(capacity=5, outputs=False), ".capacity"),
                     (dict(dtype=2), ".dtype"), (dict(dtype=-1), ".dtype"), (dict(scope=2), ".scope")):
        with pytest.raises(fp.FusionPicError) as e:
            raw(**kw)
        assert prop + " <- " in str(e.value) and e.value.code == -1, (kw, str(e.value))
    for kw, prop in ((dict(where={"vx": (1, 1)}), ".range"), (dict(where={"vx": (0, 1)}, species=5), ".species"), (dict(where={"q": (0, 1)}), ".axis"),
                     (dict(where=None, every=(7, 7)), ".id_rem"), (dict(where=None, capacity=(1 << 24) + 1), ".capacity"),
                     (dict(where={"vx": (float("nan"), None)}), ".range")):
        with pytest.raises(fp.FusionPicError) as e:
            sim.select(**kw)
        assert prop + " <- " in str(e.value), (kw, str(e.value))
    s = fp._select_spec({"vx": (0, 1)}, 0, None)
    matched = ctypes.c_uint64()
    for args in ((None, 0, 0, None, None, None, fp.F32, ctypes.byref(matched)), (ctypes.byref(s), 0, 0, None, None, None, fp.F32, None)):
        assert lib.fpic_select(sim._h, *args) == -1
        assert b"Non-optional property is undefined" in lib.fpic_last_error(sim._h)
    sim.destroy()


def test_an_rz_handle_is_refused(fp):
    from helpers import make_spec
    sim = fp.makeCylindricalParticlePusher(make_spec(16, 16, 8))
    with pytest.raises(fp.FusionPicError, match="needs a CART3D handle"):
        sim.select({"vx": (-1.0, 1.0)})
    with pytest.raises(fp.FusionPicError, match="needs a CART3D handle"):
        sim.count(None)
    sim.destroy()
