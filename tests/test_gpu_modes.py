"""The modes diagnostic of the CART3D box (fpic_modes_now / _record / _history): the complex Fourier amplitudes of the node
fields at chosen wave vectors against the long-double restatement of the rule (tests/modes_reference.py) applied to what
readField returns, within the DERIVED bound

    |got - ref| <= (N + 16) 2^-53 (sum |F|) / N      per component, for any order of the sum

(N: the worst-case bound of a sum of N terms; 16: the three table roundings, the two complex products, the scaling), and bit
for bit wherever a test says so: exact integer fields, A(-m) = conj A(m), sub-masks, permuted mode lists, two calls, twin
handles, recorded rows against a twin, the ranks of a communicator.  Then the refusals, the decomposition (in-process groups
and the stand-in RCCL), the Node host, and the cold-plasma frequency read off one recorded mode."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import modes_reference as mr
import series_reference as sr
from helpers import ROOT
from test_gpu_histogram import box_spec, group_of, plain_box, two_species_box

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "fp64"]
ALL = mr.FIELDS
E_FIELDS = ("ex", "ey", "ez", "phi")


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def rho_factor(spec):
    """the header's factor of FPIC_MODE_RHO: q0 W / (2^42 dV), formed as the library forms it"""
    dv = (spec["radius"] / spec["nr"]) * (spec["length_y"] / spec["ny"]) * (spec["height"] / spec["nz"])
    return spec["particle_charge"] * spec.get("macro_weight", 1.0) / (4398046511104.0 * dv)


def fields_of(fp, sim, spec):
    """float64 [nz][ny][nx][8]: what the eight quantities are summed over, from readField"""
    nx, ny, nz = spec["nr"], spec["ny"], spec["nz"]
    F = np.zeros((nz, ny, nx, 8))
    F[..., 0:4] = sim.readField(fp.F3_E).astype(np.float64).reshape(nz, ny, nx, 4)
    if spec["solver"] == "yee":
        F[..., 4:7] = sim.readField(fp.F3_B_NODES).astype(np.float64).reshape(nz, ny, nx, 4)[..., :3]
    F[..., 7] = sim.readField(fp.F3_RHO_FIXED).astype(np.float64).reshape(nz, ny, nx) * rho_factor(spec)
    return F


def rows_of(sim, modes, fields=ALL, scope="global"):
    """float64 [M][nq][2] as the library wrote them"""
    return sim._modes_rows(modes, fields, scope)[0]


def within_bound(got, F, modes, fields=ALL, what=""):
    """got [M][nq][2] against the long-double reference over F [nz][ny][nx][8]; prints the figures before it asserts"""
    sel = [mr.FIELDS.index(f) for f in mr.FIELDS if f in fields]
    ref = mr.amplitudes(F[..., sel], modes)
    tol = mr.tolerance(F[..., sel])
    err = np.maximum(np.abs(got[..., 0] - ref.real.astype(np.float64)), np.abs(got[..., 1] - ref.imag.astype(np.float64))).max(axis=0)
    print(what, "worst error / bound per quantity:", ["%.2e" % (e / t) if t else ("0" if e == 0 else "inf") for e, t in zip(err, tol)])
    assert (err <= tol).all(), (what, err, tol)
    return ref


# ---- 1. exact: small integers at modes whose twiddles are all in {1, -1, i, -i}
def test_exact_integer_field(fp):
    shape, n = (8, 8, 8), 8
    rng = np.random.default_rng(11)
    Ef = rng.integers(-8, 9, shape + (3,)).astype(np.float64)            # E[i][j][k][component]
    modes = np.array([(a, b, c) for a in (0, 2, -2, 4) for b in (0, 2, -2, 4) for c in (0, 2, -2, 4)], dtype=np.int32)
    # the integer sums: i^(-(2 t / 2)) with t = (m i) mod 8 in {0, 2, 4, 6}, Gaussian integers throughout
    unit = {0: (1, 0), 2: (0, -1), 4: (-1, 0), 6: (0, 1)}
    F = np.transpose(Ef, (2, 1, 0, 3)).astype(np.int64)                    # [k][j][i][c]
    want = np.zeros((len(modes), 3, 2))
    for a, (mx, my, mz) in enumerate(modes):
        w = np.zeros((n, n, n, 2), dtype=np.int64)
        for k in range(n):
            for j in range(n):
                for i in range(n):
                    z = complex(*unit[(mx * i) % n]) * complex(*unit[(my * j) % n]) * complex(*unit[(mz * k) % n])
                    w[k, j, i] = (int(z.real), int(z.imag))
        for c in range(3):
            want[a, c] = ((F[..., c] * w[..., 0]).sum() / 512.0, (F[..., c] * w[..., 1]).sum() / 512.0)
    rows = {}
    for precision in PRECISIONS:
        sim, _ = plain_box(fp, precision, 16, shape)
        sim.set(E=Ef)
        got = rows_of(sim, modes, ("ex", "ey", "ez"))
        assert got.tobytes() == want.tobytes(), precision                 # bit for bit (a zero is +0.0 on both sides)
        # A(-m) = conj A(m): equal real parts bit for bit, imaginary parts each other's negative (a zero compares equal to
        # its negative; every other double differs from it in the sign bit alone)
        neg = rows_of(sim, np.where(modes == 4, 4, -modes).astype(np.int32), ("ex", "ey", "ez"))      # (-4 is the bin of 4)
        assert neg[..., 0].tobytes() == got[..., 0].tobytes() and np.array_equal(neg[..., 1], -got[..., 1])
        rows[precision] = got
        sim.destroy()
    assert rows["fp32"].tobytes() == rows["fp64"].tobytes()
    assert np.abs(want).max() > 0.1 and (want[:, :, 1] != 0).any()


# ---- 2. against the reference on a written field: odd shapes, two nodes on an axis, rows longer than one staged segment
#         (300), an x table too long for LDS (2050: the other instantiation of the pass), more rows than workgroups (4 x 40 x 30)
WRITTEN = [(12, 10, 9), (5, 6, 7), (2, 16, 3), (33, 2, 17), (300, 3, 2), (2050, 2, 2), (4, 40, 30)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", WRITTEN)
def test_written_field(fp, precision, shape):
    rng = np.random.default_rng(sum(shape))
    sim, L = plain_box(fp, precision, 16, shape)
    spec = box_spec(shape, L, 16, 1e-12, solver="none", macro_weight=2.5e5)
    sim.set(E=rng.normal(0, 1, shape + (3,)))
    F = fields_of(fp, sim, spec)
    modes = mr.mode_list(shape, rng)
    got = rows_of(sim, modes)
    ref = within_bound(got, F, modes, what="%s %s" % (shape, precision))
    assert np.abs(ref[:, :3]).max() > 1e6 * mr.tolerance(F)[:3].max()      # (the amplitudes are far above the bound)
    assert not got[:, 3:].any()                                            # phi, B and the charge of an unstepped box: zeros
    neg = rows_of(sim, -modes)
    assert neg[..., 0].tobytes() == got[..., 0].tobytes() and np.array_equal(neg[..., 1], -got[..., 1])   # conj, bit for bit
    sim.destroy()


# ---- 3. stepped boxes: all eight quantities; on 16^3 also against the series at every node
def stepped(fp, precision, solver, shape, seed=3):
    sim, spec, _ = two_species_box(fp, precision, solver, shape=shape, n=8000, ni=4000, seed=seed)
    sim.precalc()
    sim.step(5)
    if solver == "yee":
        sim.density()
    return sim, spec


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
@pytest.mark.parametrize("shape", [(16, 16, 16), (20, 18, 12)])
def test_stepped_boxes(fp, precision, solver, shape):
    sim, spec = stepped(fp, precision, solver, shape)
    rng = np.random.default_rng(5)
    modes = mr.mode_list(shape, rng, extra=25)[:32]
    assert len(modes) == 32
    F = fields_of(fp, sim, spec)
    got = rows_of(sim, modes)
    within_bound(got, F, modes, what="%s %s %s" % (shape, solver, precision))
    live = [0, 1, 2, 7] + ([4, 5, 6] if solver == "yee" else [3])        # (the full-EM box keeps no potential: its fourth component is zero)
    assert all(np.abs(got[:, q]).max() > 0 for q in live)
    if solver != "yee":
        assert not got[:, 4:7].any()
    if shape == (16, 16, 16):      # both diagnostics see the same arrays: the point series on every node
        L = (spec["radius"], spec["length_y"], spec["height"])
        S = sim.series(points=sr.node_points(L, shape, 0))["points"]
        assert (S[:, 7] == 1).all()
        G = F.copy()
        G[..., :7] = S[:, :7].reshape(16, 16, 16, 7)
        within_bound(got, G, modes, what="series %s %s" % (solver, precision))
    sim.destroy()


# ---- 4. sub-masks and order
@pytest.mark.parametrize("precision,solver", [("fp32", "yee"), ("fp64", "poisson_fft")])
def test_sub_masks_and_permutations(fp, precision, solver):
    shape = (20, 18, 12)
    sim, spec = stepped(fp, precision, solver, shape)
    rng = np.random.default_rng(9)
    modes = mr.mode_list(shape, rng)
    full = rows_of(sim, modes)
    for sub in (("ey",), ("rho",), ("bz", "ex"), ("phi", "rho", "by"), E_FIELDS, ("bx", "by", "bz"), ALL[1:]):
        got = rows_of(sim, modes, sub)
        idx = [ALL.index(f) for f in ALL if f in sub]
        assert got.tobytes() == np.ascontiguousarray(full[:, idx]).tobytes(), sub
    for trial in range(3):                    # (the same number of modes: the lane map, and with it the order of the sum, is the request's)
        perm = rng.permutation(len(modes))
        got = rows_of(sim, modes[perm])
        assert got.tobytes() == np.ascontiguousarray(full[perm]).tobytes(), trial
    F = fields_of(fp, sim, spec)              # another number of modes is another order of the same sum: inside the bound
    within_bound(rows_of(sim, modes[:5]), F, modes[:5], what="5 of them")
    within_bound(rows_of(sim, modes[:1]), F, modes[:1], what="1 of them")
    d = sim.modes(modes, ("ez", "rho"))
    assert sorted(d) == ["ez", "rho"] and d["ez"].dtype == np.complex128 and d["ez"].shape == (len(modes),)
    assert np.array_equal(d["rho"], full[:, 7, 0] + 1j * full[:, 7, 1])
    sim.destroy()


# ---- 5. determinism and non-interference
def state_digest(fp, sim, solver):
    h = hashlib.sha256()
    for s in range(2):
        p = sim.getParticles(species=s)
        h.update(p["position"].tobytes()); h.update(p["velocity"].tobytes())
    fields = [fp.F3_E, fp.F3_RHO_FIXED, fp.F3_PHI] if solver != "yee" else [fp.F3_E, fp.F3_B_NODES, fp.F3_EDGE_E, fp.F3_J_FIXED, fp.F3_RHO_FIXED, fp.F3_FACE_B]
    for w in fields:
        h.update(sim.readField(w).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
def test_determinism_and_non_interference(fp, precision, solver):
    shape = (16, 16, 16)
    a, spec = stepped(fp, precision, solver, shape, seed=6)
    b, _ = stepped(fp, precision, solver, shape, seed=6)
    modes = mr.mode_list(shape, np.random.default_rng(2))
    before = state_digest(fp, a, solver)
    assert before == state_digest(fp, b, solver)
    first = rows_of(a, modes)
    assert rows_of(a, modes).tobytes() == first.tobytes()                  # two calls
    assert rows_of(b, modes).tobytes() == first.tobytes()                  # a twin handle
    assert state_digest(fp, a, solver) == before                            # the call changed nothing
    for _ in range(3):
        a.step(); b.step()
        rows_of(a, modes)                                                   # ... and the next steps do not notice calls
    assert state_digest(fp, a, solver) == state_digest(fp, b, solver)
    a.destroy(); b.destroy()


# ---- 6. recording
@pytest.mark.parametrize("precision,solver", [("fp32", "poisson_fft"), ("fp64", "yee")])
def test_recording(fp, precision, solver):
    shape = (16, 16, 16)
    a, spec, _ = two_species_box(fp, precision, solver, shape=shape, n=8000, ni=4000, seed=6)
    b, _, _ = two_species_box(fp, precision, solver, shape=shape, n=8000, ni=4000, seed=6)
    rng = np.random.default_rng(41)
    modes = mr.mode_list(shape, rng)[:16]
    pts = rng.uniform(0, 1, (4, 3)) * 0.016
    a.precalc(); b.precalc()
    before = a.stats()["bytes_grid_state"]
    a.recordModes(3, 64, modes, ALL)
    armed = a.stats()["bytes_grid_state"]
    assert armed - before >= 64 * 16 * 8 * 16                              # the ring (and the request's block) are counted
    a.recordSeries(2, 64, points=pts)
    a.recordEnergy(3, 64)
    want, want_s, want_e = [], [], []
    for t in range(1, 31):
        a.substeps(1); b.substeps(1)
        if t % 3 == 0:
            want.append(rows_of(b, modes))
            want_e.append(b._energy_row("global"))
        if t % 2 == 0:
            want_s.append(b.series(points=pts)["points"])
    sub, out, names, dropped = a._modes_history_rows("global")
    assert dropped == 0 and sub.tolist() == list(range(3, 31, 3)) and names == list(ALL) and out.shape == (10, 16, 8, 2)
    for r, w in enumerate(want):
        assert out[r].tobytes() == w.tobytes(), r                          # every row: the twin stopped at that sub-step
    assert not np.array_equal(out[0], out[-1])
    # recording alongside the series and the energy rows leaves theirs unchanged
    hist, sd = a.seriesHistory()
    erows, ed = a.energyHistory()
    assert sd == ed == 0 and len(want_s) == len(hist["substep"]) and len(want_e) == len(erows)
    assert all(hist["points"][r].tobytes() == w.tobytes() for r, w in enumerate(want_s))
    assert all(g.tobytes() == w.tobytes() for g, w in zip(erows, want_e))
    again, dropped = a.modesHistory()
    assert len(again["substep"]) == 0 and dropped == 0 and again["ex"].shape == (0, 16)      # drained
    # re-armed with another request, every sub-step, into a ring of 4 rows: 10 recorded, the newest 4, 6 dropped
    a.recordModes(1, 4, modes[:3], ("rho", "ex"))
    twin = []
    for _ in range(10):
        a.substeps(1); b.substeps(1)
        twin.append(rows_of(b, modes[:3], ("ex", "rho")))
    # a query drains nothing
    n, d = ctypes.c_uint64(), ctypes.c_uint64()
    a._check(a._lib.fpic_modes_history(a._h, fp.DIAG_GLOBAL, None, None, 0, ctypes.byref(n), ctypes.byref(d)))
    assert (n.value, d.value) == (4, 6)
    hist, dropped = a.modesHistory()
    assert dropped == 6 and hist["substep"].tolist() == list(range(37, 41)) and sorted(hist) == ["ex", "rho", "substep"]
    for r, w in enumerate(twin[-4:]):       # all four rows of the wrapped ring (two runs of slots on the device): the twin's, bit for bit
        assert np.array_equal(hist["ex"][r], w[:, 0, 0] + 1j * w[:, 0, 1]) and np.array_equal(hist["rho"][r], w[:, 1, 0] + 1j * w[:, 1, 1]), r
    assert not np.array_equal(hist["ex"][0], hist["ex"][1])
    held = a.stats()["bytes_grid_state"]
    a.recordModes(0)
    off = a.stats()["bytes_grid_state"]
    assert off < held                                                      # every = 0 frees the ring and the block
    a.substeps(2)
    assert len(a.modesHistory()[0]["substep"]) == 0
    a.recordModes(3, 64, modes, ALL)
    assert a.stats()["bytes_grid_state"] == off + (armed - before)         # ... all of it: arming again costs what it cost before
    a.recordModes(0)
    assert a.stats()["bytes_grid_state"] == off
    a.destroy(); b.destroy()


# ---- 7. the decomposition: in-process groups against one handle.  The library cuts nz into equal slabs and asks for
# 1 <= ghost_planes < nz / world (+ 2 more planes per slab for a decomposed solve), so the smallest slab a rank can own is
# two planes (three with a decomposed solve): those are the cases here, beside world 3 on a grid that is no power of two.
DECOMPOSED = [  # world, shape, ghost, dist, em, precision
    (2, (16, 16, 32), 2, 0, False, "fp32"), (2, (16, 16, 32), 2, 1, False, "fp64"), (2, (16, 16, 32), 2, 2, False, "fp32"),
    (4, (16, 16, 32), 2, 2, False, "fp64"), (3, (12, 16, 18), 1, 0, False, "fp64"), (3, (12, 16, 6), 1, 0, False, "fp32"),
    (2, (16, 16, 32), 2, 0, True, "fp32"), (4, (16, 16, 32), 2, 0, True, "fp64")]


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("world,shape,ghost,dist,em,precision", DECOMPOSED)
def test_decomposed_group(fp, monkeypatch, world, shape, ghost, dist, em, precision, compact):
    import decomp_scene as ds
    if not compact:
        monkeypatch.setenv("FPIC_DOMAIN_COMPACT", "0")
    sc = ds.build(fp, dict(world=world, shape=shape, ghost=ghost, every=1, em=em, distributed_solve=dist, precision=precision, n=12000, seed=world + dist))
    spec = sc["spec"]
    one = fp.makeCylindricalParticlePusher(spec, precision=precision)
    one.set(position=sc["pos"], velocity=sc["vel"])
    if em:
        one.set(edge_E=sc["E"], face_B=sc["B"])
    else:
        one.precalc()
    g = group_of(fp, sc)
    if not compact:
        monkeypatch.delenv("FPIC_DOMAIN_COMPACT")
    rng = np.random.default_rng(3)
    modes = mr.mode_list(shape, rng)
    assert (modes[:, 2] != 0).sum() > 10                                   # a wrong plane offset shows in these
    fields = ALL
    nzl = shape[2] // world

    def compare(what):
        F = fields_of(fp, one, spec)
        got1 = rows_of(one, modes, fields)
        within_bound(got1, F, modes, fields, what + " one handle")
        parts = [rows_of(s, modes, fields, "local") for s in g.sims]
        gotg = g.modes(modes, fields)
        total = parts[0].copy()
        for p in parts[1:]:
            total += p
        for q, f in enumerate(fields):                                     # the members' LOCAL rows add up, in rank order, to the group's
            assert np.array_equal(gotg[f], total[:, q, 0] + 1j * total[:, q, 1]), f
        if dist < 2:       # the fields are the one handle's bit for bit: the group's row is another order of the same sum
            within_bound(total, F, modes, fields, what + " group")
            for r, p in enumerate(parts):                                  # ... and each member's row is the sum over its own planes
                ref = mr.amplitudes_slab(F[r * nzl:(r + 1) * nzl], modes, r * nzl, shape[2])
                err = np.maximum(np.abs(p[..., 0] - ref.real.astype(np.float64)), np.abs(p[..., 1] - ref.imag.astype(np.float64))).max(axis=0)
                assert (err <= mr.tolerance(F)).all(), (what, r, err)
        else:              # the interface solve is not the same arithmetic: the tolerances of the energy rows in that mode
            tol = 1e-4 if precision == "fp32" else 1e-9
            scale = np.abs(got1).max(axis=(0, 2))
            assert (np.abs(total - got1).max(axis=(0, 2)) <= tol * scale + mr.tolerance(F)).all(), what

    if not em:
        compare("after precalc")
    one.recordModes(1, 16, modes, fields)
    g.recordModes(1, 16, modes, fields)
    seen = []
    for frame in range(2):
        one.step(); g.step()
        seen.append(g.modes(modes, fields))
    if em:
        one.density(); g.density()                                         # (the full-EM cycle deposits currents: the charge of these positions)
    compare("after 2 frames")
    hg, dg = g.modesHistory()
    h1, d1 = one.modesHistory()
    assert dg == d1 == 0 and hg["substep"].tolist() == h1["substep"].tolist() == [1, 2, 3, 4]
    for f in fields:                                                       # the recorded group history: the group's modes() at those sub-steps
        assert np.array_equal(hg[f][1], seen[0][f]) and np.array_equal(hg[f][3], seen[1][f]), f
    # members that hold different numbers of rows: reported before anything is drained
    g.recordModes(1, 16, modes[:4], ("ex",))
    g.sims[0].recordModes(2, 16, modes[:4], ("ex",))
    g.step()
    with pytest.raises(fp.FusionPicError, match="different recorded rows"):
        g.modesHistory()
    assert [len(s.modesHistory("local")[0]["substep"]) for s in g.sims] == [1] + [2] * (world - 1)
    with pytest.raises(fp.FusionPicError, match="in-process group"):
        g.sims[0].modes(modes, scope="global")
    with pytest.raises(fp.FusionPicError, match="in-process group"):
        g.sims[0].modesHistory("global")
    one.destroy()
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
import modes_reference as mr
import test_gpu_histogram as th
sc = ds.build(fp, json.loads(sys.argv[2]))
world = sc["world"]
modes = mr.mode_list(sc["shape"], np.random.default_rng(3))
uid = fp.commUniqueId()
out, err, uneven = [None] * world, [None] * world, [None] * world
dig = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
def rank_main(r):
    try:
        s = fp.makeCylindricalParticlePusher(dict(sc["spec"], count=3 * sc["n"]), precision=sc["precision"])
        s.commInit(uid, r, world)
        s.domainInit(r, world, ghost_planes=sc["G"], migrate_every=sc["every"], distributed_solve=sc["dist_solve"])
        first = int(sc["counts"][:r].sum())
        s.domainSet(sc["pos"][first:first + sc["counts"][r]], sc["vel"][first:first + sc["counts"][r]], first_id=first)
        s.precalc()
        s.recordModes(1, 32, modes, mr.FIELDS)
        for _ in range(sc["frames"]):
            s.step()
        now = s._modes_rows(modes, mr.FIELDS, "global")[0]
        local = s._modes_rows(modes, mr.FIELDS, "local")[0]
        sub, hist, names, dropped = s._modes_history_rows("global")
        out[r] = (dig(now), sub.tolist(), dig(hist), dropped, dig(local))
        # unequal numbers of recorded rows: refused on every rank
        s.recordModes(1 if r == 0 else 2, 8, modes[:4], ("ex",))
        s.step()
        try:
            s.modesHistory("global")
            uneven[r] = "not refused"
        except fp.FusionPicError as e:
            uneven[r] = (e.code, str(e))
        s.destroy()
    except Exception as e:
        err[r] = repr(e)
threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
for t in threads: t.start()
for t in threads: t.join()
if any(err):
    print(json.dumps({"error": err})); sys.exit(0)
g = th.group_of(fp, sc)
g.recordModes(1, 32, modes, mr.FIELDS)
for _ in range(sc["frames"]):
    g.step()
parts = [s._modes_rows(modes, mr.FIELDS, "local")[0] for s in g.sims]
now = fp._modes_sum(parts)
hp = [s._modes_history_rows("local") for s in g.sims]
hist = fp._modes_sum([h[1] for h in hp])
print(json.dumps({"ranks": out, "uneven": uneven, "group": (dig(now), hp[0][0].tolist(), dig(hist), hp[0][3]), "locals": [dig(p) for p in parts]}))
'''


@pytest.mark.parametrize("world,shape,dist", [(2, (16, 16, 32), 0), (3, (12, 16, 18), 0), (2, (16, 16, 32), 1)])
def test_communicator_global_gives_every_rank_the_same_bits(fp, world, shape, dist):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "fake_rccl")])
    env = dict(os.environ, FPIC_RCCL_LIBRARY=os.path.join(ROOT, "tests", "fake_rccl", "libfakerccl.so"))
    case = dict(world=world, shape=shape, ghost=2 if world == 2 else 1, every=2 if world == 2 else 1, em=False, distributed_solve=dist,
                precision="fp32", n=12000, seed=8, frames=2)
    raw = subprocess.check_output([sys.executable, "-c", COMM_DRIVER, ROOT, json.dumps(case)], env=env, timeout=600)
    res = json.loads(raw.decode().strip().splitlines()[-1])
    assert "error" not in res, res
    ranks, group = res["ranks"], res["group"]
    assert all(r[:4] == ranks[0][:4] for r in ranks)                       # every rank the same bits (as SHA-256 digests)
    assert len(set(r[4] for r in ranks)) == world                          # ... from LOCAL rows that differ
    assert [r[4] for r in ranks] == res["locals"]                          # (the group's members hold the ranks' states)
    assert list(ranks[0][:4]) == list(group)                               # ... the sum in rank order, as the group's
    assert ranks[0][1] == [1, 2, 3, 4] and ranks[0][3] == 0
    for u in res["uneven"]:
        assert u[0] == -5 and "different numbers of recorded rows" in u[1], res["uneven"]


# ---- 8. refusals
def test_refusals(fp):
    sim, spec, _ = two_species_box(fp, "fp32", "poisson_fft", shape=(16, 12, 9), n=4000, ni=2000)
    ok = np.array([[1, 0, 0], [0, -2, 3]], dtype=np.int32)

    def refused(code, text, call, *args, **kw):
        with pytest.raises(fp.FusionPicError) as e:
            call(*args, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)

    for call in (sim.modes, lambda m, *a: sim.recordModes(1, 8, m, *a)):
        refused(-5, "modes before precalc()", call, ok)                                    # field quantities before precalc()
    sim.precalc()
    sim.recordModes(1, 8, ok, ("ex", "rho"))
    sim.substeps(2)
    for call in (sim.modes, lambda m, *a: sim.recordModes(1, 8, m, *a)):
        refused(-1, ".nmodes <- must lie in [1, FPIC_MODES_MAX (256)]", call, np.zeros((0, 3), dtype=np.int32))
        refused(-1, ".nmodes <- must lie in", call, np.stack([np.arange(257) % 8, np.arange(257) // 8 % 6, np.zeros(257)], axis=1).astype(np.int32))
        refused(-1, ".modes <- a component lies outside [-n/2, n/2]", call, [[9, 0, 0]])
        refused(-1, ".modes <- a component lies outside", call, [[0, -7, 0]])
        refused(-1, ".modes <- a component lies outside", call, [[0, 0, 5]])               # nz = 9: [-4, 4]
        refused(-1, ".modes <- the same wave vector twice", call, [[1, 2, 3], [0, 0, 0], [1, 2, 3]])
        refused(-1, ".mask <- no quantity is selected", call, ok, ())
        refused(-1, ".fields <- ", call, ok, ("ex", "jx"))
    sim.modes([[8, -6, 4], [-8, 6, -4]])                                                   # the ends of the ranges are inside
    lib, h = sim._lib, sim._h
    s, names, keep = fp._modes_spec(ok, ("ex",))
    out = np.zeros(64)
    s.mask = 0x100
    refused(-1, ".mask <- unknown bits", lambda: sim._check(lib.fpic_modes_now(h, ctypes.byref(s), fp.DIAG_LOCAL, out.ctypes.data)))
    refused(-1, ".mask <- unknown bits", lambda: sim._check(lib.fpic_modes_record(h, ctypes.byref(s), 1, 8)))
    s.mask = 1
    s.reserved[1] = 0.5
    refused(-1, ".reserved <- must be zero", lambda: sim._check(lib.fpic_modes_now(h, ctypes.byref(s), fp.DIAG_LOCAL, out.ctypes.data)))
    refused(-1, ".reserved <- must be zero", lambda: sim._check(lib.fpic_modes_record(h, ctypes.byref(s), 1, 8)))
    s.reserved[1] = 0.0
    refused(-1, ".spec <- ", lambda: sim._check(lib.fpic_modes_now(h, None, fp.DIAG_LOCAL, out.ctypes.data)))
    refused(-1, ".out <- ", lambda: sim._check(lib.fpic_modes_now(h, ctypes.byref(s), fp.DIAG_LOCAL, None)))
    refused(-1, ".spec <- ", lambda: sim._check(lib.fpic_modes_record(h, None, 1, 8)))
    s.modes = None
    refused(-1, ".modes <- Non-optional", lambda: sim._check(lib.fpic_modes_now(h, ctypes.byref(s), fp.DIAG_LOCAL, out.ctypes.data)))
    refused(-1, ".n <- ", lambda: sim._check(lib.fpic_modes_history(h, fp.DIAG_LOCAL, None, None, 0, None, None)))
    refused(-1, ".scope", lambda: sim._check(lib.fpic_modes_history(h, 7, None, None, 0, ctypes.byref(ctypes.c_uint64()), None)))
    refused(-1, ".scope", lambda: sim._check(lib.fpic_modes_now(h, ctypes.byref(s), 2, out.ctypes.data)))
    refused(-1, ".capacity <- must be at least 1", sim.recordModes, 1, 0, ok)
    refused(-1, ".every <- must be >= 0", sim.recordModes, -1, 8, ok)
    sub, n = np.zeros(8, dtype=np.uint64), ctypes.c_uint64()
    refused(-1, ".capacity <- 2 rows are pending", lambda: sim._check(lib.fpic_modes_history(h, fp.DIAG_LOCAL, sub.ctypes.data, out.ctypes.data, 1, ctypes.byref(n), None)))
    refused(-1, ".out <- ", lambda: sim._check(lib.fpic_modes_history(h, fp.DIAG_LOCAL, sub.ctypes.data, None, 8, ctypes.byref(n), None)))
    # every refused recordModes above left the running recorder's rows intact
    hist, dropped = sim.modesHistory()
    assert hist["substep"].tolist() == [1, 2] and dropped == 0 and np.abs(hist["ex"]).max() > 0
    sim.substeps(1)
    assert sim.modesHistory()[0]["substep"].tolist() == [3]
    sim.destroy()
    # the (r,z) geometry has no modes
    from helpers import make_spec
    rz = fp.makeCylindricalParticlePusher(make_spec(4, 4, 2))
    refused(-5, "needs a CART3D handle", rz.modes, ok)
    refused(-5, "needs a CART3D handle", rz.recordModes, 1, 8, ok)
    refused(-5, "needs a CART3D handle", rz.modesHistory)
    rz.destroy()


# ---- 9. the Node host
def test_modes_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    rng = np.random.default_rng(2)
    n, shape, L = 4000, (16, 16, 16), (0.016, 0.016, 0.016)
    spec = box_spec(shape, L, n, 5e-12, macro_weight=1e15 * np.prod(L) / n)
    pos, vel = rng.random((n, 3)) * L, rng.normal(0, 2e-3, (n, 3))
    modes = mr.mode_list(shape, rng)[:12]
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, p=pos.tolist(), v=vel.tolist(), modes=modes.tolist())))
    script = r"""
const fs = require('fs');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.set({position: inp.p, velocity: inp.v});
sim.precalc();
const req = {modes: inp.modes, fields: ['ex', 'phi', 'rho']};
sim.recordModes(2, 8, req);
sim.step(3);
const now = sim.modes(req);
const h = sim.modesHistory();
const errors = [];
for (const bad of [() => sim.modes({}), () => sim.modes({modes: [[1, 0, 0], [1, 0, 0]]}), () => sim.modes({modes: [[9, 0, 0]]}), () => sim.recordModes(1, 0, req),
                   () => sim.modes({modes: [[0, 0]]}), () => sim.modes({modes: [[1, 0, 0]], fields: ['jx']}), () => sim.modes({modes: [[1, 0, 0]], fields: []})]) {
  try { bad(); errors.push(null); } catch (x) { errors.push(x.message); }
}
const hex = a => Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('hex');
console.log(JSON.stringify({now: hex(now.values), fields: now.fields, isF64: now.values instanceof Float64Array && h.values instanceof Float64Array,
  substep: Array.from(h.substep), hist: hex(h.values), rows: h.rows, dropped: h.dropped, errors: errors}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    twin = fp.makeCylindricalParticlePusher(spec, precision="fp32")
    twin.set(position=pos, velocity=vel)
    twin.precalc()
    twin.recordModes(2, 8, modes, ("ex", "phi", "rho"))
    twin.step(3)
    now = rows_of(twin, modes, ("ex", "phi", "rho"))
    sub, hist, names, dropped = twin._modes_history_rows("global")
    assert out["isF64"] and out["rows"] == 3 and out["dropped"] == dropped == 0 and out["substep"] == sub.tolist() == [2, 4, 6]
    assert out["fields"] == names == ["ex", "phi", "rho"]
    assert out["now"] == now.tobytes().hex() and out["hist"] == hist.tobytes().hex()
    assert all(isinstance(e, str) and " <- " in e for e in out["errors"]), out["errors"]
    twin.destroy()


# ---- 10. physics: the cold-plasma oscillation of examples/plasma_box_node.js, its frequency from ONE recorded mode
def linear_prediction(s, stride):
    """omega * tau of a series that is a combination of exp(+-i omega tau n): s[n + m] + s[n - m] = 2 cos(m omega tau) s[n]"""
    s = np.asarray(s)
    c = np.real(np.vdot(s[stride:-stride], s[2 * stride:] + s[:-2 * stride])) / (2 * np.real(np.vdot(s[stride:-stride], s[stride:-stride])))
    return np.arccos(c) / stride


@pytest.mark.parametrize("precision", PRECISIONS)
def test_cold_plasma_frequency_from_one_mode(fp, precision):
    """The example's setup restated on its smallest box (grid 16, 8 per cell; the example's default is 32): a regular lattice
    of electrons displaced by amp sin(k x), omega_p dt = 0.05, the scheme's dispersion omega_p cos(k dx / 2).  EX at mode
    (1, 0, 0) is recorded every sub-step.  The oscillation stands, so the complex amplitude keeps one phase (mod pi) — that
    is checked — and the frequency is read off the series along that phase by linear prediction (exact for any mix of
    exp(+-i omega t)), which needs no zero crossings.
    The bar is the issue's 1e-4 against the example's formula, and this is the example's own box and formula, so it is used
    as it stands.  Measured on an MI355X: omega / omega_scheme - 1 = 9.6e-5 (fp32) and 8.4e-5 (fp64); the point series of
    the same run at node g/4 gives 1.2e-4 and 8.8e-5 (it also sees the harmonics).  Nearly all of the deviation is the
    leap-frog's own (omega_p dt)^2 / 24 = 1.04e-4 at omega_p dt = 0.05, which the example's formula leaves out."""
    eps0, me, qe = 8.8541878128e-12, 9.109e-31, -1.602e-19
    g, ppc, dx, dt = 16, 8, 1e-3, 2e-12
    L, wp = g * dx, 0.05 / 2e-12
    density = wp * wp * eps0 * me / (qe * qe)
    n = g ** 3 * ppc
    spec = dict(radius=L, length_y=L, height=L, nr=g, ny=g, nz=g, dt=dt, nparticles=0, count=n, particle_mass=me, particle_charge=qe,
                geometry="cart3d", solver="poisson_fft", macro_weight=density * L ** 3 / n)
    k, amp, per = 2 * np.pi / L, 0.02 * dx, g * 2
    c = (np.arange(per) + 0.5) * L / per
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    pos = np.stack([(X + amp * np.sin(k * X)).ravel(), Y.ravel(), Z.ravel()], axis=1)
    sim = fp.makeCylindricalParticlePusher(spec, precision=precision)
    sim.set(position=pos, velocity=np.zeros_like(pos))
    sim.precalc()
    node = g // 4
    sim.recordModes(1, 512, [[1, 0, 0]], ("ex",))
    sim.recordSeries(1, 512, points=[[node * dx, 0, 0]])
    sim.substeps(500)                                  # about four periods
    hist, dropped = sim.modesHistory()
    pts, _ = sim.seriesHistory()
    assert dropped == 0 and len(hist["substep"]) == 500
    A = hist["ex"][:, 0]
    phase = np.angle(A[0])
    along, across = np.real(A * np.exp(-1j * phase)), np.imag(A * np.exp(-1j * phase))
    assert np.abs(across).max() <= 1e-3 * np.abs(along).max()              # a standing wave: one phase, mod pi
    expected = wp * np.cos(k * dx / 2)
    got = linear_prediction(along, 20) / dt
    point = linear_prediction(pts["points"][:, 0, 0], 20) / dt
    print(precision, "omega from the mode / scheme: %.3e   from the point series / scheme: %.3e   mode / point: %.3e"
          % (got / expected - 1, point / expected - 1, got / point - 1))
    assert abs(got / expected - 1) < 1e-4
    # the same bar against the scheme's dispersion with the leap-frog's own term kept, sin(omega dt / 2) = (dt / 2) omega_p
    # cos(k dx / 2): what a defect of the diagnostic cannot hide behind (measured: -8e-6 and -2e-5)
    complete = 2 / dt * np.arcsin(0.5 * dt * expected)
    print(precision, "omega from the mode / scheme with the leap-frog term: %.3e" % (got / complete - 1))
    assert abs(got / complete - 1) < 1e-4
    sim.destroy()
