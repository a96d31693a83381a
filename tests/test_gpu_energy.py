"""Energy and momentum diagnostics of the CART3D box, reduced on the GPU (fpic_energy_now / _record / _history):
the values against numpy over a full read-back and against the CPU oracle, recording that leaves the run bit-identical,
the history against a twin handle bit for bit, the ring's drop count, energy conservation and momentum in physical runs,
the decomposition (in-process group and the communicator over the stand-in RCCL) against one handle, and the Node host."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu

ME, QE, MP = 9.109e-31, -1.602e-19, 1.67e-27
C = 2.998e8
EPS0 = 8.8541878128e-12
MU0 = 1.0 / (EPS0 * C ** 2)


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


@pytest.fixture(scope="module")
def eo():
    import es3d_oracle
    return es3d_oracle


def box_spec(shape, L, count, dt, solver="poisson_fft", **kw):
    s = dict(radius=L[0], length_y=L[1], height=L[2], nr=shape[0], ny=shape[1], nz=shape[2], dt=dt, nparticles=0, count=count,
             particle_mass=ME, particle_charge=QE, geometry="cart3d", solver=solver, macro_weight=1.0)
    s.update(kw)
    return s


def em_dt(shape, L, frac=0.5):
    return frac / (C * np.sqrt(sum((shape[a] / L[a]) ** 2 for a in range(3))))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def two_species_box(fp, precision, solver, shape=(32, 32, 32), n=20000, ni=8000, seed=3):
    """electrons + ions in a box with a uniform external B"""
    rng = np.random.default_rng(seed)
    L = tuple(1e-3 * s for s in shape)
    dt = em_dt(shape, L) if solver == "yee" else 5e-12
    spec = box_spec(shape, L, n, dt, solver=solver, macro_weight=1e15 * np.prod(L) / n)
    sim = fp.makeCylindricalParticlePusher(spec, precision=precision)
    ions = sim.addSpecies(MP, -QE, ni)
    pos, vel = rng.random((n, 3)) * L, rng.normal(0, 0.03, (n, 3))
    pi, vi = rng.random((ni, 3)) * L, rng.normal(0, 1e-3, (ni, 3))
    sim.set(position=pos, velocity=vel)
    sim.set(position=pi, velocity=vi, species=ions)
    sim.addB(0.0, 0.02, 0.05)
    return sim, spec, dict(pos=pos, vel=vel, pi=pi, vi=vi)


def check_particles(sim, e, spec, masses):
    W = spec["macro_weight"]
    for s, m in enumerate(masses):
        v = sim.getParticles(np.float64, species=s)["velocity"]
        assert int(e["count"][s]) == len(v)
        v2 = (v ** 2).sum(axis=1)
        assert rel(e["kinetic"][s], 0.5 * m * W * C ** 2 * v2.sum()) <= 1e-12
        p = m * W * C * v.sum(axis=0)
        scale = m * W * C * np.sqrt(len(v) * v2.sum())   # (a momentum near zero: relative to what its terms add up to)
        assert np.abs(e["momentum"][s] - p).max() <= 1e-12 * max(np.abs(p).max(), 1e-3 * scale)
        assert rel(e["speed_max"][s], np.sqrt(v2.max())) <= 1e-12


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_values_electrostatic(fp, precision):
    sim, spec, _ = two_species_box(fp, precision, "poisson_fft")
    sim.precalc()
    sim.step(10)
    e = sim.energy()
    assert e["substep"] == 20 and e["nspecies"] == 2
    assert sim.energy("local")["kinetic"].tobytes() == e["kinetic"].tobytes()   # undecomposed: LOCAL is GLOBAL
    dv = np.prod([spec["radius"] / 32, spec["length_y"] / 32, spec["height"] / 32])
    e4 = sim.readField(fp.F3_E, np.float64)
    assert rel(e["field_e"], 0.5 * EPS0 * (e4[:, :3] ** 2).sum() * dv) <= 1e-12
    assert e["field_b"] == 0 and e["field_b_external"] == 0
    check_particles(sim, e, spec, [ME, MP])
    # the same state gives the same bits
    assert sim.energy()["kinetic"].tobytes() == e["kinetic"].tobytes()
    sim.destroy()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_values_full_em(fp, eo, precision):
    shape = (16, 16, 16)
    rng = np.random.default_rng(9)
    n = 20000
    L = tuple(1e-3 * s for s in shape)
    spec = box_spec(shape, L, n, em_dt(shape, L), solver="yee", macro_weight=1e15 * np.prod(L) / n)
    dtype = np.float32 if precision == "fp32" else np.float64
    sim, ora = fp.makeCylindricalParticlePusher(spec, precision=precision), eo.OracleES3D(spec, dtype)
    pos, vel = rng.random((n, 3)) * L, rng.normal(0, 0.05, (n, 3))
    for s in (sim, ora):
        s.set(position=pos, velocity=vel)
    sim.addB(0.0, 0.0, 0.01); ora.add_b(0.0, 0.0, 0.01)
    sim.precalc(); ora.precalc()
    sim.step(10); ora.step(10)
    e_open = sim.energy()                       # the chained lattice step has left B at half time: formed in registers
    dv = np.prod(L) / np.prod(shape)
    lat_e = sim.readField(fp.F3_EDGE_E, np.float64)[:, :3]
    lat_b = sim.readField(fp.F3_FACE_B, np.float64)[:, :3]    # (closes the chain: B of the integer time stored)
    e = sim.energy()
    for key in ("field_e", "field_b", "kinetic", "momentum"):
        assert np.asarray(e_open[key]).tobytes() == np.asarray(e[key]).tobytes(), key
    assert rel(e["field_e"], 0.5 * EPS0 * (lat_e ** 2).sum() * dv) <= 1e-12
    assert rel(e["field_b"], 0.5 / MU0 * (lat_b ** 2).sum() * dv) <= 1e-12
    assert rel(e["field_b_external"], 0.5 / MU0 * 0.01 ** 2 * np.prod(L)) <= 1e-12
    check_particles(sim, e, spec, [ME])
    total = e["field_e"] + e["field_b"] + e["kinetic"].sum()
    want = ora.em_field_energy() + ora.kinetic_energy()
    assert rel(total, want) <= (2e-3 if precision == "fp32" else 1e-7)
    sim.destroy()


def twin_run(fp, precision, solver, record):
    sim, _, _ = two_species_box(fp, precision, solver, shape=(16, 16, 16), n=8000, ni=4000, seed=5)
    sim.precalc()
    if record:
        sim.recordEnergy(1, 64)
    sim.step(20)
    return sim


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
@pytest.mark.parametrize("solver", ["poisson_fft", "yee"])
def test_recording_changes_nothing(fp, precision, solver):
    a, b = twin_run(fp, precision, solver, False), twin_run(fp, precision, solver, True)
    rows, dropped = b.energyHistory()
    assert len(rows) == 40 and dropped == 0
    for s in range(2):
        pa, pb = a.getParticles(species=s), b.getParticles(species=s)
        for k in ("position", "velocity"):
            assert pa[k].tobytes() == pb[k].tobytes(), (s, k)
    fields = [fp.F3_E, fp.F3_RHO_FIXED, fp.F3_PHI] if solver != "yee" else [fp.F3_E, fp.F3_B_NODES, fp.F3_EDGE_E, fp.F3_J_FIXED, fp.F3_FACE_B]
    for w in fields:   # (FACE_B last: forming B of the integer time compares the open chain state)
        assert a.readField(w).tobytes() == b.readField(w).tobytes(), w
    a.step(1); b.step(1)
    assert a.getParticles()["velocity"].tobytes() == b.getParticles()["velocity"].tobytes()
    a.destroy(); b.destroy()


@pytest.mark.parametrize("precision,solver", [("fp32", "poisson_fft"), ("fp64", "yee")])
def test_history_rows_equal_the_twin(fp, precision, solver):
    a, _, _ = two_species_box(fp, precision, solver, shape=(16, 16, 16), n=8000, ni=4000, seed=6)
    b, _, _ = two_species_box(fp, precision, solver, shape=(16, 16, 16), n=8000, ni=4000, seed=6)
    a.precalc(); b.precalc()
    a.recordEnergy(3, 64)
    want = []
    for t in range(1, 31):
        a.substeps(1); b.substeps(1)
        if t % 3 == 0:
            want.append(b._energy_row("global"))
    rows, dropped = a.energyHistory()
    assert dropped == 0 and len(rows) == 10
    assert [int(r["substep"]) for r in rows] == list(range(3, 31, 3))
    for got, w in zip(rows, want):
        assert got.tobytes() == w.tobytes()
    assert len(a.energyHistory()[0]) == 0          # drained
    # a ring of 4 rows, 10 recorded: the newest 4, 6 dropped
    a.recordEnergy(1, 4)
    a.substeps(10)
    rows, dropped = a.energyHistory()
    assert dropped == 6 and [int(r["substep"]) for r in rows] == list(range(37, 41))
    assert rows[-1].tobytes() == a._energy_row("global").tobytes()
    a.recordEnergy(0)
    a.substeps(2)
    assert len(a.energyHistory()[0]) == 0
    a.destroy(); b.destroy()


def test_cold_plasma_energy_budget(fp):
    """a cold-plasma oscillation (as test_gpu_es3d's, at omega_p dt = 0.004): over half a plasma period the recorded field
    energy swings from zero to the whole energy and back while field + kinetic energy stays within 1 % (the leap-frog's
    half-step offset between v and E alone makes it wobble by omega_p dt / 2 of itself)"""
    nx, L, per_cell, dt, wp_dt = 32, 1.0, 4, 1e-10, 0.004
    n = nx * per_cell * 4 * 4
    wp = wp_dt / dt
    density = wp ** 2 * EPS0 * ME / QE ** 2
    spec = box_spec((nx, 4, 4), (L, L / 8, L / 8), n, dt, macro_weight=density * L * (L / 8) ** 2 / n)
    sim = fp.makeCylindricalParticlePusher(spec)
    xs = (np.arange(nx * per_cell) + 0.5) / (nx * per_cell) * L
    ys = (np.arange(4) + 0.5) / 4 * (L / 8)
    X, Y, Z = np.meshgrid(xs, ys, ys, indexing="ij")
    pos = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    vel = np.zeros_like(pos)
    vel[:, 0] = 2e-3 * np.sin(2 * np.pi / L * pos[:, 0])
    sim.set(position=pos, velocity=vel)
    sim.precalc()
    sim.recordEnergy(4, 1024)
    sim.step(400)
    rows, dropped = sim.energyHistory()
    assert dropped == 0 and len(rows) == 200
    fe = rows["field_e"]
    total = fe + rows["kinetic"][:, 0]
    assert fe.max() > 0.9 * total.mean() and fe[0] < 0.05 * fe.max() and fe[-1] < 0.2 * fe.max()
    assert (total.max() - total.min()) / total.mean() < 0.01
    sim.destroy()


def test_momentum_without_b(fp):
    """no external B: the total momentum of the history stays within test_gpu_es3d's bar (1e-3 max |dv| sqrt(n) in units
    of c), converted to kg m/s"""
    n = 200000
    shape, L = (32, 32, 32), (0.032, 0.032, 0.032)
    spec = box_spec(shape, L, n, 2e-12, macro_weight=1e15 * np.prod(L) / n)
    sim = fp.makeCylindricalParticlePusher(spec)
    rng = np.random.default_rng(11)
    vel = rng.standard_normal((n, 3)) * 1e-3
    sim.set(position=rng.random((n, 3)) * L, velocity=vel)
    sim.precalc()
    sim.recordEnergy(1, 64)
    p0 = sim.energy()["momentum"][0]
    sim.step(4)
    rows, _ = sim.energyHistory()
    dv = np.abs(sim.getParticles(np.float64)["velocity"] - vel.astype(np.float32)).max()
    bar = 1e-3 * dv * np.sqrt(n) * ME * spec["macro_weight"] * C
    assert dv > 0 and len(rows) == 8
    assert np.abs(rows["momentum"][:, 0, :] - p0).max() <= bar
    sim.destroy()


# ---- decomposition: members of an in-process group against one handle of the same scene (tests/decomp_scene.py)
def group_of(fp, sc):
    import decomp_scene as ds
    world, counts = sc["world"], sc["counts"]
    sims = []
    for r in range(world):
        s = fp.makeCylindricalParticlePusher(dict(sc["spec"], count=3 * sc["n"]), precision=sc["precision"])
        s.domainInit(r, world, ghost_planes=sc["G"], migrate_every=sc["every"], distributed_solve=sc["dist_solve"])
        first = int(counts[:r].sum())
        s.domainSet(sc["pos"][first:first + counts[r]], sc["vel"][first:first + counts[r]], first_id=first)
        sims.append(s)
    g = fp.BoxGroup(sims)
    if sc["em"]:
        for s in sims:
            s.set(edge_E=sc["E"], face_B=sc["B"])
    else:
        g.precalc()
    return g, ds


def compare_rows(got, want, field_tol, particle_tol=1e-12):
    assert got["count"].tolist() == want["count"].tolist()
    assert got["substep"] == want["substep"]
    assert rel(got["kinetic"], want["kinetic"]) <= particle_tol
    scale = np.abs(want["momentum"]).max() + 1e-6 * np.sqrt(want["kinetic"].max())   # (kg m/s vs sqrt(J): only a floor near zero)
    assert np.abs(got["momentum"] - want["momentum"]).max() <= particle_tol * scale
    assert rel(got["speed_max"], want["speed_max"]) <= particle_tol
    assert rel(got["field_e"], want["field_e"]) <= field_tol
    assert rel(got["field_b"] + 1e-300, want["field_b"] + 1e-300) <= field_tol


@pytest.mark.parametrize("world,dist,every,precision", [(2, 0, 1, "fp32"), (2, 1, 1, "fp32"), (2, 2, 1, "fp32"), (4, 0, 2, "fp32"),
                                                        (4, 1, 2, "fp32"), (4, 2, 2, "fp32"), (4, 2, 2, "fp64")])
def test_decomposed_group_sums_equal_one_handle(fp, world, dist, every, precision):
    import decomp_scene as ds
    sc = ds.build(fp, dict(world=world, shape=(16, 16, 32), ghost=2, every=every, em=False, distributed_solve=dist, precision=precision,
                           n=20000, seed=world + dist))
    one = fp.makeCylindricalParticlePusher(sc["spec"], precision=precision)
    one.set(position=sc["pos"], velocity=sc["vel"])
    one.precalc()
    g, _ = group_of(fp, sc)
    # distributed_solve 0 and 1 (a power-of-two grid: the library's own transforms) are the one handle's run bit for bit;
    # 2 (the interface solve) is not the same arithmetic: fields agree to rounding, and so do the particles they push
    tol = 1e-12 if dist == 0 else (1e-4 if precision == "fp32" else 1e-9)
    ptol = 1e-12 if dist < 2 else tol
    for frame in range(3):
        one.step(); g.step()   # (every sub-step with every = 1, every other one with 2, begins with a migration)
        compare_rows(g.energy(), one.energy(), tol, ptol)
    with pytest.raises(fp.FusionPicError):
        g.sims[0].energy("global")     # a group member has no communicator: the host sums the LOCAL values
    assert sum(s.domainStats()["migrated"] for s in g.sims) > 0
    one.destroy()
    for s in g.sims:
        s.destroy()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_decomposed_full_em_group(fp, precision):
    import decomp_scene as ds
    sc = ds.build(fp, dict(world=2, shape=(16, 16, 32), ghost=2, every=2, em=True, distributed_solve=False, precision=precision, n=20000, seed=4))
    one = fp.makeCylindricalParticlePusher(sc["spec"], precision=precision)
    one.set(position=sc["pos"], velocity=sc["vel"])
    one.set(edge_E=sc["E"], face_B=sc["B"])
    g, _ = group_of(fp, sc)
    for s in g.sims:
        s.recordEnergy(1, 16)
    for frame in range(2):
        one.step(); g.step()
        compare_rows(g.energy(), one.energy(), 1e-12)
    hist = [s.energyHistory("local")[0] for s in g.sims]
    assert all(len(h) == 4 for h in hist)
    last = fp._energy_dict(fp._energy_sum([h[-1] for h in hist]))
    compare_rows(last, one.energy(), 1e-12)
    one.destroy()
    for s in g.sims:
        s.destroy()


# ---- the communicator: ranks as threads of one process over the stand-in RCCL (tests/fake_rccl, as test_gpu_fake_rccl.py)
COMM_DRIVER = r'''
import json, os, sys, threading
sys.path.insert(0, os.path.join(sys.argv[1], "fusion-sim_amd"))
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import fusionpic as fp
import decomp_scene as ds
import test_gpu_energy as te
sc = ds.build(fp, json.loads(sys.argv[2]))
world = sc["world"]
uid = fp.commUniqueId()
out, err = [None] * world, [None] * world
def rank_main(r):
    try:
        s = fp.makeCylindricalParticlePusher(dict(sc["spec"], count=3 * sc["n"]), precision=sc["precision"])
        s.commInit(uid, r, world)
        s.domainInit(r, world, ghost_planes=sc["G"], migrate_every=sc["every"], distributed_solve=sc["dist_solve"])
        first = int(sc["counts"][:r].sum())
        s.domainSet(sc["pos"][first:first + sc["counts"][r]], sc["vel"][first:first + sc["counts"][r]], first_id=first)
        s.precalc()
        s.recordEnergy(1, 32)
        for _ in range(sc["frames"]):
            s.step()
        now = s._energy_row("global")
        rows, dropped = s.energyHistory("global")
        out[r] = (now.tobytes().hex(), rows.tobytes().hex(), dropped)
        s.destroy()
    except Exception as e:
        err[r] = repr(e)
threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
for t in threads: t.start()
for t in threads: t.join()
if any(err):
    print(json.dumps({"error": err})); sys.exit(0)
g, _ = te.group_of(fp, sc)
for s in g.sims:
    s.recordEnergy(1, 32)
for _ in range(sc["frames"]):
    g.step()
grp_now = fp._energy_sum([s._energy_row("local") for s in g.sims])
hists = [s.energyHistory("local")[0] for s in g.sims]
grp_rows = np.array([fp._energy_sum([h[i] for h in hists]) for i in range(len(hists[0]))], dtype=fp.ENERGY_DTYPE)
print(json.dumps({"ranks": out, "group_now": grp_now.tobytes().hex(), "group_rows": grp_rows.tobytes().hex()}))
'''


@pytest.mark.parametrize("world,dist", [(2, 0), (4, 2)])
def test_communicator_global_equals_group_sums(fp, world, dist):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "fake_rccl")])
    env = dict(os.environ, FPIC_RCCL_LIBRARY=os.path.join(ROOT, "tests", "fake_rccl", "libfakerccl.so"))
    case = dict(world=world, shape=(16, 16, 32), ghost=2, every=2, em=False, distributed_solve=dist, precision="fp32", n=20000, seed=8, frames=3)
    raw = subprocess.check_output([sys.executable, "-c", COMM_DRIVER, ROOT, json.dumps(case)], env=env, timeout=300)
    res = json.loads(raw.decode().strip().splitlines()[-1])
    assert "error" not in res, res
    dec = lambda h: np.frombuffer(bytes.fromhex(h), dtype=fp.ENERGY_DTYPE)
    ranks = res["ranks"]
    assert all(r[0] == ranks[0][0] and r[1] == ranks[0][1] and r[2] == 0 for r in ranks)   # every rank the same bits
    now, rows = dec(ranks[0][0])[0], dec(ranks[0][1])
    want_now, want_rows = dec(res["group_now"])[0], dec(res["group_rows"])
    assert len(rows) == len(want_rows) == 6
    tol = 1e-12 if dist == 0 else 1e-4
    compare_rows(fp._energy_dict(now), fp._energy_dict(want_now), tol, 1e-12)
    for a, b in zip(rows, want_rows):
        compare_rows(fp._energy_dict(a), fp._energy_dict(b), tol, 1e-12)


def test_energy_through_the_javascript_host(fp, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    rng = np.random.default_rng(2)
    n, shape, L = 4000, (16, 16, 16), (0.016, 0.016, 0.016)
    spec = box_spec(shape, L, n, 5e-12, macro_weight=1e15 * np.prod(L) / n)
    (tmp_path / "in.json").write_text(json.dumps(dict(spec=spec, p=(rng.random((n, 3)) * L).tolist(), v=rng.normal(0, 2e-3, (n, 3)).tolist())))
    script = r"""
const fs = require('fs');
const empic = require(process.argv[1]);
const inp = JSON.parse(fs.readFileSync(process.argv[2]));
const sim = empic.makeCylindricalParticlePusher(inp.spec);
sim.set({position: inp.p, velocity: inp.v});
sim.precalc();
sim.recordEnergy(2, 8);
sim.step(3);
const e = sim.energy();
const h = sim.energyHistory();
console.log(JSON.stringify({e: {substep: e.substep, field_e: e.field_e, kinetic: Array.from(e.kinetic), momentum: Array.from(e.momentum),
  count: Array.from(e.count), speed_max: Array.from(e.speed_max)}, n: h.rows.length, dropped: h.dropped, last: h.rows[h.rows.length - 1].field_e,
  last_substep: h.rows[h.rows.length - 1].substep}));
sim.destroy();
"""
    shim = os.path.join(ROOT, "fusion-sim_amd", "js", "empic_native.js")
    raw = subprocess.check_output([node, "-e", script, shim, str(tmp_path / "in.json")], timeout=300)
    out = json.loads(raw.decode().strip().splitlines()[-1])
    e = out["e"]
    assert e["substep"] == 6 and e["count"] == [n] and len(e["momentum"]) == 3
    assert all(np.isfinite(x) for x in [e["field_e"], *e["kinetic"], *e["momentum"], *e["speed_max"]])
    assert e["field_e"] > 0 and e["kinetic"][0] > 0
    assert out["n"] == 3 and out["dropped"] == 0 and out["last_substep"] == 6 and out["last"] == e["field_e"]
