"""The model behind tests/test_gpu_sequences.py: a seed becomes a small scene of the CART3D box and a list of operations with
all their parameters — nothing of the library, no GPU.  tests/test_sequence_model.py holds the generator to its coverage
conditions on the CPU; the GPU tests replay the lists.

A sequence is a list of STEPS.  A step is one state-changing operation (STATE_KINDS) followed directly by the reading calls of
its `reads` (READ_KINDS): nothing changes the state between the operation and its reads.  Large arrays are not part of a step:
a step carries a `tag`, and particles(seed, tag, n) draws the arrays of that step, the same ones at every call.

The draws that are tied to the seed and not to its generator: the solver is SOLVERS[(seed + seed // 3) % 3], the staged binning
is forced (FPIC_TWO_LEVEL_MIN=1) on every third seed — so the forced seeds meet every solver."""
import math
import os
import re

import numpy as np

import gas_reference as gasref
import pair_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 2.998e8
EPS0 = 8.8541878128e-12
ME, QE, MP, LOG_LAMBDA = pair_scene.ME, pair_scene.QE, pair_scene.MP, pair_scene.LOG_LAMBDA

SHAPE = (24, 20, 12)                    # several 16 x 16 x 8 tiles, a multiple of none; nz splits into 2 and 3 slabs
L = tuple(1e-3 * s for s in SHAPE)
N0, N1 = 3000, 750
SOLVERS = ("none", "poisson_fft", "yee")
# the background of tests/test_gpu_collide.py
BACKGROUND = dict(drift=(0.01, 0.0, -0.02), vth=(0.05, 0.02, 0.1))

STATE_KINDS = ("substeps", "sort", "set", "setRange", "load", "collide_exchange", "collide_elastic", "collide_relax", "pair_like", "pair_unlike",
               "loadCheckpoint")
# (readField follows saveCheckpoint: under full EM it reads B of the integer time, which closes an open lattice step, and a save
# in the same row of reads is to meet the step still open)
READ_KINDS = ("getParticles", "getRange", "getCells", "count", "select", "histogram_lds", "histogram_global", "moments", "energy", "series", "modes",
              "saveCheckpoint", "readField")
POSITION_KINDS = ("set", "setRange", "load")     # may write positions: the fields are stale afterwards

# the committed seeds (chosen so that the coverage conditions of tests/test_sequence_model.py hold; none is skipped at run time)
SEEDS = [0, 1, 2, 4, 5, 6, 8, 16, 21, 22, 46, 54]
RESUME = [("poisson_fft", "fp32"), ("yee", "fp64")]


def em_dt(shape, lengths, frac=0.5):
    return frac / (C * math.sqrt(sum((shape[a] / lengths[a]) ** 2 for a in range(3))))


def compact_range():
    """kCollideCompactMin, kCollideCompactMax of the kernel header: the K between which the compacting pass serves a request"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_collide_kernels.hpp")).read()
    m = re.search(r"kCollideCompactMin\s*=\s*1ull\s*<<\s*(\d+)\s*,\s*kCollideCompactMax\s*=\s*1ull\s*<<\s*(\d+)\s*;", text)
    return 1 << int(m.group(1)), 1 << int(m.group(2))


def hist_lds_bins():
    """kHistLdsBins of the kernel header: above it a histogram counts with global atomics"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_hist_kernels.hpp")).read()
    return int(re.search(r"constexpr\s+\w+\s+kHistLdsBins\s*=\s*(\d+)\s*;", text).group(1))


def pair_tau(W, dv, ma, qa, mb, qb, n_l=2, g=0.03, var=0.05):
    """the time of one application at which a pair of relative speed g (c) in a cell of N_L = n_l has the variance `var`
    (include/fusionpic.h: kappa = (qa qb)^2 log_lambda tau W / (8 pi eps0^2 m_ab^2 c^3 dV), var = kappa N_L / g^3): long
    enough that a pair really turns, in either precision"""
    mab = ma * mb / (ma + mb)
    kappa1 = (qa * qb) ** 2 * LOG_LAMBDA * W / (8 * math.pi * EPS0 ** 2 * mab ** 2 * C ** 3 * dv)
    return var * g ** 3 / (kappa1 * n_l)


def particles(seed, tag, n, lengths=L):
    """positions (metres) and velocities (c) of n particles: thermal, plus a fast fifth that crosses more than a cell per
    electrostatic sub-step (the mixture of test_box_randomised_against_the_oracle)"""
    rng = np.random.default_rng([0xA11CE, seed, tag])
    pos = rng.random((n, 3)) * lengths
    vel = rng.normal(0, 0.02, (n, 3)) + rng.normal(0, 0.4, (n, 3)) * (rng.random((n, 1)) < 0.2)
    return pos, vel


def given_field(seed):
    """the static E of a `none` scene, V/m"""
    return np.random.default_rng([0xF1E1D, seed]).normal(0, 5e4, SHAPE + (3,))


def scene(seed):
    rng = np.random.default_rng([0x5CE9E, seed])
    solver = SOLVERS[(seed + seed // 3) % 3]
    counts = [N0, N1] + ([int(rng.integers(1, 8))] if rng.random() < 0.5 else [])
    dt = em_dt(SHAPE, L) if solver == "yee" else 5e-12
    W = 1e15 * float(np.prod(L)) / N0
    dv = float(np.prod(L)) / float(np.prod(SHAPE))
    sc = dict(seed=seed, solver=solver, precision="fp32" if rng.random() < 0.5 else "fp64", sort_interval=int(rng.integers(0, 4)),
              staged=seed % 3 == 0, counts=counts, masses=[ME, MP, 4 * MP][:len(counts)], charges=[QE, -QE, -2 * QE][:len(counts)],
              shape=SHAPE, L=L, dt=dt, macro_weight=W, dv=dv, addB=[float(x) for x in rng.normal(0, 0.05, 3)] if rng.random() < 0.5 else None,
              registered=bool(rng.random() < 0.5))
    sc["spec"] = dict(radius=L[0], length_y=L[1], height=L[2], nr=SHAPE[0], ny=SHAPE[1], nz=SHAPE[2], dt=dt, nparticles=0, count=N0,
                      particle_mass=ME, particle_charge=QE, geometry="cart3d", solver=solver, macro_weight=W)
    sc["tau_like"] = [pair_tau(W, dv, sc["masses"][a], sc["charges"][a], sc["masses"][a], sc["charges"][a]) for a in range(2)]
    sc["tau_unlike"] = pair_tau(W, dv, ME, QE, MP, -QE, n_l=1)
    if sc["registered"]:
        kind = ("exchange", "elastic", "relax")[int(rng.integers(0, 3))]
        kw = dict(nu_tau=0.2, seed=int(rng.integers(1, 1 << 40)), stream=1, epoch=int(rng.integers(0, 1000)), **BACKGROUND)
        if kind == "elastic":
            kw["mass_ratio"] = 2.0
        sc["collide_every"] = dict(every=int(rng.integers(1, 4)), kind=kind, species=0, kw=kw)
        unlike = bool(rng.random() < 0.5)
        sc["pair_every"] = dict(every=int(rng.integers(1, 4)), a=0, b=1 if unlike else None,
                                kw=dict(log_lambda=LOG_LAMBDA, tau=sc["tau_unlike"] if unlike else sc["tau_like"][0], seed=int(rng.integers(1, 1 << 40)), stream=2,
                                        epoch=int(rng.integers(0, 1000))))
        pts = rng.random((3, 3)) * L
        fields = ["ex", "ey", "ez", "phi"] + (["bx", "by", "bz"] if solver == "yee" else ["rho"])   # (full EM deposits no charge in a sub-step)
        sc["recorders"] = dict(energy=dict(every=1, capacity=4),
                               series=dict(every=2, capacity=3, points=pts, tracers=[int(x) for x in rng.choice(N1, 4, replace=False)], species=1),
                               modes=dict(every=3, capacity=2, modes=[(1, 0, 0), (-2, 3, 1), (0, 0, 5)], fields=fields))
    return sc


def _threshold_rate(rng):
    """a P_max on either side of both pass thresholds of collide_compacts, as nu_tau; the side's name"""
    lo, hi = compact_range()
    side = int(rng.integers(0, 4))
    target = (lo * 0.9, lo * 1.1, hi * 0.9, hi * 1.1)[side]
    return -math.log1p(-target * 2.0 ** -32), ("below_lo", "above_lo", "below_hi", "above_hi")[side]


def _read(rng, kind, sc, saved, index):
    ns = len(sc["counts"])
    species = int(rng.integers(0, ns))
    n = sc["counts"][species]
    r = dict(kind=kind, species=species)
    if kind == "getRange":
        first = int(rng.integers(0, n))
        stride = int(rng.integers(1, 4))
        r.update(first=first, stride=stride, count=int(rng.integers(1, (n - first + stride - 1) // stride + 1)))
    elif kind in ("count", "select"):
        where = {}
        if rng.random() < 0.8:
            lo = float(rng.uniform(0.0, 0.6))
            where["xyz"[int(rng.integers(0, 3))]] = (lo, lo + float(rng.uniform(0.2, 0.4)))
        if rng.random() < 0.6:
            where[("vx", "vy", "vz")[int(rng.integers(0, 3))]] = (None, float(rng.uniform(-0.01, 0.03)))
        if rng.random() < 0.3:
            where["v2"] = (float(rng.uniform(0, 1e-4)), None)
        mod = int(rng.integers(2, 6))
        r.update(where=where, every=(mod, int(rng.integers(0, mod))) if rng.random() < 0.5 else None)
    elif kind in ("histogram_lds", "histogram_global"):
        edge = hist_lds_bins()
        bins = (24, 32) if kind == "histogram_lds" else (160, edge // 160 + 1)
        assert (bins[0] * bins[1] <= edge) == (kind == "histogram_lds")
        axes = (("x", "vx"), ("z", "vy"), ("y", "v2"))[int(rng.integers(0, 3))]
        r.update(axes=axes, bins=bins, ranges=((0.0, 1.0), (0.0, 0.01) if axes[1] == "v2" else (-0.06, 0.06)))
    elif kind == "moments":
        r.update(which="order1")
    elif kind == "series":
        r.update(points=rng.random((2, 3)) * L, tracers=[int(x) for x in rng.choice(n, min(n, 5), replace=False)])
    elif kind == "modes":
        r.update(modes=[(1, 0, 0), (0, -2, 3)], fields=("ex", "ey", "ez", "phi"))
    elif kind == "saveCheckpoint":
        r.update(file=len(saved))
        saved.append(index)
    return r


def sequence(seed):
    """the steps of a seed: 12 to 16 state-changing operations, the first a substeps, each with four reading calls"""
    sc = scene(seed)
    rng = np.random.default_rng([0x0B5, seed])
    ns = len(sc["counts"])
    nsteps = int(rng.integers(12, 17))
    others = [k for k in STATE_KINDS if k != "substeps"]
    cycle = [others[i] for i in rng.permutation(len(others))]
    at = 0
    seen = {k: 0 for k in STATE_KINDS}
    saved = []            # the step index at which file f was saved
    last_substeps = -1    # the index of the newest substeps step
    steps = []
    for index in range(nsteps):
        if index == 0 or (steps[-1]["kind"] != "substeps" and rng.random() < 0.6) or (steps[-1]["kind"] == "substeps" and rng.random() < 0.15):
            kind = "substeps"
        else:
            kind = cycle[at % len(cycle)]
            at += 1
            # a rewind needs a file with a substeps after it (something to rewind)
            if kind == "loadCheckpoint" and not any(s < last_substeps for s in saved):
                kind = cycle[at % len(cycle)]
                at += 1
        st = dict(kind=kind, tag=index + 1, precalc=False)
        species = int(rng.integers(0, ns))
        n = sc["counts"][species]
        if kind == "substeps":
            st["k"] = int(rng.choice([1, 2, 3, 5]))
            last_substeps = index
        elif kind == "set":
            st.update(species=species, what=("position", "velocity", "both")[int(rng.integers(0, 3))])
        elif kind in ("setRange", "load"):
            species = int(rng.integers(0, 2))            # (a strict sub-range needs more than a handful of particles)
            n = sc["counts"][species]
            first = int(rng.integers(1, n - 1))
            st.update(species=species, first=first, count=int(rng.integers(1, n - first)), what=("position", "velocity", "both")[int(rng.integers(0, 3))])
            if kind == "load":
                lo = [float(x) for x in rng.uniform(0, 0.4, 3) * L]
                st.update(seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), lo=lo, hi=[float(lo[a] + rng.uniform(0.3, 0.6) * L[a]) for a in range(3)],
                          drift=[float(x) for x in rng.normal(0, 0.01, 3)], vth=float(rng.uniform(0.01, 0.05)), lattice=bool(rng.random() < 0.5),
                          paired=bool(rng.random() < 0.4))
        elif kind.startswith("collide_"):
            what = kind[len("collide_"):]
            kw = dict(species=0, seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), epoch=int(rng.integers(0, 1000)), **BACKGROUND)
            if what == "relax":
                kw["nu_tau"] = float(rng.uniform(0.1, 0.5))
            else:
                x_max, st["side"] = _threshold_rate(rng)
                if what == "elastic":
                    kw["mass_ratio"] = float(rng.choice([0.5, 2.0]))
                if what == "elastic" and rng.random() < 0.5:     # the null-collision form: x_max = nu_tau + sigma_tau g_max
                    kw.update(nu_tau=x_max / 2, g_max=0.5, sigma_tau=x_max)
                else:
                    kw["nu_tau"] = x_max
            st.update(what=what, kw=kw)
        elif kind in ("pair_like", "pair_unlike"):
            a = int(rng.integers(0, 2))
            st.update(a=a, b=None if kind == "pair_like" else 1 - a,
                      kw=dict(log_lambda=LOG_LAMBDA, tau=sc["tau_like"][a] if kind == "pair_like" else sc["tau_unlike"],
                              seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), epoch=int(rng.integers(0, 1000))))
        elif kind == "loadCheckpoint":
            files = [f for f, s in enumerate(saved) if s < last_substeps]
            st["file"] = files[int(rng.integers(0, len(files)))]
        if kind in POSITION_KINDS and st["what"] != "velocity":
            st["precalc"] = sc["solver"] != "none" or bool(rng.random() < 0.5)
        # the reads: four kinds in a row of the cycle of READ_KINDS, begun at a place that moves with the seed, the kind and its occurrence
        off = (seed * 4 + STATE_KINDS.index(kind) * 5 + seen[kind] * 4) % len(READ_KINDS)
        seen[kind] += 1
        st["reads"] = [_read(rng, READ_KINDS[(off + i) % len(READ_KINDS)], sc, saved, index) for i in range(4)]
        steps.append(st)
    return steps


def compares_face_b(index):
    """Whether the comparison of A with its twin after step `index` reads B of the integer time (FPIC_F3_FACE_B), which closes
    an open chained lattice step of a full-EM handle.  Every other step leaves it open, so that the reads of that step — a
    saveCheckpoint among them — and the save that fills the next twin meet the open step."""
    return index % 2 == 1


def can_have_rebinned(sc, steps, position_kinds=POSITION_KINDS):
    """per step: True for a substeps after which a fused re-binning push can have reordered the particles — sort_interval > 0, an
    electrostatic cycle, and more than sort_interval sub-steps since the particles were last put into the caller's order or
    binned afresh (the first sub-step bins; the re-binning push is the sort_interval + 1st)"""
    out, since = [], 0
    for st in steps:
        if st["kind"] == "substeps":
            since += st["k"]
            out.append(sc["solver"] != "yee" and sc["sort_interval"] > 0 and since > sc["sort_interval"])
        else:
            if (st["kind"] in position_kinds and st["what"] != "velocity") or st["kind"] in ("loadCheckpoint", "sort"):
                since = 0
            out.append(False)
    return out


# ---- relation 3: the decomposition.  Six cases: 2 and 3 ranks, ghost planes 2, migrate_every 1..3, electrostatic and full EM,
# distributed_solve 0 and 1.  distributed_solve = 1 is documented as bit-identical to one handle on power-of-two grids (the
# library's own transforms), so it runs on 16 x 8 x 16 — and on two ranks, because three do not divide a power of two.  Full EM
# keeps ghost_planes + 2 halo planes per side and needs slabs of 8 planes.
GROUP_CASES = [
    dict(world=2, shape=(24, 20, 12), em=False, distributed_solve=0, every=1, precision="fp32", staged=True),
    dict(world=3, shape=(24, 20, 12), em=False, distributed_solve=0, every=2, precision="fp64", staged=False),
    dict(world=2, shape=(16, 8, 16), em=False, distributed_solve=1, every=3, precision="fp64", staged=False),
    dict(world=3, shape=(20, 12, 24), em=True, distributed_solve=0, every=3, precision="fp32", staged=False),
    dict(world=2, shape=(16, 8, 16), em=True, distributed_solve=1, every=2, precision="fp64", staged=True),
    dict(world=2, shape=(24, 20, 16), em=True, distributed_solve=0, every=1, precision="fp32", staged=False),
]
GROUP_STATE_KINDS = ("step", "collide_exchange", "collide_elastic", "collide_relax", "reload", "pair_refused")
GROUP_READ_KINDS = ("count", "select", "histogram", "moments", "energy")
# a cold background at rest: no collision may push a particle beyond the ghost planes between two migrations
GROUP_BACKGROUND = dict(drift=(0.0, 0.01, 0.0), vth=(0.03, 0.03, 0.02))


def group_case(index):
    case = dict(GROUP_CASES[index], ghost=2, seed=7000 + index, n=3000, precalc=True)
    case["collide_every"] = dict(every=1 + index % 3, kind=("relax", "exchange", "elastic")[index % 3],
                                 kw=dict(nu_tau=0.2, seed=900 + index, stream=3, epoch=17 * index, **GROUP_BACKGROUND))
    if case["collide_every"]["kind"] == "elastic":
        case["collide_every"]["kw"]["mass_ratio"] = 0.05
    return case


def group_sequence(index):
    """12 to 16 operations on a group and on one handle: mostly frames, each collision kind, one full reload, the refusal of the
    binary collisions once; two reads after each"""
    rng = np.random.default_rng([0x6409, index])
    n = 3000
    nsteps = int(rng.integers(12, 17))
    others = ["collide_exchange", "collide_elastic", "collide_relax", "reload", "pair_refused"]
    cycle = [others[i] for i in rng.permutation(len(others))]
    steps, at = [], 0
    for i in range(nsteps):
        if i % 2 == 0 or at >= len(cycle) + 2:
            st = dict(kind="step")
        else:
            kind = (cycle + ["collide_relax", "collide_exchange"])[at]
            at += 1
            st = dict(kind=kind)
            if kind.startswith("collide_"):
                what = kind[len("collide_"):]
                kw = dict(species=0, seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), epoch=int(rng.integers(0, 1000)), **GROUP_BACKGROUND)
                if what == "relax":
                    kw["nu_tau"] = 0.3
                else:
                    kw["nu_tau"], st["side"] = _threshold_rate(rng)
                if what == "elastic":
                    kw["mass_ratio"] = 0.05
                st.update(what=what, kw=kw)
            elif kind == "reload":
                st["population"] = dict(first=0, count=n, seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), drift=(0.0, 0.01, 0.0), vth=0.02,
                                        lattice=bool(rng.random() < 0.5))
        reads = []
        for j in range(2):
            kind = GROUP_READ_KINDS[(index + 2 * i + j) % len(GROUP_READ_KINDS)]
            r = dict(kind=kind)
            if kind in ("count", "select"):
                lo = float(rng.uniform(0.0, 0.6))
                r.update(where={"xyz"[int(rng.integers(0, 3))]: (lo, lo + 0.3), "vz": (None, float(rng.uniform(-0.01, 0.03)))},
                         every=(3, int(rng.integers(0, 3))) if rng.random() < 0.5 else None)
            elif kind == "histogram":
                r.update(axes=("z", "vz"), bins=(24, 32), ranges=((0.0, 1.0), (-0.3, 0.3)))
            elif kind == "moments":
                r.update(which="order1")
            reads.append(r)
        st["reads"] = reads
        steps.append(st)
    return steps


# ---- the resume with registered operators: N sub-steps in one run, or t (a common multiple of both periods) and N - t
RESUME_EVERY = (2, 3)
RESUME_T, RESUME_N = 6, 11


def resume_scene(solver, precision):
    """the scene of seed 1000 with the given solver and precision, a background operator every 2nd and a binary operator
    every 3rd sub-step"""
    sc = scene(1000)
    dt = em_dt(SHAPE, L) if solver == "yee" else 5e-12
    sc.update(solver=solver, precision=precision, dt=dt, sort_interval=2, staged=False, registered=True)
    sc["spec"] = dict(sc["spec"], solver=solver, dt=dt)
    sc["collide_every"] = dict(every=RESUME_EVERY[0], kind="elastic", species=0, kw=dict(nu_tau=0.2, mass_ratio=2.0, seed=4242, stream=1, epoch=5, **BACKGROUND))
    sc["pair_every"] = dict(every=RESUME_EVERY[1], a=0, b=1, kw=dict(log_lambda=LOG_LAMBDA, tau=sc["tau_unlike"], seed=4343, stream=2, epoch=90))
    sc.pop("recorders", None)
    return sc


# ---- named sequences: states the issue names that a random list reaches only by luck, written out
def _named_reads(rng, sc, saved, index, kinds):
    return [_read(rng, k, sc, saved, index) for k in kinds]


def pending_rebinning():
    """A checkpoint saved from, and loaded into, a handle one of whose species is binned WITH A RE-BINNING PENDING.  With the
    staged binning forced, precalc() bins a species whose positions were just rewritten, and lays out the next bin table of
    the other species from the census its last push left: that re-binning stays pending until the next sub-step (the step
    carries expect_sort_pass: precalc() must report a binning pass).  In that state: a save, a velocity-only operation, a
    rewind to a file saved earlier, and later a rewind to the file saved while pending."""
    sc = scene(300)
    sc.update(solver="poisson_fft", precision="fp32", sort_interval=2, staged=True, registered=False, dt=5e-12, name="pending_rebinning")
    sc["spec"] = dict(sc["spec"], solver="poisson_fft", dt=5e-12)
    for key in ("collide_every", "pair_every", "recorders"):
        sc.pop(key, None)
    rng = np.random.default_rng([0x9E9D, 300])
    relax = dict(species=0, seed=77, stream=3, epoch=9, nu_tau=0.3, **BACKGROUND)
    plan = [
        (dict(kind="substeps", k=3), ("getParticles", "count", "moments", "saveCheckpoint")),                                  # file 0: plain
        (dict(kind="setRange", species=1, first=10, count=200, what="position", precalc=True, expect_sort_pass=True),
         ("saveCheckpoint", "select", "histogram_lds", "energy")),                                                             # file 1: saved while pending
        (dict(kind="collide_relax", what="relax", kw=relax), ("moments", "series", "modes", "readField")),
        (dict(kind="loadCheckpoint", file=0), ("getRange", "getCells", "histogram_global", "count")),                          # loaded while pending
        (dict(kind="substeps", k=2), ("moments", "select", "energy", "readField")),
        (dict(kind="set", species=0, what="position", precalc=True, expect_sort_pass=True), ("count", "moments", "saveCheckpoint", "getCells")),   # species 1 pending
        (dict(kind="loadCheckpoint", file=1), ("select", "moments", "histogram_lds", "series")),                               # the file of a pending handle
        (dict(kind="substeps", k=5), ("moments", "count", "energy", "readField")),
        (dict(kind="load", species=0, first=100, count=900, what="both", seed=4711, stream=2, lo=[0.0, 0.0, 0.0], hi=[L[0] / 2, L[1], L[2]], drift=[0.0, 0.0, 0.0],
              vth=0.02, lattice=True, paired=True, precalc=True, expect_sort_pass=True), ("saveCheckpoint", "moments", "select", "getRange")),
        (dict(kind="substeps", k=3), ("moments", "histogram_lds", "count", "getParticles")),
    ]
    steps, saved = [], []
    for index, (st, kinds) in enumerate(plan):
        st = dict(dict(tag=index + 1, precalc=False), **st)
        st["reads"] = _named_reads(rng, sc, saved, index, kinds)
        steps.append(st)
    return sc, steps


NAMED = {"pending_rebinning": pending_rebinning}


# ================================================================================================ generation 2
# The six newest operator families under the same relations (tests/test_gpu_sequences2.py).  Generation 1 above stays what it
# is: tests/test_sequence_model.py pins its scenes and step lists to digests.  The scene of a generation-2 seed is the
# generation-1 scene of that seed with more operators registered; its steps are drawn by their own generator.
STATE_KINDS2 = STATE_KINDS + ("force_field", "force_accel", "gas_exchange", "gas_elastic", "load_profile", "load_radial")
READ_KINDS2 = READ_KINDS + ("fusionYield", "fusionSpectrum")
STATS_KINDS2 = ("forceStats", "gasStats", "fusionStats", "fusionGrid", "fusionSpectrumRead")      # on scenes with registered operators
POSITION_KINDS2 = POSITION_KINDS + ("load_profile", "load_radial")
READS2 = 6
GAS_G = (0.05, 0.3)
GROUP_GAS_G = (0.02, 1.5)          # (a group's particles stream at up to 0.9 along z, and after a cold reload most relative speeds lie below 0.05)
FUSION_G, FUSION_NODES = (0.02, 0.3), 64
LOS = (1.0, 2.0, -2.0)
FORCE_FIELD_AMP, FORCE_ACCEL_AMP = 1e6, 3e16      # V/m on electrons (100 times that on the ions), m/s^2

# chosen by tests/test_sequence_model.py's conditions (coverage and no vacuous request); none is skipped at run time
SEEDS2 = [0, 9, 10, 15, 16, 35, 38, 101, 107, 116, 122, 149]


def gas_compact_range():
    """kGasCompactMin, kGasCompactMax of the kernel header: the K between which the queue serves a request"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_gas_kernels.hpp")).read()
    m = re.search(r"kGasCompactMin\s*=\s*1ull\s*<<\s*(\d+)\s*,\s*kGasCompactMax\s*=\s*1ull\s*<<\s*(\d+)\s*;", text)
    return 1 << int(m.group(1)), 1 << int(m.group(2))


def gas_window_first_max():
    """kGasWindowFirstMax of the kernel header: the share of the box's volume below which the window is tested first"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_gas_kernels.hpp")).read()
    return float(re.search(r"constexpr\s+double\s+kGasWindowFirstMax\s*=\s*([0-9.eE+-]+)\s*;", text).group(1))


def gas_table(g=GAS_G):
    """sigma g constant over the table: a candidate inside the table is accepted with nearly the local density's share, so
    that a request with a handful of candidates still collides somebody"""
    lo, hi = g
    return 3e-19 * (lo / np.linspace(lo, hi, 96 if g == GAS_G else 1024))


def fusion_table():
    return 1e-28 * (1.0 + np.sin(40.0 * np.linspace(FUSION_G[0], FUSION_G[1], FUSION_NODES)) ** 2)


def gas_density(K, tau, g=GAS_G):
    """the density at which a request has (within a few units) the candidate word bound K"""
    return -math.log1p(-K * 2.0 ** -32) / (C * tau * gasref.bound(gas_table(g), g[0], g[1]))


def window_volume(kw, lengths=L):
    if "lo" not in kw:
        return 1.0
    return float(np.prod([(kw["hi"][a] - kw["lo"][a]) / lengths[a] for a in range(3)]))


def _window(rng, which, lengths=L):
    """whole: the box; narrow: a strict sub-box of 0.125 .. 0.343 of the volume; wide: one of 0.512 .. 0.857"""
    if which == "whole":
        return {}
    span = rng.uniform(0.5, 0.7, 3) if which == "narrow" else rng.uniform(0.8, 0.95, 3)
    lo = rng.uniform(0, 1, 3) * (1 - span)
    return dict(lo=[float(lo[a] * lengths[a]) for a in range(3)], hi=[float((lo[a] + span[a]) * lengths[a]) for a in range(3)])


def _tapers(rng, least, most):
    """tables on 0 .. 3 axes, of 2, 5 or 9 nodes"""
    out = [None, None, None]
    for a in rng.permutation(3)[:int(rng.integers(0, 4))]:
        out[int(a)] = [float(x) for x in rng.uniform(least, most, int(rng.choice([2, 5, 9])))]
    return out


def _waves(rng, n, amp):
    out = []
    for _ in range(n):
        mode = rng.integers(-3, 4, 3)
        if not mode.any():
            mode[int(rng.integers(0, 3))] = 1
        out.append(dict(amp=[float(x) for x in rng.normal(0, amp, 3)], mode=[int(m) for m in mode],
                        nu=float(rng.uniform(0.05, 0.45) * rng.choice([-1.0, 1.0])), phase=float(rng.random())))
    return out


def _force_kw(rng, kind, species, window, epoch, envelope=None, scale=1.0, lengths=L):
    amp = FORCE_ACCEL_AMP if kind == "accel" else FORCE_FIELD_AMP * (1 if species == 0 else 100)
    kw = dict(kind=kind, species=species, waves=_waves(rng, int(rng.choice([1, 4, 2, 3], p=[0.3, 0.3, 0.2, 0.2])), amp * scale), taper=_tapers(rng, 0.5, 1.5),
              epoch=epoch, **_window(rng, window, lengths))
    if envelope is not None:
        kw["envelope"] = envelope
    return kw


def _gas_kw(rng, what, species, window, tau, K, background, g=GAS_G, lengths=L, taper_min=0.6):
    kw = dict(species=species, density=gas_density(K, tau, g), tau=tau, sigma=gas_table(g), g_lo=g[0], g_hi=g[1], seed=int(rng.integers(1, 1 << 40)),
              stream=int(rng.integers(0, 8)), epoch=int(rng.integers(0, 1000)), taper=_tapers(rng, taper_min, 1.0), **background, **_window(rng, window, lengths))
    if what == "elastic":
        kw["mass_ratio"] = 2.0 if background is BACKGROUND else 0.05
    return kw


def _gas_side(rng):
    lo, hi = gas_compact_range()
    side = int(rng.integers(0, 4))
    return (lo * 0.9, lo * 1.1, hi * 0.9, hi * 1.1)[side], ("below_lo", "above_lo", "below_hi", "above_hi")[side]


def _fusion_kw(rng, tau):
    return dict(sigma=fusion_table(), g_lo=FUSION_G[0], g_hi=FUSION_G[1], tau=tau, seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)),
                epoch=int(rng.integers(0, 1000)))


def spectrum_axis(masses, a, b, form):
    """the axis of a spectrum of species a with b (None: with itself): "cm", or the laboratory energy of the lighter reactant
    re-emitted ("product": isotropic, "los": along LOS) with a q_value of the size of the reacting energy; the ranges leave yield
    below and above"""
    ma, mb = masses[a], masses[a if b is None else b]
    hk = 0.5 * (ma * mb / (ma + mb)) * C * C
    if form == "cm":
        return dict(axis="cm", bins=7, lo=hk * 0.04 ** 2, hi=hk * 0.2 ** 2)
    m3, m4 = min(ma, mb), max(ma, mb)
    w = (0.05, 0.2) if b is None else (0.08, 0.25)
    out = dict(axis="product", bins=16, lo=0.5 * m3 * C * C * w[0] ** 2, hi=0.5 * m3 * C * C * w[1] ** 2, q_value=hk * 0.01, product_mass=m3, other_mass=m4)
    if form == "los":
        out["los"] = LOS
    return out


def _registered2(sc, rng, every=None, envelope=(None, None)):
    """the generation-2 operators of a scene with registered operators, beside collide_every, pair_every and the recorders:
    two forces on different species (the first with an envelope from sub-step envelope[0] to envelope[1]), a windowed
    background operator, a yield tally and a spectrum; every: the periods of the last three (drawn from 1 .. 3)"""
    every = every or [int(x) for x in rng.integers(1, 4, 3)]
    e0 = int(rng.integers(0, 1000))
    a = int(rng.integers(2, 4)) if envelope[0] is None else envelope[0]
    b = a + int(rng.integers(3, 6)) if envelope[1] is None else envelope[1]
    first = int(rng.integers(0, 2))
    sc["force_on"] = [
        _force_kw(rng, "field", first, ("whole", "narrow", "wide")[int(rng.integers(0, 3))], e0, envelope=dict(start=e0 + a, stop=e0 + b, values=[0.3, 1.0, 0.5]), scale=0.3),
        _force_kw(rng, "accel", 1 - first, ("whole", "wide")[int(rng.integers(0, 2))], int(rng.integers(0, 1000)), scale=0.3)]
    sc["force_window"] = (a, b)
    lo, hi = gas_compact_range()
    what = ("exchange", "elastic")[int(rng.integers(0, 2))]
    sc["gas_every"] = dict(every=every[0], kind=what,
                           kw=_gas_kw(rng, what, 0, ("whole", "narrow", "wide")[int(rng.integers(0, 3))], every[0] * sc["dt"], math.sqrt(lo * hi), BACKGROUND))
    unlike = bool(rng.random() < 0.5)
    sc["fusion_every"] = dict(every=every[1], a=0, b=1 if unlike else None, kw=_fusion_kw(rng, every[1] * sc["dt"]))
    unlike = bool(rng.random() < 0.5)
    form = ("product", "los", "cm")[int(rng.integers(0, 3))]
    sc["spectrum_every"] = dict(every=every[2], a=0, b=1 if unlike else None, form=form,
                                kw=dict(_fusion_kw(rng, every[2] * sc["dt"]), **spectrum_axis(sc["masses"], 0, 1 if unlike else None, form)))


def scene2(seed):
    sc = scene(seed)
    sc["generation"] = 2
    if sc["registered"]:
        _registered2(sc, np.random.default_rng([0x5CE92, seed]))
    return sc


def _read2(rng, kind, sc, saved, index):
    if kind in READ_KINDS:
        return _read(rng, kind, sc, saved, index)
    if kind in STATS_KINDS2:
        return dict(kind=kind, species=0)
    like = bool(rng.random() < 0.5)
    a = int(rng.integers(0, 2))
    b = None if like else 1 - a
    r = dict(kind=kind, species=a, a=a, b=b, kw=_fusion_kw(rng, sc["dt"]))
    if kind == "fusionSpectrum":
        r["form"] = ("product", "los", "cm")[int(rng.integers(0, 3))]
        r["kw"].update(spectrum_axis(sc["masses"], a, b, r["form"]))
    return r


def _sub_box(rng):
    lo = [float(x) for x in rng.uniform(0, 0.4, 3) * L]
    return lo, [float(lo[a] + rng.uniform(0.3, 0.6) * L[a]) for a in range(3)]


def _table(rng, least, most, nodes=None):
    return [float(x) for x in rng.uniform(least, most, int(rng.integers(2, 10)) if nodes is None else nodes)]


def _radial(rng, lengths=L, flow=0.01):
    """a sphere or a cylinder with density, thermal and flow tables; half of them reach across the periodic boundary"""
    sphere = bool(rng.random() < 0.4)
    axis = 0 if sphere else int(rng.integers(0, 3))
    spanned = [a for a in range(3) if sphere or a != axis]
    r_max = float(rng.uniform(0.5, 0.95) * min(lengths[a] for a in spanned) / 2)
    center = [float(x) for x in rng.random(3) * lengths]
    if rng.random() < 0.5:
        center[spanned[int(rng.integers(0, len(spanned)))]] = float(rng.uniform(0, 0.5) * r_max)
    out = dict(geometry="sphere" if sphere else "cylinder", center=center, r_max=r_max, axis=axis, density=_table(rng, 0.1, 1.0, 5), thermal=_table(rng, 0.5, 1.5, 4),
               flow_radial=[float(x) for x in rng.normal(0, flow, 3)])
    if not sphere:
        out.update(flow_azimuthal=[float(x) for x in rng.normal(0, flow, 4)], flow_axial=[float(x) for x in rng.normal(0, flow, 2)])
    return out


def radial_is_across(radial, lengths=L):
    spanned = [a for a in range(3) if radial["geometry"] == "sphere" or a != radial["axis"]]
    return any(radial["center"][a] - radial["r_max"] < 0 or radial["center"][a] + radial["r_max"] > lengths[a] for a in spanned)


def sequence2(seed, nsteps=None):
    """the steps of a generation-2 seed: 14 to 17 state-changing operations of STATE_KINDS2, the first a substeps, each with
    READS2 reading calls of READ_KINDS2 and, on a scene with registered operators, every read of STATS_KINDS2.  A force step
    carries `t`, the sub-steps the handle has behind it (a one-shot force's time is the handle's own count plus its epoch),
    and `active`: whether its envelope holds then."""
    sc = scene2(seed)
    rng = np.random.default_rng([0x0B52, seed])
    ns = len(sc["counts"])
    nsteps = int(rng.integers(14, 18)) if nsteps is None else nsteps
    others = [k for k in STATE_KINDS2 if k != "substeps"]
    cycle = [others[i] for i in rng.permutation(len(others))]
    at = t = 0
    seen = {k: 0 for k in STATE_KINDS2}
    saved = []
    last_substeps = -1
    steps = []
    for index in range(nsteps):
        if index == 0 or (steps[-1]["kind"] != "substeps" and rng.random() < 0.6) or (steps[-1]["kind"] == "substeps" and rng.random() < 0.1):
            kind = "substeps"
        else:
            kind = cycle[at % len(cycle)]
            at += 1
            if kind == "loadCheckpoint" and not any(s < last_substeps for s in saved):
                kind = cycle[at % len(cycle)]
                at += 1
        st = dict(kind=kind, tag=index + 1, precalc=False)
        if kind in STATE_KINDS and kind != "substeps" and kind != "loadCheckpoint":
            st = dict(_step1(rng, sc, kind), tag=index + 1, precalc=False)
        elif kind == "substeps":
            st["k"] = int(rng.choice([1, 2, 3, 5]))
            t += st["k"]
            last_substeps = index
        elif kind == "loadCheckpoint":
            files = [f for f, s in enumerate(saved) if s < last_substeps]
            st["file"] = files[int(rng.integers(0, len(files)))]
        elif kind.startswith("force_"):
            species = int(rng.integers(0, ns))
            window = "whole" if species == 2 else ("whole", "narrow", "wide")[int(rng.integers(0, 3))]      # (the third species may have one particle)
            epoch = int(rng.integers(0, 1000))
            envelope, active = None, True
            if rng.random() < 0.5:
                s = epoch + t
                if rng.random() < 0.7:
                    envelope = dict(start=max(0, s - int(rng.integers(0, 3))), stop=s + int(rng.integers(1, 4)))
                else:
                    active = False
                    start = s + int(rng.integers(1, 4)) if s < 4 or rng.random() < 0.5 else s - int(rng.integers(2, 5))
                    envelope = dict(start=start, stop=start + 1 if start < s else start + 3)      # (over before s, or not begun)
                envelope["values"] = _table(rng, 0.2, 1.2, int(rng.integers(3, 6))) if rng.random() < 0.6 else None
            st.update(what=kind[len("force_"):], window=window, active=active, t=t, kw=_force_kw(rng, kind[len("force_"):], species, window, epoch, envelope))
        elif kind.startswith("gas_"):
            what = kind[len("gas_"):]
            K, side = _gas_side(rng)
            low = side.endswith("_lo")             # (few candidates: the first species, and no small window)
            species = 0 if low else int(rng.integers(0, 2))
            window = ("whole", "wide")[int(rng.integers(0, 2))] if low else ("whole", "narrow", "wide")[int(rng.integers(0, 3))]
            st.update(what=what, side=side, window=window, kw=_gas_kw(rng, what, species, window, sc["dt"], K, BACKGROUND, taper_min=0.9 if low else 0.6))
        elif kind in ("load_profile", "load_radial"):
            species = int(rng.integers(0, 2))
            n = sc["counts"][species]
            first = int(rng.integers(1, n - 1))
            lo, hi = _sub_box(rng)
            st.update(species=species, first=first, count=int(rng.integers(1, n - first)), what=("position", "velocity", "both")[int(rng.integers(0, 3))],
                      seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), lo=lo, hi=hi, drift=[float(x) for x in rng.normal(0, 0.01, 3)],
                      vth=float(rng.uniform(0.01, 0.05)), lattice=bool(rng.random() < 0.5))
            if kind == "load_profile":
                axes = rng.permutation(3)[:int(rng.integers(1, 4))]
                st["density"] = [_table(rng, 0.1, 1.0) if a in axes else None for a in range(3)]
                st["thermal"] = [_table(rng, 0.5, 1.5) if rng.random() < 0.5 else None for a in range(3)] if rng.random() < 0.6 else None
                st["shear"] = dict(axis=int(rng.integers(0, 3)), component=int(rng.integers(0, 3)), values=[float(x) for x in rng.normal(0, 0.01, int(rng.integers(2, 8)))]) \
                    if rng.random() < 0.6 else None
            else:
                st["radial"] = _radial(rng)
        else:
            raise AssertionError(kind)
        if kind in POSITION_KINDS2 and st["what"] != "velocity":
            st["precalc"] = sc["solver"] != "none" or bool(rng.random() < 0.5)
        off = (seed * 4 + STATE_KINDS2.index(kind) * 5 + seen[kind] * READS2) % len(READ_KINDS2)
        seen[kind] += 1
        st["reads"] = [_read2(rng, READ_KINDS2[(off + i) % len(READ_KINDS2)], sc, saved, index) for i in range(READS2)]
        if sc["registered"]:
            st["reads"] += [_read2(rng, k, sc, saved, index) for k in STATS_KINDS2]
        steps.append(st)
    return steps


def _step1(rng, sc, kind):
    """a step of a generation-1 kind other than substeps and loadCheckpoint, drawn as sequence() draws it"""
    ns = len(sc["counts"])
    st = dict(kind=kind)
    species = int(rng.integers(0, ns))
    if kind == "set":
        st.update(species=species, what=("position", "velocity", "both")[int(rng.integers(0, 3))])
    elif kind in ("setRange", "load"):
        species = int(rng.integers(0, 2))
        n = sc["counts"][species]
        first = int(rng.integers(1, n - 1))
        st.update(species=species, first=first, count=int(rng.integers(1, n - first)), what=("position", "velocity", "both")[int(rng.integers(0, 3))])
        if kind == "load":
            lo, hi = _sub_box(rng)
            st.update(seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), lo=lo, hi=hi, drift=[float(x) for x in rng.normal(0, 0.01, 3)],
                      vth=float(rng.uniform(0.01, 0.05)), lattice=bool(rng.random() < 0.5), paired=bool(rng.random() < 0.4))
    elif kind.startswith("collide_"):
        what = kind[len("collide_"):]
        kw = dict(species=0, seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), epoch=int(rng.integers(0, 1000)), **BACKGROUND)
        if what == "relax":
            kw["nu_tau"] = float(rng.uniform(0.1, 0.5))
        else:
            kw["nu_tau"], st["side"] = _threshold_rate(rng)
            if what == "elastic":
                kw["mass_ratio"] = float(rng.choice([0.5, 2.0]))
        st.update(what=what, kw=kw)
    elif kind in ("pair_like", "pair_unlike"):
        a = int(rng.integers(0, 2))
        st.update(a=a, b=None if kind == "pair_like" else 1 - a,
                  kw=dict(log_lambda=LOG_LAMBDA, tau=sc["tau_like"][a] if kind == "pair_like" else sc["tau_unlike"],
                          seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), epoch=int(rng.integers(0, 1000))))
    elif kind != "sort":
        raise AssertionError(kind)
    return st


def substeps_of(steps):
    return sum(st.get("k", 0) for st in steps)


def epoch_control():
    """(seed, step index) of the control of the one-shot force's time: the first active force without an envelope on a handle
    with sub-steps behind it (a twin given epoch + t + 1 must differ)"""
    for seed in SEEDS2:
        for i, st in enumerate(sequence2(seed)):
            if st["kind"].startswith("force_") and "envelope" not in st["kw"] and st["t"] > 0:
                return seed, i
    raise AssertionError("no force step for the control")


# ---- the references of the suite on a state: per species dict(frac=, vel=, cell=, ids=) — the stored box fractions and
# velocities in the caller's order and the deposit's cells.  On the CPU the state is initial_state(); the GPU tests read it
# from a handle just before the call they check.
TALLY_KEYS = ("sigma", "g_lo", "g_hi", "tau", "seed", "stream", "epoch")


def cell_volume(sc):
    """as the library forms it"""
    return (sc["L"][0] / sc["shape"][0]) * (sc["L"][1] / sc["shape"][1]) * (sc["L"][2] / sc["shape"][2])


def initial_state(sc):
    out = []
    shape = np.array(sc["shape"])
    for sp, n in enumerate(sc["counts"]):
        pos, vel = particles(sc["seed"], 1000 + sp, n)
        frac = pos / np.array(sc["L"])
        ijk = np.minimum((frac * shape).astype(np.int64), shape - 1)
        out.append(dict(frac=frac, vel=vel, cell=ijk[:, 0] + shape[0] * (ijk[:, 1] + shape[1] * ijk[:, 2]), ids=np.arange(n)))
    return out


def gas_want(sc, state, what, kw):
    """gas_reference's counts of a windowed background request on a state"""
    req = gasref.request(sc["L"], dict(exchange=gasref.EXCHANGE, elastic=gasref.ELASTIC)[what], **{k: v for k, v in kw.items() if k != "species"})
    s = state[kw["species"]]
    return gasref.counts(gasref.apply(req, s["ids"], s["frac"], s["vel"]))


def fusion_want(sc, state, a, b, kw):
    """fusion_reference's tally of species a with b (None: with itself), and its request"""
    import fusion_reference as fref
    req = fref.request(*[kw[k] for k in TALLY_KEYS[:4]], sc["macro_weight"], cell_volume(sc), seed=kw["seed"], stream=kw["stream"], epoch=kw["epoch"], like=b is None)
    args = [state[a]["cell"], state[a]["ids"], state[a]["vel"]] + ([] if b is None else [state[b]["cell"], state[b]["ids"], state[b]["vel"]])
    return req, fref.apply(req, int(np.prod(sc["shape"])), *args)


def spectrum_want(sc, state, a, b, kw):
    """fusion_spectrum_reference's spectrum of the same"""
    import fusion_spectrum_reference as sref
    req, tally = fusion_want(sc, state, a, b, kw)
    axis = sref.request(sc["masses"][a], sc["masses"][a if b is None else b], **{k: v for k, v in kw.items() if k not in TALLY_KEYS})
    args = [state[a]["cell"], state[a]["ids"], state[a]["vel"]] + ([] if b is None else [state[b]["cell"], state[b]["ids"], state[b]["vel"]])
    return sref.apply(req, axis, int(np.prod(sc["shape"])), *args, tally=tally)


def force_inside(sc, state, kw):
    """the particles of the request's species inside its window"""
    lo = np.array(kw.get("lo", (0.0, 0.0, 0.0))) / np.array(sc["L"])
    hi = np.array(kw.get("hi", sc["L"])) / np.array(sc["L"])
    p = state[kw["species"]]["frac"]
    return int(np.all((lo <= p) & (p < hi), axis=1).sum())


# ---- the named sequence of the resets: fusionGrid(reset=True) and fusionSpectrumRead(reset=True) zero "behind the copy"
def resets():
    """A scene with operators registered (the tally and the spectrum every sub-step, so that no piece is empty); the steps
    marked `reset` are followed, after their reads, by both reads with reset: directly after a substeps, after a one-shot
    operation, and after a loadCheckpoint."""
    sc = scene(RESET_SEED)
    assert sc["registered"]
    sc.update(solver="poisson_fft", precision="fp32", sort_interval=2, staged=False, dt=5e-12, name="resets", generation=2)
    sc["spec"] = dict(sc["spec"], solver="poisson_fft", dt=5e-12)
    sc["recorders"]["modes"]["fields"] = ["ex", "ey", "ez", "phi", "rho"]
    rng = np.random.default_rng([0x9E9D, RESET_SEED])
    _registered2(sc, rng, every=[2, 1, 1])
    relax = dict(species=0, seed=78, stream=3, epoch=9, nu_tau=0.3, **BACKGROUND)
    plain_reads = ("moments", "fusionYield", "count", "fusionSpectrum")
    plan = [
        (dict(kind="substeps", k=3, reset=True), plain_reads),
        (dict(kind="substeps", k=2), ("getParticles", "energy", "select", "getCells")),
        (dict(kind="collide_relax", what="relax", kw=relax, reset=True), plain_reads),
        (dict(kind="substeps", k=2), ("saveCheckpoint", "moments", "count", "fusionYield")),
        (dict(kind="substeps", k=3), ("histogram_lds", "series", "modes", "readField")),
        (dict(kind="loadCheckpoint", file=0, reset=True), plain_reads),
        (dict(kind="substeps", k=2), ("moments", "fusionSpectrum", "energy", "getRange")),
    ]
    steps, saved = [], []
    for index, (st, kinds) in enumerate(plan):
        st = dict(dict(tag=index + 1, precalc=False), **st)
        st["reads"] = [_read2(rng, k, sc, saved, index) for k in kinds + STATS_KINDS2]
        steps.append(st)
    return sc, steps


RESET_SEED = 301
NAMED2 = {"resets": resets}


# ---- relation 3, generation 2: the six GROUP_CASES with a force and a windowed background operator registered beside the
# background operator, one-shot forces and windowed collisions of both kinds, a full reload from a density profile and one
# from a radial body, and the refusal of both fusion calls once
GROUP_STATE_KINDS2 = ("step", "force_field", "force_accel", "gas_exchange", "gas_elastic", "reload_profile", "reload_radial", "fusion_refused")
GROUP_KICK_MAX = 0.02          # the thermal speed of GROUP_BACKGROUND: no application may change a velocity by more


def group_lengths(index):
    return tuple(1e-3 * s for s in GROUP_CASES[index]["shape"])


def group_dt(index):
    case = GROUP_CASES[index]
    return em_dt(case["shape"], group_lengths(index)) if case["em"] else 5e-12


def group_case2(index):
    case = group_case(index)
    rng = np.random.default_rng([0x64092, index, 1])
    lengths, dt = group_lengths(index), group_dt(index)
    e0 = int(rng.integers(0, 1000))
    case["force_on"] = _force_kw(rng, ("field", "accel")[index % 2], 0, ("wide", "whole", "narrow")[index % 3], e0,
                                 envelope=dict(start=e0 + 2, stop=e0 + 9, values=[0.3, 1.0, 0.5]), scale=0.1, lengths=lengths)
    lo, hi = gas_compact_range()
    every = 1 + (index + 1) % 3
    what = ("exchange", "elastic")[index % 2]
    case["gas_every"] = dict(every=every, kind=what, kw=_gas_kw(rng, what, 0, ("whole", "narrow", "wide")[index % 3], every * dt, math.sqrt(lo * hi), GROUP_BACKGROUND,
                                                                g=GROUP_GAS_G, lengths=lengths))
    return case


def group_sequence2(index):
    """17 operations on a group and on one handle: frames, and between them each kind of GROUP_STATE_KINDS2 once; two reads after each"""
    rng = np.random.default_rng([0x64092, index])
    n = 3000
    lengths, dt = group_lengths(index), group_dt(index)
    others = [k for k in GROUP_STATE_KINDS2 if k != "step"]
    cycle = [others[i] for i in rng.permutation(len(others))]
    steps, at = [], 0
    for i in range(17):
        if i % 2 == 0 or at >= len(cycle):
            st = dict(kind="step")
        else:
            kind = cycle[at]
            at += 1
            st = dict(kind=kind)
            if kind.startswith("force_"):
                what = kind[len("force_"):]
                window = ("whole", "narrow", "wide")[int(rng.integers(0, 3))]
                st.update(what=what, window=window, kw=_force_kw(rng, what, 0, window, int(rng.integers(0, 1000)), scale=0.2, lengths=lengths))
            elif kind.startswith("gas_"):
                what = kind[len("gas_"):]
                K, side = _gas_side(rng)
                low = side.endswith("_lo")
                window = "whole" if low else ("whole", "narrow", "wide")[int(rng.integers(0, 3))]
                st.update(what=what, side=side, window=window, kw=_gas_kw(rng, what, 0, window, dt, K, GROUP_BACKGROUND, g=GROUP_GAS_G, lengths=lengths,
                                                                          taper_min=0.9 if low else 0.6))
            elif kind.startswith("reload_"):
                pop = dict(first=0, count=n, seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), drift=(0.0, 0.01, 0.0), vth=0.02,
                           lattice=bool(rng.random() < 0.5))
                if kind == "reload_profile":
                    pop.update(density=[_table(rng, 0.2, 1.0), None, _table(rng, 0.2, 1.0)], thermal=[None, _table(rng, 0.5, 1.2), None],
                               shear=dict(axis=2, component=0, values=[float(x) for x in rng.normal(0, 0.005, 5)]))
                else:
                    pop["radial"] = _radial(rng, lengths, flow=0.005)
                st["population"] = pop
        reads = []
        for j in range(2):
            kind = GROUP_READ_KINDS[(index + 2 * i + j) % len(GROUP_READ_KINDS)]
            r = dict(kind=kind)
            if kind in ("count", "select"):
                lo = float(rng.uniform(0.0, 0.6))
                r.update(where={"xyz"[int(rng.integers(0, 3))]: (lo, lo + 0.3), "vz": (None, float(rng.uniform(-0.01, 0.03)))},
                         every=(3, int(rng.integers(0, 3))) if rng.random() < 0.5 else None)
            elif kind == "histogram":
                r.update(axes=("z", "vz"), bins=(24, 32), ranges=((0.0, 1.0), (-0.3, 0.3)))
            elif kind == "moments":
                r.update(which="order1")
            reads.append(r)
        st["reads"] = reads
        steps.append(st)
    return steps


def kick_bound(kw, dt, charge=QE, mass=ME):
    """the largest |dv| (units of c) one application of a force request can give a component: kq sum_k max|amp_k| times the
    largest taper product and envelope value"""
    kq = dt / C if kw["kind"] == "accel" else abs(charge) * dt / (mass * C)
    amp = sum(max(abs(x) for x in w["amp"]) for w in kw["waves"])
    taper = float(np.prod([1.0 if t is None else max(abs(x) for x in t) for t in kw["taper"]]))
    env = kw.get("envelope") or {}
    return kq * amp * taper * (max(abs(x) for x in env["values"]) if env.get("values") else 1.0)


# ---- the second resume: all six families registered, the periods dividing RESUME_T, a force envelope across the cut
RESUME2_EVERY = dict(collide=RESUME_EVERY[0], pair=RESUME_EVERY[1], gas=3, fusion=2, spectrum=1)
RESUME2_ENVELOPE = (RESUME_T - 2, RESUME_T + 2)


def resume_scene2(solver, precision):
    sc = resume_scene(solver, precision)
    sc["generation"] = 2
    _registered2(sc, np.random.default_rng([0x5CE92, 1000]), every=[RESUME2_EVERY["gas"], RESUME2_EVERY["fusion"], RESUME2_EVERY["spectrum"]], envelope=RESUME2_ENVELOPE)
    return sc


# ================================================================================================ generation 3
# The sinks and the sources (remove, removeEvery, renumber, inject, injectEvery, reserve, population) under the random call
# sequences (tests/test_gpu_sequences3.py): the only operators that change a species' count, its id span and its capacity.
# Generations 1 and 2 above stay what they are (pinned by digests).  The scene of a generation-3 seed is the generation-2
# scene of that seed ON A BOX OF UNIT EDGES: select() then returns the stored values exactly (metres = box fractions), so its
# rows feed the numpy references and an upload without rounding.  What follows from the edge lengths is scaled with them:
# the electrostatic dt is 5e-9 (the fast fifth of particles() still crosses more than a cell per sub-step), the full-EM dt is
# em_dt's; the number density is 1e9 m^-3, so that omega_p dt is what it was on the millimetre box (0.009: at 1e15 m^-3 it
# would be 9, and the leapfrog would run away to infinities within a sequence); macro_weight, dv and the pair times are
# recomputed from it; the given field of a `none` scene and the amplitudes of the forces are scaled by dt_old / dt (the kick
# per sub-step stays), the density of a windowed background by tau_old / tau (the candidates stay), the fusion tables by
# (tau W / dv)_old / (tau W / dv) (the yields stay).
#
# A removal's count depends on the pushes, so the CPU cannot know n after the first remove: every parameter that depends on
# n is carried as a fraction or a rule and resolved by the replay against population() just before the call (resolve_range,
# resolve_tracers, resolve_inject).  What the CPU does know is WHICH species are thinned: a step carries `thinned` (the
# species thinned before it) and `thinned_after`; a caller-order operation or read on a thinned species carries
# refused=True — the replay expects the refusal by name with nothing changed, and holds the model's `thinned` against
# population() at every step.
L3 = (1.0, 1.0, 1.0)
DT3 = 5e-9
DENSITY3 = 1e9
REMOVE_KINDS3 = ("remove_window", "remove_outside", "remove_thinned_by_id")          # the removals that must take somebody
INJECT_KINDS3 = ("inject_volume", "inject_flux", "inject_pair")
NEW_KINDS3 = REMOVE_KINDS3 + ("remove_nothing",) + INJECT_KINDS3 + ("inject_refused", "reserve", "renumber")
STATE_KINDS3 = STATE_KINDS2 + NEW_KINDS3
STATS_KINDS3 = STATS_KINDS2 + ("removeStats", "injectStats")
CALLER_ORDER_KINDS3 = ("set", "setRange", "load", "load_profile", "load_radial")     # refused on a thinned species
CALLER_ORDER_READS3 = ("getParticles", "getRange", "getCells")                       # refused on a thinned species; saveCheckpoint: on any
UNBINNING_KINDS3 = REMOVE_KINDS3 + INJECT_KINDS3 + ("reserve",)                      # leave a species as an upload leaves one
ID_PRIMES3 = (2, 3, 5, 7)       # the moduli of remove_thinned_by_id: none is used twice on a species (classes of different primes always meet)
READS3 = 4

# chosen by tests/test_sequence_model.py's conditions (coverage, no vacuous removal on the initial particles); none is
# skipped at run time.  The replay asserts 0 < removed < n for every removal of REMOVE_KINDS3 on the GPU: a seed that fails
# that there is to be replaced by another one, not skipped, and the replacement noted here.
SEEDS3 = [8, 24, 82, 89, 176, 648, 1986, 2568, 3060, 3317, 3975, 4778]


def particles3(seed, tag, n):
    return particles(seed, tag, n, lengths=L3)


def given_field3(seed):
    return given_field(seed) * (5e-12 / DT3)


def _unit_box(kw):
    """lo, hi of a request drawn on the millimetre box, in the unit box"""
    for key in ("lo", "hi"):
        if key in kw:
            kw[key] = [float(kw[key][a] / L[a]) for a in range(3)]
    return kw


def _to_unit(sc):
    """a generation-1/2 scene on the box of unit edges (see the head of this generation)"""
    old = dict(dt=sc["dt"], W=sc["macro_weight"], dv=sc["dv"])
    dt = em_dt(SHAPE, L3) if sc["solver"] == "yee" else DT3
    W = DENSITY3 * float(np.prod(L3)) / N0
    dv = float(np.prod(L3)) / float(np.prod(SHAPE))
    sc.update(generation=3, L=L3, dt=dt, macro_weight=W, dv=dv, kick_scale=old["dt"] / dt, sigma_scale=(old["dt"] * old["W"] / old["dv"]) / (dt * W / dv))
    sc["spec"] = dict(sc["spec"], radius=L3[0], length_y=L3[1], height=L3[2], dt=dt, macro_weight=W)
    sc["tau_like"] = [pair_tau(W, dv, sc["masses"][a], sc["charges"][a], sc["masses"][a], sc["charges"][a]) for a in range(2)]
    sc["tau_unlike"] = pair_tau(W, dv, ME, QE, MP, -QE, n_l=1)
    if sc["registered"]:
        pe = sc["pair_every"]
        pe["kw"]["tau"] = sc["tau_like"][0] if pe["b"] is None else sc["tau_unlike"]
        if "recorders" in sc:
            sc["recorders"]["series"]["points"] = sc["recorders"]["series"]["points"] / np.array(L)
        for kw in sc.get("force_on", []):
            _unit_box(kw)
            for w in kw["waves"]:
                w["amp"] = [x * sc["kick_scale"] for x in w["amp"]]
        if "gas_every" in sc:
            ge = sc["gas_every"]
            _unit_box(ge["kw"])
            ge["kw"]["density"] *= ge["kw"]["tau"] / (ge["every"] * dt)
            ge["kw"]["tau"] = ge["every"] * dt
            for key in ("fusion_every", "spectrum_every"):
                sc[key]["kw"]["tau"] = sc[key]["every"] * dt
                sc[key]["kw"]["sigma"] = sc[key]["kw"]["sigma"] * sc["sigma_scale"]
    return sc


def _brick(rng, widths, axes=None):
    """{axis: (lo, lo + w)} on 1 .. 3 spatial axes (or the given number), w drawn from `widths`"""
    out = {}
    for a in rng.permutation(3)[:int(rng.integers(1, 4)) if axes is None else axes]:
        w = float(rng.uniform(*widths))
        lo = float(rng.uniform(0.0, 1.0 - w))
        out["xyz"[int(a)]] = (lo, lo + w)
    return out


def _source3(rng, kind, count):
    """the keywords of a source but its species: sequence numbers from `first`, a sub-box of the unit box; a flux source's
    plane lies on a face of the box on four draws of ten"""
    lo = [float(x) for x in rng.uniform(0, 0.4, 3)]
    kw = dict(kind=kind, count=int(count), first=int(rng.integers(0, 1 << 20)), seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)),
              lo=lo, hi=[float(lo[a] + rng.uniform(0.3, 0.6)) for a in range(3)], lattice=bool(rng.random() < 0.5))
    if kind == "volume":
        kw.update(drift=[float(x) for x in rng.normal(0, 0.01, 3)], vth=float(rng.uniform(0.01, 0.05)), paired=bool(rng.random() < 0.5))
    else:
        axis = int(rng.integers(0, 3))
        drift = [float(x) for x in rng.normal(0, 0.01, 3)]
        drift[axis] = 0.0
        face = rng.random() < 0.4
        kw.update(axis=axis, side=int(rng.choice([-1, 1])), plane=float(rng.choice([0.0, 1.0])) if face else float(rng.uniform(0.1, 0.9)), drift=drift,
                  vth=[float(x) for x in rng.uniform(0.01, 0.05, 3)])
    return kw


def _registered3(sc, rng):
    """the sinks and the sources of a scene with registered operators, beside generation 2's set: a spatial sink on species
    0 every 2nd and an every=(3, r) sink on species 1 every 3rd sub-step; a volume source into species 0 and 1 on one seed,
    stream and sequence every sub-step (a neutral pair) and a flux source into species 0 every 2nd"""
    sc["remove_every"] = [dict(every=2, species=0, where=_brick(rng, (0.15, 0.3), axes=1), every_id=None, outside=False),
                          dict(every=3, species=1, where=None, every_id=(3, int(rng.integers(0, 3))), outside=False)]
    pair = dict(_source3(rng, "volume", rng.integers(20, 61)), epoch=int(rng.integers(0, 50)))
    flux = dict(_source3(rng, "flux", rng.integers(20, 61)), epoch=int(rng.integers(0, 50)))
    sc["inject_every"] = [dict(every=1, species=0, kw=pair), dict(every=1, species=1, kw=dict(pair)), dict(every=2, species=0, kw=flux)]


def reserved3(sc, total):
    """the capacities a scene with registered sources reserves up front for `total` sub-steps: count + sum of count_source x
    ceil(total / every) — no application of the hook can fail"""
    out = list(sc["counts"])
    for op in sc.get("inject_every", []):
        out[op["species"]] += op["kw"]["count"] * -(-total // op["every"])
    return out


def scene3(seed):
    sc = _to_unit(scene2(seed))
    if sc["registered"]:
        _registered3(sc, np.random.default_rng([0x5CE93, seed]))
    return sc


def _fusion_kw3(rng, sc):
    kw = _fusion_kw(rng, sc["dt"])
    kw["sigma"] = kw["sigma"] * sc["sigma_scale"]
    return kw


def _read3(rng, kind, sc, saved, index, thinned):
    """a read of generation 3: what depends on n is a fraction (getRange: first_frac, count_frac; series: tracer_fracs of the
    id span, and the replay adds a dead id once one exists); refused=True on a caller-order read of a thinned species and on
    a saveCheckpoint while any species is thinned (that save makes no file)"""
    if kind in STATS_KINDS3:
        return dict(kind=kind, species=0)
    if kind in ("fusionYield", "fusionSpectrum"):
        like = bool(rng.random() < 0.5)
        a = int(rng.integers(0, 2))
        b = None if like else 1 - a
        r = dict(kind=kind, species=a, a=a, b=b, kw=_fusion_kw3(rng, sc))
        if kind == "fusionSpectrum":
            r["form"] = ("product", "los", "cm")[int(rng.integers(0, 3))]
            r["kw"].update(spectrum_axis(sc["masses"], a, b, r["form"]))
        return r
    if kind == "saveCheckpoint":
        r = dict(kind=kind, species=int(rng.integers(0, len(sc["counts"]))), refused=bool(thinned))
        if not thinned:
            r["file"] = len(saved)
            saved.append(index)
        return r
    r = _read(rng, kind, sc, [], index)
    if kind == "getRange":
        n = sc["counts"][r["species"]]
        r.update(first_frac=r.pop("first") / n, count_frac=float(rng.random()))
        del r["count"]
    elif kind == "series":
        n = sc["counts"][r["species"]]
        r["points"] = r["points"] / np.array(L)
        r["tracer_fracs"] = [x / n for x in r.pop("tracers")]
    if kind in CALLER_ORDER_READS3:
        r["refused"] = r["species"] in thinned
    return r


def resolve_range(first_frac, count_frac, n, stride=1):
    """(first, count) of a strict sub-range of n particles: 0 < first, first + stride (count - 1) < n - 1 where n allows it"""
    first = min(max(1, int(first_frac * n)), max(n - 2, 0))
    most = max(1, (n - 1 - first + stride - 1) // stride)
    return first, max(1, min(most, 1 + int(count_frac * most)))


def resolve_tracers(fracs, id_span, ids):
    """the tracer ids of a series: the fractions of the id span, and one dead id (the smallest) once one exists"""
    tr = sorted({min(int(f * id_span), id_span - 1) for f in fracs})
    dead = np.setdiff1d(np.arange(id_span, dtype=np.int64), np.asarray(ids, dtype=np.int64))
    if len(dead) and int(dead[0]) not in tr:
        tr.append(int(dead[0]))
    return tr


def resolve_inject(st, n, capacity):
    """(capacity to reserve first or None, count): with reserve_first the species grows by the drawn count; otherwise the
    source injects what fits of it, and reserves only if nothing does"""
    room = capacity - n
    if st["reserve_first"] or room == 0:
        return capacity + st["count"], st["count"]
    return None, min(st["count"], room)


def _step3(rng, sc, kind, used_primes):
    """a step of a new kind"""
    st = dict(kind=kind)
    species = int(rng.integers(0, 2))
    if kind == "remove_window":
        where = {}
        while not 1 <= len(where) <= 3:
            where = _read(rng, "count", sc, [], 0)["where"]
        st.update(species=species, where=where, every=None, outside=False)
    elif kind == "remove_outside":
        st.update(species=species, where=_brick(rng, (0.62, 0.94)), every=None, outside=True)
    elif kind == "remove_thinned_by_id":
        if all(p in used_primes[species] for p in ID_PRIMES3):      # (every modulus used on this species: the other one)
            species = 1 - species
        free = [p for p in ID_PRIMES3 if p not in used_primes[species]]
        if not free:
            return _step3(rng, sc, "remove_window", used_primes)
        mod = int(free[int(rng.integers(0, len(free)))])
        used_primes[species].add(mod)
        st.update(species=species, where=_brick(rng, (0.5, 0.8), axes=1) if rng.random() < 0.5 else None, every=(mod, int(rng.integers(0, mod))), outside=False)
    elif kind == "remove_nothing":
        where = ({"vx": (10.0, None)}, {"v2": (None, 0.0)}, {"x": (0.25, 0.5), "vz": (20.0, 30.0)})[int(rng.integers(0, 3))]
        st.update(species=species, where=where, every=None, outside=False)
    elif kind in ("inject_volume", "inject_flux"):
        st.update(species=species, kw=_source3(rng, kind[len("inject_"):], rng.integers(50, 401)), reserve_first=bool(sc["registered"] or rng.random() < 0.5))
        st["count"] = st["kw"].pop("count")
    elif kind == "inject_pair":
        st.update(species=None, kw=dict(_source3(rng, ("volume", "flux")[int(rng.integers(0, 2))], rng.integers(50, 301)), paired=False), reserve_first=True)
        st["count"] = st["kw"].pop("count")
        if st["kw"]["kind"] == "flux":
            del st["kw"]["paired"]
    elif kind == "inject_refused":
        st.update(species=species, kw=dict(kind="volume", seed=int(rng.integers(1, 1 << 40)), vth=0.01))
    elif kind == "reserve":
        st.update(species=species, extra=int(rng.choice([1, 7, 333, 1024, 1500])))
    elif kind == "renumber":
        st.update(species=None)
    else:
        raise AssertionError(kind)
    return st


def _step2_unit(rng, sc, kind, t):
    """what a force_*, gas_*, load_profile or load_radial step of a scene on the unit box carries, drawn as sequence3() draws
    it (t: the sub-steps behind the step)"""
    ns = len(sc["counts"])
    st = {}
    if kind.startswith("force_"):
        species = int(rng.integers(0, ns))
        window = "whole" if species == 2 else ("whole", "narrow", "wide")[int(rng.integers(0, 3))]
        epoch = int(rng.integers(0, 1000))
        envelope, active = None, True
        if rng.random() < 0.4:
            s = epoch + t
            if rng.random() < 0.7:
                envelope = dict(start=max(0, s - int(rng.integers(0, 3))), stop=s + int(rng.integers(1, 4)))
            else:
                active = False
                start = s + int(rng.integers(1, 4)) if s < 4 or rng.random() < 0.5 else s - int(rng.integers(2, 5))
                envelope = dict(start=start, stop=start + 1 if start < s else start + 3)
            envelope["values"] = _table(rng, 0.2, 1.2, int(rng.integers(3, 6))) if rng.random() < 0.6 else None
        st.update(what=kind[len("force_"):], window=window, active=active, t=t,
                  kw=_force_kw(rng, kind[len("force_"):], species, window, epoch, envelope, scale=sc["kick_scale"], lengths=L3))
    if kind.startswith("gas_"):
        what = kind[len("gas_"):]
        K, side = _gas_side(rng)
        low = side.endswith("_lo")
        species = 0 if low else int(rng.integers(0, 2))
        window = ("whole", "wide")[int(rng.integers(0, 2))] if low else ("whole", "narrow", "wide")[int(rng.integers(0, 3))]
        st.update(what=what, side=side, window=window, kw=_gas_kw(rng, what, species, window, sc["dt"], K, BACKGROUND, lengths=L3, taper_min=0.9 if low else 0.6))
    if kind in ("load_profile", "load_radial"):
        species = int(rng.integers(0, 2))
        lo = [float(x) for x in rng.uniform(0, 0.4, 3)]
        st.update(species=species, first_frac=float(rng.uniform(0.001, 0.9)), count_frac=float(rng.random()), what=("position", "velocity", "both")[int(rng.integers(0, 3))],
                  seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), lo=lo, hi=[float(lo[a] + rng.uniform(0.3, 0.6)) for a in range(3)],
                  drift=[float(x) for x in rng.normal(0, 0.01, 3)], vth=float(rng.uniform(0.01, 0.05)), lattice=bool(rng.random() < 0.5))
        if kind == "load_profile":
            axes = rng.permutation(3)[:int(rng.integers(1, 4))]
            st["density"] = [_table(rng, 0.1, 1.0) if a in axes else None for a in range(3)]
            st["thermal"] = [_table(rng, 0.5, 1.5) if rng.random() < 0.5 else None for a in range(3)] if rng.random() < 0.6 else None
            st["shear"] = dict(axis=int(rng.integers(0, 3)), component=int(rng.integers(0, 3)), values=[float(x) for x in rng.normal(0, 0.01, int(rng.integers(2, 8)))]) \
                if rng.random() < 0.6 else None
        else:
            st["radial"] = _radial(rng, lengths=L3)
    return st


def sequence3(seed, nsteps=None):
    """the steps of a generation-3 seed: 14 to 18 state-changing operations of STATE_KINDS3, the first a substeps, each with
    READS3 reading calls of READ_KINDS2 (six, and every read of STATS_KINDS3, on a scene with registered operators).  The
    forced opening: after one to three steps comes the seed's first removal (of REMOVE_KINDS3), then a substeps with
    k >= sort_interval + 1 (a re-binning push on a thinned species), then one of each of collide_*, gas_*, pair_*, force_* in
    a drawn order, the fusionYield and fusionSpectrum reads among theirs — no renumber and no loadCheckpoint before the block
    ends.  The other steps take new and old kinds in turn from two shuffled cycles.  A step carries `thinned` /
    `thinned_after` (see the head of this generation) and, where the library must refuse it, refused=True."""
    sc = scene3(seed)
    rng = np.random.default_rng([0x0B53, seed])
    ns = len(sc["counts"])
    nsteps = int(rng.integers(14, 19)) if nsteps is None else nsteps
    olds = [k for k in STATE_KINDS2 if k != "substeps"]
    news = list(NEW_KINDS3)
    old_cycle = [olds[i] for i in rng.permutation(len(olds))]
    new_cycle = [news[i] for i in rng.permutation(len(news))]
    first_removal = REMOVE_KINDS3[int(rng.integers(0, 3))]
    forced = [("collide_exchange", "collide_elastic", "collide_relax")[int(rng.integers(0, 3))], ("gas_exchange", "gas_elastic")[int(rng.integers(0, 2))],
              ("pair_like", "pair_unlike")[int(rng.integers(0, 2))], ("force_field", "force_accel")[int(rng.integers(0, 2))]]
    forced = [forced[i] for i in rng.permutation(4)]
    block_at = int(rng.integers(1, 4))
    ks = [k for k in (1, 2, 3, 5) if k >= sc["sort_interval"] + 1]
    block = [first_removal, ("substeps", int(ks[int(rng.integers(0, len(ks)))]))]
    for k in forced:
        if rng.random() < 0.3:
            block.append("substeps")
        block.append(k)
    reads_per_step = 6 if sc["registered"] else READS3
    at_old = at_new = t = 0
    turn = int(rng.integers(0, 2))
    seen = {k: 0 for k in STATE_KINDS3}
    saved = []
    last_substeps = -1
    thinned = set()
    used_primes = [set(), set()]
    steps = []
    in_block = None      # the index into block while it runs
    for index in range(nsteps):
        k_forced, from_block = None, False
        if index == block_at:
            in_block = 0
        if in_block is not None and in_block < len(block):
            kind = block[in_block]
            in_block += 1
            from_block = True
            if isinstance(kind, tuple):
                kind, k_forced = kind
        elif index == 0 or (steps[-1]["kind"] != "substeps" and rng.random() < 0.5) or (steps[-1]["kind"] == "substeps" and rng.random() < 0.1):
            kind = "substeps"
        else:
            while True:
                if turn:
                    kind = new_cycle[at_new % len(new_cycle)]
                    at_new += 1
                else:
                    kind = old_cycle[at_old % len(old_cycle)]
                    at_old += 1
                before_block = in_block is None
                if before_block and kind in REMOVE_KINDS3 + ("renumber",):
                    continue          # (the block's removal is the seed's first; a renumber before it has nothing to do)
                if kind == "loadCheckpoint" and not any(s < last_substeps for s in saved):
                    continue          # (a rewind needs a file with a substeps after it)
                if kind == "loadCheckpoint" and sc["registered"] and thinned:
                    continue          # (with operators registered a rewind is drawn only before the first removal of the hook)
                break
            turn ^= 1
        st = dict(kind=kind, tag=index + 1, precalc=False)
        if kind in STATE_KINDS and kind not in ("substeps", "loadCheckpoint"):
            st = dict(_step1(rng, sc, kind), tag=index + 1, precalc=False)
            if kind in ("setRange", "load"):
                n = sc["counts"][st["species"]]
                st.update(first_frac=st.pop("first") / n, count_frac=st.pop("count") / n)
            if kind == "load":
                _unit_box(st)
        elif kind == "substeps":
            st["k"] = int(rng.choice([1, 2, 3, 5])) if k_forced is None else k_forced
            t += st["k"]
            last_substeps = index
        elif kind == "loadCheckpoint":
            files = [f for f, s in enumerate(saved) if s < last_substeps]
            st["file"] = files[int(rng.integers(0, len(files)))]
        elif kind.startswith("force_") or kind.startswith("gas_") or kind in ("load_profile", "load_radial"):
            st.update(_step2_unit(rng, sc, kind, t))
        else:
            st = dict(_step3(rng, sc, kind, used_primes), tag=index + 1, precalc=False)
            kind = st["kind"]
        st["thinned"] = sorted(thinned)
        st["refused"] = (kind in CALLER_ORDER_KINDS3 and st["species"] in thinned) or (kind == "renumber" and sc["registered"] and bool(thinned))
        if kind in POSITION_KINDS2 and st["what"] != "velocity" and not st["refused"]:
            st["precalc"] = sc["solver"] != "none" or bool(rng.random() < 0.5)
        # who is thinned after the step: the sinks of the hook thin species 0 from the 2nd and species 1 from the 3rd sub-step on
        if kind in REMOVE_KINDS3:
            thinned.add(st["species"])
        elif kind == "loadCheckpoint":
            thinned.clear()
            used_primes[0].clear(), used_primes[1].clear()
        elif kind == "renumber" and not st["refused"]:
            thinned.clear()
            used_primes[0].clear(), used_primes[1].clear()
        elif kind == "substeps" and sc["registered"]:
            thinned |= {op["species"] for op in sc["remove_every"] if t >= op["every"]}
        st["thinned_after"] = sorted(thinned)
        off = (seed * 4 + STATE_KINDS3.index(kind) * 5 + seen[kind] * reads_per_step) % len(READ_KINDS2)
        seen[kind] += 1
        kinds = [READ_KINDS2[(off + i) % len(READ_KINDS2)] for i in range(reads_per_step)]
        if from_block and kind == forced[0]:      # the block's first old kind carries both fusion reads
            for want, slot in (("fusionYield", 0), ("fusionSpectrum", 1)):
                if want not in kinds:
                    kinds[[i for i, k in enumerate(kinds) if k not in ("fusionYield", "fusionSpectrum")][slot]] = want
        st["reads"] = [_read3(rng, k, sc, saved, index, thinned) for k in kinds]
        if sc["registered"]:
            st["reads"] += [_read3(rng, k, sc, saved, index, thinned) for k in STATS_KINDS3]
        steps.append(st)
    return steps


def can_have_rebinned3(sc, steps):
    """can_have_rebinned with the new kinds: per step, True for a substeps that can leave a species reordered by a fused
    re-binning push.  A removal that takes somebody, an injection and a reserve leave the species as an upload does (the next
    sub-step bins afresh) and reset the count like a position write; a refused step changes nothing.  The sinks and sources of
    the hook do the same from inside substeps(): a sub-step on which one is due ends with its species un-binned, so the count
    is followed sub-step by sub-step — on a scene with registered operators, whose pair source is due every sub-step, no
    substeps ever qualifies, and the condition rests on the scenes without."""
    hook = [op["every"] for op in sc.get("remove_every", []) + sc.get("inject_every", [])] if sc["registered"] else []
    out, since, t = [], 0, 0
    for st in steps:
        if st["kind"] == "substeps":
            pushed = False
            for _ in range(st["k"]):
                t += 1
                since += 1
                pushed = pushed or since > sc["sort_interval"]
                if any(t % every == 0 for every in hook):
                    since, pushed = 0, False
            out.append(sc["solver"] != "yee" and sc["sort_interval"] > 0 and pushed)
        else:
            if not st["refused"] and ((st["kind"] in POSITION_KINDS2 and st["what"] != "velocity") or st["kind"] in ("loadCheckpoint", "sort") + UNBINNING_KINDS3):
                since = 0
            out.append(False)
    return out


def initial_state3(sc):
    """initial_state on the unit box"""
    out = []
    for sp, n in enumerate(sc["counts"]):
        pos, vel = particles3(sc["seed"], 1000 + sp, n)
        out.append(dict(frac=pos, vel=vel, cell=cells_of(pos, sc["shape"]), ids=np.arange(n)))
    return out


def cells_of(frac, shape):
    """the deposit's cells of stored box fractions, as initial_state computes them — in the arithmetic of the stored type,
    whose one rounding of u n decides the cell (tests/em_reference.py: cells_and_weights), n itself folding to 0
    (tests/load_reference.py: plane); in float64 no fraction below 1 reaches n and this is initial_state's number"""
    frac, shape = np.asarray(frac), np.array(shape)
    ijk = (frac * shape.astype(frac.dtype)).astype(np.int64)
    ijk = np.where(ijk >= shape, 0, ijk)
    return ijk[:, 0] + shape[0] * (ijk[:, 1] + shape[1] * ijk[:, 2])


# ---- the named sequences of generation 3: plain programs (lists of tuples) the GPU module runs line by line
TURNOVER_CASES = [("poisson_fft", "fp32"), ("yee", "fp64"), ("none", "fp64")]
TURNOVER_PIECES = (1, 2, 3, 5, 5, 3, 2, 1, 1, 2, 3, 5, 5, 2)           # forty sub-steps
TURNOVER = dict(capacity=1500, count=96, sink_every=2, sink=dict(where={"x": (0.0, 0.5)}, species=1))


def _plain3(seed, solver, precision, name, sort_interval=2, staged=False):
    sc = scene(seed)
    dt = em_dt(SHAPE, L) if solver == "yee" else 5e-12
    sc.update(solver=solver, precision=precision, dt=dt, sort_interval=sort_interval, staged=staged, registered=False, name=name, addB=None if solver == "none" else sc["addB"])
    sc["spec"] = dict(sc["spec"], solver=solver, dt=dt)
    for key in ("collide_every", "pair_every", "recorders"):
        sc.pop(key, None)
    return _to_unit(sc)


def turnover(solver, precision):
    """Source against sink over forty sub-steps in pieces of 1, 2, 3 and 5, on species 1: its capacity reserved to 1500, a
    volume source of 96 every sub-step, a sink x in [0, 0.5) every second.  The id span ends at 750 + 40 x 96 = 4590, three
    times the capacity, while n stays in the hundreds.  Under full EM the same source (seed, stream, sequence) also feeds
    species 0: a neutral pair.  The `none` case has E = 0 and no addB — no velocity ever changes — and carries the ledger."""
    sc = _plain3(310, solver, precision, "turnover")
    rng = np.random.default_rng([0x9E9D, 310])
    src = dict(_source3(rng, "volume", TURNOVER["count"]), paired=False, epoch=3)
    src["lo"][0], src["hi"][0] = 0.05, 0.55      # (nine tenths inside the sink: under full EM nobody crosses the box in forty sub-steps, and n must stay below the capacity)
    sc["turnover"] = dict(TURNOVER, source=src, pieces=TURNOVER_PIECES, feeds=[0, 1] if solver == "yee" else [1], zero_field=solver == "none")
    sc["zero_field"] = solver == "none"
    sc["capacities"] = [N0 + (40 * TURNOVER["count"] if solver == "yee" else 0), TURNOVER["capacity"]] + sc["counts"][2:]
    # reads of every kind after every piece: those by id and per particle on the turned-over species 1, the caller-order ones on
    # species 0 (never thinned); a save is refused from the second sub-step on
    reads = []
    for index in range(len(TURNOVER_PIECES)):
        row = [_read3(rng, k, sc, [], index, {1}) for k in READ_KINDS2]
        for r in row:
            if r["kind"] in ("count", "select", "histogram_lds", "histogram_global", "moments", "series"):
                r["species"] = 1
            elif r["kind"] in CALLER_ORDER_READS3:
                r.update(species=0, refused=False)
        reads.append(row)
    return sc, reads


REWINDS = dict(grow=(500, 200), substeps=(3, 4, 3, 5))


def rewinds():
    """An unregistered electrostatic fp32 scene with sort_interval = 2 and the staged binning forced; the program is
    tests/test_gpu_sequences3.py's test_rewinds (the issue's list, line by line): files of three sizes loaded into a thinned
    and into a grown handle, stale slots behind n after each."""
    sc = _plain3(311, "poisson_fft", "fp32", "rewinds", sort_interval=2, staged=True)
    rng = np.random.default_rng([0x9E9D, 311])
    sc["rewinds"] = dict(REWINDS, sources=[dict(_source3(rng, "volume", REWINDS["grow"][0]), paired=False), dict(_source3(rng, "flux", REWINDS["grow"][1]))],
                         remove=dict(where={"y": (0.1, 0.15)}), odd=dict(where={"vz": (None, 0.0)}))
    return sc


HOOK_OVERFLOW = dict(count=(40, 96), room=2 * 96 + 95)      # species 1 holds two applications of 96 and 95 more: the third is the first that does not fit


def hook_overflow():
    """A source registered on species 1 whose third application does not fit, behind a sink, a background operator and a
    source into species 0 that does: substeps(5) raises FPIC_ERR_STATE naming fpic_reserve after the third sub-step's hook
    has run up to that source."""
    sc = _plain3(312, "poisson_fft", "fp64", "hook_overflow", sort_interval=1)
    rng = np.random.default_rng([0x9E9D, 312])
    sc["hook"] = dict(collide=dict(kind="relax", species=0, kw=dict(nu_tau=0.3, seed=91, stream=1, epoch=4, **BACKGROUND)),
                      sink=dict(species=0, where={"z": (0.2, 0.5)}),      # (on the other species: a sink on species 1 would make the room)
                      sources=[dict(species=0, kw=dict(_source3(rng, "flux", HOOK_OVERFLOW["count"][0]), epoch=2)),
                               dict(species=1, kw=dict(_source3(rng, "volume", HOOK_OVERFLOW["count"][1]), paired=False, epoch=0))])
    sc["capacities"] = [N0 + 5 * HOOK_OVERFLOW["count"][0], N1 + HOOK_OVERFLOW["room"]] + sc["counts"][2:]
    return sc


NAMED3 = {"turnover": turnover, "rewinds": rewinds, "hook_overflow": hook_overflow}


# ---- the resumes of generation 3: the generation-2 families registered, and (i) a source alone — the species grows and is
# never thinned, so the cut goes through a file into a fresh handle that reserves and registers with epoch = the applications
# made so far — or (ii) a sink as well: a thinned species has no file, so both runs clear every registration at T, renumber
# and register again (epochs + T); only one of them then goes through the file.
RESUME3_SOURCE = dict(every=2, count=64)
RESUME3_SINK = dict(every=3, species=0, where={"x": (0.25, 0.5)})


def resume_scene3(solver, precision, sink):
    sc = _to_unit(resume_scene2(solver, precision))
    rng = np.random.default_rng([0x5CE93, 1000])
    src = dict(_source3(rng, "volume", RESUME3_SOURCE["count"]), paired=False, epoch=7)
    sc["inject_every"] = [dict(every=RESUME3_SOURCE["every"], species=s, kw=dict(src)) for s in (0, 1)]      # a neutral pair on one seed, stream and sequence
    sc["remove_every"] = [dict(RESUME3_SINK, every_id=None, outside=False)] if sink else []
    sc["capacities"] = reserved3(sc, RESUME_N)
    return sc


# ================================================================================================ generation 4
# The ioniser and the burner (ionize, ionizeEvery, burn, burnEvery) under the random call sequences
# (tests/test_gpu_sequences4.py): the two operators that couple the most state — a burner is a sink on two species and a
# source on up to two others in one application, an ioniser appends to two species, one of which may be its own projectile
# species.  Generations 1 to 3 above stay what they are (pinned by digests).  The scene of a generation-4 seed is the
# generation-3 scene of that seed with more species behind its own (scene4: sc["roles"] names them): p3 and p4, the products
# of the burners (an "alpha" of 4 m_p and twice the ion's charge, a "proton"), one particle each; on about half the seeds a
# separate electron species for the ioniser's secondaries (otherwise they join the projectile species 0); and short_b and
# short_i, one particle with a capacity of one each, the targets of the two refusals (a capacity only grows, so a target that is
# to be one slot short of a count the replay learns only then is a species nothing else fills).  The ion target is species 1.
#
# As in generation 3 the CPU cannot know n after the first removal.  The events of a burn or an ionisation are the
# reference's on A's own rows read just before the call (resolve at replay time, as resolve_inject does): without registered
# operators the replay reserves every target to n + events, an exact fit; with them, the capacity plus the events (the room of
# the hook stays).  WHICH species are thinned the model still knows: a burn kind with events thins its reactants, products
# and ionisation targets grow and are not thinned by growing, the *_nothing and *_refused kinds thin nobody.  On a scene with
# registered operators p3 is emptied before the run (a product species that starts empty; it is thinned from the start, and
# stays so): the second burner's reactant is then thinned whatever the first has produced, and the model need not know when
# the chain first reacts.  The second burner is due every third sub-step, behind the every-third sink on species 1: species 1
# is thinned by then whether or not the chain reacts.
IONIZE_KINDS4 = ("ionize", "ionize_nothing", "ionize_refused")
BURN_KINDS4 = ("burn_unlike", "burn_like", "burn_untracked")                        # the burns that must have events
NEW_KINDS4 = IONIZE_KINDS4 + BURN_KINDS4 + ("burn_nothing", "burn_refused")
STATE_KINDS4 = STATE_KINDS3 + NEW_KINDS4
STATS_KINDS4 = STATS_KINDS3 + ("ionizeStats", "burnStats")
BURN_G = (0.005, 3.0)              # the relative speeds of the thermal four fifths lie inside, some pairs of the fast fifth above
BURN_G_SATURATED = (0.02, 0.06)    # the seed's saturated burn: about half the pairs lie inside (it must not use a species up)
HOOK_BURN_P = (0.02, 0.05)         # a registered first burner: some tens of events per application
BURN_SIGMA = 1e-28
IONIZE_SHARE = (0.05, 0.3)         # K 2^-32 of a one-shot ionisation: the share of the projectiles that are candidates
HOOK_IONIZE_SHARE = 0.04
HOOK_GROWTH4 = 4                   # reserved4: every hook application is given this many times its events on the initial particles
HOOK_FLOOR4 = 16                   # ... and at least this many

# chosen by tests/test_sequence_model.py's conditions; none is skipped at run time.  The replay asserts 4 <= burnt, a survivor
# of every reactant and ionised > 0 on the GPU: a seed that fails that there is to be replaced, not skipped, and noted here.
# (13 replaces 103, whose burn_like on species 1 — some forty like pairs, the smallest burn of any seed — had 2 events on the GPU after two removals.)
SEEDS4 = [0, 2, 12, 13, 21, 59, 111, 129, 131, 149, 165, 187]


def burn_table(g=BURN_G):
    """sigma g constant over the table (as gas_table): the probability of a pair inside the table is tau's, times N_L"""
    return BURN_SIGMA * (g[0] / np.linspace(g[0], g[1], 64))


def burn_tau(sc, p, g=BURN_G):
    """the tau at which a pair inside the table with N_L = 1 reacts with the probability p (include/fusionpic.h:
    P = (((W N_L) tau) / dV) (sigma (g c)))"""
    return p * sc["dv"] / (sc["macro_weight"] * BURN_SIGMA * g[0] * C)


def burn_q(m3, m4, u3=0.1):
    """the q_value at which product 3 leaves a slow pair with the speed u3 (c) in the pair's frame"""
    return u3 * u3 * C * C * m3 * (m3 + m4) / (2.0 * m4)


def _burn4(rng, sc, a, b, tracked, p, nothing=None, g=BURN_G):
    """a burn request of species a with b (None: with itself) into p3 and p4 (tracked) or p3 alone"""
    roles = sc["roles"]
    m3, m4 = sc["masses"][roles["p3"]], sc["masses"][roles["p4"]]
    g = (50.0, 60.0) if nothing == "above" else g
    kw = dict(sigma=burn_table(g), g_lo=g[0], g_hi=g[1], tau=burn_tau(sc, 1e-30 if nothing == "tau" else p, g), seed=int(rng.integers(1, 1 << 40)),
              stream=int(rng.integers(0, 8)), epoch=int(rng.integers(0, 1000)))
    return dict(a=a, b=b, products=[roles["p3"], roles["p4"] if tracked else None], other_mass=0.0 if tracked else m4, q_value=burn_q(m3, m4), p=p, kw=kw)


def _ionize4(rng, sc, share, tau, window=None, nothing=False):
    """an ionisation request of species 0: the gas steps' keywords with K = share 2^32 candidates; the threshold lies at or
    below the table's start, as the library requires (on a third of the draws AT it)"""
    g = (50.0, 60.0) if nothing else GAS_G
    window = ("whole", "narrow", "wide")[int(rng.integers(0, 3))] if window is None else window
    kw = _gas_kw(rng, "exchange", 0, window, tau, share * 2.0 ** 32, BACKGROUND, g=g, lengths=L3)
    return dict(species=0, electron=sc["roles"]["electron"], ion=1, g_threshold=g[0] * (1.0 if rng.random() < 0.33 else 0.8), window=window, kw=kw)


def _species4(sc, separate, short=True):
    """the species of generation 4 behind a scene's own, one particle each; sc["roles"] names them"""
    sc["generation"] = 4
    base = len(sc["counts"])
    more = [("p3", 4 * MP, -2 * QE), ("p4", MP, -QE)] + ([("electron", ME, QE)] if separate else []) + ([("short_b", MP, -QE), ("short_i", MP, -QE)] if short else [])
    sc["roles"] = {name: base + i for i, (name, _, _) in enumerate(more)}
    if not separate:
        sc["roles"]["electron"] = 0
    for _, mass, charge in more:
        sc["counts"].append(1)
        sc["masses"].append(mass)
        sc["charges"].append(charge)
    return sc


def scene4(seed):
    sc = scene3(seed)
    rng = np.random.default_rng([0x5CE94, seed])
    _species4(sc, bool(rng.random() < 0.5))
    sc["empty"] = [sc["roles"]["p3"]] if sc["registered"] else []      # emptied before the run: thinned from the start
    if sc["registered"]:
        _registered4(sc, rng)
    return sc


def _registered4(sc, rng):
    """behind generation 3's set: one ioniser (period 1 .. 3) and two burners — the first on species 0 (with itself or with
    species 1) into p3 and p4, the second, every third sub-step, on p3 with species 1 into p4 alone: the chain"""
    roles = sc["roles"]
    every = int(rng.integers(1, 4))
    sc["ionize_every"] = [dict(_ionize4(rng, sc, HOOK_IONIZE_SHARE, every * sc["dt"]), every=every)]
    unlike = bool(rng.random() < 0.5)
    first = dict(_burn4(rng, sc, 0, 1 if unlike else None, True, float(rng.uniform(*HOOK_BURN_P))), every=int(rng.integers(1, 4)))
    m4 = sc["masses"][roles["p4"]]
    second = dict(a=roles["p3"], b=1, products=[roles["p4"], None], other_mass=sc["masses"][roles["p3"]], q_value=burn_q(m4, sc["masses"][roles["p3"]]), p=4.0, every=3,
                  kw=dict(sigma=burn_table(), g_lo=BURN_G[0], g_hi=BURN_G[1], tau=burn_tau(sc, 4.0), seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)),
                          epoch=int(rng.integers(0, 1000))))
    sc["burn_every"] = [first, second]


def ionize_want(sc, state, op, epoch=None, pops=None):
    """ionize_reference's application of a request to a state (per species dict(frac=, vel=, ids=)); pops: (n, id span) of
    the electron and the ion target (default: nobody thinned)"""
    import ionize_reference as iref
    kw = dict(op["kw"], epoch=op["kw"]["epoch"] if epoch is None else epoch)
    req = iref.request(sc["L"], g_threshold=op["g_threshold"], **{k: v for k, v in kw.items() if k != "species"})
    s = state[op["species"]]
    (ne, se), (ni, si) = pops or [(len(state[k]["ids"]),) * 2 for k in (op["electron"], op["ion"])]
    return req, iref.application(req, np.asarray(s["ids"]), s["frac"], s["vel"], ne, se, ni, si)


def burn_want(sc, state, op, epoch=None, pops=None):
    """burn_reference's application of a request to a state (per species dict(frac=, vel=, cell=, ids=)); pops: (n, id span)
    of p3 and p4 (default: nobody thinned)"""
    import burn_reference as bref
    a, b, (p3, p4) = op["a"], op["b"], op["products"]
    kw = dict(op["kw"], epoch=op["kw"]["epoch"] if epoch is None else epoch)
    m = sc["masses"]
    req = bref.request(kw["sigma"], kw["g_lo"], kw["g_hi"], kw["tau"], sc["macro_weight"], cell_volume(sc), m[a], m[a if b is None else b], m[p3],
                       m[p4] if p4 is not None else op["other_mass"], q_value=op["q_value"], seed=kw["seed"], stream=kw["stream"], epoch=kw["epoch"], like=b is None)
    side = lambda k: dict(cell=state[k]["cell"], ids=state[k]["ids"], pos=state[k]["frac"], vel=state[k]["vel"])
    (n3, s3), (n4, s4) = pops or [(len(state[k]["ids"]),) * 2 if k is not None else (0, 0) for k in (p3, p4)]
    return req, bref.application(req, side(a), None if b is None else side(b), n3, s3, n4, s4, tracked_b=p4 is not None)


def hook_events4(sc):
    """the events of the ioniser and of the first burner at their first application, on the scene's initial particles"""
    state = initial_state3(sc)
    io, bu = sc["ionize_every"][0], sc["burn_every"][0]
    return (ionize_want(sc, state, io, epoch=io["every"] + io["kw"]["epoch"])[1]["m"], burn_want(sc, state, bu, epoch=bu["every"] + bu["kw"]["epoch"])[1]["m"])


def reserved4(sc, total):
    """reserved3, extended.  The worst case of an ioniser is every projectile, of a burner half of everybody, at every
    application, on species that the applications themselves make grow: capacities of hundreds of thousands for species
    of thousands.  So every application of the hook is bounded by HOOK_GROWTH4 times its events on the initial particles
    (at least HOOK_FLOOR4), and the replay asserts that no application of the hook was refused.  The chain consumes what the
    first burner (and a one-shot burn, which reserves its own share) has put into p3: its events are bounded by the first
    burner's."""
    out = reserved3(sc, total)
    roles = sc["roles"]
    ionised, burnt = hook_events4(sc)
    io, bu = sc["ionize_every"][0], sc["burn_every"][0]
    grow_i = max(HOOK_GROWTH4 * ionised, HOOK_FLOOR4) * (total // io["every"])
    grow_b = max(HOOK_GROWTH4 * burnt, HOOK_FLOOR4) * (total // bu["every"])
    out[io["electron"]] += grow_i
    out[io["ion"]] += grow_i
    out[roles["p3"]] += grow_b
    out[roles["p4"]] += 2 * grow_b
    return out


def resolve_events4(st, pops, m, registered):
    """{species: capacity to reserve before the call} of a new kind whose reference has m events on A's rows: an exact fit
    (n + m) without registered operators, the capacity plus m with them (p4 twice: the chain may burn what a one-shot burn has
    put into p3); the target of a refusal one slot short"""
    kind = st["kind"]
    targets = [st["electron"], st["ion"]] if kind in IONIZE_KINDS4 else [k for k in st["products"] if k is not None]
    out = {}
    for k in targets:
        out[k] = pops[k]["capacity"] + m if registered else pops[k]["n"] + m
    if registered and kind in BURN_KINDS4 + ("burn_nothing", "burn_refused"):
        p4 = st["p4"]
        out[p4] = pops[p4]["capacity"] + 2 * m
    if kind in ("ionize_refused", "burn_refused"):
        out[st["short"]] = pops[st["short"]]["n"] + m - 1
    return out


def _step4(rng, sc, kind, saturated=False):
    """a step of a generation-4 kind"""
    roles = sc["roles"]
    if kind in IONIZE_KINDS4:
        st = dict(_ionize4(rng, sc, float(rng.uniform(*IONIZE_SHARE)), sc["dt"], nothing=kind == "ionize_nothing"), kind=kind)
        if kind == "ionize_refused":
            st.update(ion=roles["short_i"], short=roles["short_i"])
        return st
    nothing = None if kind != "burn_nothing" else ("above", "tau")[int(rng.integers(0, 2))]
    form = dict(burn_unlike="unlike", burn_like="like", burn_refused="unlike").get(kind) or ("unlike", "like")[int(rng.integers(0, 2))]
    a = 0 if form == "unlike" or saturated else int(rng.integers(0, 2))
    p = 4.0 if saturated else float(rng.uniform(0.5, 0.9)) if a == 1 else float(rng.uniform(0.05, 0.2))      # (species 1 has some forty like pairs)
    st = dict(_burn4(rng, sc, a, 1 if form == "unlike" else None, kind != "burn_untracked", p, nothing, BURN_G_SATURATED if saturated else BURN_G), kind=kind, form=form, saturated=saturated, nothing=nothing, p4=roles["p4"])
    if kind == "burn_refused":
        st["products"][1] = roles["short_b"]
        st["short"] = roles["short_b"]
    return st


def sequence4(seed):
    """the steps of a generation-4 seed.  Step 0 is a substeps whose reads hold a saveCheckpoint.  The forced block, after one
    or two steps: the seed's first removal (of REMOVE_KINDS3), a substeps with k >= sort_interval + 1 (a re-binning push on a
    thinned species), an `ionize`, such a substeps again, the seed's saturated burn (of BURN_KINDS4, on species 0), such a
    substeps again — the three substeps carry the fusionYield and fusionSpectrum reads —, then a removal of every second id
    of the product species p3 (every later burn puts its products into a THINNED species: their ids are id span + l, not
    n + l), and no renumber and no loadCheckpoint before the block ends.  Then every kind of NEW_KINDS4 once more in a drawn order (so every seed holds every
    new kind), half of them directly behind such a substeps, and between them seven to nine kinds of generations 1 to 3 from a cycle
    that starts where the seed puts it.  A step carries `thinned`, `thinned_after` and `refused` as in generation 3; reads
    as in generation 3, with ionizeStats and burnStats on a scene with registered operators."""
    sc = scene4(seed)
    rng = np.random.default_rng([0x0B54, seed])
    roles = sc["roles"]
    olds = [k for k in STATE_KINDS3 if k != "substeps"]
    old_cycle = [olds[(i + 5 * seed) % len(olds)] for i in rng.permutation(len(olds))]
    ks = [k for k in (1, 2, 3, 5) if k >= sc["sort_interval"] + 1][:2]
    push = lambda: ("substeps", int(ks[int(rng.integers(0, len(ks)))]), True)
    first_removal = REMOVE_KINDS3[int(rng.integers(0, 3))]
    plan = [("substeps", None, False)] + [("old", None, False) for _ in range(int(rng.integers(0, 2)))]
    plan += [(first_removal, None, False), push(), ("ionize", None, False), push(), (BURN_KINDS4[int(rng.integers(0, 3))], "saturated", False), push()]
    plan.append(("thin_product", None, False))
    block_end = len(plan)
    news = [NEW_KINDS4[i] for i in rng.permutation(len(NEW_KINDS4))]
    n_old = int(rng.integers(7, 10))
    rest = [("new", k) for k in news] + [("old", None)] * n_old
    rest = [rest[i] for i in rng.permutation(len(rest))]
    for which, k in rest:
        if which == "new":
            if rng.random() < 0.5:
                plan.append(push())
            plan.append((k, None, False))
        else:
            if rng.random() < 0.35:
                plan.append(("substeps", None, False))
            plan.append(("old", None, False))
    plan.append(("substeps", None, False))
    reads_per_step = 6 if sc["registered"] else READS3
    t = 0
    seen = {k: 0 for k in STATE_KINDS4}
    saved, last_substeps = [], -1
    thinned = set(sc["empty"])
    used_primes = [set(), set()]
    steps = []
    for index, (kind, arg, fusion_reads) in enumerate(plan):
        if kind == "old":
            while True:
                kind = old_cycle.pop() if old_cycle else olds[int(rng.integers(0, len(olds)))]
                if kind == "loadCheckpoint" and (not any(s < last_substeps for s in saved) or (sc["registered"] and thinned)):
                    continue
                if index < block_end and kind in REMOVE_KINDS3 + ("renumber",):
                    continue          # (the block's removal is the seed's first; a renumber before it has nothing to do)
                break
        st = dict(kind=kind, tag=index + 1, precalc=False)
        if kind == "thin_product":      # every second id of p3, which the block's burn has just filled with consecutive ids: it cannot be vacuous
            kind = "remove_thinned_by_id"
            st = dict(kind=kind, species=roles["p3"], where=None, every=(2, int(rng.integers(0, 2))), outside=False, tag=index + 1, precalc=False)
        elif kind in STATE_KINDS and kind not in ("substeps", "loadCheckpoint"):
            st = dict(_step1(rng, sc, kind), tag=index + 1, precalc=False)
            if kind in ("setRange", "load"):
                n = sc["counts"][st["species"]]
                st.update(first_frac=st.pop("first") / n, count_frac=st.pop("count") / n)
            if kind == "load":
                _unit_box(st)
        elif kind == "substeps":
            st["k"] = int(rng.choice([1, 2, 3, 5])) if arg is None else arg
            t += st["k"]
            last_substeps = index
        elif kind == "loadCheckpoint":
            files = [f for f, s in enumerate(saved) if s < last_substeps]
            st["file"] = files[int(rng.integers(0, len(files)))]
        elif kind in STATE_KINDS2:
            st.update(_step2_unit(rng, sc, kind, t))
        elif kind in NEW_KINDS3:
            st = dict(_step3(rng, sc, kind, used_primes), tag=index + 1, precalc=False)
            kind = st["kind"]
            if kind == "reserve" and rng.random() < 0.5:      # (the new species too: a product, the electrons)
                st["species"] = (roles["p3"], roles["p4"], roles["electron"])[int(rng.integers(0, 3))]
        else:
            st = dict(_step4(rng, sc, kind, saturated=arg == "saturated"), tag=index + 1, precalc=False)
        st["thinned"] = sorted(thinned)
        st["refused"] = (kind in CALLER_ORDER_KINDS3 and st["species"] in thinned) or (kind == "renumber" and sc["registered"] and bool(thinned))
        if kind in POSITION_KINDS2 and st["what"] != "velocity" and not st["refused"]:
            st["precalc"] = sc["solver"] != "none" or bool(rng.random() < 0.5)
        if kind in REMOVE_KINDS3:
            thinned.add(st["species"])
        elif kind in BURN_KINDS4:
            thinned |= {st["a"]} | ({st["b"]} if st["b"] is not None else set())
        elif kind == "loadCheckpoint" or (kind == "renumber" and not st["refused"]):
            thinned.clear()
            used_primes[0].clear(), used_primes[1].clear()
        elif kind == "substeps" and sc["registered"]:
            thinned |= {op["species"] for op in sc["remove_every"] if t >= op["every"]}
            bu = sc["burn_every"][0]
            if t >= bu["every"]:
                thinned |= {bu["a"]} | ({bu["b"]} if bu["b"] is not None else set())
        st["thinned_after"] = sorted(thinned)
        off = (seed * 4 + STATE_KINDS4.index(kind) * 5 + seen[kind] * reads_per_step) % len(READ_KINDS2)
        seen[kind] += 1
        kinds = [READ_KINDS2[(off + i) % len(READ_KINDS2)] for i in range(reads_per_step)]
        forced_reads = ("fusionYield", "fusionSpectrum") if fusion_reads and index < block_end else ("saveCheckpoint",) if index == 0 else ()
        for slot, want in enumerate(forced_reads):
            if want not in kinds:
                kinds[[i for i, k in enumerate(kinds) if k not in forced_reads][slot]] = want
        st["reads"] = [_read3(rng, k, sc, saved, index, thinned) for k in kinds]
        if sc["registered"]:
            st["reads"] += [_read3(rng, k, sc, saved, index, thinned) for k in STATS_KINDS3] + [dict(kind=k, species=0) for k in STATS_KINDS4[len(STATS_KINDS3):]]
        steps.append(st)
    return steps


def can_have_rebinned4(sc, steps):
    """can_have_rebinned3 with the new kinds: an ionisation or a burn with events leaves its targets (and a burn its
    reactants) as an upload leaves a species; a registered ioniser or burner does the same from inside substeps()"""
    hook = [op["every"] for key in ("remove_every", "inject_every", "ionize_every", "burn_every") for op in sc.get(key, [])] if sc["registered"] else []
    out, since, t = [], 0, 0
    for st in steps:
        if st["kind"] == "substeps":
            pushed = False
            for _ in range(st["k"]):
                t += 1
                since += 1
                pushed = pushed or since > sc["sort_interval"]
                if any(t % every == 0 for every in hook):
                    since, pushed = 0, False
            out.append(sc["solver"] != "yee" and sc["sort_interval"] > 0 and pushed)
        else:
            if not st["refused"] and ((st["kind"] in POSITION_KINDS2 and st["what"] != "velocity") or st["kind"] in ("loadCheckpoint", "sort") + UNBINNING_KINDS3 + ("ionize",) + BURN_KINDS4):
                since = 0
            out.append(False)
    return out


# ---- the named scenes of generation 4: plain programs the GPU module runs line by line
def _plain4(seed, solver, precision, name, separate=True, **kw):
    sc = _species4(_plain3(seed, solver, precision, name, **kw), separate, short=False)
    sc["empty"] = []
    return sc


def flat_ionize_density(K, tau, sigma, g_lo, g_hi):
    """the density at which a request with the table sigma has the candidate word bound K (gas_density for any table)"""
    return -math.log1p(-K * 2.0 ** -32) / (C * tau * gasref.bound(sigma, g_lo, g_hi))


CHAIN_CASES = [("none", "fp64"), ("poisson_fft", "fp32")]
CHAIN_PIECES = (1, 2, 3, 5, 5, 3, 1)          # twenty sub-steps


def chain(solver, precision):
    """Two registered burners — a like burner on species 0 whose products land in species 2 and 3, and an unlike burner on
    species 2 with species 1 — beside a registered ioniser whose PROJECTILE species is species 2 (its secondaries go to a species
    of their own, its ions to species 1): everything that happens to species 2 happens in the hook.  Twenty sub-steps in
    pieces of 1, 2, 3 and 5.  The `none` case has E = 0 and no addB — no velocity changes but by the three operators — and
    carries the ledger."""
    sc = _plain4(410, solver, precision, "chain")
    assert len(sc["counts"]) == 5
    roles = sc["roles"]
    rng = np.random.default_rng([0x9E9D, 410])
    first = dict(_burn4(rng, sc, 0, None, True, 0.03), every=1)
    m3, m4 = sc["masses"][roles["p3"]], sc["masses"][roles["p4"]]
    second = dict(a=roles["p3"], b=1, products=[roles["p4"], None], other_mass=m3, q_value=burn_q(m4, m3), p=4.0, every=2,
                  kw=dict(sigma=burn_table(), g_lo=BURN_G[0], g_hi=BURN_G[1], tau=burn_tau(sc, 4.0), seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)),
                          epoch=int(rng.integers(0, 1000))))
    io = dict(_ionize4(rng, sc, 0.15, sc["dt"], window="whole"), every=1, species=roles["p3"])
    io["kw"]["species"] = roles["p3"]
    sc.update(ionize_every=[io], burn_every=[first, second], pieces=CHAIN_PIECES, zero_field=solver == "none")
    sc["capacities"] = [N0, N1 + 6000, 1 + 3000, 1 + 4000, 1 + 6000]
    return sc


RESERVE_AFTER_REGISTER = dict(before=2, after=3, extra=1500, capacities=(N0 + 400, N1 + 400, 300, 300))


def reserve_after_register():
    """burnEvery and ionizeEvery registered beside collidePairEvery and fusionYieldEvery on the same species, all due every
    sub-step; after two sub-steps reserve() on a reactant (species 0), on a product (p3) and on the ion target (species 1),
    each across a stride of 1024; then three sub-steps.  The shape of generation 3's bug for the two new
    families, whose buffers are sized per application from n and from the id span."""
    sc = _plain4(411, "poisson_fft", "fp32", "reserve_after_register", separate=False)
    rng = np.random.default_rng([0x9E9D, 411])
    kw = lambda: dict(seed=int(rng.integers(1, 1 << 40)), stream=int(rng.integers(0, 8)), epoch=int(rng.integers(0, 1000)))
    fusion = _fusion_kw3(rng, sc)
    sc.update(pair_every=dict(every=1, a=0, b=1, kw=dict(log_lambda=LOG_LAMBDA, tau=sc["tau_unlike"], **kw())), fusion_every=dict(every=1, a=0, b=1, kw=fusion),
              ionize_every=[dict(_ionize4(rng, sc, 0.02, sc["dt"], window="whole"), every=1)], burn_every=[dict(_burn4(rng, sc, 0, 1, True, 0.05), every=1)],
              plan=dict(RESERVE_AFTER_REGISTER, reserve=[0, sc["roles"]["p3"], 1]))
    sc["capacities"] = list(RESERVE_AFTER_REGISTER["capacities"])
    return sc


HOOK_ORDER = dict(count=500, substeps=3)


def hook_order(precision="fp64"):
    """A source of a fast beam into the projectile species 0, an ioniser whose table only the fast reach and whose
    secondaries go to a species of their own (one particle before the run), and a saturated like burner ON THAT SPECIES, all
    due on sub-step 1: the ioniser can only find the beam if it runs behind the source, the burner can only find a pair if it
    runs behind the ioniser (tests/test_gpu_ionize.py::test_order_in_the_hook, with the burner behind it)."""
    sc = _plain4(412, "poisson_fft", precision, "hook_order")
    roles = sc["roles"]
    rng = np.random.default_rng([0x9E9D, 412])
    beam = dict(kind="volume", lo=[0.4, 0.4, 0.4], hi=[0.6, 0.6, 0.6], seed=int(rng.integers(1, 1 << 40)), stream=5, vth=0.001, drift=[0.0, 0.0, 0.8], first=0, count=HOOK_ORDER["count"],
                epoch=0)
    flat = np.full(2, 3.0e-19)
    io = dict(species=0, electron=roles["electron"], ion=1, g_threshold=0.6, window="whole", every=1,
              kw=dict(species=0, density=flat_ionize_density(0.9 * 2.0 ** 32, sc["dt"], flat, 0.6, 0.9), tau=sc["dt"], sigma=flat, g_lo=0.6, g_hi=0.9, seed=int(rng.integers(1, 1 << 40)), stream=1,
                      epoch=int(rng.integers(0, 1000)), taper=[None, None, None], drift=(0.0, 0.0, 0.001), vth=(0.002, 0.002, 0.002)))
    bu = dict(_burn4(rng, sc, roles["electron"], None, True, 4.0), every=1)
    sc.update(inject_every=[dict(every=1, species=0, kw=beam)], ionize_every=[io], burn_every=[bu], substeps=HOOK_ORDER["substeps"])
    sc["capacities"] = [N0 + 3 * HOOK_ORDER["count"], N1 + 6000, 1 + 3000, 1 + 3000, 1 + 6000]
    return sc


def burner_fails_behind_an_ioniser():
    """An ioniser and, behind it, a burner whose third application is ONE SLOT SHORT: the mate runs first and by hand, and the
    replay gives A's product species the room of the first two applications and of the third but one (room_of: the events are
    the mate's, which A's equal bit for bit if the relation holds).  substeps(5) raises FPIC_ERR_STATE naming fpic_reserve;
    the handle equals the mate that stopped before that burner, the ioniser's application of that sub-step in place and
    settled; after reserve() the run goes on."""
    sc = _plain4(418, "poisson_fft", "fp64", "burner_fails_behind_an_ioniser", separate=False, sort_interval=1)
    rng = np.random.default_rng([0x9E9D, 418])
    sc.update(ionize_every=[dict(_ionize4(rng, sc, 0.05, sc["dt"], window="whole"), every=1)], burn_every=[dict(_burn4(rng, sc, 0, 1, True, 0.1), every=1)], fails_at=3)
    sc["capacities"] = [N0 + 2000, N1 + 2000, 1 + 2000, 1 + 2000]      # the mate's; A's p3 is given room_of(events)
    return sc


def room_of(n, events):
    """the capacity at which the last of `events` applications is one slot short"""
    return n + sum(events) - 1


NAMED4 = {"chain": chain, "reserve_after_register": reserve_after_register, "hook_order": hook_order, "burner_fails_behind_an_ioniser": burner_fails_behind_an_ioniser}


# ---- the resumes of generation 4: generation 3's scene with a source (no sink) and (i) an ioniser alone — nobody is thinned,
# the cut goes through a file into a fresh handle that reserves and registers again with shifted epochs — or (ii) a burner
# as well: a thinned species has no file, so both runs clear every registration at T (clearIonization and clearBurn among
# them), renumber and register again; only one of them goes through the file.
def resume_scene4(solver, precision, burner):
    sc = _species4(resume_scene3(solver, precision, False), True, short=False)
    sc["empty"] = []
    rng = np.random.default_rng([0x5CE94, 1000])
    sc["ionize_every"] = [dict(_ionize4(rng, sc, 0.1, 2 * sc["dt"], window="whole"), every=2)]
    sc["burn_every"] = [dict(_burn4(rng, sc, 0, 1, True, 0.1), every=3)] if burner else []
    ionised, burnt = hook_events4(sc) if burner else (ionize_want(sc, initial_state3(sc), sc["ionize_every"][0], epoch=2 + sc["ionize_every"][0]["kw"]["epoch"])[1]["m"], 0)
    caps = sc["capacities"] + [1] * (len(sc["counts"]) - len(sc["capacities"]))
    grow_i = max(HOOK_GROWTH4 * ionised, HOOK_FLOOR4) * (RESUME_N // 2)
    grow_b = max(HOOK_GROWTH4 * burnt, HOOK_FLOOR4) * (RESUME_N // 3)
    caps[sc["roles"]["electron"]] += grow_i
    caps[1] += grow_i
    caps[sc["roles"]["p3"]] += grow_b
    caps[sc["roles"]["p4"]] += grow_b
    sc["capacities"] = caps
    return sc
