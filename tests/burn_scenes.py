"""Scenes of the burn tests (tests/test_burn_reference.py on the CPU, where their conditions are checked;
tests/test_gpu_burn.py on the GPU), computed once and never changed.  The particles are those of the fusion tally's scenes
(tests/fusion_scene.py: the 16^3 box with positions on eighths of a cell and float32 velocities, so a handle of either
precision stores exactly what the reference is given) and two scenes of their own:

    "like"      like cells of 0, 1, 2, 3 ... 65 (one above rank_max: the bitonic network), 129, 1024, 1025, a pair at rest
    "unlike"    unlike cells from (1,1) to (130,7), each species the `many` one somewhere, ties
    "full"      six consecutive cells of one chunk: three of 1300 + 700 (the run is cut by the LDS total), one of 2048 + 2048
                (full) and two overfull ones (2049 of either species)
    "full_like" the like species' share of that: five consecutive cells of one chunk, 2047, 2048, 2 (the run is cut by the total in
                front of the third) and an overfull one of 2049 behind it, then 3
    "wide"      a grid with three different edges, 5 x 6 x 7 cells: a wrong linearisation i + nx (j + ny k) aliases its cells.
                fpic_create takes every axis of 2 nodes or more; 5 x 6 x 7 is the smallest grid with three different edges that the
                suite already steps under both field solvers (tests/test_gpu_moments.py), so the scene runs with both, like the others

The sizes are read from the kernel headers, so a change of them moves the boundary cases with it.  Three taus per scene: P about
1e-3 in a cell of N_L = 64 (few events: most workgroups empty their stage at most once), P about 0.3 there (many blocked), and
P >= 1 for every pair inside the table with a non-zero cross-section (saturated)."""
import os
import re

import numpy as np

import burn_reference as ref
import fusion_scene
import pair_scene
from helpers import ROOT

CSRC = os.path.join(ROOT, "fusion-sim_amd", "csrc")


def _constant(header, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, header)).read()).group(1))


PAIR_CHUNK = _constant("fes_pair_kernels.hpp", "kPairChunk")
PAIR_CELL_MAX = _constant("fes_pair_kernels.hpp", "kPairCellMax")
PAIR_ENTRIES = 2 * PAIR_CELL_MAX                                          # kPairEntries = 2 * kPairCellMax
RANK_MAX = _constant("fes_pair_kernels.hpp", "kPairRankMax")
assert PAIR_CELL_MAX == ref.CELL_MAX and RANK_MAX + 1 in fusion_scene.LIKE_COUNTS

MD, MT, MA, MP, MN = 3.3435837724e-27, 5.0073567446e-27, 6.6446573357e-27, 1.67262192369e-27, 1.67492749804e-27
QP = 1.602176634e-19
Q_DT = 17.589e6 * QP                                 # J
W = fusion_scene.W
SEEDS = dict(seed=0xB0510D7123456789, stream=3, epoch=9)

FULL_CELLS = [(5, 8, 7), (6, 8, 7), (7, 8, 7), (8, 8, 7), (9, 8, 7), (10, 8, 7)]      # consecutive linear cells of one chunk
FULL_COUNTS = [(1300, 700), (1300, 700), (1300, 700), (PAIR_CELL_MAX, PAIR_CELL_MAX), (PAIR_CELL_MAX + 1, 3), (10, PAIR_CELL_MAX + 1)]
_full = pair_scene.cell_index(np.array(FULL_CELLS, dtype=np.float64) + 0.5)
assert sum(a + b for a, b in FULL_COUNTS[:3]) > PAIR_ENTRIES and np.all(np.diff(_full) == 1) and _full[0] // PAIR_CHUNK == _full[-1] // PAIR_CHUNK

FULL_LIKE_COUNTS = [PAIR_CELL_MAX - 1, PAIR_CELL_MAX, 2, PAIR_CELL_MAX + 1, 3]       # (the first is odd: its triple saturates)
assert sum(FULL_LIKE_COUNTS[:2]) <= PAIR_ENTRIES < sum(FULL_LIKE_COUNTS[:3]) and FULL_LIKE_COUNTS[2] <= RANK_MAX < PAIR_CELL_MAX

WIDE_SHAPE = (5, 6, 7)
WIDE_L = (5.0, 6.0, 7.0)
WIDE_COUNTS = {(0, 0, 0): (3, 1), (4, 0, 0): (1, 1), (0, 5, 0): (7, 3), (0, 0, 6): (2, 9), (4, 5, 6): (5, 5), (1, 1, 1): (70, 20), (3, 2, 0): (1, 0)}


def table(g_lo=fusion_scene.G_LO):
    S, lo, hi = fusion_scene.table(g_lo)
    return dict(sigma=S, g_lo=lo, g_hi=hi)


def tau_for(p, n_l=64.0, g=0.02):
    """the tau at which a pair of relative speed g in a cell of N_L = n_l has about the probability p"""
    S = table()["sigma"]
    return p / (W * n_l * float(S.max()) * g * ref.C / fusion_scene.DV)


# saturated: the smallest non-zero cross-section, the table's first speed, N_L = 1
TAUS = {"rare": tau_for(1e-3), "many": tau_for(0.3), "saturated": 4.0 / (W * 1.0 * 1e-29 * fusion_scene.G_LO * ref.C / fusion_scene.DV)}

_made = {}


def particles(name):
    """dict(shape, L, like, a=(pos, vel), b=(pos, vel) or None): positions in metres (float64), velocities float32"""
    if name in _made:
        return _made[name]
    shape, L = fusion_scene.SHAPE, fusion_scene.L
    if name == "like":
        s = fusion_scene.like_scene()
        out = dict(like=True, a=(s["pos"], s["vel"]), b=None)
    elif name == "unlike":
        s = fusion_scene.unlike_scene()
        out = dict(like=False, a=(s["pos_a"], s["vel_a"]), b=(s["pos_b"], s["vel_b"]))
    elif name == "full":
        out = dict(like=False, a=pair_scene.populate([c[0] for c in FULL_COUNTS], 61, 0.01, FULL_CELLS), b=pair_scene.populate([c[1] for c in FULL_COUNTS], 62, 0.008, FULL_CELLS))
    elif name == "full_like":
        out = dict(like=True, a=pair_scene.populate(FULL_LIKE_COUNTS, 65, 0.01, FULL_CELLS[:len(FULL_LIKE_COUNTS)]), b=None)
    elif name == "wide":
        shape, L = WIDE_SHAPE, WIDE_L
        cells = list(WIDE_COUNTS)
        out = dict(like=False, a=pair_scene.populate([WIDE_COUNTS[c][0] for c in cells], 63, 0.01, cells), b=pair_scene.populate([WIDE_COUNTS[c][1] for c in cells], 64, 0.008, cells))
    else:
        raise KeyError(name)
    out.update(shape=shape, L=L)
    _made[name] = out
    return out


def cells_of(frac, shape):
    """the deposit's cell of stored fractions: floor(fraction x edge), linearised (the scenes keep 1/8 of a cell clear of every
    face, so the rounding of a stored fraction cannot move it)"""
    c = np.floor(np.asarray(frac, dtype=np.float64) * np.array(shape, dtype=np.float64)).astype(np.int64)
    return c[:, 0] + shape[0] * (c[:, 1] + shape[1] * c[:, 2])


def request(name, tau, tracked_b=False, m3=MA, m4=MN, q_value=Q_DT, g_lo=fusion_scene.G_LO, **seeds):
    p = particles(name)
    dv = float(np.prod(np.array(p["L"]) / np.array(p["shape"])))
    t = table(g_lo)
    return ref.request(t["sigma"], t["g_lo"], t["g_hi"], tau, W, dv, MD, MD if p["like"] else MT, m3, m4, q_value=q_value, like=p["like"], **dict(SEEDS, **seeds))


def stored(name, dtype):
    """(A, B) as the handle stores the scene: ids 0 .. n-1, stored fractions and velocities of the dtype, the cells"""
    p = particles(name)
    out = []
    for side in (p["a"], p["b"]):
        if side is None:
            out.append(None)
            continue
        pos, vel = side
        frac = (np.asarray(pos) / np.array(p["L"])).astype(dtype)
        out.append(dict(cell=cells_of(frac, p["shape"]), ids=np.arange(len(pos)), pos=frac, vel=np.asarray(vel).astype(dtype)))
    return out


_reference = {}


def reference(name, which, dtype=np.float32, tracked_b=False):
    """what the reference gives for a scene at TAUS[which] with empty products whose ids start at 0: computed once, shared"""
    key = (name, which, np.dtype(dtype).name, tracked_b)
    if key not in _reference:
        A, B = stored(name, dtype)
        req = request(name, TAUS[which], tracked_b=tracked_b, m4=MP if tracked_b else MN)
        _reference[key] = (req, ref.application(req, A, B, 0, 0, 0, 0, tracked_b=tracked_b))
    return _reference[key]


SCENES = ("like", "unlike", "full", "full_like", "wide")
