"""The scenes that take fpic_pair and fpic_fusion off the 16^3 box of tests/pair_scene.py, shared by
tests/test_pair_wide_reference.py (CPU: the conditions below and the reference against its 50-digit twin),
tests/test_gpu_pair_wide.py and tests/pair_forms_child.py; computed once and never changed.

The grid is 37 x 33 x 29 cells of 1 m (dV = 1): 35409 cells, one more than a multiple of 16 (the scan's ragged tail), more
than two turns of the scan, 554 chunks of 64 cells for 512 workgroups with 17 cells in the last, 3 x 3 x 4 electrostatic and
5 x 5 x 4 full-EM tiles, partial on every axis; and nx, ny, nz all differ, so a slip in the linearisation i + nx (j + ny k)
aliases cells.  A position is (i + f) with f in {1/8 .. 7/8}: the stored fraction (i + f) / 37 is rounded here (the box is no
power of two), by at most 37 x 2^-24 of a cell in fp32 against the 1/8 margin, so the cell is floor(position) in both
precisions (tests/test_pair_wide_reference.py holds that).  Velocities are float32 values.

wide_like(): electrons spread over all cells (counts 0, 1, 2, 3, ...; the first and the last cell populated) and crafted
    counts (LIKE_CRAFTED: linear cell -> count; a spread particle never lands in a crafted cell): six consecutive cells of one
    chunk that are cut by the total, hold a full and an overfull cell; four cells of 900 across a chunk boundary; the cells on
    both sides of the scan's turns, 32768 being also the first cell of chunk 512 = a workgroup's second chunk.
wide_unlike(): electrons and protons spread the same way and nine consecutive crafted cells of one chunk (UNLIKE_CRAFTED).
big_like(): 4 194 304 + 4097 electrons, uniform over the cells: the smallest count at which the LDS index passes take a
    second trip (2048 workgroups x 2048 slots and one turn more)."""
import numpy as np

from pair_scene import LOG_LAMBDA, ME, MP, QE, TAU, weight  # noqa: F401  (the scenes' constants, for their users)

SHAPE = (37, 33, 29)
L = (37.0, 33.0, 29.0)
DV = 1.0
NCELLS = SHAPE[0] * SHAPE[1] * SHAPE[2]
BOX_KW = dict(nr=SHAPE[0], ny=SHAPE[1], nz=SHAPE[2], radius=L[0], length_y=L[1], height=L[2])     # over box_spec's shape of the 16^3 scenes

LIKE_RUN_AT = 100 * 64 + 10                    # chunk 100
LIKE_RUN = [1500, 1500, 1500, 2048, 2049, 600]
LIKE_STRADDLE_AT = 200 * 64 - 2                # the last two cells of chunk 199 and the first two of chunk 200
LIKE_STRADDLE = [900, 900, 900, 900]
LIKE_TURNS = {16383: 301, 16384: 302, 32767: 303, 32768: 305}
LIKE_CRAFTED = {**{LIKE_RUN_AT + k: n for k, n in enumerate(LIKE_RUN)}, **{LIKE_STRADDLE_AT + k: n for k, n in enumerate(LIKE_STRADDLE)}, **LIKE_TURNS}

UNLIKE_RUN_AT = 300 * 64 + 20                  # chunk 300
UNLIKE_RUN = [(2048, 2048), (2048, 2049), (5, 2048), (2048, 5), (1300, 700), (1300, 700), (1300, 700), (0, 500), (500, 0)]
UNLIKE_CRAFTED = {UNLIKE_RUN_AT + k: c for k, c in enumerate(UNLIKE_RUN)}

N_SPREAD_A, N_SPREAD_B = 60000, 30000
N_BIG = 4194304 + 4097
SEEDS = dict(seed=0x5EED0123456789AB, stream=7, epoch=11)     # the request of every pair test on these scenes, CPU and GPU
BIG_EVERY = 97                                 # the cells of big_like the references are run on: every 97th linear cell


def cell_index(pos):
    """the deposit's cell of positions in metres: floor(position), linearised"""
    c = np.floor(np.asarray(pos, dtype=np.float64)).astype(np.int64)
    return c[:, 0] + SHAPE[0] * (c[:, 1] + SHAPE[1] * c[:, 2])


def ijk(cell):
    cell = np.asarray(cell, dtype=np.int64)
    return np.stack([cell % SHAPE[0], (cell // SHAPE[0]) % SHAPE[1], cell // (SHAPE[0] * SHAPE[1])], axis=1)


def populate(rng, n_spread, crafted, vth, ends=True):
    """positions (metres, float64) and velocities (float32): n_spread particles in cells drawn uniformly from the cells that
    are not crafted, two in the first and three in the last cell, crafted[c] in the cell c; in a random order (the caller's
    index is the id)"""
    where = rng.integers(0, NCELLS, size=n_spread)
    where = where[~np.isin(where, list(crafted))]
    extra = [0, 0, NCELLS - 1, NCELLS - 1, NCELLS - 1] if ends else []
    where = np.concatenate([where, np.array(extra, dtype=np.int64), np.repeat(np.array(list(crafted), dtype=np.int64), list(crafted.values()))])
    rng.shuffle(where)
    n = len(where)
    pos = ijk(where).astype(np.float64) + rng.integers(1, 8, size=(n, 3)) / 8.0
    vel = (rng.normal(0.0, 1.0, size=(n, 3)) * vth).astype(np.float32)
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel


_made = {}


def wide_like():
    """electrons with themselves: {pos, vel, W}"""
    if "like" not in _made:
        pos, vel = populate(np.random.default_rng(101), N_SPREAD_A, LIKE_CRAFTED, 0.01)
        _made["like"] = dict(pos=pos, vel=vel, W=weight(64, 0.01))
    return _made["like"]


def wide_unlike():
    """electrons (a) with protons (b): {pos_a, vel_a, pos_b, vel_b, W}"""
    if "unlike" not in _made:
        pa, va = populate(np.random.default_rng(102), N_SPREAD_A, {c: n[0] for c, n in UNLIKE_CRAFTED.items()}, 0.01)
        pb, vb = populate(np.random.default_rng(103), N_SPREAD_B, {c: n[1] for c, n in UNLIKE_CRAFTED.items()}, 0.0005)
        _made["unlike"] = dict(pos_a=pa, vel_a=va, pos_b=pb, vel_b=vb, W=weight(7, 0.01, mb=MP, qb=-QE))
    return _made["unlike"]


def big_like():
    """electrons with themselves, N_BIG of them: {pos, vel, W, cell}"""
    if "big" not in _made:
        rng = np.random.default_rng(104)
        where = rng.integers(0, NCELLS, size=N_BIG)
        pos = ijk(where).astype(np.float64)
        pos += rng.integers(1, 8, size=(N_BIG, 3)) / 8.0
        vel = rng.standard_normal(size=(N_BIG, 3), dtype=np.float32) * np.float32(0.01)
        for a in (pos, vel, where):
            a.setflags(write=False)
        _made["big"] = dict(pos=pos, vel=vel, W=weight(118, 0.01), cell=where)
    return _made["big"]


def like_pairs(counts, cell_max=2048):
    """(pairs, cells) of the like pairing of cells holding `counts` particles: n // 2 pairs, and two more for an odd cell"""
    counts = np.asarray(counts, dtype=np.int64)
    counts = counts[(counts >= 2) & (counts <= cell_max)]
    return int((counts // 2 + 2 * (counts % 2)).sum()), int(len(counts))
