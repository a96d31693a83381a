"""The scenes the binary collision operator (fpic_pair) is tested on, shared by tests/test_pair_reference.py (CPU: the
reference against its 50-digit twin on these very particles) and tests/test_gpu_pair.py, computed once and never changed.

A 16^3 box of 16 m: a position (i + f) with f a multiple of 1/8 strictly inside (0, 1) is the fraction (i + f) / 16 of the
box exactly, in fp32, in fp64 and in the test's own arithmetic, so the cell of a particle is floor(position) everywhere.
Velocities are float32 values, so an fp32 and an fp64 handle store the same numbers.  The populated cells are adjacent, at a
tile edge (the planes 7 | 8 of every axis: tiles are 16x16x8 cells, 8x8x8 under full EM) and at the periodic corner."""
import numpy as np

SHAPE = (16, 16, 16)
L = (16.0, 16.0, 16.0)
DV = 1.0
ME, QE, MP = 9.1093837015e-31, -1.602176634e-19, 1.67262192369e-27
LOG_LAMBDA = 10.0
TAU = 1e-9

CELLS = [(15, 15, 15), (0, 0, 0), (1, 0, 0), (0, 15, 15), (7, 7, 7), (8, 7, 7), (7, 8, 7), (7, 7, 8), (8, 8, 8), (15, 0, 0), (3, 3, 3), (4, 3, 3)]
LIKE_COUNTS = [1025, 0, 1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024]
# (Na, Nb): Nf = 0 both ways, (1,1), (5,1), (7,3), (64,64), (65,64), (130,7), and each species the `many` one somewhere
UNLIKE_COUNTS = [(130, 7), (3, 0), (0, 2), (1, 1), (5, 1), (1, 5), (7, 3), (3, 7), (64, 64), (65, 64), (64, 65), (7, 130)]


def cell_index(pos):
    """the deposit's cell of positions in metres (exact: see above)"""
    c = np.floor(np.asarray(pos, dtype=np.float64)).astype(np.int64)
    return c[:, 0] + SHAPE[0] * (c[:, 1] + SHAPE[1] * c[:, 2])


def populate(counts, seed, vth, cells=CELLS):
    """positions (metres, float64) and velocities (float32) of sum(counts) particles, counts[k] of them in cells[k], in a
    random order (the caller's index is the id)"""
    rng = np.random.default_rng(seed)
    where = np.repeat(np.arange(len(cells)), counts)
    rng.shuffle(where)
    n = len(where)
    pos = np.asarray(cells, dtype=np.float64)[where] + rng.integers(1, 8, size=(n, 3)) / 8.0
    vel = (rng.normal(0.0, 1.0, size=(n, 3)) * np.asarray(vth)).astype(np.float32)
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel


def weight(n_l, vth, var=0.05, ma=ME, qa=QE, mb=ME, qb=QE):
    """the macro weight at which a pair of relative speed vth in a cell of N_L = n_l has the variance `var`"""
    import pair_reference as ref
    k1 = ref.request(LOG_LAMBDA, TAU, ma, qa, mb, qb, 1.0, DV)["kappa"]
    return var * vth ** 3 / (k1 * n_l)


_made = {}


def like_scene():
    """electrons with themselves: {pos, vel, W}"""
    if "like" not in _made:
        pos, vel = populate(LIKE_COUNTS, 11, 0.01)
        _made["like"] = dict(pos=pos, vel=vel, W=weight(64, 0.01))
    return _made["like"]


def unlike_scene():
    """electrons (a) with protons (b): {pos_a, vel_a, pos_b, vel_b, W}"""
    if "unlike" not in _made:
        pa, va = populate([c[0] for c in UNLIKE_COUNTS], 12, 0.01)
        pb, vb = populate([c[1] for c in UNLIKE_COUNTS], 13, 0.0005)
        _made["unlike"] = dict(pos_a=pa, vel_a=va, pos_b=pb, vel_b=vb, W=weight(7, 0.01, mb=MP, qb=-QE))
    return _made["unlike"]
