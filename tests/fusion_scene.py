"""The scenes the fusion yield tally (fpic_fusion) is tested on (tests/test_gpu_fusion.py), computed once and never changed:
the 16^3 box of tests/pair_scene.py with positions on eighths of a cell, so that the cell of a particle is floor(position) in
fp32, in fp64 and in the test's own arithmetic, and float32 velocities, so that an fp32 and an fp64 handle store the same
numbers and the tally — integers of double arithmetic on those numbers — is the same in both.

The table has 97 nodes from g_lo = 1/128 to g_hi = 1/32: dg = 1/4096 and inv_dg = 4096 exactly.  Thermal speeds of 0.01 put a
few per cent of the pairs below the table and a fifth above it.  Two like cells hold a chosen pair each: one at rest relative
to each other (g = 0: below this table, inside the one that starts at 0 and yielding 0 there) and one at g = 1/64 exactly, the
table's node 32."""
import numpy as np

import pair_scene

SHAPE, L, DV = pair_scene.SHAPE, pair_scene.L, pair_scene.DV
NCELLS = SHAPE[0] * SHAPE[1] * SHAPE[2]
W, TAU = 1e10, 1e-9
N, G_LO, G_HI = 97, 1.0 / 128, 1.0 / 32
NODE_G = 1.0 / 64

CELLS = pair_scene.CELLS + [(3, 4, 3), (4, 4, 3), (3, 3, 4), (4, 4, 4)]
LIKE_COUNTS = [1025, 0, 1, 2, 3, 4, 5, 63, 64, 65, 129, 1024, 2, 2, 6, 7]      # [12]: the pair at rest, [13]: the pair on a node
REST, NODE = 12, 13
# (Na, Nb) from (1,1) to (130,7): Nf = 0 both ways, each species the `many` one somewhere, ties, one wave's worth and above
UNLIKE_COUNTS = pair_scene.UNLIKE_COUNTS + [(2, 2), (129, 65), (1, 64), (33, 200)]
cell_index = pair_scene.cell_index


def table(g_lo=G_LO):
    """(S, g_lo, g_hi): a smooth cross-section of the size of D-T's (m^2) with a zero stretch at the low end"""
    g = g_lo + np.arange(N) * ((G_HI - g_lo) / (N - 1))
    S = 5e-28 * np.maximum(0.0, np.sin(100.0 * (g - 0.009))) ** 2 + np.where(g > 0.012, 1e-29, 0.0)
    S.setflags(write=False)
    return S, g_lo, G_HI


_made = {}


def like_scene():
    """deuterons with themselves: {pos, vel}"""
    if "like" not in _made:
        pos, vel = pair_scene.populate(LIKE_COUNTS, 21, 0.01, CELLS)
        vel = vel.copy()
        cell = cell_index(pos)
        want = lambda k: np.flatnonzero(cell == cell_index(np.array([CELLS[k]], dtype=np.float64) + 0.5)[0])
        rest, node = want(REST), want(NODE)
        assert len(rest) == 2 and len(node) == 2
        vel[rest[1]] = vel[rest[0]]
        vel[node[0]] = (np.float32(NODE_G), 0, 0)
        vel[node[1]] = (0, 0, 0)
        vel.setflags(write=False)
        _made["like"] = dict(pos=pos, vel=vel)
    return _made["like"]


def unlike_scene():
    """deuterons (a) with tritons (b): {pos_a, vel_a, pos_b, vel_b}"""
    if "unlike" not in _made:
        pa, va = pair_scene.populate([c[0] for c in UNLIKE_COUNTS], 22, 0.01, CELLS)
        pb, vb = pair_scene.populate([c[1] for c in UNLIKE_COUNTS], 23, 0.008, CELLS)
        _made["unlike"] = dict(pos_a=pa, vel_a=va, pos_b=pb, vel_b=vb)
    return _made["unlike"]
