"""Scenes of the particle-source tests (tests/test_inject_reference.py on the CPU, tests/test_gpu_inject.py on the GPU): the
populations, the requests of both kinds, and the counts that straddle the generation pass's loop boundaries.  The launch shape
is read from the kernel header, so a change of it moves the boundary cases with it."""
import os
import re

from helpers import ROOT

_HEADER = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_inject_kernels.hpp")).read()


def _constant(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _HEADER).group(1))


THREADS = _constant("kInjectThreads")
BLOCKS = _constant("kInjectBlocks")
GROUP = _constant("kInjectGroup")       # slots per lane and turn: the lane's vector
CHUNK = THREADS * GROUP                 # slots a workgroup takes per turn
STRIDE = BLOCKS * CHUNK                 # slots the grid takes per turn

SHAPE = (8, 8, 8)
L = (0.02, 0.03, 0.025)
DT = 2e-11                              # c dt = 6 mm; with the scenes' thermal speeds a flux particle flies at most 3 mm: inside a cell
N = 3001                                # the population before a source (odd: the new slots start inside a lane's vector)
M = 2003                                # particles of one application
SUB = dict(lo=(0.1 * L[0], 0.0, 0.25 * L[2]), hi=(0.9 * L[0], L[1], 0.75 * L[2]))

VOLUME = [
    dict(seed=0xC0FFEE0123456789, stream=5, vth=0.01, **SUB),
    dict(seed=77, stream=2, drift=(0.01, 0.0, -0.02), vth=(0.05, 0.02, 0.1), mode=(2, 1, -3), xamp=(2e-5, 0.0, -1e-5), xphase=0.125,
         vamp=(1e-3, 2e-3, 0.0), vphase=0.3, **SUB),
    dict(seed=5, stream=9, lattice=True, paired=True, vth=(0.02, 0.03, 0.01)),
]
FLUX = [
    dict(axis=0, side=1, plane=0.0, seed=11, stream=1, vth=(0.05, 0.02, 0.03), drift=(0.0, 0.01, -0.01)),
    dict(axis=1, side=-1, plane=L[1], seed=12, stream=2, vth=0.04, lattice=True),
    dict(axis=2, side=-1, plane=0.4 * L[2], seed=13, stream=3, vth=(0.01, 0.02, 0.08), drift=(0.02, 0.0, 0.0), **SUB),
]
SCENES = [dict(kind="volume", n=N, count=M, capacity=N + M, first=N, **r) for r in VOLUME] + \
         [dict(kind="flux", n=N, count=M, capacity=N + M + 5, first=7, **r) for r in FLUX]


def boundary_counts(n=N):
    """counts of one application into a species of n: one particle, and one less / exactly / one more than what ends the
    first vector of the new slots, a workgroup's turn and the grid's turn"""
    head = (-n) % GROUP or GROUP        # new slots that fill the lane's vector the old ones end in (a whole vector if n is aligned)
    out = {1}
    for edge in (head, GROUP, CHUNK - n % CHUNK, CHUNK, STRIDE - n % STRIDE, STRIDE):
        out.update({edge - 1, edge, edge + 1})
    return sorted(c for c in out if c > 0)


def load_request(scene):
    """the keywords of a scene that the loader's request takes"""
    return {k: v for k, v in scene.items() if k not in ("kind", "n", "count", "capacity", "first", "axis", "side", "plane")}
