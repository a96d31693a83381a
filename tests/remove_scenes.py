"""The scenes of tests/test_gpu_remove.py: populations and requests, and the counts and planted slots of its loop and chunk
boundary cases.  tests/test_remove_reference.py checks their conditions on the CPU (every scene removes 0 < removed < n, the
plain and the outside form partition the candidates, the boundary cases straddle their boundaries), so that a GPU case cannot
pass by removing nothing."""
import os
import re

import numpy as np

from helpers import ROOT

N = 6000            # particles of the request scenes
SIGMA = 0.03        # thermal speed, units of c


def kernel_constants():
    """kRemoveChunk, kRemoveBlocks and kRemoveThreads of the kernel header, so that a new launch shape moves the cases"""
    text = open(os.path.join(ROOT, "fusion-sim_amd", "csrc", "fes_remove_kernels.hpp")).read()
    get = lambda name: int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    return get("kRemoveChunk"), get("kRemoveBlocks"), get("kRemoveThreads")


CHUNK, BLOCKS, THREADS = kernel_constants()
WAVES = BLOCKS * THREADS // 64          # a wave owns a chunk at a time
GRID_STRIDE = WAVES * CHUNK             # slots one turn of the grid covers
SCAN_TURN = 1024                        # chunks per turn of the scan (load_scan_kernel)
LANES = {"fp32": 4, "fp64": 2}          # slots per 16-byte vector


def population(n=N, seed=11):
    """positions as fractions of the box in [0, 1), velocities in units of c; float64"""
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)), rng.normal(0, SIGMA, (n, 3))


# one term per axis code, three terms, seven terms; each also runs with outside=True, the starred ones with the id rule
ONE_TERM = [
    {"x": (0.25, 0.5)}, {"y": (None, 0.125)}, {"z": (0.75, None)}, {"vx": (0.01, None)}, {"vy": (None, -0.02)}, {"vz": (-0.01, 0.01)},
    {"v2": (0.002, None)},
]
THREE_TERMS = {"x": (0.1, 0.9), "vy": (-0.03, 0.03), "v2": (None, 0.004)}
SEVEN_TERMS = {"x": (0.05, 0.95), "y": (0.05, 0.95), "z": (0.05, 0.95), "vx": (-0.05, 0.05), "vy": (-0.05, 0.05), "vz": (-0.05, 0.05), "v2": (None, 0.006)}


def requests():
    out = []
    for where in ONE_TERM + [THREE_TERMS, SEVEN_TERMS]:
        for outside in (False, True):
            out.append(dict(where=where, every=None, outside=outside))
    for where in (ONE_TERM[0], ONE_TERM[6], THREE_TERMS, SEVEN_TERMS):
        for outside in (False, True):
            out.append(dict(where=where, every=(3, 1), outside=outside))
    out.append(dict(where=None, every=(5, 2), outside=False))      # no term: whoever the id rule passes
    return out


REQUESTS = requests()
ALL = dict(where=None, every=None, outside=False)                   # removes everybody
NONE = [dict(where=None, every=None, outside=True), dict(where={"vx": (10.0, None)}, every=None, outside=False),
        dict(where={"x": (None, None)}, every=(7, 3), outside=True)]   # remove nobody


def boundary_counts(precision):
    """the species sizes of the loop and chunk boundary cases (the two around a grid stride are cases of their own)"""
    lanes = LANES[precision]
    return [1, lanes - 1, lanes + 1, CHUNK - 1, CHUNK, CHUNK + 1, SCAN_TURN * CHUNK + 1]


def planted(n, precision):
    """the slots (= ids of a species as loaded) whose particle leaves in a boundary case of n particles: the first and the
    last slot of a chunk, a slot of the last partial vector, one alone in its chunk"""
    lanes = LANES[precision]
    slots = {0, n - 1, min(CHUNK - 1, n - 1), (n - 1) // lanes * lanes}
    if n > CHUNK:
        slots |= {CHUNK, (n - 1) // CHUNK * CHUNK}
    if n > 3 * CHUNK:
        slots |= {2 * CHUNK + 77, SCAN_TURN * CHUNK - 1}
    return np.array(sorted(s for s in slots if 0 <= s < n), dtype=np.int64)
