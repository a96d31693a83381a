"""Scenes of the ionisation tests (tests/test_ionize_reference.py on the CPU, where their conditions are checked;
tests/test_ionize_host.py; tests/test_gpu_ionize.py on the GPU): the requests, the projectile counts, and the event counts
that straddle the passes' boundaries.  The particles are those of the gas operator's scenes (test_gas_reference.scene: stored
fractions on a 2^-20 grid of a box with power-of-two edges, velocities exact in float32, so a handle of either precision
stores exactly what the reference is given).  The launch shapes are read from the kernel headers, so a change of them moves
the boundary cases with it."""
import os
import re

import numpy as np

import ionize_reference as ref
from helpers import ROOT
from test_gas_reference import (BACKGROUND, DT, G_HI, G_LO, L, ME, P30, QE, SHAPE, TABLE, TAPERS, WINDOW, WINDOW_WIDE, big_n, compact_range, density_for, scene,
                                window_first_max)

CSRC = os.path.join(ROOT, "fusion-sim_amd", "csrc")


def _constant(header, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, header)).read()).group(1))


GAS_THREADS = _constant("fes_gas_kernels.hpp", "kGasThreads")           # the deciding pass has gas_kernel's shape
GAS_BLOCKS = _constant("fes_gas_kernels.hpp", "kGasBlocks")
THREADS = _constant("fes_ionize_kernels.hpp", "kIonizeThreads")         # the generation pass: an event per lane
BLOCKS = _constant("fes_ionize_kernels.hpp", "kIonizeBlocks")
SCAN_CHUNK = 32 * _constant("fes_remove_kernels.hpp", "kRenumberChunk")  # ids per chunk of the popcount scan
VECTOR, WAVE, QUEUE = 4, 64, 4 * GAS_THREADS                             # a lane's group, a wave, the hand-out queue of one turn

MI = 1836.0 * ME
THR = 0.04                                       # g_threshold of most scenes: below the table's first speed
N_BIG = big_n()                                  # just above one full trip of the deciding pass's grid
SIZES = [1, 3, 4, 5, 255, 257, 1023, 1025, 100003]


def ion(K, seed, stream=0, epoch=0, sigma=TABLE, g_lo=G_LO, g_hi=G_HI, g_threshold=THR, **kw):
    """the keywords of a request, as both the wrapper and the reference take them (but species, electron, ion)"""
    out = dict(g_threshold=g_threshold, density=density_for(K, sigma, g_lo, g_hi), tau=DT, sigma=sigma, g_lo=g_lo, g_hi=g_hi, seed=seed, stream=stream, epoch=epoch,
               **BACKGROUND)
    out.update(kw)
    return out


FLAT = np.full(2, 3.0e-19)
# everybody is a candidate (P_max = 1) and the acceptance is g / g_hi: about a third of the projectiles have an event
DENSE = dict(ion(P30, 0x1051E0AA, stream=2, epoch=6, sigma=FLAT, g_lo=THR, g_hi=0.5), density=1e32)

SCENES = {
    # the window first (0.375 of the box), the wave-shared loop (K above the queue's range), both tapers
    "window": ion(P30, 0x1051E00123456789, stream=5, epoch=3, taper=TAPERS, **WINDOW),
    # the word first on the whole box, through the queue (K = 2^27 lies in its range)
    "whole": ion(2.0 ** 27, 0x1051E00123456790, stream=6, epoch=4),
    # the table starts AT the threshold
    "at threshold": ion(P30, 0x1051E00123456791, stream=7, epoch=5, g_threshold=G_LO, taper=(None, TAPERS[2], None), **WINDOW_WIDE),
    "dense": DENSE,
}
# few candidates: with these epochs the reference has exactly no event (but candidates), and exactly one, among scene(1025)
SPARSE_N = 1025
SPARSE = {"no event": ion(2.0 ** 32 * 4e-3, 0x1051E0BB, stream=3, epoch=0), "one event": ion(2.0 ** 32 * 4e-3, 0x1051E0BB, stream=3, epoch=1)}
# event counts past a lane's vector, a wave, a workgroup of the generation pass, the queue's entries; the last two with ids in
# more than one chunk of the popcount scan, and id spans that are no multiple of 32
DENSE_SIZES = [30, 300, 1101, 4101]
EVENT_BOUNDS = [VECTOR, WAVE, THREADS, QUEUE]


def threshold_scenes():
    """requests on either side of every threshold the host chooses a form by: K just below, just above and between the two
    ends of the queue's range, in a window on either side of kGasWindowFirstMax and on the whole box (the gas pass's grid)"""
    lo, hi = compact_range()
    out = {}
    for k, target in enumerate((lo * 0.999, lo * 1.001, (lo * hi) ** 0.5, hi * 0.999, hi * 1.001)):
        for w, (name, window) in enumerate((("narrow", WINDOW), ("wide", WINDOW_WIDE), ("whole", {}))):
            out["K %d %s" % (k, name)] = ion(target, 0x1051E0C0DE + 16 * k + w, stream=8, epoch=1, taper=TAPERS if w != 1 else (None, None, None), **window)
    return out


THRESHOLD_SCENES = threshold_scenes()
THRESHOLD_N = 100003                             # (the smallest K is 2^24 (1 - 0.001): a few hundred candidates, some events)
_reference = {}


def keywords(name):
    return SCENES.get(name) or SPARSE.get(name) or THRESHOLD_SCENES[name]


def reference(name, n):
    """(request, what the reference gives for scene(n) with ids 0 .. n-1) of a scene: computed once, shared, unchanged"""
    key = (name, n)
    if key not in _reference:
        req = ref.request(L, **keywords(name))
        frac, vel = scene(n)
        _reference[key] = (req, ref.apply(req, np.arange(n), frac, vel))
    return _reference[key]


def exact_cases():
    """every (scene, n) the GPU test compares exactly"""
    cases = [(name, n) for name in ("window", "whole", "at threshold") for n in SIZES + ([N_BIG] if name != "at threshold" else [])]
    cases += [("dense", n) for n in DENSE_SIZES] + [(name, SPARSE_N) for name in SPARSE] + [(name, THRESHOLD_N) for name in THRESHOLD_SCENES]
    return cases
