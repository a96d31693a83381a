"""The rounded parts of the loader's rule — the three normals of the Box-Muller transform and the sine of the phase — evaluated
with 50 digits by mpmath from the same exact inputs (the random words; the float64 phase), and the deviation of a float64
result from them in ulps.  Used by tests/test_load_reference.py (the numpy reference against these values) and by
scripts/probe_load.py (the kernel against them); the bound of tests/test_gpu_load.py is built from the two deviations."""
import numpy as np

import load_reference as ref

ULP_PARTICLES = 100000


def ulp_scene(L):
    """the request whose first ULP_PARTICLES particles the deviations are measured on: whole box, a mode along x and z"""
    return ref.request(L, seed=0x0123456789ABCDEF, stream=7, mode=(3, 0, -2), xphase=0.125, vphase=0.3125)


def exact_normals_and_sines(req, i):
    """(hi, lo): float64 arrays [n][4] whose sum is the 50-digit value of n0, n1, n2 and sinpi(2 (theta + vphase)), theta
    being the float64 phase of the reference (exact inputs: only the functions are in question)"""
    import mpmath
    i = np.asarray(i, dtype=np.uint64)
    w = [x.astype(np.uint64) for x in ref.philox(i & ~np.uint64(1) if req["paired"] else i, req["stream"], 1, ref.TAG, req["seed_lo"], req["seed_hi"])]
    _, theta = ref.base(req, i)
    arg = 2.0 * (theta + req["vphase"])
    hi, lo = np.empty((len(i), 4)), np.empty((len(i), 4))
    with mpmath.workdps(50):
        two32 = mpmath.mpf(2) ** 32
        for k in range(len(i)):
            r1 = mpmath.sqrt(-2 * mpmath.log((mpmath.mpf(int(w[0][k])) + 0.5) / two32))
            r3 = mpmath.sqrt(-2 * mpmath.log((mpmath.mpf(int(w[2][k])) + 0.5) / two32))
            u2, u4 = mpmath.mpf(int(w[1][k])) / two32, mpmath.mpf(int(w[3][k])) / two32
            vals = (r1 * mpmath.cospi(2 * u2), r1 * mpmath.sinpi(2 * u2), r3 * mpmath.cospi(2 * u4), mpmath.sinpi(mpmath.mpf(float(arg[k]))))
            for c, v in enumerate(vals):
                hi[k, c] = float(v)
                lo[k, c] = float(v - mpmath.mpf(hi[k, c]))
    return hi, lo


def ulps(got, hi, lo):
    """|got - (hi + lo)| in units of the spacing of float64 at |hi| (got - hi is exact for neighbours of hi)"""
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo) / np.spacing(np.maximum(np.abs(hi), np.finfo(np.float64).tiny))
