"""An independent reference for the energy and momentum diagnostics of the 3-D box (fpic_energy_now), built from the
definitions in include/fusionpic.h and the fixed-point contract of the particle pass, with numpy and the standard
library only: nothing here is imported from the library, its Python package or the oracle.

The particle pass promises exact sums: every term t of a species (|v|^2, vx, vy, vz, as doubles formed from the stored
values) becomes the integer floor(t * 2^80), and these integers are added without rounding.  So the reference holds
them as Python integers, converted to the nearest double as the kernel converts its 128-bit sum, and scaled the way the
host scales them.  Count, kinetic energy, momentum and speed_max are then predicted bit for bit.

Field sums are floating-point sums in a fixed order; the reference is the correctly rounded sum (math.fsum) of the same
float64 squares, against which a test allows the rounding of the kernel's summation depth."""
import math
from fractions import Fraction

import numpy as np

C = 2.998e8                       # the speed of light of the library (fes_host_push.inc.hpp, empic.js)
EPS0 = 8.8541878128e-12
MU0 = 1.0 / (EPS0 * C * C)        # as the host forms it
FIX_BITS = 80                     # resolution 2^-80
FIX_RANGE = 2.0 ** 15             # |term| < 2^15: a term times 2^32 particles stays below 2^127


# ---- floor(d * 2^80) as an exact integer
def fix_floor_scalar(d):
    """floor(d * 2^80) of one finite double, exactly (a Python integer)"""
    num, den = float(d).as_integer_ratio()
    return (num << FIX_BITS) // den


def fix_floor_fraction(d):
    """the same through fractions.Fraction: a second, independent route"""
    return math.floor(Fraction(float(d)) * (1 << FIX_BITS))


def _fix_parts(d):
    """d (finite float64) -> (t, sh), int64 arrays with floor(d * 2^80) = t * 2^sh, |t| < 2^53, 0 <= sh < 96"""
    d = np.ascontiguousarray(d, dtype=np.float64).ravel()
    if not np.all(np.isfinite(d)):
        raise ValueError("fix_floor: the terms must be finite")
    if np.any(np.abs(d) >= 2.0 ** 95):
        raise ValueError("fix_floor: |term| >= 2^95 is beyond what the decomposition handles")
    f, e = np.frexp(d)                                   # d = f * 2^e, 0.5 <= |f| < 1 (f = 0 for zeros)
    mant = (f * 2.0 ** 53).astype(np.int64)              # exact: a 53-bit integer
    s = e.astype(np.int64) - 53 + FIX_BITS               # d * 2^80 = mant * 2^s
    right = np.minimum(np.maximum(-s, 0), 63)            # (|mant| < 2^53: a shift by 63 leaves 0 or -1)
    t = mant >> right                                    # arithmetic shift: the floor for either sign
    return t, np.maximum(s, 0)


def fix_floor(d):
    """floor(d * 2^80) of every element of a finite float64 array, as a list of Python integers"""
    t, sh = _fix_parts(d)
    return [int(a) << int(b) for a, b in zip(t.tolist(), sh.tolist())]


def fix_sum(d):
    """sum over the array of floor(d * 2^80), exactly, as one Python integer — vectorised for tens of millions of terms.
    Each t (|t| < 2^53) is offset to t + 2^53 >= 0 and split into three 19-bit limbs; the limbs are summed per shift with
    np.bincount, whose float64 sums stay exact while they are below 2^53 (2^19 * 2^34 terms)."""
    t, sh = _fix_parts(d)
    if t.size == 0:
        return 0
    if t.size >= 1 << 34:
        raise ValueError("fix_sum: too many terms for exact limb sums")
    u = (t + (1 << 53)).astype(np.uint64)
    nb = int(sh.max()) + 1
    cnt = np.bincount(sh, minlength=nb)
    limbs = [np.bincount(sh, weights=((u >> np.uint64(19 * k)) & np.uint64((1 << 19) - 1)).astype(np.float64), minlength=nb)
             for k in range(3)]
    total = 0
    for b in range(nb):
        if cnt[b]:
            part = sum(int(limbs[k][b]) << (19 * k) for k in range(3)) - (int(cnt[b]) << 53)
            total += part << b
    return total


# ---- the 128-bit sum back to a double, as the kernel does it
def wrap128(s):
    """a Python integer as the kernel's 128-bit two's complement holds it"""
    s &= (1 << 128) - 1
    return s - (1 << 128) if s >> 127 else s


def from_fix(s):
    """the 128-bit sum s as the double nearest to s * 2^-80, ties to even: the kernel converts the magnitude in one
    rounding (its top 64 bits with a sticky bit for the rest) and scales by 2^-80 exactly; Python's int -> float rounds
    the same way"""
    return float(wrap128(int(s))) * 2.0 ** -FIX_BITS


# ---- one species' row
def v_squared(v):
    """|v|^2 of the stored velocities [n][3] as the kernel forms it: in float64, ((x*x + y*y) + z*z), no fused
    multiply-add"""
    v = np.asarray(v)
    x, y, z = (v[:, a].astype(np.float64) for a in range(3))
    return (x * x + y * y) + z * z


def species_sums(v):
    """{count, v2 (Python integer), m (three Python integers), v2max} of the stored velocities [n][3] (finite, in range)"""
    v = np.asarray(v)
    v2 = v_squared(v)
    return dict(count=int(v.shape[0]), v2=fix_sum(v2), m=[fix_sum(v[:, a].astype(np.float64)) for a in range(3)],
                v2max=float(v2.max()) if v2.size else 0.0)


def species_row(v, mass, W):
    """{count, kinetic, momentum[3], speed_max} as fpic_energy reports them, from the stored velocities: the host's
    scales 0.5 m W c c and m W c, formed left to right, times the converted sums; speed_max = sqrt(max |v|^2)"""
    s = species_sums(v)
    ke = 0.5 * mass * W * C * C
    pm = mass * W * C
    return dict(count=s["count"], kinetic=ke * from_fix(s["v2"]), momentum=np.array([pm * from_fix(m) for m in s["m"]]),
                speed_max=math.sqrt(s["v2max"]))


# ---- fields
def square_sum(*arrays):
    """the correctly rounded sum of the float64 squares of every element of the arrays (each square rounded once, as
    the kernel rounds it)"""
    parts = []
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).ravel()
        parts.append(a * a)
    return math.fsum(np.concatenate(parts)) if parts else 0.0


def field_e(E, dv):
    """0.5 eps0 dV sum |E|^2 over the given nodes (E: [..][3])"""
    return 0.5 * EPS0 * dv * square_sum(np.asarray(E)[..., :3])


def field_b(B, dv):
    """0.5 / mu0 dV sum |B|^2 over the given nodes"""
    return 0.5 / MU0 * dv * square_sum(np.asarray(B)[..., :3])
