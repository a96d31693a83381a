"""The rule of the particle sources (fpic_inject; include/fusionpic.h) in numpy and Python integers, nothing of the library.
Written from the header's text.  Both kinds are built on the loader's restatement (tests/load_reference.py: the words, the
fractions, the positions, the Box-Muller parts), imported and not copied; the tallies are the sinks' exact integers
(tests/remove_reference.py: floor(q 2^80) of the stored velocity components and of the squared norm formed in float64).

    req = request(L, dt, kind="flux", axis=2, side=-1, plane=0.5 * L[2], seed=..., stream=..., lo=..., hi=..., drift=..., vth=...)
    j = sequence(first, count, k=3, epoch=0)                 the sequence numbers of application k
    pos, vel = stored(req, j, np.float32)                    what a handle of that precision holds for them
    application(req, j, dtype, mass=, charge=, weight=)      the result dict of fpic_inject for them"""
import numpy as np

import load_reference as lr
import remove_reference as rr

C = 2.998e8           # the push's speed of light
ID_END = (1 << 32) - 1      # fpic_load's bound on 32-bit indices: first + count <= 2^32 - 1


def request(L, dt, kind="volume", axis=0, side=0, plane=0.0, **load):
    """the host's part of a request: the loader's (load_reference.request) and, for a flux source, the plane and the step in
    box fractions; its normal axis reads the time fraction where the loader reads a position (lo 0, width 1)"""
    assert kind in ("volume", "flux")
    req = dict(lr.request(L, **load), kind=kind)
    if kind == "flux":
        assert axis in (0, 1, 2) and side in (1, -1) and not req["paired"]
        assert req["drift"][axis] == 0 and not np.any(req["m"]) and not np.any(req["xamp_f"]) and not np.any(req["vamp"])
        La = float(lr._three(L)[axis])
        assert 0.0 <= plane <= La
        lo_f, w_f = req["lo_f"].copy(), req["w_f"].copy()
        lo_f[axis], w_f[axis] = 0.0, 1.0
        t1, t2 = [a for a in range(3) if a != axis]
        step = dt * C
        req.update(axis=axis, t1=t1, t2=t2, side=float(side), plane_f=plane / La, step_f=step / La, lo_f=lo_f, w_f=w_f)
    return req


def sequence(first, count, k=0, epoch=0):
    """the sequence numbers of application k of a registration (k counts from the epoch on); None if first + count would pass 2^32 - 1"""
    at = first + (epoch + k) * count
    if at + count > ID_END:
        return None
    return np.arange(at, at + count, dtype=np.uint64)


def fits(n, capacity, id_span, count):
    return n + count <= capacity and id_span + count <= ID_END


def states(req, j):
    """float64 positions (box fractions, before the cast and the wrap) and velocities (units of c) of the sequence numbers j"""
    j = np.asarray(j, dtype=np.uint64)
    if req["kind"] == "volume":
        return lr.positions(req, j), lr.velocities(req, j)
    p, _ = lr.base(req, j)
    r1, c, s, r3, _ = lr.normal_parts(req, j)
    n0, n1 = r1 * c, r1 * s
    ax, t1, t2 = req["axis"], req["t1"], req["t2"]
    v = np.empty_like(p)
    v[:, t1] = req["drift"][t1] + req["vth"][t1] * n0
    v[:, t2] = req["drift"][t2] + req["vth"][t2] * n1
    v[:, ax] = req["side"] * (req["vth"][ax] * r3)
    ft = p[:, ax].copy()
    d = v[:, ax] * req["step_f"]
    e = d * ft
    p[:, ax] = req["plane_f"] + e
    return p, v


def normal_speed(req, j):
    """the Rayleigh deviate s of a flux source's sequence numbers"""
    return lr.normal_parts(req, j)[3]


def stored(req, j, dtype):
    p, v = states(req, j)
    return lr.wrap01(p.astype(dtype)), v.astype(dtype)


def application(req, j, dtype, mass=1.0, charge=1.0, weight=1.0):
    """the result of one application that injects the sequence numbers j into a handle of precision dtype"""
    _, vel = stored(req, j, dtype)
    sums, nan = rr.tally(vel, np.ones(len(vel), dtype=bool))
    ke, pm = 0.5 * mass * weight * C * C, mass * weight * C
    n = len(vel)
    return {"applications": 1, "injected": n, "energy_fixed": sums[0], "momentum_fixed": sums[1:],
            "energy": float("nan") if nan[0] else ke * rr.fixed_to_double(sums[0]),
            "momentum": [float("nan") if nan[1 + a] else pm * rr.fixed_to_double(sums[1 + a]) for a in range(3)],
            "charge": (float(n) * charge) * weight}


def add_results(parts):
    """the totals of several applications of one source (the doubles are not formed: compare the integers)"""
    return {"applications": sum(p["applications"] for p in parts), "injected": sum(p["injected"] for p in parts),
            "energy_fixed": sum(p["energy_fixed"] for p in parts), "momentum_fixed": [sum(p["momentum_fixed"][a] for p in parts) for a in range(3)]}


def tally_fast(vel):
    """rr.tally over every row for a LARGE array, the same exact integers: a finite float64 q is m 2^e with a 53-bit integer m,
    so floor(q 2^80) is m shifted by e + 80 — left exactly, right with the floor an arithmetic shift makes.  The terms are
    summed per shift in two 27-bit halves (no 64-bit overflow below 2^36 rows).  Values must lie inside the fixed-point range."""
    v = np.asarray(vel).astype(np.float64)
    v2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    sums = []
    for col in (v2, v[:, 0], v[:, 1], v[:, 2]):
        assert np.all(np.isfinite(col)) and np.all(np.abs(col) < rr.FIX_RANGE)
        frac, exp = np.frexp(col)
        m = (frac * 2.0 ** 53).astype(np.int64)          # exact: |frac| in [0.5, 1) or 0
        shift = exp.astype(np.int64) - 53 + 80
        total = 0
        for s in np.unique(shift):
            part = m[shift == s]
            if s < 0:
                part = part >> np.int64(min(-int(s), 63))      # floor
                s = 0
            hi, lo = part >> np.int64(27), part & np.int64((1 << 27) - 1)
            total += ((int(hi.sum()) << 27) + int(lo.sum())) << int(s)
        sums.append(total)
    return sums
