"""The rule of the prescribed external forces (fpic_force) restated in plain numpy, from the text of include/fusionpic.h and
DESIGN.md 4.22.  It shares no code with the library: float64 throughout in the stated operation order (numpy never fuses a
multiply with an add), cospi from tests/load_reference.py, the exact integer sums from tests/energy_reference.py.

    req = request(L, dt, charge, mass, waves=[dict(amp=..., mode=..., nu=..., phase=...)], kind=FIELD, lo=..., hi=...,
                  taper=(None, tab, None), envelope=dict(start=, stop=, values=), epoch=...)
    out = kicked(req, count, position, velocity)   position: stored box fractions, velocity: stored, units of c
    out["inside"], out["v"] (float64 v' of every particle; a particle outside keeps v), out["active"]
    stored(req, count, position, velocity)         v' cast to the dtype of `velocity`; outside: the same bits
    tallies(before, after, inside)                 the exact integers work_fixed, impulse_fixed[3] and `kicked`
    derived(t, mass, W)                            work (J), impulse (kg m/s)

`count` is the handle's sub-step count at the application; s = (count + epoch) mod 2^64."""
import math

import numpy as np

import energy_reference as eref
from load_reference import cospi

FIELD, ACCEL = 0, 1
C = 2.998e8
FOREVER = (1 << 64) - 1
MAX_WAVES, MAX_OPS, TABLE_MAX = 4, 8, 1025


def _three(v):
    return np.array([v, v, v] if np.ndim(v) == 0 else list(v), dtype=np.float64)


def request(L, dt, charge, mass, waves, kind=FIELD, lo=None, hi=None, taper=(None, None, None), envelope=None, epoch=0):
    L = _three(L)
    lo = np.zeros(3) if lo is None else _three(lo)
    hi = L.copy() if hi is None else _three(hi)
    ws = []
    for w in waves:
        ws.append(dict(amp=_three(w["amp"]), mode=np.array(w.get("mode", (0, 0, 0)), dtype=np.float64), nu=float(w.get("nu", 0.0)), phase=float(w.get("phase", 0.0))))
    assert 1 <= len(ws) <= MAX_WAVES
    env = dict(start=0, stop=FOREVER, values=None)
    if envelope is not None:
        env = dict(start=int(envelope.get("start", 0)), stop=int(envelope.get("stop", FOREVER)),
                   values=None if envelope.get("values") is None else np.asarray(envelope["values"], dtype=np.float64))
    kq = dt / C if kind == ACCEL else (charge * dt) / (mass * C)
    lo_f, hi_f = lo / L, hi / L
    return dict(kind=kind, kq=float(kq), lo_f=lo_f, hi_f=hi_f, w=hi_f - lo_f, waves=ws, epoch=int(epoch), envelope=env,
                taper=[None if t is None else np.asarray(t, dtype=np.float64) for t in taper])


def s_of(req, count):
    return (int(count) + req["epoch"]) & FOREVER


def active(req, count):
    return req["envelope"]["start"] <= s_of(req, count) <= req["envelope"]["stop"]


def lookup(tab, f):
    """a table of K + 1 nodes at the fractions f of its span: g = f K, j = min((int) g, K - 1), s = g - j,
    tab[j] + (tab[j+1] - tab[j]) s.  Returns (value, j)."""
    tab = np.asarray(tab, dtype=np.float64)
    K = tab.size - 1
    g = np.asarray(f, dtype=np.float64) * float(K)
    j = np.minimum(np.trunc(g).astype(np.int64), K - 1)
    s = g - j.astype(np.float64)
    return tab[j] + (tab[j + 1] - tab[j]) * s, j


def envelope_value(req, count):
    e = req["envelope"]
    if e["values"] is None:
        return 1.0
    s = s_of(req, count)
    g = np.float64(float(s - e["start"]) * float(e["values"].size - 1)) / np.float64(float(e["stop"] - e["start"]))
    return float(lookup_at(e["values"], g))


def lookup_at(tab, g):
    """the same interpolation at the node coordinate g (the envelope forms g itself)"""
    K = tab.size - 1
    j = min(int(g), K - 1)
    r = np.float64(g) - np.float64(j)
    return tab[j] + (tab[j + 1] - tab[j]) * r


def tfrac(req, count):
    s = float(s_of(req, count))                       # (double) s: the nearest double of the 64-bit integer
    out = []
    for w in req["waves"]:
        tw = np.float64(w["nu"]) * np.float64(s)
        out.append(float(tw - np.floor(tw)))
    return out


def inside(req, position):
    p = np.asarray(position).astype(np.float64)
    return np.all((req["lo_f"] <= p) & (p < req["hi_f"]), axis=1)


def taper_value(req, position):
    """(taper, j per axis) at every position (meaningful for particles inside); no table anywhere: None"""
    p = np.asarray(position).astype(np.float64)
    t, js, first = None, [None, None, None], True
    for a in range(3):
        if req["taper"][a] is None:
            continue
        f = (p[:, a] - req["lo_f"][a]) / req["w"][a]
        val, js[a] = lookup(req["taper"][a], f)
        t = val if first else t * val
        first = False
    return t, js


def cosines(req, count, position):
    """c_k of every wave at every position: [n][nwaves]"""
    p = np.asarray(position).astype(np.float64)
    out = []
    for w, tf in zip(req["waves"], tfrac(req, count)):
        m = w["mode"]
        theta = (m[0] * p[:, 0] + m[1] * p[:, 1]) + m[2] * p[:, 2]
        arg = (theta - tf) + w["phase"]
        out.append(cospi(2.0 * arg))
    return np.stack(out, axis=1)


def kicked(req, count, position, velocity):
    v = np.asarray(velocity).astype(np.float64)
    n = v.shape[0]
    if not active(req, count):
        return dict(active=False, inside=np.zeros(n, dtype=bool), v=v.copy(), d=np.zeros_like(v))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ins = inside(req, position)
        c = cosines(req, count, position)
        e = req["waves"][0]["amp"][None, :] * c[:, 0:1]
        for k in range(1, len(req["waves"])):
            e = e + req["waves"][k]["amp"][None, :] * c[:, k:k + 1]
        scale = np.float64(req["kq"]) * np.float64(envelope_value(req, count))
        t, js = taper_value(req, position)
        sc = np.full(n, scale) if t is None else scale * t
        d = sc[:, None] * e
        out = v + d
    out[~ins] = v[~ins]
    d[~ins] = 0
    return dict(active=True, inside=ins, v=out, d=d, c=c, e=e, sc=sc, scale=float(scale), taper=t, taper_j=js)


def stored(req, count, position, velocity):
    """what the handle holds afterwards, in the dtype of `velocity`; a particle outside keeps its bits"""
    velocity = np.asarray(velocity)
    k = kicked(req, count, position, velocity)
    out = velocity.copy()
    out[k["inside"]] = k["v"][k["inside"]].astype(velocity.dtype)
    return out, k


def tallies(before, after, ins):
    """the exact tallies of one application from the stored velocities before and after it and who was inside"""
    b, a = np.asarray(before)[ins], np.asarray(after)[ins]
    work = eref.fix_sum(eref.v_squared(a)) - eref.fix_sum(eref.v_squared(b)) if b.size else 0
    imp = [eref.fix_sum(a[:, k].astype(np.float64)) - eref.fix_sum(b[:, k].astype(np.float64)) if b.size else 0 for k in range(3)]
    return dict(kicked=int(np.count_nonzero(ins)), work_fixed=work, impulse_fixed=imp)


def derived(t, mass, W):
    """work and impulse as the library reports them: the scales of the energy diagnostics (formed left to right) times the
    double nearest to the sum 2^-80"""
    ke, pm = 0.5 * mass * W * C * C, mass * W * C
    return dict(work=ke * eref.from_fix(t["work_fixed"]), impulse=[pm * eref.from_fix(x) for x in t["impulse_fixed"]])


def add_tallies(a, b):
    return dict(kicked=a["kicked"] + b["kicked"], work_fixed=a["work_fixed"] + b["work_fixed"],
                impulse_fixed=[x + y for x, y in zip(a["impulse_fixed"], b["impulse_fixed"])])


ZERO = dict(kicked=0, work_fixed=0, impulse_fixed=[0, 0, 0])
