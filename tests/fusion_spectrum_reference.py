"""The rule of the fusion product spectrum (fpic_fusion_spectrum) restated in numpy float64 and Python integers, from the text of
include/fusionpic.h and DESIGN.md 4.19.  It shares no code with the library: the pair sets and the integer q of every pair are
tests/fusion_reference.py's (the restatement of fpic_fusion, which the spectrum is defined on), Philox4x32-10 is
load_reference.py's, everything else is float64 in the stated operation order (numpy never fuses a multiply with an add; every
operation is one of + - x / sqrt, so the library can and must agree bit for bit), and the sums are Python integers.

    axis = request(m_a, m_b, axis="product", bins=.., lo=.., hi=.., q_value=.., product_mass=.., other_mass=.., los=None)
    out = apply(req, axis, ncells, cell_a, ids_a, v_a, cell_b, ids_b, v_b)     req: fusion_reference.request(...)
    out["bins"], out["under"], out["over"]     Python integers in units of 2**out["unit_exponent"] reactions
    out["x"], out["entry"], out["tries"]       per pair inside the table: the place on the axis (J), the entry it adds to and the
                                               try its direction took (isotropic product axis; else 0)
    and every key of fusion_reference.apply (pairs, below, above, cells, ..., reactions_exact, q, what, g, plan).
apply() asserts that no pair reaches the direction fallback (sixteen rejections) unless allow_fallback is set, so a comparison
with the library on its scenes is exact with no allowance.
"""
import numpy as np

import fusion_reference as ref
from load_reference import philox

CM, PRODUCT = 0, 1
AXES = {"cm": CM, "product": PRODUCT}
DIR_TAG = 0xF0520
DIR_SIDE = 16
BLOCKS = 8
TRIES = 2 * BLOCKS
BINS_MAX = 256
C = ref.C


def request(m_a, m_b, axis="product", bins=64, lo=0.0, hi=1.0, q_value=0.0, product_mass=None, other_mass=None, los=None):
    """the host's part of a request (rule_of): m_a, m_b the masses of species_a and species_b"""
    m_a, m_b, lo, hi, q_value = (float(x) for x in (m_a, m_b, lo, hi, q_value))
    M = m_a + m_b
    cc = C * C
    m_ab = (m_a * m_b) / M
    r = dict(axis=AXES[axis], bins=int(bins), lo=lo, hi=hi, inv_w=float(bins) / (hi - lo), f_a=m_a / M, f_b=m_b / M, hk=(0.5 * m_ab) * cc, q_value=q_value,
             kf=0.0, h3=0.0, n=None)
    if r["axis"] == PRODUCT:
        m3, m4 = float(product_mass), float(other_mass)
        r["kf"] = ((2.0 * m4) / (m3 * (m3 + m4))) / cc
        r["h3"] = (0.5 * m3) * cc
    if los is not None and any(float(x) != 0 for x in los):
        lx, ly, lz = (float(x) for x in los)
        norm = float(np.sqrt((lx * lx + ly * ly) + lz * lz))
        r["n"] = (lx / norm, ly / norm, lz / norm)
    return r


def edges(axis):
    return axis["lo"] + (axis["hi"] - axis["lo"]) * np.arange(axis["bins"] + 1, dtype=np.float64) / axis["bins"]


def unit_of(w):
    return ((np.asarray(w, dtype=np.float64) + 0.5) * 2.0 ** -31) - 1.0


def try_direction(wa, wb):
    """one try each: (taken, n) with n (m, 3), rows of rejected tries undefined"""
    x1, x2 = unit_of(wa), unit_of(wb)
    s = x1 * x1 + x2 * x2
    ok = s < 1.0
    r = np.sqrt(np.where(ok, 1.0 - s, 0.0))
    return ok, np.stack([(2.0 * x1) * r, (2.0 * x2) * r, 1.0 - (2.0 * s)], axis=1)


def directions(req, ids, side_b):
    """the isotropic directions of the pairs whose owners have the ids `ids`; side_b: the owner is of species_b of an unlike
    request.  Returns n (m, 3) and the try that was taken (TRIES: the fallback (0, 0, 1))"""
    ids = np.asarray(ids, dtype=np.uint64)
    tag = DIR_TAG + DIR_SIDE * np.asarray(side_b, dtype=np.uint64)
    n = np.tile(np.array([0.0, 0.0, 1.0]), (len(ids), 1))
    tries = np.full(len(ids), TRIES, dtype=np.int64)
    for a in range(BLOCKS):
        w = philox(ids, req["epoch"], req["stream"], tag + np.uint64(a), req["seed_lo"], req["seed_hi"])
        for t, (wa, wb) in enumerate(((w[0], w[1]), (w[2], w[3]))):
            ok, cand = try_direction(wa, wb)
            take = ok & (tries == TRIES)
            n[take] = cand[take]
            tries[take] = 2 * a + t
    return n, tries


def cm_energy(axis, g):
    return axis["hk"] * (g * g)


def product_energy(axis, K, f_o, f_p, vo, vp, n):
    """f_o, f_p arrays (m,), vo, vp, n arrays (m, 3)"""
    et = axis["q_value"] + K
    et = np.where(et > 0, et, 0.0)
    u3 = np.sqrt(et * axis["kf"])
    w = [(f_o * vo[:, i] + f_p * vp[:, i]) + u3 * n[:, i] for i in range(3)]
    return axis["h3"] * ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])


def entry_of(axis, x):
    """0 .. bins - 1 the bins, bins: under, bins + 1: over"""
    x = np.asarray(x, dtype=np.float64)
    bins = axis["bins"]
    with np.errstate(invalid="ignore"):
        under, over = x < axis["lo"], ~(x < axis["hi"])
        t = np.where(under | over, 0.0, (x - axis["lo"]) * axis["inv_w"])
    k = np.minimum(t.astype(np.int64), bins - 1)
    return np.where(under, bins, np.where(over, bins + 1, k))


def pair_places(req, axis, g, ids_o, side_b, vo, vp):
    """one pair each: g as fusion_reference.tally returns it, the owner's id, whether the owner is of species_b of an unlike
    request, the float64 velocities (m, 3).  Returns x (J) and the try the direction took (0 where none is drawn)"""
    K = cm_energy(axis, np.asarray(g, dtype=np.float64))
    tries = np.zeros(len(K), dtype=np.int64)
    if axis["axis"] == CM:
        return K, tries
    side_b = np.asarray(side_b, dtype=bool) & (not req["like"])
    f_o = np.where(side_b, axis["f_b"], axis["f_a"])
    f_p = np.where(side_b | req["like"], axis["f_a"], axis["f_b"])
    if axis["n"] is None:
        n, tries = directions(req, ids_o, side_b)
    else:
        n = np.tile(np.array(axis["n"], dtype=np.float64), (len(K), 1))
    return product_energy(axis, K, f_o, f_p, np.asarray(vo, dtype=np.float64), np.asarray(vp, dtype=np.float64), n), tries


def places(req, axis, out, ids, v, na):
    """the pairs of a fusion_reference.apply() that are inside the table: (x, tries, index into the pairs); ids and v are the
    concatenation (species a, then species b), na the number of species a's"""
    plan = out["plan"]
    inside = np.flatnonzero(out["what"] == 0)
    owner, partner = plan["owner"][inside], plan["partner"][inside]
    v = np.asarray(v, dtype=np.float64)
    x, tries = pair_places(req, axis, out["g"][inside], np.asarray(ids, dtype=np.uint64)[owner], owner >= na, v[owner], v[partner])
    return x, tries, inside


def apply(req, axis, ncells, cell_a, ids_a, v_a, cell_b=None, ids_b=None, v_b=None, allow_fallback=False, tally=None):
    """the whole spectrum on stored velocities; tally: the fusion_reference.apply() of the same arguments, if at hand"""
    out = dict(tally if tally is not None else ref.apply(req, ncells, cell_a, ids_a, v_a, cell_b, ids_b, v_b))
    bins = axis["bins"]
    sums = [0] * (bins + 2)
    if "plan" in out:
        like = req["like"]
        ids = np.asarray(ids_a, dtype=np.uint64) if like else np.concatenate([np.asarray(ids_a, dtype=np.uint64), np.asarray(ids_b, dtype=np.uint64)])
        v = (np.asarray(v_a) if like else np.concatenate([v_a, v_b])).astype(np.float64)
        x, tries, inside = places(req, axis, out, ids, v, len(ids_a))
        assert allow_fallback or not (tries == TRIES).any()
        entry = entry_of(axis, x)
        for k, i in zip(entry.tolist(), inside.tolist()):
            sums[k] += out["q"][i]
        out.update(x=x, entry=entry, tries=tries, inside=inside)
    assert sum(sums) == out["reactions_exact"]
    out.update(bins=sums[:bins], under=sums[bins], over=sums[bins + 1], edges=edges(axis))
    return out
