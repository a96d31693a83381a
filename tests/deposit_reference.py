"""Plain numpy reference of the (r,z) deposit, stage by stage, independent of the oracle and of the product: no ctypes, no
import of either.  Written from DESIGN section 2 / 4.6, the header comments of csrc/fpic_kernels.hpp (deposit_cell,
raster_first, cic_sums_kernel, stamp_finish_kernel) and include/fusionpic.h (FPIC_BUF_CELL_SUMS).

Inputs: the stored, normalised particle state as getParticles() returns it in the handle's precision T (float32 or float64),
nr, nz, and the 11 x 11 stamp of tests/golden/stamp.json.  Decisions (which cell, clipped or not) are taken in T, one IEEE
rounding per operation, as the definition says; everything that is a VALUE is computed in numpy's long double (64-bit
mantissa on x86: its own error is 2^-11 of a float64 rounding and is left out of the bounds).

Stages
  cells    ideal: r = sqrt(x*x + y*y), clipped unless 0 <= r <= 1 and 0 <= z <= 1 (NaN is clipped), ic = trunc(r nr),
           jc = trunc(z nz); r == 1 lands on column nr, z == 1 on row nz.  Rasterised (b sub-pixel bits): the fixed-point
           rule above raster_first, centre = first + 5 in -5 .. nr+5 / -5 .. nz+5, dropped only when nothing of the sprite
           reaches the grid (and for a coordinate that is not finite).
  stage 1  per-cell sums on the (nr+11) x (nz+11) apron grid, cell (ic, jc) at [jc + 5, ic + 5]: the count as an exact
           integer, the colour 0.001 (v_r, v_theta, v_z) with v_r = (vx x + vy y) / r, v_theta = (vy x - vx y) / r and 0.001
           the constant of T.  r == 0 gives NaN in channels 0 and 1 of its cell and finite values in 2 and 3.
           shape 'cic': the colour (count channel included) times the bilinear weights around (r nr - 0.5, z nz - 0.5) on
           the four cell centres; corners outside 0 .. nr-1 / 0 .. nz-1 are dropped, nothing lies on the apron.
  stage 2  moments = stamp (*) sums, cropped at the grid's edges; apron cells contribute to the grid cells in reach; a NaN
           cell makes its whole 11 x 11 footprint NaN (0 x NaN).  'cic': the sums grid is the moments grid.
  stage 3  norm = 1000 (m_c / m_3 for c < 3, m_3 itself) 0.5 / x_c where m_3 > 0, else 0; x_c = (i + 0.5) / nr.
  stage 4  avg = ratio norm + (1 - ratio) avg_prev, ratio = 0.01 in T.

Bounds (eps = machine epsilon of T; one rounded operation errs by at most eps/2 of its result, every count K below is a
count of rounded operations charged a whole eps each, so each bound has a factor of two in hand and no fitted constant)

  stage 1, count   equal as integers.  The device holds the sum of 0.001's: |sum / 0.001 - rint| < 0.25 is asserted so that
                   the rounding cannot hide a half.  A chain of k float additions of 0.001 is off by at most k^2 eps / 2 of
                   one 0.001: < 0.06 for k <= 1000 in float32, which is why assert_cell_population() refuses a scene with
                   more than 1000 particles in one cell.
  stage 1, colour  |got - want| <= (K + n_cell) eps M_cell, per cell and channel.
                   M_cell = sum over the cell's particles of m_p, with m_p = 0.001 (|vx x| + |vy y|) / r for channel 0,
                   0.001 (|vy x| + |vx y|) / r for channel 1 and 0.001 |v_z| for channel 2.  (First proposed: sum |c_p|.  v_r and v_theta are differences:
                   their rounding errors scale with the terms, not with what is left after they cancel, so m_p takes the
                   terms.  m_p >= |c_p|.)
                   K = 8 for channels 0 and 1: x*x, y*y, their sum, sqrt, x/r, vx*(x/r), the sum of two products, * 0.001.
                   K = 1 for channel 2.
                   n_cell, the number of particles in the cell, stands for P, the number of floating additions into the
                   cell's global word.  Each work item whose window holds the cell converts its (double) window sum to T
                   and adds it once: two roundings of at most eps/2 of a partial sum <= M_cell each, and it has at least
                   one particle in the cell; each spilled particle is one addition.  So P <= n_cell always.  (First
                   proposed: the tighter 'work items that can reach the cell' when stats()['deposit_spilled'] is 0.  The
                   code says otherwise: a re-binning launch sums against the windows of the OLD tiles and does not record
                   its spill count, and the adaptive policy reads the count with a lag, so the statistic cannot certify
                   that nothing spilled.)  In float64 the window's own double additions round too: n_cell eps/2, which the
                   whole eps charged per addition covers.
  stage 1, 'cic'   |got - want| <= eps sum_p m_p ((K + 2 + n_cell) w_p + nr wz_p + nz wr_p), with m_p = 0.001 for the
                   count channel and K = 0 there.  The two products colour * (wr * wz) are the + 2.  The weights are NOT
                   known to a relative eps (first proposed: 'two more roundings in K'): gi = fl(fl(r nr) - 0.5) carries
                   an ABSOLUTE error of up to eps nr / 2 + eps nr / 2, so wr = gi - floor(gi) (an exact subtraction) is off
                   by up to eps nr whatever its size, likewise wz by eps nz; the deposit is continuous in gi, gj across
                   cell boundaries and the grid's edge, so the same bound holds where floor() falls the other way.
                   r is taken as the definition computes it, in T.
  stage 2          |got - want| <= (121 + 2) eps sum |w s| + 123 tiny, per cell and channel, from the device's own sums:
                   121 additions, the product and the conversion of the weight.  tiny (the smallest normal of T) covers
                   products of the stamp's outermost ring (1.6e-34) that underflow; it is 1e-38 in float32.  The sets of NaN
                   cells and of touched cells (m_3 > 0) must be equal.
  stage 3          |got - want| <= 4 eps |want|: m_c / m_3, * 1000, x_c = (i + 0.5) / nr, / x_c (* 0.5 is exact).
  stage 4          |got - want| <= 4 eps (|ratio norm| + |(1 - ratio) avg_prev|): 1 - ratio, two products, one sum.
  the CPU oracle   blends particle by particle in T, so its moments are held to stage 1 and 2 in one:
                   (K + 2 + N_f) eps (stamp (*) M) with N_f the number of particles whose footprint holds the cell
                   (one product and one addition each, in N_f's place stood 121 above).
"""
import json
import os

import numpy as np

APRON = 5                # cells around the grid that a rasterised sprite's centre can have
REACH = 5                # (11 - 1) / 2
SIDE = 11
CELL_LIMIT = 1000        # particles per cell up to which the count's read-back is provably exact
K_COLOUR = (8, 8, 1, 0)  # rounded operations of one particle's colour, per channel
W = np.longdouble        # working type of every value of the reference

assert np.finfo(W).eps < 1e-18, "the reference needs a long double wider than float64"


def load_stamp():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stamp.json")) as f:
        s = json.load(f)
    assert s["nshape"] == SIDE
    w = np.asarray(s["red"], dtype=np.float64)
    assert w.size == SIDE * SIDE and np.array_equal(w, w.astype(np.float32).astype(np.float64))   # float32 values
    return w.reshape(SIDE, SIDE)     # [row from the top][column]: weight[(di + 5) + 11 (5 - dj)]


def real(precision):
    return {"fp32": np.float32, "fp64": np.float64}[precision]


def eps(T):
    return float(np.finfo(T).eps)


def milli(T):
    """0.001 as T holds it"""
    return W(T(0.001))


# ------------------------------------------------------------------ cells
def radius(pos, T):
    """r as the definition computes it: three operations in T"""
    p = np.asarray(pos, dtype=T)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(all="ignore"):
        return np.sqrt(x * x + y * y)


def ideal_cells(pos, nr, nz, T, variant=None):
    """(ic, jc, visible): ic in 0 .. nr, jc in 0 .. nz where visible.  (variant: the deliberately wrong forms 'round' and
    'clip_r1' that tests/test_deposit_reference.py shows to be caught.)"""
    p = np.asarray(pos, dtype=T)
    r, z = radius(p, T), p[:, 2]
    cut = np.rint if variant == "round" else np.trunc
    with np.errstate(all="ignore"):
        visible = (r >= 0) & ((r < 1) if variant == "clip_r1" else (r <= 1)) & (z >= 0) & (z <= 1)
        ic = cut(np.where(visible, r, T(0)) * T(nr)).astype(np.int64)
        jc = cut(np.where(visible, z, T(0)) * T(nz)).astype(np.int64)
    return ic, jc, visible


def raster_first(u, Wd, bits, y_down, T):
    """First column (first row counted from the bottom when y_down) of the 11 pixels a rasteriser with `bits` sub-pixel bits
    covers for clip coordinate 2u - 1 on Wd pixels, and whether the coordinate is usable.  Window positions are fixed point
    in units of 2^-bits pixel, in pixel-centre coordinates (pixel k's centre at k 2^bits): X = rint(X0 + ndc Wb), Wb = Wd/2
    2^bits, X0 = Wb - 2^bits / 2, y running downwards; the square X +- 11 2^(bits-1) with left / top edges inclusive covers
    the centres from ceil((X - 11 2^(bits-1)) / 2^bits) on."""
    u = np.asarray(u, dtype=T)
    one = 1 << bits
    with np.errstate(all="ignore"):
        ndc = T(2) * u - T(1)
        wb = T(T(Wd) * T(0.5)) * T(one)
        x0 = T(wb - T(T(one) * T(0.5)))
        s = x0 + ndc * (T(-wb) if y_down else wb)
        ok = (s > T(-2.0 ** 30)) & (s < T(2.0 ** 30))
        X = np.rint(np.where(ok, s, T(0))).astype(np.int64)           # round half to even
    a = X - (11 * one) // 2
    p0 = -((-a) // one)                                                # ceil(a / 2^bits)
    return (Wd - 1 - (p0 + 10) if y_down else p0), ok


def raster_cells(pos, nr, nz, bits, T):
    """(ic, jc, visible): the centre cell of the rasterised sprite, ic in -5 .. nr+4 ... where visible"""
    p = np.asarray(pos, dtype=T)
    i0, oki = raster_first(radius(p, T), nr, bits, False, T)
    j0, okj = raster_first(p[:, 2], nz, bits, True, T)
    visible = oki & okj & (i0 < nr) & (i0 + 10 >= 0) & (j0 < nz) & (j0 + 10 >= 0)
    return i0 + REACH, j0 + REACH, visible


def sprite_cells(pos, nr, nz, T, bits=0, variant=None):
    return raster_cells(pos, nr, nz, bits, T) if bits else ideal_cells(pos, nr, nz, T, variant)


# ------------------------------------------------------------------ stage 1
def colours(pos, vel, T, variant=None):
    """(c [n][4], m [n][4]) in W: the colour 0.001 (v_r, v_theta, v_z, 1) and the magnitudes of its terms.  (variant
    'flip_theta': the deliberately wrong sign.)"""
    p, v = np.asarray(pos, dtype=T).astype(W), np.asarray(vel, dtype=T).astype(W)
    x, y = p[:, 0], p[:, 1]
    k = milli(T)
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)
        c = np.stack([k * (v[:, 0] * x + v[:, 1] * y) / r, k * (v[:, 1] * x - v[:, 0] * y) / r, k * v[:, 2], k * np.ones_like(r)], axis=1)
        m = np.stack([k * (np.abs(v[:, 0] * x) + np.abs(v[:, 1] * y)) / r, k * (np.abs(v[:, 1] * x) + np.abs(v[:, 0] * y)) / r,
                      k * np.abs(v[:, 2]), k * np.ones_like(r)], axis=1)
    if variant == "flip_theta":
        c[:, 1] = -c[:, 1]
    zero = radius(pos, T) == 0          # 0 / 0 in T
    c[zero, 0:2] = np.nan
    m[zero, 0:2] = 0
    return c, m


def _scatter(shape, index, values):
    out = np.zeros(shape, dtype=W)
    np.add.at(out, index, values)
    return out


def cell_sums(pos, vel, nr, nz, T, bits=0, variant=None):
    """Stage 1.  Returns dict(count int64 [nz+11][nr+11], colour W [nz+11][nr+11][3] (NaN where a particle sits at r == 0),
    mag W [..][3] (M_cell; the NaN particles left out), nan bool [..] (cells holding an r == 0 particle))."""
    ic, jc, vis = sprite_cells(pos, nr, nz, T, bits, variant)
    c, m = colours(pos, vel, T, variant)
    gw, gh = nr + 1 + 2 * APRON, nz + 1 + 2 * APRON
    ii, jj = ic[vis] + APRON, jc[vis] + APRON
    assert ii.size == 0 or (ii.min() >= 0 and ii.max() < gw and jj.min() >= 0 and jj.max() < gh)
    count = np.zeros((gh, gw), dtype=np.int64)
    np.add.at(count, (jj, ii), 1)
    cv, mv = c[vis], m[vis]
    nanp = np.isnan(cv[:, 0])
    nan = np.zeros((gh, gw), dtype=bool)
    nan[jj[nanp], ii[nanp]] = True
    colour = _scatter((gh, gw, 3), (jj, ii), np.where(np.isnan(cv[:, :3]), 0, cv[:, :3]))
    mag = _scatter((gh, gw, 3), (jj, ii), mv[:, :3])
    colour[nan, 0:2] = np.nan
    return dict(count=count, colour=colour, mag=mag, nan=nan)


def assert_cell_population(count):
    assert count.max() <= CELL_LIMIT, "%d particles in one cell: the count's read-back is not provably exact" % count.max()


def colour_bound(ref, T):
    """stage 1: (K + n_cell) eps M_cell, [nz+11][nr+11][3]"""
    K = np.asarray(K_COLOUR[:3], dtype=W)
    return (K + ref["count"][..., None].astype(W)) * W(eps(T)) * ref["mag"]


def cic_sums(pos, vel, nr, nz, T, variant=None):
    """Stage 1 of shape 'cic' on the nr x nz grid: dict(sums W [nz][nr][4] (NaN in 0, 1 where an r == 0 particle reaches),
    bound W [nz][nr][4], nan bool [nz][nr])."""
    _, _, vis = ideal_cells(pos, nr, nz, T)
    c, m = colours(pos, vel, T)
    p = np.asarray(pos, dtype=T)
    r, z = radius(p, T).astype(W)[vis], p[:, 2].astype(W)[vis]
    c, m = c[vis], m[vis]
    gi, gj = r * nr - W(0.5), z * nz - W(0.5)
    fi, fj = np.floor(gi), np.floor(gj)
    wr, wz = [1 - (gi - fi), gi - fi], [1 - (gj - fj), gj - fj]
    if variant == "exchange":       # (deliberately wrong: the weights of an axis' two corners exchanged)
        wr, wz = wr[::-1], wz[::-1]
    ci, cj = fi.astype(np.int64), fj.astype(np.int64)
    sums, n = np.zeros((nz, nr, 4), dtype=W), np.zeros((nz, nr), dtype=np.int64)
    lin, absw = np.zeros((nz, nr, 4), dtype=W), np.zeros((nz, nr, 4), dtype=W)
    nan = np.zeros((nz, nr), dtype=bool)
    K = np.asarray(K_COLOUR, dtype=W) + 2
    for b in range(2):
        for a in range(2):
            i, j = ci + a, cj + b
            ok = (i >= 0) & (i < nr) & (j >= 0) & (j < nz)
            w = (wr[a] * wz[b])[ok, None]
            cc, mm = c[ok], m[ok]
            at = (j[ok], i[ok])
            np.add.at(sums, at, np.where(np.isnan(cc), 0, cc) * w)
            np.add.at(n, at, 1)
            np.add.at(lin, at, mm * w)
            np.add.at(absw, at, mm * (nr * wz[b] + nz * wr[a])[ok, None])
            nanp = np.isnan(cc[:, 0])
            nan[j[ok][nanp], i[ok][nanp]] = True
    bound = W(eps(T)) * ((K + n[..., None].astype(W)) * lin + absw)
    sums[nan, 0:2] = np.nan
    return dict(sums=sums, bound=bound, nan=nan)


# ------------------------------------------------------------------ stage 2
def stamp_moments(sums, nr, nz, stamp, shift=(0, 0)):
    """moments [nz][nr][C] in W and sum |w s| from a sums grid [nz+11][nr+11][C]: a particle of cell (ic, jc) adds
    weight[(di + 5) + 11 (5 - dj)] of its sums to cell (ic + di, jc + dj).  NaN cells spread NaN over their whole footprint.
    (`shift` moves the stamp; the wrong variants of tests/test_deposit_reference.py use it.)"""
    s = np.asarray(sums).astype(W)
    nanc = np.isnan(s)
    s0 = np.where(nanc, 0, s)
    out, mag = np.zeros((nz, nr, s.shape[2]), dtype=W), np.zeros((nz, nr, s.shape[2]), dtype=W)
    nan = np.zeros((nz, nr, s.shape[2]), dtype=bool)
    pad = ((2 * REACH, 2 * REACH), (2 * REACH, 2 * REACH), (0, 0))
    s0, nanc = np.pad(s0, pad), np.pad(nanc, pad)
    for dj in range(-REACH, REACH + 1):
        for di in range(-REACH, REACH + 1):
            w = W(stamp[REACH - dj, di + REACH])
            # target (i, j) takes source cell (i - di, j - dj), which sits at padded index + APRON + 2 REACH
            j0, i0 = APRON + 2 * REACH - dj - shift[1], APRON + 2 * REACH - di - shift[0]
            src = s0[j0:j0 + nz, i0:i0 + nr]
            out += w * src
            mag += np.abs(w * src)
            nan |= nanc[j0:j0 + nz, i0:i0 + nr]
    out[nan] = np.nan
    return out, mag


def moments_bound(mag, T):
    return (SIDE * SIDE + 2) * (W(eps(T)) * mag + W(np.finfo(T).tiny))


# ------------------------------------------------------------------ stages 3 and 4
def normalise(moments, nr, nz, half_over_x=True):
    m = np.asarray(moments).astype(W).reshape(nz, nr, 4)
    xc = ((np.arange(nr).astype(W) + W(0.5)) / nr)[None, :, None]
    with np.errstate(all="ignore"):
        touched = m[..., 3:4] > 0
        q = np.concatenate([m[..., :3] / m[..., 3:4], m[..., 3:4]], axis=2)
        out = 1000 * q * (W(0.5) / xc if half_over_x else 1)
    return np.where(touched, out, 0)


def average(norm, avg_prev, T, swapped=False):
    """(avg, sum of the magnitudes of its two terms)"""
    ratio = W(T(0.01))
    a, b = (1 - ratio, ratio) if swapped else (ratio, 1 - ratio)
    n, p = np.asarray(norm).astype(W), np.asarray(avg_prev).astype(W)
    with np.errstate(all="ignore"):
        return a * n + b * p, np.abs(a * n) + np.abs(b * p)


# ------------------------------------------------------------------ comparisons
def over_bound(got, want, bound):
    """largest |got - want| / bound over the cells where want is a number; infinite when the NaN sets differ.  A zero bound
    asks for equality (0 over 0 counts as 0)."""
    got, want, bound = np.asarray(got).astype(W), np.asarray(want).astype(W), np.asarray(bound).astype(W)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0, err / bound[ok])
    return float(ratio.max()) if ratio.size else 0.0


def split_sums(buf, nr, nz):
    """the FPIC_BUF_CELL_SUMS read-back as [nz+11][nr+11][4] float64"""
    return np.asarray(buf, dtype=np.float64).reshape(nz + 1 + 2 * APRON, nr + 1 + 2 * APRON, 4)


def counts_of(sums, T):
    """(integers, largest distance from an integer) of the count channel of a sums read-back"""
    q = sums[..., 3].astype(W) / milli(T)
    n = np.rint(q)
    return n.astype(np.int64), float(np.abs(q - n).max())


def as_readback(ref, T):
    """a stage-1 reference as the device would hand it back: [nz+11][nr+11][4] float64 holding values of T"""
    out = np.concatenate([ref["colour"], (ref["count"].astype(W) * milli(T))[..., None]], axis=2)
    return out.astype(T).astype(np.float64)


def measure_sums(got, ref, T):
    """Stage 1 figures of a sums read-back `got` [nz+11][nr+11][4] against cell_sums(): cells whose count differs, the
    largest distance of a count from an integer, the largest colour error over bound."""
    assert_cell_population(ref["count"])
    n, frac = counts_of(got, T)
    return dict(count_cells_wrong=int((n != ref["count"]).sum()), count_frac=frac,
                colour=over_bound(got[..., :3], ref["colour"], colour_bound(ref, T)))


def measure_cic(got, ref, T):
    """Stage 1 figure of shape 'cic': got [nz][nr][4] against cic_sums()"""
    return dict(cic=over_bound(got, ref["sums"], ref["bound"]))


def measure_moments(got, sums, nr, nz, stamp, T, identity=False):
    """Stage 2 figures: got [nz][nr][4] from the sums read-back it was made of; touched cells (m_3 > 0) that differ"""
    if identity:
        want = np.asarray(sums).astype(W)
        bound = np.zeros_like(want)
    else:
        want, mag = stamp_moments(sums, nr, nz, stamp)
        bound = moments_bound(mag, T)
    got = np.asarray(got, dtype=np.float64).reshape(nz, nr, 4)
    return dict(moments=over_bound(got, want, bound), touched_wrong=int(((got[..., 3] > 0) != (want[..., 3] > 0)).sum()))


def measure_finish(norm, avg, moments, avg_prev, nr, nz, T):
    """Stages 3 and 4 figures from the moments and the previous average they were made of"""
    want = normalise(moments, nr, nz)
    norm = np.asarray(norm, dtype=np.float64).reshape(nz, nr, 4)
    want_avg, mag = average(norm, np.asarray(avg_prev, dtype=np.float64).reshape(nz, nr, 4), T)
    return dict(norm=over_bound(norm, want, 4 * W(eps(T)) * np.abs(want)),
                avg=over_bound(np.asarray(avg, dtype=np.float64).reshape(nz, nr, 4), want_avg, 4 * W(eps(T)) * mag))


def assert_figures(fig, where=""):
    """every figure of the measure_* functions at its bar: integers equal, counts within 0.25 of an integer, error over
    bound at most 1"""
    for k, v in fig.items():
        if k in ("count_cells_wrong", "touched_wrong"):
            assert v == 0, (where, k, v, fig)
        elif k == "count_frac":
            assert v < 0.25, (where, k, v, fig)
        else:
            assert v <= 1.0, (where, k, v, fig)
