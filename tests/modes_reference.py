"""The rule of the modes diagnostic (fpic_modes_*, include/fusionpic.h) in numpy, nothing of the library.  Written from the
header's contract: for a quantity F on the N = nx ny nz nodes (node index i + nx (j + ny k)) and a wave vector m,

  A(m) = (1/N) sum_k sum_j sum_i F[k][j][i] wx[(mx i) mod nx] wy[(my j) mod ny] wz[(mz k) mod nz],   wa[t] = exp(-2 pi i t / na)

with integer index arithmetic (a negative m is reduced into [0, n) first).  Two evaluations:

  amplitudes()  in numpy.longdouble throughout (tables from exact rational angles t / n reduced mod 1, the sums in extended
                precision): the reference the GPU rows are compared with; its own error is negligible against the bound
  naive()       a plain sequential float64 evaluation with the float64 tables of table(), as the header states the rule

tolerance() is the derived bound of the issue: per component |got - ref| <= (N + 16) 2^-53 (sum |F|) / N for ANY order of the
sum (N: the worst-case bound of a sum of N terms; 16: the three table roundings, the two complex products, the scaling).
"""
import numpy as np

FIELDS = ("ex", "ey", "ez", "phi", "bx", "by", "bz", "rho")
TWO_PI = np.longdouble(2) * np.longdouble("3.14159265358979323846264338327950288419716939937510")


def reduce(m, n):
    """m mod n in [0, n) (python's % on ints already floors)"""
    return int(m) % int(n)


def table(n, dtype=np.float64):
    """w[t] = exp(-2 pi i t / n) as an array [n][2] of `dtype`: entries with 4 t divisible by n exact, t < n / 2 from the
    angle in long double rounded once, t > n / 2 the bit-for-bit conjugate mirror"""
    w = np.zeros((n, 2), dtype=dtype)
    for t in range(n // 2 + 1):
        if (4 * t) % n == 0:
            re, im = [(1, 0), (0, -1), (-1, 0)][4 * t // n]
        else:
            a = TWO_PI * np.longdouble(t) / np.longdouble(n)
            re, im = np.cos(a), -np.sin(a)
        w[t] = (re, im)
        if 0 < t and 2 * t < n:
            w[n - t] = (w[t, 0], -w[t, 1])
    return w


def _phases(m, n, dtype):
    """w[(m i) mod n] for i < n, complex of the precision of dtype"""
    t = (reduce(m, n) * np.arange(n, dtype=np.int64)) % n
    w = table(n, dtype)
    return (w[t, 0] + 1j * w[t, 1]).astype(np.clongdouble if dtype == np.longdouble else np.complex128)


def amplitudes(F, modes, dtype=np.longdouble):
    """F: real array [nz][ny][nx] or [nz][ny][nx][nq]; modes: int triples [M][3] -> complex [M] or [M][nq], in `dtype`
    arithmetic (long double: the reference).  z may be a slab: pass planes=(k0, nz_global) through amplitudes_slab()."""
    return amplitudes_slab(F, modes, 0, np.shape(F)[0], dtype)


def amplitudes_slab(F, modes, k0, nz, dtype=np.longdouble):
    """as amplitudes(), of the planes [k0, k0 + F.shape[0]) of a box of nz planes: k in the twiddle is the global plane and
    the divisor the global N (a rank's LOCAL row)"""
    F = np.asarray(F)
    vec = F.ndim == 3
    G = (F[..., None] if vec else F).astype(dtype)
    nk, ny, nx, nq = G.shape
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    out = np.zeros((len(modes), nq), dtype=ct)
    for a, (mx, my, mz) in enumerate(np.asarray(modes, dtype=np.int64).reshape(-1, 3)):
        wx, wy = _phases(mx, nx, dtype), _phases(my, ny, dtype)
        wz = _phases(mz, nz, dtype)[k0:k0 + nk]
        rows = np.tensordot(G.astype(ct), wx, axes=([2], [0]))          # [nk][ny][nq]
        planes = np.tensordot(rows, wy, axes=([1], [0]))               # [nk][nq]
        out[a] = np.tensordot(planes, wz, axes=([0], [0])) / dtype(nx * ny * nz)
    return out[:, 0] if vec else out


def naive(F, modes):
    """the rule as stated, float64, one term after the other in the order k, j, i: [M] complex128 of a scalar field
    [nz][ny][nx] (slow: for small grids)"""
    F = np.asarray(F, dtype=np.float64)
    nz, ny, nx = F.shape
    tx, ty, tz = table(nx), table(ny), table(nz)
    out = np.zeros(len(modes), dtype=np.complex128)
    for a, (mx, my, mz) in enumerate(np.asarray(modes, dtype=np.int64).reshape(-1, 3)):
        mx, my, mz = reduce(mx, nx), reduce(my, ny), reduce(mz, nz)
        re = im = 0.0
        for k in range(nz):
            wz = complex(*tz[(mz * k) % nz])
            for j in range(ny):
                w = complex(*ty[(my * j) % ny]) * wz
                for i in range(nx):
                    v = F[k, j, i] * (complex(*tx[(mx * i) % nx]) * w)
                    re, im = re + v.real, im + v.imag
        out[a] = complex(re, im) / (nx * ny * nz)
    return out


def tolerance(F):
    """the bound per component for the quantities of F ([nz][ny][nx] or [..][nq]) over the WHOLE box F: float64 [nq] or scalar"""
    F = np.asarray(F, dtype=np.float64)
    N = F.shape[0] * F.shape[1] * F.shape[2]
    s = np.abs(F).sum(axis=(0, 1, 2))
    return (N + 16) * 2.0 ** -53 * s / N


def mode_list(shape, rng, extra=20):
    """the list the GPU tests use: the axis units, (0,0,0), the Nyquist corners of the even axes, `extra` random triples with
    negatives, all distinct and within [-n/2, n/2]"""
    nx, ny, nz = shape
    out = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
    for a, n in enumerate(shape):
        if n % 2 == 0:
            m = [0, 0, 0]
            m[a] = n // 2
            if tuple(m) not in out:      # (two nodes on an axis: the Nyquist corner is the axis unit)
                out.append(tuple(m))
    while len(out) < 4 + 3 + extra:
        m = tuple(int(rng.integers(-(n // 2), n // 2 + 1)) for n in shape)
        if m not in out:
            out.append(m)
        if len(set(out)) >= np.prod([2 * (n // 2) + 1 for n in shape]):
            break
    return np.array(out, dtype=np.int32)
