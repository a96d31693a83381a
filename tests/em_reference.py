"""Float64 / exact-integer reference of one sub-step of the CART3D pushes (full EM, `solver:'yee'`, and the electrostatic
push), written from the DEFINITION TEXT (the header comment of the oracle's implementation
file) and from the equations, not from anybody's loops: plain numpy on whole arrays, neighbours by np.roll, no ctypes, no
import of the oracle or of the product.  It referees both of them (tests/test_em_reference.py, test_gpu_em_reference.py).

Conventions: every field array is value[i][j][k][3] ([nx][ny][nz][3]); positions are normalised by the box (u in [0, 1)),
velocities are in units of c; E in V/m, B in T.  The Yee lattice holds Ex at (i+1/2, j, k), Ey at (i, j+1/2, k), Ez at
(i, j, k+1/2), Bx at (i, j+1/2, k+1/2), By at (i+1/2, j, k+1/2), Bz at (i+1/2, j+1/2, k).

Every float function returns, next to its result, the SUM OF THE ABSOLUTE VALUES of the terms it added: a rounding bound of a
T-precision evaluation of the same expression is a small multiple of eps_T times that sum (never of the result, which may be
the small difference of large terms).
"""
from fractions import Fraction

import numpy as np

SPEED_OF_LIGHT = 2.998e8
EPS0 = 8.8541878128e-12
WEIGHT_ONE = 1 << 14            # the linear weights are 14-bit fixed point: w0 + w1 = 2^14
S = 1 << 15                     # one cell in DOUBLED fixed-point coordinates
J_UNIT = 96 * (1 << 42)         # J_fixed of one particle of Z = 1 moving one whole cell, summed over the four edges


def _prev(a, axis):
    """a at index - 1 along `axis` (periodic)"""
    return np.roll(a, 1, axis=axis)


def _next(a, axis):
    return np.roll(a, -1, axis=axis)


# ---------------------------------------------------------------------------------------------------------- node centring
def node_fields(E_edge, B_face):
    """Node-centred E = mean of the 2 edge samples next to the node along the component's own axis; node-centred B = mean
    of the 4 face samples around the node in the plane ACROSS the component's axis.  Returns (E_n, B_n, |E|, |B|): the last
    two are the means of the absolute samples."""
    E_edge, B_face = np.asarray(E_edge, np.float64), np.asarray(B_face, np.float64)
    En, Ea, Bn, Ba = (np.empty_like(E_edge) for _ in range(4))
    for m in range(3):
        e = E_edge[..., m]
        En[..., m] = 0.5 * (e + _prev(e, m))
        Ea[..., m] = 0.5 * (np.abs(e) + _prev(np.abs(e), m))
        u, v = (m + 1) % 3, (m + 2) % 3
        b = B_face[..., m]
        four = lambda a: a + _prev(a, u) + _prev(a, v) + _prev(_prev(a, u), v)
        Bn[..., m] = 0.25 * four(b)
        Ba[..., m] = 0.25 * four(np.abs(b))
    return En, Bn, Ea, Ba


# ------------------------------------------------------------------------------------------ cells, weights, gather (CIC)
def cells_and_weights(u, n, T):
    """The discrete part of the definition, exact: g = u n rounded ONCE in T, i = trunc(g), f = g - i, i folded into
    [0, n) (u n may round up to n), w1 = (trunc(f 2^15) + 1) >> 1 in [0, 2^14].  u: [N] or [N][3] of T with n an int or a
    3-tuple.  Returns integer arrays (i, w1)."""
    T = np.dtype(T).type
    u = np.asarray(u)
    assert u.dtype == np.dtype(T), "positions must come in the precision whose rounding decides the cell"
    n = np.asarray(n, dtype=np.int64)
    g = u * n.astype(T)                                   # one rounding in T
    i = np.trunc(g).astype(np.int64)
    f = g - i.astype(T)                                   # exact
    i = np.where(i >= n, i - n, i)
    w1 = (np.trunc(f * T(S)).astype(np.int64) + 1) >> 1
    return i, w1


def fixed_coordinate(u, n, T):
    """doubled fixed-point lattice coordinate 2 (cell 2^14 + w1) in [0, n 2^15] of a normalised coordinate"""
    i, w1 = cells_and_weights(u, n, T)
    return 2 * (i * WEIGHT_ONE + w1)


def gather(nodes, i, w1):
    """Trilinear (CIC) interpolation of a node array [nx][ny][nz][C] at the cells i [N][3] with the weights w1 / 2^14
    [N][3], in float64.  Returns (value [N][C], sum of |weight x node value| [N][C])."""
    nodes = np.asarray(nodes, np.float64)
    shape = np.array(nodes.shape[:3])
    f1 = w1 / float(WEIGHT_ONE)
    f = (1.0 - f1, f1)
    val = np.zeros((len(i), nodes.shape[3]))
    mag = np.zeros_like(val)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                w = f[a][:, 0] * f[b][:, 1] * f[c][:, 2]
                idx = (i + np.array([a, b, c])) % shape
                at = nodes[idx[:, 0], idx[:, 1], idx[:, 2]]
                val += w[:, None] * at
                mag += w[:, None] * np.abs(at)
    return val, mag


# ------------------------------------------------------------------------------------------------------------ Boris, drift
def boris(v, E_p, B_p, h, c=SPEED_OF_LIGHT, E_abs=None):
    """v (units of c) -> v after one Boris step with h = q dt / 2m: half kick a = (h/c) E, rotation about B with
    t = h B and s = 2 t / (1 + t^2), half kick.  B_p is [N][3] (the particle's own t: full EM) or [3] (one t for the
    whole handle: the electrostatic push in a uniform external B).  Returns (v_new [N][3], magnitude [N]) with
    magnitude = |v|_inf + 2 |h/c| max_m E_abs (E_abs: the gather's sum of absolute terms; default |E_p|)."""
    v = np.asarray(v, np.float64)
    E_p = np.broadcast_to(np.asarray(E_p, np.float64), v.shape)
    t = h * np.broadcast_to(np.asarray(B_p, np.float64), v.shape)
    a = (h / c) * E_p
    s = 2.0 * t / (1.0 + (t * t).sum(axis=1, keepdims=True))
    vm = v + a
    vp = vm + np.cross(vm + np.cross(vm, t), s)
    E_abs = np.abs(E_p) if E_abs is None else np.broadcast_to(E_abs, v.shape)
    return vp + a, np.abs(v).max(axis=1) + 2.0 * abs(h / c) * np.abs(E_abs).max(axis=1)


def drift(u, v, k):
    """u + k v (k = dt c / L per axis) wrapped into [0, 1).  Returns (u_new, |u| + |k v|)."""
    u, v, k = np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(k, np.float64)
    r = u + k * v
    r = r - np.floor(r)
    return np.where(r < 1.0, r, 0.0), np.abs(u) + np.abs(k * v)


def periodic_distance(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, 1.0 - d)


# ------------------------------------------------------------------------------------------------------- the exact current
def nearest_image(a, b, shape):
    """b moved by whole boxes to the periodic image nearest to a (doubled fixed-point coordinates, [N][3])"""
    box = np.asarray(shape, dtype=np.int64) * S
    d = b - a
    d = np.where(2 * d > box, d - box, np.where(2 * d < -box, d + box, d))
    return a + d


def relay_point(a, b):
    """Where the move a -> b (b the nearest image) is cut, per axis: the midpoint when both ends lie in one cell (both
    coordinates are even, the midpoint is an integer); else the face at the lower side of the higher of the two cells:
    the common face of two neighbouring cells."""
    ca, cb = a // S, b // S
    return np.where(ca == cb, (a + b) // 2, np.maximum(ca, cb) * S)


def relay_midpoint(a, b):
    """a WRONG relay point (sensitivity control): the midpoint even across a face"""
    return (a + b) // 2


def _segment(p1, p2, cell, shape, Z, J, rule):
    """adds the fluxes of the straight segments p1 -> p2 [N][3], each integrated with the linear weights of `cell` [N][3]
    (unwrapped cell indices; the weights are extrapolated where the segment leaves the cell):
        flux(m; b, c) = Z 12 S^2 (p2_m - p1_m) Int_0^1 W_u,b(t) W_v,c(t) dt,   W_1 = l / S, W_0 = 1 - l / S.
    The integrand is quadratic in t, Simpson's rule on t = 0, 1/2, 1 is exact; with L the numerators of the weights,
        12 S^2 Int = 2 [ L_u(0) L_v(0) + (L_u(0) + L_u(1)) (L_v(0) + L_v(1)) + L_u(1) L_v(1) ]   -- an integer.
    rule='midpoint' (a WRONG variant, the sensitivity control) takes 12 S^2 W_u(1/2) W_v(1/2) instead."""
    shape = np.asarray(shape, dtype=np.int64)
    l1, l2 = p1 - cell * S, p2 - cell * S
    c0 = cell % shape
    for m in range(3):
        u, v = (m + 1) % 3, (m + 2) % 3
        for b in (0, 1):
            for c in (0, 1):
                Lu1, Lu2 = (l1[:, u], l2[:, u]) if b else (S - l1[:, u], S - l2[:, u])
                Lv1, Lv2 = (l1[:, v], l2[:, v]) if c else (S - l1[:, v], S - l2[:, v])
                if rule == "simpson":
                    integral = 2 * (Lu1 * Lv1 + (Lu1 + Lu2) * (Lv1 + Lv2) + Lu2 * Lv2)
                else:
                    integral = 3 * (Lu1 + Lu2) * (Lv1 + Lv2)
                flux = Z * (p2[:, m] - p1[:, m]) * integral
                idx = [None] * 3
                idx[m], idx[u], idx[v] = c0[:, m], (c0[:, u] + b) % shape[u], (c0[:, v] + c) % shape[v]
                node = idx[0] + shape[0] * (idx[1] + shape[1] * idx[2])
                np.add.at(J, (node, m), flux)


def current_exact(a, b, shape, Z, relay=relay_point, rule="simpson"):
    """J_fixed [nodes][3] (int64; node index i + nx (j + ny k); component m on the edge of direction m that starts at the
    node) of the moves a -> b given in doubled fixed-point coordinates [N][3]: nearest image, taken in pieces() that skip no
    cell, each piece cut at its relay point, its first segment integrated with the weights of the cell it starts in, the
    second with those of the cell it ends in.  The integral is multiplied out in int64 (see _segment; |flux| < 2^60 for
    moves of a few cells)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    J = np.zeros((int(np.prod(shape)), 3), dtype=np.int64)
    for p, q in pieces(a, nearest_image(a, b, shape)):
        r = relay(p, q)
        _segment(p, r, p // S, shape, int(Z), J, rule)
        _segment(r, q, q // S, shape, int(Z), J, rule)
    return J


def pieces(a, b):
    """The straight pieces [(from, to), ...] of the moves a -> b (b the nearest image).  A segment is integrated with the
    weights of ONE cell, and at the relay point the weights of two cells agree only when the cells share that face: a
    move that skips a cell on some axis (|v| > c) first takes whole-cell steps on those axes (to a + S or a - S there, a elsewhere)
    until no axis skips; every piece is cut at its own relay point.  (Moves that skip nothing: one piece.)"""
    out = []
    while True:
        dc = b // S - a // S
        w = a + S * (np.where(dc >= 2, 1, 0) - np.where(dc <= -2, 1, 0))
        stepping = (w != a).any(axis=1)
        if not stepping.any():
            return out + [(a, b)]
        out.append((a[stepping], w[stepping]))
        a = np.where(stepping[:, None], w, a)
        # (the particles that do not step wait for the last piece with their own a)


def current_exact_fractions(a, b, shape, Z):
    """The same line integral particle by particle in fractions.Fraction with Simpson's rule spelled out on the weights
    themselves (slow; the cross-check of the int64 form).  Asserts that no edge value is fractional."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    J = {}
    straight = [(p, relay_point(p, q), q) for p, q in pieces(a, nearest_image(a, b, shape))]
    for rows in (rows for piece in straight for rows in zip(*piece)):
        ends = [[int(x) for x in row] for row in rows]                         # Python integers from here on
        for p1, p2, inside in ((ends[0], ends[1], ends[0]), (ends[1], ends[2], ends[2])):
            cell = [x // S for x in inside]

            def weight(axis, hi, t):
                local = Fraction(p1[axis]) + t * (p2[axis] - p1[axis]) - cell[axis] * S
                return local / S if hi else 1 - local / S

            for m in range(3):
                u, v = (m + 1) % 3, (m + 2) % 3
                for bb in (0, 1):
                    for cc in (0, 1):
                        at = lambda t: weight(u, bb, t) * weight(v, cc, t)
                        integral = (at(Fraction(0)) + 4 * at(Fraction(1, 2)) + at(Fraction(1))) / 6
                        idx = [0, 0, 0]
                        idx[m], idx[u], idx[v] = cell[m] % shape[m], (cell[u] + bb) % shape[u], (cell[v] + cc) % shape[v]
                        key = (idx[0] + shape[0] * (idx[1] + shape[1] * idx[2]), m)
                        J[key] = J.get(key, Fraction(0)) + Z * 12 * S * S * (p2[m] - p1[m]) * integral
    out = np.zeros((int(np.prod(shape)), 3), dtype=np.int64)
    for (node, m), value in J.items():
        assert value.denominator == 1, "a fractional edge flux"
        out[node, m] = int(value)
    return out


def first_moment(a, b, shape, Z):
    """sum over the nodes of J_fixed[:, m], from the moves alone: 12 2^30 Z sum_p (b_m - a_m)   (= 96 2^42 Z per cell)"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return 12 * (1 << 30) * int(Z) * (nearest_image(a, b, shape) - a).sum(axis=0)


def divergence(J_fixed, shape):
    """sum over the axes of J_m(node) - J_m(node - 1 along m), [nx][ny][nz]"""
    Jg = np.asarray(J_fixed).reshape(shape[2], shape[1], shape[0], 3).transpose(2, 1, 0, 3)
    return sum(Jg[..., m] - np.roll(Jg[..., m], 1, axis=m) for m in range(3))


def continuity_residual(J, a, b, shape, Z):
    """96 (rho(b) - rho(a)) + div J per node: zero at every node for a charge-conserving current"""
    return 96 * (cic_charge(b, shape, Z) - cic_charge(a, shape, Z)) + divergence(J, shape)


def cic_charge(p, shape, Z):
    """Z wx wy wz (14-bit weights) of the doubled coordinates p on the nodes, [nx][ny][nz] int64"""
    rho = np.zeros(shape, dtype=np.int64)
    h = p // 2
    cell, w1 = h // WEIGHT_ONE, h % WEIGHT_ONE
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                w = [(w1[:, m] if bit else WEIGHT_ONE - w1[:, m]) for m, bit in enumerate((a, b, c))]
                idx = (cell + np.array([a, b, c])) % np.array(shape)
                np.add.at(rho, (idx[:, 0], idx[:, 1], idx[:, 2]), Z * w[0] * w[1] * w[2])
    return rho


# -------------------------------------------------------------------------------------------------------------- the lattice
def _curl_of_edges(E, d):
    """(curl E) on the faces and the sum of the absolute terms: (curl E)_x (i, j+1/2, k+1/2) = dEz/dy - dEy/dz, forward"""
    out, mag, A = np.empty_like(E), np.empty_like(E), np.abs(E)
    for m in range(3):
        u, v = (m + 1) % 3, (m + 2) % 3
        out[..., m] = (_next(E[..., v], u) - E[..., v]) / d[u] - (_next(E[..., u], v) - E[..., u]) / d[v]
        mag[..., m] = (_next(A[..., v], u) + A[..., v]) / d[u] + (_next(A[..., u], v) + A[..., u]) / d[v]
    return out, mag


def _curl_of_faces(B, d):
    """(curl B) on the edges: (curl B)_x (i+1/2, j, k) = dBz/dy - dBy/dz, backward differences"""
    out, mag, A = np.empty_like(B), np.empty_like(B), np.abs(B)
    for m in range(3):
        u, v = (m + 1) % 3, (m + 2) % 3
        out[..., m] = (B[..., v] - _prev(B[..., v], u)) / d[u] - (B[..., u] - _prev(B[..., u], v)) / d[v]
        mag[..., m] = (A[..., v] + _prev(A[..., v], u)) / d[u] + (A[..., u] + _prev(A[..., u], v)) / d[v]
    return out, mag


def current_density(J_fixed, shape, d, dt, q0W):
    """J (A/m^2) on the edges [nx][ny][nz][3] = q0 W / (96 2^42 dt) J_fixed / (area of the dual face)"""
    J = np.asarray(J_fixed).reshape(shape[2], shape[1], shape[0], 3).transpose(2, 1, 0, 3).astype(np.float64)
    area = np.array([d[1] * d[2], d[2] * d[0], d[0] * d[1]])
    return J * (q0W / (J_UNIT * dt)) / area


def yee_substep(E, B, J_fixed, dt, d, q0W, c=SPEED_OF_LIGHT, eps0=EPS0):
    """B^(n+1/2) = B^n - dt/2 curl E^n;  E^(n+1) = E^n + dt (c^2 curl B^(n+1/2) - J / eps0);
    B^(n+1) = B^(n+1/2) - dt/2 curl E^(n+1).  d = (dx, dy, dz).  Returns (E1, B1, |E1|, |B1|) where the last two are the
    sums of the absolute values of ALL terms of the expanded expressions (the terms of B^(n+1/2) enter E^(n+1) scaled by
    c^2 dt / d, about 1e7 next to E of 1e4: the result says nothing about the rounding)."""
    E, B = np.asarray(E, np.float64), np.asarray(B, np.float64)
    shape = E.shape[:3]
    J = current_density(J_fixed, shape, d, dt, q0W)
    curl, mag = _curl_of_edges(E, d)
    Bh, Bh_abs = B - 0.5 * dt * curl, np.abs(B) + 0.5 * dt * mag
    curl, _ = _curl_of_faces(Bh, d)
    E1 = E + dt * (c * c * curl - J / eps0)
    E1_abs = np.abs(E) + dt * (c * c * _curl_of_faces(Bh_abs, d)[1] + np.abs(J) / eps0)
    curl, _ = _curl_of_edges(E1, d)
    B1 = Bh - 0.5 * dt * curl
    B1_abs = Bh_abs + 0.5 * dt * _curl_of_edges(E1_abs, d)[1]
    return E1, B1, E1_abs, B1_abs
