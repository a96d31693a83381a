// fes_load_radial_core.hpp — the rule of a radial load (fpic_load_radial) on top of fes_load_core.hpp and the look-up of
// fes_load_profile_core.hpp: a spherical or cylindrical population whose density, thermal speed and flows are tables of the
// radius.  Plain C++ that compiles for the host and the device, shared with a host test
// (tests/native/load_radial_core_test.cpp, g++).  All arithmetic is double, every operation rounded once
// (-ffp-contract=off); the radius takes only + - * / and comparisons, so it can be held bit for bit to an independent
// reference.
//
// A table of K + 1 nodes is uniformly spaced over [0, r_max] (node 0 on the centre or the axis, node K at r_max) and linear
// between the nodes; rho is the radius in units of r_max.  f0, f1, f2 are the unit fractions of the plain rule (the random
// words or the lattice words of the three axes).
//   mass       in units of the node spacing, with d0 = d[j], D = d[j+1] - d[j], J = (double) j, the mass of interval j up to
//              the place s in [0, 1] is a polynomial in s without a constant term, evaluated in Horner form:
//                  sphere (weight rho^2)   JJ = J J;  a1 = d0 JJ;  a2 = d0 J + 0.5 (D JJ);  a3 = (d0 + (2 J) D) / 3;  a4 = 0.25 D
//                                          M(s) = (a1 + (a2 + (a3 + a4 s) s) s) s
//                  cylinder (weight rho)   a1 = d0 J;  a2 = 0.5 (d0 + D J);  a3 = D / 3
//                                          M(s) = (a1 + (a2 + a3 s) s) s
//              (every product written "x s" is s times the sum so far, every sum "a + (...)".)
//   cumulative the host sums C[0] = 0, C[j+1] = C[j] + M_j(1) in sequence, M_j(1) by the same evaluation at s = 1.
//   radius     f = f0 (sphere) or the fraction of axis b (cylinder):
//                  t = f C[K];  j = the largest index with C[j] <= t, held to K - 1 (warp's bisection);  r = t - C[j];
//                  lo = 0, hi = 1;  52 times: mid = 0.5 (lo + hi); if M_j(mid) <= r: lo = mid, else hi = mid;  s = lo;
//                  rho = (J + s) / K, and 1 - 2^-53 if that is not below 1.
//              An interval without mass has C[j] == C[j+1] and is never chosen.  Without a density table the table is {1, 1}:
//              uniform in the volume (the area).
//   direction  sphere:   mu = 2 f1 - 1;  q = sqrt(1 - mu mu);  cs = cospi(2 f2), sn = sinpi(2 f2);  dir = (q cs, q sn, mu)
//              cylinder about axis a (b = (a + 1) mod 3, c = (a + 2) mod 3):  dir_a = 0, dir_b = cospi(2 f_c), dir_c = sinpi(2 f_c)
//   position   (box fractions) p_k = center[k]/L_k + (rho (r_max/L_k)) dir_k; for the cylinder's own axis the plain rule's
//              p_a = lo_f[a] + f_a w_f[a].  theta, the displacement, the cast and wrap01 are the plain rule's.
//   velocity   vth_eff[k] = vth[k] thermal(rho) (no table: no multiply);
//              sphere:   drift_eff[k] = drift[k] + u_r dir_k
//              cylinder: drift_eff[a] = drift[a] + u_a;  drift_eff[b] = (drift[b] + u_r dir_b) + u_t (-dir_c);
//                        drift_eff[c] = (drift[c] + u_r dir_c) + u_t dir_b
//              (a flow without a table adds nothing); the tables are read by lookup at f' = rho; then the plain rule's
//              velocity with these two.
#ifndef FES_LOAD_RADIAL_CORE_HPP
#define FES_LOAD_RADIAL_CORE_HPP
#include "fes_load_profile_core.hpp"

namespace fesload {

constexpr int kRadialHalvings = 52;

// the tables as the kernels read them, one block: dens, cum, then the others.  k = the INTERVALS of a table, 0: no table
struct Radial {
    const double* dens;
    const double* cum;
    const double* therm;
    const double* ur;
    const double* ut;
    const double* ua;
    uint32_t dk, tk, rk, zk, ak;      // density (never 0), thermal, radial, azimuthal, axial
    uint32_t geometry;
    int32_t axis;
    int needs_pos;                    // a thermal or a flow table: the velocity reads the radius and the direction
    uint32_t lds_doubles;             // the doubles of the whole block: what a workgroup stages
    double c_f[3], rl[3];             // center / L, r_max / L
};

// the coefficients of M_j, a[0] = a1 ..; the cylinder leaves a[3] unused
FES_HIST_HD void mass_coefficients(bool sphere, double d0, double d1, uint32_t j, double (&a)[4])
{
    const double D = d1 - d0, J = static_cast<double>(j);
    if (sphere) {
        const double JJ = J * J;
        a[0] = d0 * JJ;
        const double dj = d0 * J, Dj = D * JJ;
        const double half = 0.5 * Dj;
        a[1] = dj + half;
        const double twoJ = 2.0 * J;
        const double tD = twoJ * D;
        const double sum = d0 + tD;
        a[2] = sum / 3.0;
        a[3] = 0.25 * D;
    } else {
        a[0] = d0 * J;
        const double DJ = D * J;
        const double sum = d0 + DJ;
        a[1] = 0.5 * sum;
        a[2] = D / 3.0;
        a[3] = 0.0;
    }
}

FES_HIST_HD double mass_at(bool sphere, const double (&a)[4], double s)
{
    double h;
    if (sphere) {
        h = a[3] * s;
        h = a[2] + h;
        h = h * s;
    } else {
        h = a[2] * s;
    }
    h = a[1] + h;
    h = h * s;
    h = a[0] + h;
    return h * s;
}

// C[0 .. n) from d[0 .. n), summed in sequence
inline void radial_cumulative(bool sphere, const double* d, uint32_t n, double* C)
{
    C[0] = 0.0;
    for (uint32_t j = 0; j + 1 < n; ++j) {
        double a[4];
        mass_coefficients(sphere, d[j], d[j + 1], j, a);
        const double m = mass_at(sphere, a, 1.0);
        C[j + 1] = C[j] + m;
    }
}

// f -> rho through the density table (d, C) of K intervals; j and s are the interval and the place in it
FES_HIST_HD double radius_of(bool sphere, const double* d, const double* C, uint32_t K, double f, uint32_t& j, double& s)
{
    const double t = f * C[K];
    uint32_t lo = 0, hi = K;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (C[mid] <= t) lo = mid; else hi = mid;
    }
    j = lo;
    const double r = t - C[j];
    double a[4];
    mass_coefficients(sphere, d[j], d[j + 1], j, a);
    double sl = 0.0, sh = 1.0;
    for (int k = 0; k < kRadialHalvings; ++k) {
        const double sum = sl + sh;
        const double mid = 0.5 * sum;
        const bool below = mass_at(sphere, a, mid) <= r;
        sl = below ? mid : sl;
        sh = below ? sh : mid;
    }
    s = sl;
    const double at = static_cast<double>(j) + s;
    double rho = at / static_cast<double>(K);
    if (!(rho < 1.0)) rho = kBelowOne;
    return rho;
}

// the polar part of the sphere's direction from the fraction f1: mu = cos of the polar angle, q = its sine
FES_HIST_HD void polar_of(double f1, double& mu, double& q)
{
    const double twice = 2.0 * f1;
    mu = twice - 1.0;
    const double mm = mu * mu;
    const double q2 = 1.0 - mm;
    q = sqrt(q2);
}

// the undisplaced position of particle i, its phase, its radius rho and the unit vector dir from the centre (the axis)
FES_HIST_HD void radial_base_of(const Rule& r, const Radial& q, uint32_t i, double (&p)[3], double& theta, double& rho, double (&dir)[3])
{
    uint32_t w[4];
    if (r.flags & FPIC_LOAD_LATTICE) {
        for (int a = 0; a < 3; ++a) w[a] = lattice_word(i, r.mult[a], r.shift[a]);
    } else {
        philox(i, r.stream, 0u, kTag, r.seed_lo, r.seed_hi, w);
    }
    const double f0 = fraction_of(w[0]), f1 = fraction_of(w[1]), f2 = fraction_of(w[2]);
    const bool sphere = q.geometry == FPIC_LOAD_SPHERE;
    const int ax = sphere ? -1 : q.axis;
    double fr, fc, fa = 0.0;         // the fractions of the radius, the angle and the cylinder's own axis
    if (sphere) { fr = f0; fc = f2; }
    else if (ax == 0) { fa = f0; fr = f1; fc = f2; }
    else if (ax == 1) { fa = f1; fr = f2; fc = f0; }
    else { fa = f2; fr = f0; fc = f1; }
    uint32_t j;
    double s;
    rho = radius_of(sphere, q.dens, q.cum, q.dk, fr, j, s);
    const double cs = cospi_(2.0 * fc), sn = sinpi_(2.0 * fc);
    if (sphere) {
        double mu, qq;
        polar_of(f1, mu, qq);
        dir[0] = qq * cs; dir[1] = qq * sn; dir[2] = mu;
    } else {
        dir[0] = ax == 0 ? 0.0 : ax == 2 ? cs : sn;      // (axis b = a + 1 takes the cosine, c = a + 2 the sine)
        dir[1] = ax == 1 ? 0.0 : ax == 0 ? cs : sn;
        dir[2] = ax == 2 ? 0.0 : ax == 1 ? cs : sn;
    }
    for (int k = 0; k < 3; ++k) {
        if (k == ax) {
            const double t = fa * r.w_f[k];
            p[k] = r.lo_f[k] + t;
        } else {
            const double e = rho * q.rl[k];
            const double off = e * dir[k];
            p[k] = q.c_f[k] + off;
        }
    }
    const double tx = r.m[0] * p[0], ty = r.m[1] * p[1], tz = r.m[2] * p[2];
    const double txy = tx + ty;
    theta = txy + tz;
}

// velocity_of with vth_eff and drift_eff in place of vth and drift
FES_HIST_HD void radial_velocity_of(const Rule& r, const Radial& q, uint32_t i, double theta, double rho, const double (&dir)[3], double (&v)[3])
{
    double n[3];
    normals_of(r, i, n);
    const bool sphere = q.geometry == FPIC_LOAD_SPHERE;
    const int ax = sphere ? -1 : q.axis, bx = ax == 2 ? 0 : ax + 1;
    const double scale = q.tk ? lookup(q.therm, q.tk, rho) : 1.0;
    const double u_r = q.rk ? lookup(q.ur, q.rk, rho) : 0.0;
    const double u_t = q.zk ? lookup(q.ut, q.zk, rho) : 0.0;
    const double u_a = q.ak ? lookup(q.ua, q.ak, rho) : 0.0;
    const bool flip = (r.flags & FPIC_LOAD_PAIRED) && (i & 1u);
    const double s = r.waved ? sinpi_(2.0 * (theta + r.vphase)) : 0.0;
    for (int k = 0; k < 3; ++k) {
        const double vth = q.tk ? r.vth[k] * scale : r.vth[k];
        double drift = r.drift[k];
        if (k == ax) {
            if (q.ak) drift = drift + u_a;
        } else {
            if (q.rk) {
                const double part = u_r * dir[k];
                drift = drift + part;
            }
            if (q.zk) {           // theta-hat = (-dir_c, dir_b): the other transverse component, negated on axis b
                const int o = 3 - (ax < 0 ? 0 : ax) - k;
                const double other = o == 0 ? dir[0] : o == 1 ? dir[1] : dir[2];
                const double part = u_t * (k == bx ? -other : other);
                drift = drift + part;
            }
        }
        const double th = vth * n[k];
        const double dt = drift + (flip ? -th : th);
        const double wv = r.vamp[k] * s;
        v[k] = dt + wv;
    }
}

// The checks of a radial request, in the order the messages name them: nullptr if it is good, else the message.
inline const char* check_radial(const struct fpic_load_radial& p, const double (&L)[3])
{
    if (p.geometry != FPIC_LOAD_SPHERE && p.geometry != FPIC_LOAD_CYLINDER) return ".geometry <- must be FPIC_LOAD_SPHERE or FPIC_LOAD_CYLINDER";
    if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) return ".reserved <- must be zero";
    if (p.axis < 0 || p.axis > 2) return ".axis <- must be 0, 1 or 2";
    const bool sphere = p.geometry == FPIC_LOAD_SPHERE;
    if (sphere && p.axis != 0) return ".axis <- must be 0 for a sphere";
    if (!(p.r_max > 0) || !std::isfinite(p.r_max)) return ".r_max <- must be positive and finite";
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(p.center[a]) || !(p.center[a] >= 0) || !(p.center[a] <= L[a])) return ".center <- must lie within the box";
        if ((sphere || a != p.axis) && !(2.0 * p.r_max <= L[a])) return ".r_max <- the diameter must not exceed the box length on an axis the body spans";
    }
    if (sphere && (p.azimuthal_n || p.axial_n)) return ".azimuthal_n <- a sphere takes no azimuthal or axial flow";
    const uint32_t counts[5] = { p.density_n, p.thermal_n, p.radial_n, p.azimuthal_n, p.axial_n };
    const double* const tabs[5] = { p.density, p.thermal, p.radial, p.azimuthal, p.axial };
    static const char* const bad_n[5] = { ".density_n <- a table has 2 .. FPIC_LOAD_TABLE_MAX nodes (0: none)", ".thermal_n <- a table has 2 .. FPIC_LOAD_TABLE_MAX nodes (0: none)",
                                          ".radial_n <- a table has 2 .. FPIC_LOAD_TABLE_MAX nodes (0: none)", ".azimuthal_n <- a table has 2 .. FPIC_LOAD_TABLE_MAX nodes (0: none)",
                                          ".axial_n <- a table has 2 .. FPIC_LOAD_TABLE_MAX nodes (0: none)" };
    static const char* const null_tab[5] = { ".density <- the table is null but its node count is not zero", ".thermal <- the table is null but its node count is not zero",
                                             ".radial <- the table is null but its node count is not zero", ".azimuthal <- the table is null but its node count is not zero",
                                             ".axial <- the table is null but its node count is not zero" };
    static const char* const not_finite[5] = { ".density <- values must be finite", ".thermal <- values must be finite", ".radial <- values must be finite",
                                               ".azimuthal <- values must be finite", ".axial <- values must be finite" };
    for (int t = 0; t < 5; ++t)
        if (counts[t] == 1 || counts[t] > kTableMax) return bad_n[t];
    for (int t = 0; t < 5; ++t)
        if (counts[t] && !tabs[t]) return null_tab[t];
    for (int t = 0; t < 5; ++t)
        for (uint32_t j = 0; j < counts[t]; ++j) {
            if (!std::isfinite(tabs[t][j])) return not_finite[t];
            if (t == 0 && tabs[t][j] < 0) return ".density <- values must not be negative";
            if (t == 1 && tabs[t][j] < 0) return ".thermal <- values must not be negative";
        }
    if (p.density_n) {
        double C[kTableMax];
        radial_cumulative(sphere, p.density, p.density_n, C);
        const double total = C[p.density_n - 1];
        if (!std::isfinite(total)) return ".density <- the total of the table must be finite";
        if (!(total > 0)) return ".density <- the table holds no mass (its total is 0)";
    }
    return nullptr;
}

// The tables of a checked request laid out in one block of doubles, as the kernels' buffer holds them: the density, its
// cumulative masses, then the thermal, radial, azimuthal and axial tables.  Returns the doubles needed; with `block` it
// fills them and sets q (pointers relative to `dev`, the address the block will have where it is read).
inline size_t radial_layout(const struct fpic_load_radial& p, const double (&L)[3], double* block, const double* dev, Radial* q)
{
    const uint32_t dn = p.density_n ? p.density_n : 2;
    size_t at = 2 * static_cast<size_t>(dn);
    if (block) {
        *q = Radial{};
        q->geometry = p.geometry;
        q->axis = p.axis;
        for (int a = 0; a < 3; ++a) {
            q->c_f[a] = p.center[a] / L[a];
            q->rl[a] = p.r_max / L[a];
        }
        for (uint32_t j = 0; j < dn; ++j) block[j] = p.density_n ? p.density[j] + 0.0 : 1.0;   // (-0 is +0)
        radial_cumulative(p.geometry == FPIC_LOAD_SPHERE, block, dn, block + dn);
        q->dens = dev; q->cum = dev + dn; q->dk = dn - 1;
    }
    const uint32_t counts[4] = { p.thermal_n, p.radial_n, p.azimuthal_n, p.axial_n };
    const double* const tabs[4] = { p.thermal, p.radial, p.azimuthal, p.axial };
    for (int t = 0; t < 4; ++t) {
        const uint32_t n = counts[t];
        if (!n) continue;
        if (block) {
            for (uint32_t j = 0; j < n; ++j) block[at + j] = tabs[t][j] + 0.0;
            (t == 0 ? q->therm : t == 1 ? q->ur : t == 2 ? q->ut : q->ua) = dev + at;
            (t == 0 ? q->tk : t == 1 ? q->rk : t == 2 ? q->zk : q->ak) = n - 1;
            q->needs_pos = 1;
        }
        at += n;
    }
    if (block) q->lds_doubles = static_cast<uint32_t>(at);
    return at;
}

} // namespace fesload
#endif
