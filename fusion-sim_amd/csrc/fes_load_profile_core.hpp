// fes_load_profile_core.hpp — the rule of a profiled load (fpic_load_profile) on top of fes_load_core.hpp: tabulated,
// separable profiles along the axes for the density, the thermal speed and one drift component.  Plain C++ that compiles
// for the host and the device, shared with a host test (tests/native/load_profile_core_test.cpp, g++).  As in
// fes_load_core.hpp all arithmetic is double, every operation rounded once (-ffp-contract=off), and every operation of a
// position is one of + - * / sqrt: the positions can be held bit for bit to an independent reference.
//
// A table of K + 1 nodes is uniformly spaced over the request's sub-box on its axis (node 0 at lo, node K at hi) and linear
// between the nodes.
//   density    the host sums the trapezoids in sequence: C[0] = 0, C[j+1] = C[j] + 0.5 (d[j] + d[j+1]).  With f the unit
//              fraction the plain rule draws on that axis (the random word or the lattice word):
//                  t    = f C[K]
//                  j    = the largest index with C[j] <= t, held to K - 1 (a binary search; an interval without mass has
//                         C[j] == C[j+1] and is never chosen)
//                  r    = t - C[j]
//                  disc = d[j] d[j] + (2 (d[j+1] - d[j])) r, held to 0 from below
//                  den  = d[j] + sqrt(disc)
//                  s    = den > 0 ? (2 r) / den : 0, held to 1 from above
//                  f'   = (j + s) / K; if !(f' < 1): f' = 1 - 2^-53
//              (s solves d[j] s + (d[j+1] - d[j]) s^2 / 2 = r in the form that does not cancel.)  Without a table f' = f.
//              The position is p_a = lo_f[a] + f' w_f[a]; theta, the displacement, the cast and wrap01 are the plain rule's.
//   lookup     (thermal, shear) with K the table's intervals and f' the fraction on its axis:
//                  g = f' K; j = min((int) g, K - 1); s = g - j; value = tab[j] + (tab[j+1] - tab[j]) s
//   velocity   vth_eff[a] = ((vth[a] sx) sy) sz, the thermal tables' values at the UNDISPLACED position (a missing table is a
//              factor of exactly 1: no multiply); drift_eff[c] = drift[c] + shear(f' of shear_axis) for c = shear_component;
//              then velocity_of's arithmetic with these two.  PAIRED negates the thermal term as in the plain rule.
#ifndef FES_LOAD_PROFILE_CORE_HPP
#define FES_LOAD_PROFILE_CORE_HPP
#include "fes_load_core.hpp"

namespace fesload {

constexpr uint32_t kTableMax = FPIC_LOAD_TABLE_MAX;
constexpr double kBelowOne = 1.0 - 1.0 / 9007199254740992.0;   // 1 - 2^-53: the largest double below 1

// the tables as the kernels read them.  k = the INTERVALS of a table (its nodes - 1), 0: no table
struct Profile {
    const double* dens[3];
    const double* cum[3];
    const double* therm[3];
    const double* shear;
    uint32_t dk[3], tk[3], sk;
    int32_t shear_axis, shear_comp;
    int needs_pos;            // a thermal or a shear table: the velocity reads the undisplaced position
    uint32_t lds_doubles;     // the doubles of the searched tables (every d and C): what a workgroup stages
};

// C[0 .. n) from d[0 .. n), summed in sequence
inline void cumulative(const double* d, uint32_t n, double* C)
{
    C[0] = 0.0;
    for (uint32_t j = 0; j + 1 < n; ++j) {
        const double pair = d[j] + d[j + 1];
        const double area = 0.5 * pair;
        C[j + 1] = C[j] + area;
    }
}

// f -> f' through the density table (d, C) of K intervals; j and s are the interval and the place in it
FES_HIST_HD double warp(const double* d, const double* C, uint32_t K, double f, uint32_t& j, double& s)
{
    const double t = f * C[K];
    uint32_t lo = 0, hi = K;                     // C[lo] <= t (C[0] = 0); the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (C[mid] <= t) lo = mid; else hi = mid;
    }
    j = lo;
    const double d0 = d[j], d1 = d[j + 1];
    const double r = t - C[j];
    const double sq = d0 * d0, slope = d1 - d0;
    const double twice = 2.0 * slope;
    const double lin = twice * r;
    double disc = sq + lin;
    if (disc < 0.0) disc = 0.0;
    const double den = d0 + sqrt(disc);
    const double num = 2.0 * r;
    s = den > 0.0 ? num / den : 0.0;
    if (s > 1.0) s = 1.0;
    const double at = static_cast<double>(j) + s;
    double fq = at / static_cast<double>(K);
    if (!(fq < 1.0)) fq = kBelowOne;
    return fq;
}
FES_HIST_HD double warp(const double* d, const double* C, uint32_t K, double f)
{
    uint32_t j;
    double s;
    return warp(d, C, K, f, j, s);
}

// the value of a table of K intervals at the fraction f of its axis
FES_HIST_HD double lookup(const double* tab, uint32_t K, double f, uint32_t& j, double& s)
{
    const double g = f * static_cast<double>(K);
    j = static_cast<uint32_t>(static_cast<int>(g));
    if (j > K - 1) j = K - 1;
    s = g - static_cast<double>(j);
    const double rise = tab[j + 1] - tab[j];
    const double part = rise * s;
    return tab[j] + part;
}
FES_HIST_HD double lookup(const double* tab, uint32_t K, double f)
{
    uint32_t j;
    double s;
    return lookup(tab, K, f, j, s);
}

// base_of with the density tables: the undisplaced position, its phase, and the fractions f' the other tables are read at
FES_HIST_HD void base_of(const Rule& r, const Profile& q, uint32_t i, double (&p)[3], double& theta, double (&fq)[3])
{
    uint32_t w[4];
    if (r.flags & FPIC_LOAD_LATTICE) {
        for (int a = 0; a < 3; ++a) w[a] = lattice_word(i, r.mult[a], r.shift[a]);
    } else {
        philox(i, r.stream, 0u, kTag, r.seed_lo, r.seed_hi, w);
    }
    for (int a = 0; a < 3; ++a) {
        double f = fraction_of(w[a]);
        if (q.dk[a]) f = warp(q.dens[a], q.cum[a], q.dk[a], f);
        fq[a] = f;
        const double t = f * r.w_f[a];
        p[a] = r.lo_f[a] + t;
    }
    const double tx = r.m[0] * p[0], ty = r.m[1] * p[1], tz = r.m[2] * p[2];
    const double txy = tx + ty;
    theta = txy + tz;
}

// velocity_of with vth_eff and drift_eff in place of vth and drift
FES_HIST_HD void velocity_of(const Rule& r, const Profile& q, uint32_t i, double theta, const double (&fq)[3], double (&v)[3])
{
    double n[3], scale[3], add = 0.0;
    normals_of(r, i, n);
    for (int b = 0; b < 3; ++b) scale[b] = q.tk[b] ? lookup(q.therm[b], q.tk[b], fq[b]) : 1.0;
    if (q.sk) add = lookup(q.shear, q.sk, q.shear_axis == 0 ? fq[0] : q.shear_axis == 1 ? fq[1] : fq[2]);   // (no indexed register array)
    const bool flip = (r.flags & FPIC_LOAD_PAIRED) && (i & 1u);
    const double s = r.waved ? sinpi_(2.0 * (theta + r.vphase)) : 0.0;
    for (int a = 0; a < 3; ++a) {
        double vth = r.vth[a];
        for (int b = 0; b < 3; ++b)
            if (q.tk[b]) vth = vth * scale[b];
        const double drift = (q.sk && a == q.shear_comp) ? r.drift[a] + add : r.drift[a];
        const double th = vth * n[a];
        const double dt = drift + (flip ? -th : th);
        const double wv = r.vamp[a] * s;
        v[a] = dt + wv;
    }
}

// does the profile hold any table?  (none: the call is fpic_load's)
inline bool any_table(const struct fpic_load_profile& p)
{
    return p.density_n[0] || p.density_n[1] || p.density_n[2] || p.thermal_n[0] || p.thermal_n[1] || p.thermal_n[2] || p.shear_n;
}

// The checks of a profile, in the order the messages name them: nullptr if it is good, else the message.
inline const char* check_profile(const struct fpic_load_profile& p)
{
    if (p.reserved[0] != 0 || p.reserved[1] != 0) return ".reserved <- must be zero";
    const auto nodes_bad = [](uint32_t n) { return n == 1 || n > kTableMax; };
    for (int a = 0; a < 3; ++a) {
        if (nodes_bad(p.density_n[a])) return ".density_n <- a table has 2 .. FPIC_LOAD_TABLE_MAX nodes (0: none)";
        if (nodes_bad(p.thermal_n[a])) return ".thermal_n <- a table has 2 .. FPIC_LOAD_TABLE_MAX nodes (0: none)";
    }
    if (nodes_bad(p.shear_n)) return ".shear_n <- a table has 2 .. FPIC_LOAD_TABLE_MAX nodes (0: none)";
    if (p.shear_axis < 0 || p.shear_axis > 2) return ".shear_axis <- must be 0, 1 or 2";
    if (p.shear_component < 0 || p.shear_component > 2) return ".shear_component <- must be 0, 1 or 2";
    for (int a = 0; a < 3; ++a) {
        if (p.density_n[a] && !p.density[a]) return ".density <- a table is null but its node count is not zero";
        if (p.thermal_n[a] && !p.thermal[a]) return ".thermal <- a table is null but its node count is not zero";
    }
    if (p.shear_n && !p.shear) return ".shear <- the table is null but its node count is not zero";
    for (int a = 0; a < 3; ++a) {
        double total = 0.0;
        for (uint32_t j = 0; j < p.density_n[a]; ++j) {
            const double d = p.density[a][j];
            if (!std::isfinite(d)) return ".density <- values must be finite";
            if (d < 0) return ".density <- values must not be negative";
            if (j) total += 0.5 * (p.density[a][j - 1] + d);
        }
        if (p.density_n[a] && !std::isfinite(total)) return ".density <- the total of a table must be finite";
        if (p.density_n[a] && !(total > 0)) return ".density <- a table holds no mass (its total is 0)";
        for (uint32_t j = 0; j < p.thermal_n[a]; ++j) {
            if (!std::isfinite(p.thermal[a][j])) return ".thermal <- values must be finite";
            if (p.thermal[a][j] < 0) return ".thermal <- values must not be negative";
        }
    }
    for (uint32_t j = 0; j < p.shear_n; ++j)
        if (!std::isfinite(p.shear[j])) return ".shear <- values must be finite";
    return nullptr;
}

// The tables of a checked profile laid out in one block of doubles, as the kernels' buffer holds them: per table its nodes,
// a density table followed by its cumulative masses.  Returns the doubles needed; with `block` it fills them and sets q's
// pointers relative to `dev` (the address the block will have where it is read).
inline size_t layout(const struct fpic_load_profile& p, double* block, const double* dev, Profile* q)
{
    size_t at = 0;
    if (q) *q = Profile{};
    for (int a = 0; a < 3; ++a) {
        if (const uint32_t n = p.density_n[a]) {
            if (block) {
                for (uint32_t j = 0; j < n; ++j) block[at + j] = p.density[a][j] + 0.0;   // (-0 is +0)
                cumulative(block + at, n, block + at + n);
                q->dens[a] = dev + at; q->cum[a] = dev + at + n; q->dk[a] = n - 1;
                q->lds_doubles += 2 * n;
            }
            at += 2 * static_cast<size_t>(n);
        }
        if (const uint32_t n = p.thermal_n[a]) {
            if (block) {
                for (uint32_t j = 0; j < n; ++j) block[at + j] = p.thermal[a][j] + 0.0;
                q->therm[a] = dev + at; q->tk[a] = n - 1; q->needs_pos = 1;
            }
            at += n;
        }
    }
    if (const uint32_t n = p.shear_n) {
        if (block) {
            for (uint32_t j = 0; j < n; ++j) block[at + j] = p.shear[j];
            q->shear = dev + at; q->sk = n - 1; q->needs_pos = 1;
            q->shear_axis = p.shear_axis; q->shear_comp = p.shear_component;
        }
        at += n;
    }
    return at;
}

} // namespace fesload
#endif
