// fes_fusion_core.hpp — the rule of the binary-reaction yield tally of a CART3D handle (fpic_fusion; the kernel is
// fes_fusion_kernels.hpp, the orchestration fes_fusion.inc.hpp): the host-side numbers of a request, the sort key, who pairs
// with whom in a cell, the yield of one pair in fixed point, and the checks of a request.  Plain C++ that compiles for the
// host and the device, shared with a host test (tests/native/fusion_core_test.cpp, g++); restated independently in numpy
// float64 and Python integers by tests/fusion_reference.py.
//
// It is a tally: it reads the stored velocities and writes nothing to any particle.  The result depends on the request, the
// epoch, the particles' ids, their cells and their stored velocities alone.  All arithmetic is double, every operation is one
// of + - x / sqrt and rounded once (build with -ffp-contract=off, as the library is); velocities are in units of c.
//
//   key        Philox4x32-10(counter (id, epoch, stream, 0xF0510), key (seed_lo, seed_hi))[0] — fesload::philox, with a tag
//              of its own: a tally never correlates with the Coulomb operator (0xC0120) on the same seed.
//   order      the particles of one species in a cell ascending by (key, id): fespair::before().
//   pairs      the cells, the order and the pair sets of fpic_pair (fes_pair_core.hpp).  Unlike species: Nm >= Nf the counts
//              of the cell, `many` the species with more (a tie: species_a); Nf = 0: nothing; the Nm pairs many[j] with
//              few[j mod Nf], N_L = Nf: the weights add to Nm Nf = Na Nb.  Like species: N < 2: nothing; N even: (s[2t],
//              s[2t+1]) with N_L = N; N odd: (s0,s1), (s1,s2), (s2,s0) with N_L = N / 2, then (s[3+2t], s[4+2t]) with N_L = N:
//              the weights add to N N / 2, the triple included.  like_pair(N, q) says which pair the place q owns: every pair
//              has exactly one owner, so every pair can have a lane of its own.
//   one pair   u = v_o - v_p (double, from the stored T values); g = sqrt((ux ux + uy uy) + uz uz).
//   the table  n values S[k] (m^2) at g_k = g_lo + k dg, dg = (g_hi - g_lo) / (n - 1); inv_dg = (n - 1) / (g_hi - g_lo).
//              g < g_lo: `below`; g >= g_hi: `above`; both contribute nothing.  Else t = (g - g_lo) inv_dg,
//              k = min(floor(t), n - 2), sigma = S[k] + (t - k) (S[k+1] - S[k]), then sigma = min(sigma, max S): a guard of
//              the last rounding, which never acts in exact arithmetic and keeps the bound below strict.
//   yield      y = ((((W W) N_L) tau) / dV) (sigma (g c)), real reactions: W the macro weight, dV the cell volume (m^3), tau
//              the time the application stands for (s), c = 2.998e8.
//   fixed point   y_bound = ((((W W) 2048) tau) / dV) (max S (g_hi c)); e = the smallest integer with y_bound < 2^(e + 40),
//              but not below kExponentMin; q = (int64) floor(y 2^-e).  Every operation above is monotone, so y <= y_bound and
//              q < 2^40.  A pair adds q to its cell's int64 word and q & 0xFFFFFFFF, q >> 32 to two uint64 totals, which the
//              host joins exactly (yield_hi 2^32 + yield_lo, in units of 2^e reactions).
//   the bound  a cell has at most 2048 pairs of q < 2^40: it receives fewer than 2^51 per application, so the int64 grid of a
//              registered operator is exact for at least 4096 applications between two drains (fpic_fusion_grid with reset).
//              NOTHING DETECTS AN OVERFLOW BEYOND THAT: the word wraps silently.  The totals' low word grows by less than
//              2^49 per application (a lane carries its low word into its high one before the workgroups add).
//   max S = 0  nothing can react: nothing is launched, every count but `applications` stays zero, e = 0.
#ifndef FES_FUSION_CORE_HPP
#define FES_FUSION_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_load_core.hpp"

namespace fesfusion {

constexpr uint32_t kTag = 0xF0510u;       // the fourth counter word of the key's block
constexpr double kC = 2.998e8;            // the box's c (fes_host_push.inc.hpp)
constexpr int kCellMax = 2048;            // = FPIC_PAIR_CELL_MAX: the largest N_L
constexpr int kQBits = 40;                // q < 2^40
constexpr int kExponentMin = -1000;       // 2^-e stays a finite double
enum { kInside = 0, kBelow = 1, kAbove = 2 };

// a request as the kernel reads it (the table itself is passed beside it)
struct Rule {
    uint32_t seed_lo, seed_hi, stream, epoch;
    int like;                          // species_a == species_b
    int n;                             // table entries
    int e;                             // the unit of q is 2^e reactions
    double g_lo, g_hi, inv_dg, s_max;
    double ww, tau, dv;                // W W, s, m^3
    double unit;                       // 2^-e
};

// the sort key of a particle
FES_HIST_HD uint32_t key_of(const Rule& r, uint32_t id)
{
    uint32_t w[4];
    fesload::philox(id, r.epoch, r.stream, kTag, r.seed_lo, r.seed_hi, w);
    return w[0];
}

// unlike species: whether species_a is the `many` one of a cell with na and nb particles
FES_HIST_HD bool many_is_a(uint32_t na, uint32_t nb) { return na >= nb; }
// unlike species: the place in the `few` segment of the partner of the `many` place p — the chain p belongs to
FES_HIST_HD uint32_t few_of(uint32_t p, uint32_t nf) { return p % nf; }

// like species: the pair that the place q of a cell's n sorted particles owns — false: none; else (s[q], s[partner]) with n_l
FES_HIST_HD bool like_pair(uint32_t n, uint32_t q, uint32_t& partner, double& n_l)
{
    if (n < 2u) return false;
    if (!(n & 1u)) {
        if (q & 1u) return false;
        partner = q + 1u;
        n_l = static_cast<double>(n);
        return true;
    }
    if (q < 3u) {                      // the triple: (s0,s1), (s1,s2), (s2,s0)
        partner = q == 2u ? 0u : q + 1u;
        n_l = static_cast<double>(n) * 0.5;
        return true;
    }
    if (!(q & 1u)) return false;
    partner = q + 1u;
    n_l = static_cast<double>(n);
    return true;
}

// the cross-section at g of [g_lo, g_hi): S is the table
FES_HIST_HD double sigma_at(const Rule& r, const double* S, double g)
{
    const double t = (g - r.g_lo) * r.inv_dg;
    int k = static_cast<int>(t);       // (0 <= t < about n: the truncation is the floor)
    if (k > r.n - 2) k = r.n - 2;
    const double f = t - static_cast<double>(k);
    const double d = S[k + 1] - S[k];
    const double s = S[k] + f * d;
    return s > r.s_max ? r.s_max : s;
}

// One pair: N_L and the two velocities.  Returns kInside (q is the pair's yield in units of 2^e, possibly 0), kBelow or
// kAbove (q = 0).
FES_HIST_HD int tally(const Rule& r, const double* S, double n_l, const double (&vo)[3], const double (&vp)[3], int64_t& q)
{
    q = 0;
    const double ux = vo[0] - vp[0], uy = vo[1] - vp[1], uz = vo[2] - vp[2];
    const double uxx = ux * ux, uyy = uy * uy, uzz = uz * uz;
    const double up2 = uxx + uyy;
    const double g = sqrt(up2 + uzz);
    if (g < r.g_lo) return kBelow;
    if (!(g < r.g_hi)) return kAbove;  // (a NaN velocity: above)
    const double sigma = sigma_at(r, S, g);
    const double w1 = r.ww * n_l, w2 = w1 * r.tau, w3 = w2 / r.dv;
    const double gc = g * kC, sv = sigma * gc;
    const double y = w3 * sv;
    q = static_cast<int64_t>(floor(y * r.unit));
    return kInside;
}

// the exponent of a bound: the smallest integer e with y_bound < 2^(e + 40), not below kExponentMin; 0 for y_bound == 0
inline int exponent_of(double y_bound)
{
    if (!(y_bound > 0)) return 0;
    int ex;
    (void)std::frexp(y_bound, &ex);    // y_bound = m 2^ex with m in [0.5, 1): 2^(ex-1) <= y_bound < 2^ex
    const int e = ex - kQBits;
    return e < kExponentMin ? kExponentMin : e;
}

inline double y_bound_of(double W, double tau, double dV, double s_max, double g_hi)
{
    const double ww = W * W, w1 = ww * static_cast<double>(kCellMax), w2 = w1 * tau, w3 = w2 / dV;
    const double gc = g_hi * kC, sv = s_max * gc;
    return w3 * sv;
}

inline double max_of(const double* S, int n)
{
    double m = 0;
    for (int k = 0; k < n; ++k) m = S[k] > m ? S[k] : m;
    return m;
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style,
// ".property <- what is wrong").  nspecies: the species the handle has.
inline const char* check(const fpic_fusion_spec* p, int nspecies)
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    const fpic_fusion_spec& s = *p;
    if (s.species_a < 0 || s.species_a >= nspecies) return ".species_a <- no such species";
    if (s.species_b < 0 || s.species_b >= nspecies) return ".species_b <- no such species";
    if (s.reserved_i != 0) return ".reserved <- must be zero";
    for (double z : s.reserved)
        if (!(z == 0)) return ".reserved <- must be zero";
    if (std::isnan(s.tau)) return ".tau <- must not be NaN";
    if (!(s.tau > 0) || std::isinf(s.tau)) return ".tau <- must be positive and finite";
    if (s.n < 2 || s.n > FPIC_FUSION_TABLE_MAX) return ".n <- must be 2 .. FPIC_FUSION_TABLE_MAX (4096)";
    if (!s.sigma) return ".sigma <- Non-optional property is undefined!";
    if (!(s.g_lo >= 0) || std::isinf(s.g_lo)) return ".g_lo <- must be finite and not negative";
    if (!(s.g_hi > s.g_lo) || std::isinf(s.g_hi)) return ".g_hi <- must be finite and above g_lo";
    for (int k = 0; k < s.n; ++k)
        if (!(s.sigma[k] >= 0) || std::isinf(s.sigma[k])) return ".sigma <- every entry must be finite and not negative";
    return nullptr;
}

// the bound of a checked request on this handle must be a finite double (W the macro weight, dV the cell volume)
inline const char* check_bound(const fpic_fusion_spec& s, double W, double dV)
{
    const double b = y_bound_of(W, s.tau, dV, max_of(s.sigma, s.n), s.g_hi);
    if (!(b >= 0) || std::isinf(b)) return ".sigma <- the yield bound W W 2048 tau max(sigma) g_hi c / dV is not a finite number";
    return nullptr;
}

// the kernel's form of a checked request, at `epoch`: the macro weight and the cell volume (m^3)
inline Rule rule_of(const fpic_fusion_spec& s, uint32_t epoch, double W, double dV)
{
    Rule r{};
    r.seed_lo = static_cast<uint32_t>(s.seed);
    r.seed_hi = static_cast<uint32_t>(s.seed >> 32);
    r.stream = s.stream;
    r.epoch = epoch;
    r.like = s.species_a == s.species_b;
    r.n = s.n;
    r.g_lo = s.g_lo;
    r.g_hi = s.g_hi;
    const double span = s.g_hi - s.g_lo;
    r.inv_dg = static_cast<double>(s.n - 1) / span;
    r.s_max = max_of(s.sigma, s.n);
    r.ww = W * W;
    r.tau = s.tau;
    r.dv = dV;
    r.e = exponent_of(y_bound_of(W, s.tau, dV, r.s_max, s.g_hi));
    r.unit = std::ldexp(1.0, -r.e);
    return r;
}

// the two total words as the host reports them: yield_hi 2^32 + yield_lo is the sum, yield_lo < 2^32
inline void join(uint64_t hi, uint64_t lo, uint64_t& out_hi, uint64_t& out_lo)
{
    out_hi = hi + (lo >> 32);
    out_lo = lo & 0xFFFFFFFFull;
}

} // namespace fesfusion
#endif
