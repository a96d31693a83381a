// fes_gas_core.hpp — the rule of the windowed background collisions with a tabulated cross-section of a CART3D handle
// (fpic_gas; the kernels are fes_gas_kernels.hpp, the orchestration fes_gas.inc.hpp): the host-side numbers of a request, the
// candidate test, the acceptance, the two updates, the tally terms of one particle, and the checks of a request.  Plain C++
// that compiles for the host and the device, shared with a host test (tests/native/gas_core_test.cpp, g++).  It joins pieces
// that exist: the window and the tapers of fes_force_core.hpp (fesforce::inside, taper_of), the table lookup of
// fes_fusion_core.hpp (fesfusion::sigma_at), the words, the partner and the updates of fes_collide_core.hpp.
//
// What happens to particle i (the id the box carries) depends on the request, the epoch, i and its stored state alone.  All
// arithmetic is double, every operation rounded once (build with -ffp-contract=off, as the library is); the stored T state is
// converted to double and the result is cast back to T.  Positions are box fractions, velocities in units of c.
//
//   words      W(b) = Philox4x32-10(counter (i, epoch, stream, 0x6A500 + b), key (seed_lo, seed_hi)) — fesload::philox, as
//              fescoll::words but with a tag of its own (0x10AD, 0xC0110/1, 0xC0120.., 0xF0510 are taken).
//              W(0) = (w0, w1, w2, w3): candidate, acceptance, two direction words; W(1): the partner's three normals
//              (fesload::normals_from).
//   numbers    (rule_of, on the host) column = (density c) tau; dg = (g_hi - g_lo) / (n - 1); per interval k
//              m_k = max(S[k], S[k+1]), g_{k+1} = g_lo + (k+1) dg (the last interval: g_hi), b_k = m_k g_{k+1};
//              x_max = column max_k b_k; P_max = -expm1(-x_max); K = (uint64) ldexp(P_max, 32);
//              M = mass_ratio / (1 + mass_ratio), 1 for +inf; the window's fractions as fesforce::rule_of forms them.
//   candidate  inside (fesforce::inside on the stored position, in double) and (uint64) w0 < K.  A set: the order of the two
//              tests is the pass's choice.
//   partner    vb[a] = drift[a] + vth[a] n[a]; d[a] = v[a] - vb[a]; g = sqrt((d0 d0 + d1 d1) + d2 d2).
//   table      g < g_lo: below; !(g < g_hi): above (a NaN too); neither collides.  Else sigma = fesfusion::sigma_at (with its
//              hold to max S).
//   acceptance cr = column, or column rho with rho = fesforce::taper_of (any taper table); cs = cr sigma; x = cs g;
//              x = min(x, x_max); u = (w1 + 0.5) 2^-32; ux = u x_max; collides iff ux < x.  The linearised null-collision
//              acceptance of fpic_collide (fescoll::scatter): x / x_max instead of (1 - exp(-x)) / P_max.
//   EXCHANGE   v' = vb.
//   ELASTIC    c = 1 - 2 (w2 + 0.5) 2^-32 (exact), s = sqrt(1 - c c), phi = w3 2^-32, nhat = (s cospi(2 phi), s sinpi(2 phi), c);
//              t = g nhat[a]; r = d[a] - t; q = M r; v'[a] = v[a] - q.
//   tallies    per collided particle, from the stored values before (v) and after ((T) v') in double:
//              energy += floor(((x' x' + y' y') + z' z') 2^80) - floor(((x x + y y) + z z) 2^80),
//              momentum[a] += floor(v'[a] 2^80) - floor(v[a] 2^80); a term with |term| >= 2^15 or not finite adds nothing and
//              sets the sum's bit (the forces' rule, fes_force_kernels.hpp).
#ifndef FES_GAS_CORE_HPP
#define FES_GAS_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_force_core.hpp"
#include "fes_fusion_core.hpp"

namespace fesgas {

constexpr uint32_t kTag = 0x6A500u;       // the fourth counter word of block 0; block b has kTag + b
constexpr double kC = 2.998e8;            // the box's c (fes_host_push.inc.hpp)
constexpr int kCollided = 1, kBelow = 2, kAbove = 4;   // what an update reports
// the device words of a request: candidates, below, above | the forces' ten (fesforce::kWords: collided in the place of
// `kicked`, energy in the place of work, momentum in the place of impulse, the out-of-range bits), so that
// fesforce::result_of, split_words and join_words serve them as they are
constexpr int kCounts = 3;
constexpr int kWords = kCounts + fesforce::kWords;
constexpr int kSumWords = kCounts + fesforce::kSumWords;

// a request as the kernels read it; sigma and win.tab are where the kernels read the tables (device pointers in the library)
struct Rule {
    int kind;
    uint32_t seed_lo, seed_hi, stream, epoch;
    uint64_t K;                        // candidates have w0 < K; 0 .. 2^32 - 1
    double column, x_max;
    double drift[3], vth[3];
    double M;                          // ELASTIC
    const double* sigma;
    fesfusion::Rule xs;                // n, g_lo, g_hi, inv_dg, s_max: what fesfusion::sigma_at reads
    fesforce::Rule win;                // lo_f, hi_f, w, tk, tab, tapered, whole: what fesforce::inside and taper_of read
};

FES_HIST_HD void words(const Rule& r, uint32_t i, uint32_t block, uint32_t (&w)[4])
{
    fesload::philox(i, r.epoch, r.stream, kTag + block, r.seed_lo, r.seed_hi, w);
}

// the word half of the candidate test
FES_HIST_HD bool drawn(const Rule& r, uint32_t i)
{
    uint32_t w[4];
    words(r, i, 0u, w);
    return static_cast<uint64_t>(w[0]) < r.K;
}

// A candidate's update: p its stored position, v read, and rewritten if the candidate collides.  S, tab: where the tables are
// read (r.sigma and r.win.tab, or a workgroup's copies).  Returns kCollided, kBelow, kAbove or 0.
FES_HIST_HD int scatter(const Rule& r, const double* S, const double* const (&tab)[3], uint32_t i, const double (&p)[3], double (&v)[3])
{
    uint32_t w0[4], w1[4];
    words(r, i, 0u, w0);
    words(r, i, 1u, w1);
    double n[3], vb[3], d[3];
    fesload::normals_from(w1, n);
    for (int a = 0; a < 3; ++a) {
        const double t = r.vth[a] * n[a];
        vb[a] = r.drift[a] + t;
        d[a] = v[a] - vb[a];
    }
    const double d00 = d[0] * d[0], d11 = d[1] * d[1], d22 = d[2] * d[2];
    const double d01 = d00 + d11;
    const double g = sqrt(d01 + d22);
    if (g < r.xs.g_lo) return kBelow;
    if (!(g < r.xs.g_hi)) return kAbove;   // (a NaN velocity: above)
    const double sigma = fesfusion::sigma_at(r.xs, S, g);
    double cr = r.column;
    if (r.win.tapered) cr = r.column * fesforce::taper_of(r.win, tab, p);
    const double cs = cr * sigma;
    double x = cs * g;
    if (x > r.x_max) x = r.x_max;
    const double u = (static_cast<double>(w0[1]) + 0.5) * fesload::kTwoM32;
    const double ux = u * r.x_max;
    if (!(ux < x)) return 0;
    if (r.kind == FPIC_GAS_EXCHANGE) {
        for (int a = 0; a < 3; ++a) v[a] = vb[a];
    } else {
        const double h = (static_cast<double>(w0[2]) + 0.5) * fesload::kTwoM32;
        const double c = 1.0 - 2.0 * h;
        const double cc = c * c;
        const double s = sqrt(1.0 - cc);
        const double phi2 = 2.0 * fesload::fraction_of(w0[3]);
        const double nh[3] = { s * fesload::cospi_(phi2), s * fesload::sinpi_(phi2), c };
        for (int a = 0; a < 3; ++a) {
            const double t = g * nh[a];
            const double rr = d[a] - t;
            const double q = r.M * rr;
            v[a] = v[a] - q;
        }
    }
    return kCollided;
}

// the whole rule for one live particle (the host test's form; the kernels call the pieces): what scatter reports, and
// *is_candidate
inline int apply(const Rule& r, uint32_t i, const double (&p)[3], double (&v)[3], bool* is_candidate)
{
    *is_candidate = fesforce::inside(r.win, p) && drawn(r, i);
    if (!*is_candidate) return 0;
    const double* const tab[3] = { r.win.tab[0], r.win.tab[1], r.win.tab[2] };
    return scatter(r, r.sigma, tab, i, p, v);
}

// ---- the tally terms: the forces' (fes_force_core.hpp), energy in the place of work, momentum in the place of impulse
using fesforce::Fix;
using fesforce::floor_fix;
using fesforce::tally;

// ---- the host-side numbers
inline double column_of(const fpic_gas_spec& s)
{
    const double dc = s.density * kC;
    return dc * s.tau;
}

// max_k b_k of a table
inline double bound_of(const double* S, int n, double g_lo, double g_hi)
{
    const double span = g_hi - g_lo;
    const double dg = span / static_cast<double>(n - 1);
    double best = 0;
    for (int k = 0; k + 1 < n; ++k) {
        const double m = S[k] > S[k + 1] ? S[k] : S[k + 1];
        const double step = static_cast<double>(k + 1) * dg;
        const double g1 = k == n - 2 ? g_hi : g_lo + step;
        const double b = m * g1;
        best = b > best ? b : best;
    }
    return best;
}

inline double x_max_of(const fpic_gas_spec& s) { return column_of(s) * bound_of(s.sigma, s.n, s.g_lo, s.g_hi); }

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style,
// ".property <- what is wrong").  nspecies: the species the handle has; L: the box in metres.
inline const char* check(const fpic_gas_spec* p, int nspecies, const double (&L)[3])
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    const fpic_gas_spec& s = *p;
    if (s.kind != FPIC_GAS_EXCHANGE && s.kind != FPIC_GAS_ELASTIC) return ".kind <- must be 0 (exchange) or 1 (elastic)";
    if (s.species < 0 || s.species >= nspecies) return ".species <- no such species";
    if (s.reserved_i != 0 || s.reserved_u != 0) return ".reserved <- must be zero";
    for (double z : s.reserved)
        if (!(z == 0)) return ".reserved <- must be zero";
    if (!(s.density >= 0) || std::isinf(s.density)) return ".density <- must be finite and not negative";
    if (!(s.tau > 0) || std::isinf(s.tau)) return ".tau <- must be positive and finite";
    if (s.n < 2 || s.n > FPIC_GAS_TABLE_MAX) return ".n <- must be 2 .. FPIC_GAS_TABLE_MAX (4096)";
    if (!s.sigma) return ".sigma <- Non-optional property is undefined!";
    if (!(s.g_lo >= 0) || std::isinf(s.g_lo)) return ".g_lo <- must be finite and not negative";
    if (!(s.g_hi > s.g_lo) || std::isinf(s.g_hi)) return ".g_hi <- must be finite and above g_lo";
    for (int k = 0; k < s.n; ++k)
        if (!(s.sigma[k] >= 0) || std::isinf(s.sigma[k])) return ".sigma <- every entry must be finite and not negative";
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(s.drift[a])) return ".drift <- must be finite";
        if (!std::isfinite(s.vth[a]) || s.vth[a] < 0) return ".vth <- must be finite and not negative";
    }
    if (s.kind == FPIC_GAS_ELASTIC) {
        if (!(s.mass_ratio > 0)) return ".mass_ratio <- must be positive (+inf: a fixed target) for FPIC_GAS_ELASTIC";
    } else if (!(s.mass_ratio == 0)) {
        return ".mass_ratio <- must be 0 for FPIC_GAS_EXCHANGE";
    }
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(s.lo[a]) || !std::isfinite(s.hi[a])) return ".lo, .hi <- must be finite";
        if (!(0 <= s.lo[a] && s.lo[a] < s.hi[a] && s.hi[a] <= L[a])) return ".lo, .hi <- the window must lie within 0 <= lo < hi <= L";
    }
    for (int a = 0; a < 3; ++a) {
        if (s.taper_n[a] == 1 || s.taper_n[a] > FPIC_GAS_TAPER_MAX) return ".taper_n <- a table has 2 .. FPIC_GAS_TAPER_MAX nodes (0: none)";
        if (s.taper_n[a] && !s.taper[a]) return ".taper <- a table is null but its node count is not zero";
    }
    for (int a = 0; a < 3; ++a)
        for (uint32_t k = 0; k < s.taper_n[a]; ++k)
            if (!(s.taper[a][k] >= 0 && s.taper[a][k] <= 1)) return ".taper <- the nodes must lie in [0, 1] (the density as a fraction of its peak)";
    if (!std::isfinite(x_max_of(s))) return ".sigma <- the candidate bound density c tau max(sigma g) is not a finite number";
    return nullptr;
}

// the kernels' form of a checked request at `epoch`: sigma, taper[a] = where the kernels read the tables; host_sigma = the
// host's copy of the cross-sections (s.sigma may have been dropped)
inline Rule rule_of(const fpic_gas_spec& s, const double (&L)[3], uint32_t epoch, const double* host_sigma, const double* sigma, const double* const* taper)
{
    Rule r{};
    r.kind = s.kind;
    r.seed_lo = static_cast<uint32_t>(s.seed);
    r.seed_hi = static_cast<uint32_t>(s.seed >> 32);
    r.stream = s.stream;
    r.epoch = epoch;
    r.column = column_of(s);
    r.x_max = r.column * bound_of(host_sigma, s.n, s.g_lo, s.g_hi);
    const double p_max = -std::expm1(-r.x_max);
    r.K = static_cast<uint64_t>(std::ldexp(p_max, 32));
    r.M = std::isinf(s.mass_ratio) ? 1.0 : s.mass_ratio / (1.0 + s.mass_ratio);
    r.sigma = sigma;
    r.xs.n = s.n;
    r.xs.g_lo = s.g_lo;
    r.xs.g_hi = s.g_hi;
    const double span = s.g_hi - s.g_lo;
    r.xs.inv_dg = static_cast<double>(s.n - 1) / span;
    r.xs.s_max = fesfusion::max_of(host_sigma, s.n);
    r.win.whole = 1;
    for (int a = 0; a < 3; ++a) {
        r.drift[a] = s.drift[a];
        r.vth[a] = s.vth[a];
        r.win.lo_f[a] = s.lo[a] / L[a];
        r.win.hi_f[a] = s.hi[a] / L[a];
        r.win.w[a] = r.win.hi_f[a] - r.win.lo_f[a];
        r.win.tk[a] = s.taper_n[a] ? s.taper_n[a] - 1 : 0;
        r.win.tab[a] = s.taper_n[a] ? taper[a] : nullptr;
        if (s.taper_n[a]) r.win.tapered = 1;
        if (!(r.win.lo_f[a] == 0.0 && r.win.hi_f[a] == 1.0)) r.win.whole = 0;
    }
    return r;
}

// the device words of a request (kWords of them) -> the result but `applications`; mass, W: the species' and the box's
inline void result_of(const uint64_t* w, double mass, double W, fpic_gas_result* out)
{
    fpic_force_result f{};
    fesforce::result_of(w + kCounts, mass, W, &f);
    out->candidates = w[0];
    out->below = w[1];
    out->above = w[2];
    out->collided = f.kicked;
    out->energy_fixed[0] = f.work_fixed[0];
    out->energy_fixed[1] = f.work_fixed[1];
    out->energy = f.work;
    for (int a = 0; a < 3; ++a) {
        out->momentum_fixed[a][0] = f.impulse_fixed[a][0];
        out->momentum_fixed[a][1] = f.impulse_fixed[a][1];
        out->momentum[a] = f.impulse[a];
    }
}

// the words of several ranks added exactly (fesforce::split_words for the sums, the counts as they are): kSumWords words
inline void split_words(const uint64_t* w, uint64_t* s)
{
    for (int c = 0; c < kCounts; ++c) s[c] = w[c];
    fesforce::split_words(w + kCounts, s + kCounts);
}
inline void join_words(const uint64_t* s, uint64_t* w)
{
    for (int c = 0; c < kCounts; ++c) w[c] = s[c];
    fesforce::join_words(s + kCounts, w + kCounts);
}

} // namespace fesgas
#endif
