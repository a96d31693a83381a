// fes_ionize_core.hpp — the rule of the electron-impact ionisation of a background gas of a CART3D handle (fpic_ionize; the
// passes are fes_ionize_kernels.hpp, the orchestration fes_ionize.inc.hpp): the request as the gas operator's request, the
// decision of one projectile, the outcome of an event, the tally terms, whether the events fit their targets, the checks of a
// request and the totals' conversion to the result.  Plain C++ that compiles for the host and the device, shared with a host
// test (tests/native/ionize_core_test.cpp, g++).  It joins pieces that exist: the request's shared fields, their checks and
// their host-side numbers are fpic_gas's (fesgas::check, rule_of, through gas_of), the window and the tapers
// fes_force_core.hpp's, the table lookup fes_fusion_core.hpp's, the normals and the Philox block fes_load_core.hpp's, the
// fit of a target fes_inject_core.hpp's (fesinj::fits), the fixed point fes_force_core.hpp's (floor_fix).
//
// What happens to projectile i depends on the request, the epoch, i and its stored state alone.  All arithmetic is double,
// every operation rounded once (build with -ffp-contract=off, as the library is); include/fusionpic.h states the rule in
// full.  In short, on the words W(b) = Philox4x32-10((i, epoch, stream, 0x1051E0 + b), (seed_lo, seed_hi)):
//   decide     fpic_gas's candidate, partner vb, relative speed g, below / above, lookup, tapers and acceptance, operation for
//              operation (fesgas::scatter up to its `collides`), on W(0) and W(1).  An accepted candidate is an EVENT.
//   outcome    gp2 = g g - thr thr; r = (W(2).w0 + 0.5) 2^-32; a1 = r gp2; a2 = gp2 - a1; g1 = sqrt(a1); g2 = sqrt(a2);
//              n1 = nhat(W(0).w2, w3), n2 = nhat(W(2).w1, w2) (ELASTIC's formula); v' = vb + g1 n1, vs = vb + g2 n2, vi = vb.
//              The gas atom is heavy and keeps its velocity: the ion's recoil is neglected.
//   tallies    primary: fesforce::tally of the stored velocities before and after (fpic_gas's); electron, ion: per new
//              particle floor(|v|^2 2^80) and floor(v[a] 2^80) of the STORED velocity (fpic_inject's, the energy diagnostics'
//              out-of-range rule).
#ifndef FES_IONIZE_CORE_HPP
#define FES_IONIZE_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_gas_core.hpp"
#include "fes_inject_core.hpp"

namespace fesion {

constexpr uint32_t kTag = 0x1051E0u;      // the fourth counter word of block 0; block b has kTag + b
constexpr int kEvent = fesgas::kCollided, kBelow = fesgas::kBelow, kAbove = fesgas::kAbove;   // what a decision reports
// the device words of a request: candidates, below, above | ionised | twelve 128-bit sums (lo, hi) — primary, electron, ion:
// energy, momentum x, y, z each — | the out-of-range bits (bit 4 group + quantity).  The deciding pass adds the first three,
// the generation pass the rest
constexpr int kCounts = 3;
constexpr int kGroups = 3, kSums = 4 * kGroups;
constexpr int kWords = kCounts + 1 + 2 * kSums + 1;
constexpr int kOutAt = kWords - 1;

// a request as the kernels read it: the gas operator's form (its kind and M are not read) and the squared threshold
struct Rule {
    fesgas::Rule g;
    double thr2;                       // g_threshold g_threshold
};

// the shared fields as the gas operator's request (EXCHANGE, which has no further field of its own)
inline fpic_gas_spec gas_of(const fpic_ionize_spec& s)
{
    fpic_gas_spec q{};
    q.species = s.species;
    q.kind = FPIC_GAS_EXCHANGE;
    q.seed = s.seed;
    q.stream = s.stream;
    q.epoch = s.epoch;
    q.density = s.density;
    q.tau = s.tau;
    q.g_lo = s.g_lo;
    q.g_hi = s.g_hi;
    q.n = s.n;
    q.sigma = s.sigma;
    for (int a = 0; a < 3; ++a) {
        q.drift[a] = s.drift[a];
        q.vth[a] = s.vth[a];
        q.lo[a] = s.lo[a];
        q.hi[a] = s.hi[a];
        q.taper_n[a] = s.taper_n[a];
        q.taper[a] = s.taper[a];
    }
    return q;
}

FES_HIST_HD void words(const Rule& r, uint32_t i, uint32_t block, uint32_t (&w)[4])
{
    fesload::philox(i, r.g.epoch, r.g.stream, kTag + block, r.g.seed_lo, r.g.seed_hi, w);
}

// the word half of the candidate test
FES_HIST_HD bool drawn(const Rule& r, uint32_t i)
{
    uint32_t w[4];
    words(r, i, 0u, w);
    return static_cast<uint64_t>(w[0]) < r.g.K;
}

// the partner of projectile i and the relative speed of the stored velocity v
FES_HIST_HD double partner(const Rule& r, uint32_t i, const double (&v)[3], double (&vb)[3])
{
    uint32_t w1[4];
    words(r, i, 1u, w1);
    double n[3], d[3];
    fesload::normals_from(w1, n);
    for (int a = 0; a < 3; ++a) {
        const double t = r.g.vth[a] * n[a];
        vb[a] = r.g.drift[a] + t;
        d[a] = v[a] - vb[a];
    }
    const double d00 = d[0] * d[0], d11 = d[1] * d[1], d22 = d[2] * d[2];
    const double d01 = d00 + d11;
    return sqrt(d01 + d22);
}

// A candidate's decision: p its stored position, v its stored velocity.  S, tab: where the tables are read.  Returns kEvent,
// kBelow, kAbove or 0; vb and *g: the partner and the relative speed (what outcome() takes)
FES_HIST_HD int decide(const Rule& r, const double* S, const double* const (&tab)[3], uint32_t i, const double (&p)[3], const double (&v)[3], double (&vb)[3], double* g_out)
{
    uint32_t w0[4];
    words(r, i, 0u, w0);
    const double g = partner(r, i, v, vb);
    *g_out = g;
    if (g < r.g.xs.g_lo) return kBelow;
    if (!(g < r.g.xs.g_hi)) return kAbove;   // (a NaN velocity: above)
    const double sigma = fesfusion::sigma_at(r.g.xs, S, g);
    double cr = r.g.column;
    if (r.g.win.tapered) cr = r.g.column * fesforce::taper_of(r.g.win, tab, p);
    const double cs = cr * sigma;
    double x = cs * g;
    if (x > r.g.x_max) x = r.g.x_max;
    const double u = (static_cast<double>(w0[1]) + 0.5) * fesload::kTwoM32;
    const double ux = u * r.g.x_max;
    return ux < x ? kEvent : 0;
}

// ELASTIC's direction on two words
FES_HIST_HD void nhat(uint32_t wc, uint32_t wp, double (&nh)[3])
{
    const double h = (static_cast<double>(wc) + 0.5) * fesload::kTwoM32;
    const double c = 1.0 - 2.0 * h;
    const double cc = c * c;
    const double s = sqrt(1.0 - cc);
    const double phi2 = 2.0 * fesload::fraction_of(wp);
    nh[0] = s * fesload::cospi_(phi2);
    nh[1] = s * fesload::sinpi_(phi2);
    nh[2] = c;
}

// the outcome of an event of projectile i with partner vb and relative speed g: the primary's and the secondary's velocities
// (the ion's is vb)
FES_HIST_HD void outcome(const Rule& r, uint32_t i, const double (&vb)[3], double g, double (&v1)[3], double (&vs)[3])
{
    uint32_t w0[4], w2[4];
    words(r, i, 0u, w0);
    words(r, i, 2u, w2);
    const double gg = g * g;
    const double gp2 = gg - r.thr2;
    const double share = (static_cast<double>(w2[0]) + 0.5) * fesload::kTwoM32;
    const double a1 = share * gp2;
    const double a2 = gp2 - a1;
    const double g1 = sqrt(a1), g2 = sqrt(a2);
    double n1[3], n2[3];
    nhat(w0[2], w0[3], n1);
    nhat(w2[1], w2[2], n2);
    for (int a = 0; a < 3; ++a) {
        const double t1 = g1 * n1[a], t2 = g2 * n2[a];
        v1[a] = vb[a] + t1;
        vs[a] = vb[a] + t2;
    }
}

// ---- the tally terms
using fesforce::Fix;
using fesforce::tally;    // the primary's: before / after
// what a target gained by one new particle of stored velocity w: sum[0] energy, sum[1 .. 3] momentum; the bits from `bit0` on
FES_HIST_HD void gain(const double (&w)[3], Fix* sum, unsigned long long& out, int bit0)
{
    const double w00 = w[0] * w[0], w11 = w[1] * w[1], w22 = w[2] * w[2];
    const double w01 = w00 + w11;
    const double q[4] = { w01 + w22, w[0], w[1], w[2] };
    for (int k = 0; k < 4; ++k) {
        if (fabs(q[k]) < fesforce::kFixRange) sum[k] += fesforce::floor_fix(q[k]);
        else out |= 1ull << (bit0 + k);
    }
}

// whether M events fit their targets: the electrons' (n, capacity, id span) and the ions'; nullptr, or which does not
inline const char* fit(uint64_t m, uint64_t n_e, uint64_t cap_e, uint64_t span_e, uint64_t n_i, uint64_t cap_i, uint64_t span_i)
{
    if (!fesinj::fits(n_e, cap_e, span_e, m)) return "electron";
    if (!fesinj::fits(n_i, cap_i, span_i, m)) return "ion";
    return nullptr;
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style).  The
// shared fields are held by fesgas::check itself; gas_of leaves that request's reserved words zero, so this one's are held here
inline const char* check(const fpic_ionize_spec* p, int nspecies, const double (&L)[3])
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    const fpic_ionize_spec& s = *p;
    if (s.reserved_i != 0 || s.reserved_n != 0 || s.reserved_u != 0) return ".reserved <- must be zero";
    for (double z : s.reserved)
        if (!(z == 0)) return ".reserved <- must be zero";
    const fpic_gas_spec q = gas_of(s);
    if (const char* why = fesgas::check(&q, nspecies, L)) return why;
    if (s.electron < 0 || s.electron >= nspecies) return ".electron <- no such species";
    if (s.ion < 0 || s.ion >= nspecies) return ".ion <- no such species";
    if (s.ion == s.species || s.ion == s.electron) return ".ion <- must differ from species and from electron";
    if (!(s.g_threshold >= 0) || std::isinf(s.g_threshold)) return ".g_threshold <- must be finite and not negative";
    if (s.g_lo < s.g_threshold) return ".g_lo <- the table must start at or above g_threshold";
    return nullptr;
}

// the kernels' form of a checked request at `epoch` (fesgas::rule_of's arguments)
inline Rule rule_of(const fpic_ionize_spec& s, const double (&L)[3], uint32_t epoch, const double* host_sigma, const double* sigma, const double* const* taper)
{
    Rule r{};
    r.g = fesgas::rule_of(gas_of(s), L, epoch, host_sigma, sigma, taper);
    r.thr2 = s.g_threshold * s.g_threshold;
    return r;
}
inline double x_max_of(const fpic_ionize_spec& s) { return fesgas::x_max_of(gas_of(s)); }

// the device words of a request -> the result but `applications`; mass, charge per group (primary, electron, ion); W: the box's
inline void result_of(const uint64_t* w, const double (&mass)[3], const double (&charge)[3], double W, fpic_ionize_result* out)
{
    out->candidates = w[0];
    out->below = w[1];
    out->above = w[2];
    out->ionised = w[3];
    fpic_ionize_gain* gains[3] = { &out->primary, &out->electron, &out->ion };
    for (int k = 0; k < kGroups; ++k) {
        fpic_ionize_gain& g = *gains[k];
        const uint64_t* s = w + kCounts + 1 + 8 * k;
        const uint64_t bits = w[kOutAt] >> (4 * k);
        const double ke = 0.5 * mass[k] * W * fesforce::kC * fesforce::kC, pm = mass[k] * W * fesforce::kC;   // the scales of the energy diagnostics
        g.energy_fixed[0] = s[0];
        g.energy_fixed[1] = s[1];
        g.energy = (bits & 1u) ? std::nan("") : ke * fesforce::fixed_to_double(s[0], s[1]);
        for (int a = 0; a < 3; ++a) {
            g.momentum_fixed[a][0] = s[2 + 2 * a];
            g.momentum_fixed[a][1] = s[3 + 2 * a];
            g.momentum[a] = (bits >> (1 + a) & 1u) ? std::nan("") : pm * fesforce::fixed_to_double(s[2 + 2 * a], s[3 + 2 * a]);
        }
        const double q = static_cast<double>(w[3]) * charge[k];
        g.charge = k == 0 ? 0.0 : q * W;
    }
}

} // namespace fesion
#endif
