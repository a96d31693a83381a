// fes_collide_core.hpp — the rule of the Monte Carlo collision operator of a CART3D handle (fpic_collide; the kernels are
// fes_collide_kernels.hpp, the orchestration fes_collide.inc.hpp): the host-side numbers of a request, the candidate test,
// the three updates, and the checks of a request.  Plain C++ that compiles for the host and the device, shared with a host
// test (tests/native/collide_core_test.cpp, g++).
//
// What happens to particle i (the id the box carries) depends on the request, the epoch, i and its stored velocity alone.
// All arithmetic is double, every operation rounded once (build with -ffp-contract=off, as the library is); a stored T
// velocity is converted to double and the result is cast back to T.  Velocities are in units of c.
//
//   words      W(b) = Philox4x32-10(counter (i, epoch, stream, 0xC0110 + b), key (seed_lo, seed_hi)) — fesload::philox.
//              W(0) = (w0, w1, w2, w3): candidate, acceptance, two direction words; W(1): the partner's three normals
//              (fesload::normals_from, the loader's Box-Muller step).
//   numbers    (rule_of, on the host) x_max = nu_tau + sigma_tau g_max; P_max = -expm1(-x_max); K = (uint64) ldexp(P_max, 32),
//              2^32 for x_max = +inf; M = mass_ratio / (1 + mass_ratio), 1 for +inf; decay = exp(-nu_tau),
//              sv[a] = sqrt(-expm1(-2 nu_tau)) vth[a].
//   candidate  (EXCHANGE, ELASTIC) (uint64) w0 < K: integers, so candidacy never depends on rounding.
//   partner    vb[a] = drift[a] + vth[a] n[a]; d[a] = v[a] - vb[a]; g = sqrt((d0 d0 + d1 d1) + d2 d2).
//   acceptance sigma_tau == 0: every candidate.  Else x = nu_tau + sigma_tau min(g, g_max), u = (w1 + 0.5) 2^-32, collides
//              iff u x_max < x; g > g_max is counted as clipped.
//   EXCHANGE   v' = vb.
//   ELASTIC    c = 1 - 2 (w2 + 0.5) 2^-32 (exact), s = sqrt(1 - c c), phi = w3 2^-32, nhat = (s cospi(2 phi), s sinpi(2 phi), c);
//              t = g nhat[a]; r = d[a] - t; q = M r; v'[a] = v[a] - q.
//   RELAX      every live particle: r = v[a] - drift[a]; p = decay r; k = sv[a] n[a]; q = p + k; v'[a] = drift[a] + q.
#ifndef FES_COLLIDE_CORE_HPP
#define FES_COLLIDE_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_load_core.hpp"

namespace fescoll {

constexpr uint32_t kTag = 0xC0110u;       // the fourth counter word of block 0; block b has kTag + b
constexpr int kCollided = 1, kClipped = 2;   // what an update reports

// a request as the kernels read it
struct Rule {
    int kind, nullc;                   // nullc: sigma_tau != 0, the acceptance test runs
    uint32_t seed_lo, seed_hi, stream, epoch;
    uint64_t K;                        // candidates have w0 < K; 0 .. 2^32
    double nu_tau, sigma_tau, g_max, x_max;
    double drift[3], vth[3];
    double M;                          // ELASTIC
    double decay, sv[3];               // RELAX
};

FES_HIST_HD void words(const Rule& r, uint32_t i, uint32_t block, uint32_t (&w)[4])
{
    fesload::philox(i, r.epoch, r.stream, kTag + block, r.seed_lo, r.seed_hi, w);
}

// whether particle i is a candidate of an EXCHANGE or ELASTIC request (the caller has found it live)
FES_HIST_HD bool candidate(const Rule& r, uint32_t i)
{
    uint32_t w[4];
    words(r, i, 0u, w);
    return static_cast<uint64_t>(w[0]) < r.K;
}

// a candidate's update: v is read, and rewritten if the candidate collides.  Returns kCollided | kClipped bits.
template <int KIND, bool NULLC>
FES_HIST_HD int scatter(const Rule& r, uint32_t i, double (&v)[3])
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
    double g = 0;
    int what = kCollided;
    if (NULLC || KIND == FPIC_COLLIDE_ELASTIC) {
        const double d00 = d[0] * d[0], d11 = d[1] * d[1], d22 = d[2] * d[2];
        const double d01 = d00 + d11;
        g = sqrt(d01 + d22);
    }
    if (NULLC) {
        const double gm = g < r.g_max ? g : r.g_max;
        const double sg = r.sigma_tau * gm;
        const double x = r.nu_tau + sg;
        const double u = (static_cast<double>(w0[1]) + 0.5) * fesload::kTwoM32;
        const double ux = u * r.x_max;
        what = (ux < x ? kCollided : 0) | (g > r.g_max ? kClipped : 0);
        if (!(what & kCollided)) return what;
    }
    if (KIND == FPIC_COLLIDE_EXCHANGE) {
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
    return what;
}

// the RELAX update of a live particle
FES_HIST_HD void relax(const Rule& r, uint32_t i, double (&v)[3])
{
    uint32_t w1[4];
    words(r, i, 1u, w1);
    double n[3];
    fesload::normals_from(w1, n);
    for (int a = 0; a < 3; ++a) {
        const double rr = v[a] - r.drift[a];
        const double p = r.decay * rr;
        const double k = r.sv[a] * n[a];
        const double q = p + k;
        v[a] = r.drift[a] + q;
    }
}

// the whole rule for one live particle (the host test's form; the kernels call the pieces): the bits of `what`, and
// *is_candidate
inline int apply(const Rule& r, uint32_t i, double (&v)[3], bool* is_candidate)
{
    if (r.kind == FPIC_COLLIDE_RELAX) {
        *is_candidate = false;
        relax(r, i, v);
        return kCollided;
    }
    *is_candidate = candidate(r, i);
    if (!*is_candidate) return 0;
    if (r.kind == FPIC_COLLIDE_EXCHANGE) return r.nullc ? scatter<FPIC_COLLIDE_EXCHANGE, true>(r, i, v) : scatter<FPIC_COLLIDE_EXCHANGE, false>(r, i, v);
    return r.nullc ? scatter<FPIC_COLLIDE_ELASTIC, true>(r, i, v) : scatter<FPIC_COLLIDE_ELASTIC, false>(r, i, v);
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style,
// ".property <- what is wrong").  nspecies: the species the handle has.
inline const char* check(const fpic_collide_spec* p, int nspecies)
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    const fpic_collide_spec& s = *p;
    if (s.kind != FPIC_COLLIDE_EXCHANGE && s.kind != FPIC_COLLIDE_ELASTIC && s.kind != FPIC_COLLIDE_RELAX)
        return ".kind <- must be 0 (exchange), 1 (elastic) or 2 (relax)";
    if (s.species < 0 || s.species >= nspecies) return ".species <- no such species";
    for (double z : s.reserved)
        if (!(z == 0)) return ".reserved <- must be zero";
    if (std::isnan(s.nu_tau)) return ".nu_tau <- must not be NaN";
    if (std::isnan(s.sigma_tau)) return ".sigma_tau <- must not be NaN";
    if (std::isnan(s.g_max)) return ".g_max <- must not be NaN";
    if (std::isnan(s.mass_ratio)) return ".mass_ratio <- must not be NaN";
    if (s.nu_tau < 0) return ".nu_tau <- must not be negative";
    if (s.sigma_tau < 0 || std::isinf(s.sigma_tau)) return ".sigma_tau <- must be finite and not negative";
    if (s.sigma_tau > 0) {
        if (!(s.g_max > 0) || std::isinf(s.g_max)) return ".g_max <- must be positive and finite when sigma_tau > 0";
        if (std::isinf(s.nu_tau)) return ".nu_tau <- +inf needs sigma_tau == 0 (the acceptance x / x_max would be inf / inf)";
    } else if (s.g_max != 0) {
        return ".g_max <- must be 0 when sigma_tau == 0";
    }
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(s.drift[a])) return ".drift <- must be finite";
        if (!std::isfinite(s.vth[a]) || s.vth[a] < 0) return ".vth <- must be finite and not negative";
    }
    if (s.kind == FPIC_COLLIDE_ELASTIC) {
        if (!(s.mass_ratio > 0)) return ".mass_ratio <- must be positive (+inf: a fixed target) for FPIC_COLLIDE_ELASTIC";
    } else if (s.mass_ratio != 0) {
        return ".mass_ratio <- must be 0 for a kind other than FPIC_COLLIDE_ELASTIC";
    }
    if (s.kind == FPIC_COLLIDE_RELAX) {
        if (s.sigma_tau != 0) return ".sigma_tau <- must be 0 for FPIC_COLLIDE_RELAX";
        if (!(s.nu_tau > 0) || std::isinf(s.nu_tau)) return ".nu_tau <- must be positive and finite for FPIC_COLLIDE_RELAX";
    }
    return nullptr;
}

// the kernels' form of a checked request, at `epoch`
inline Rule rule_of(const fpic_collide_spec& s, uint32_t epoch)
{
    Rule r{};
    r.kind = s.kind;
    r.nullc = s.sigma_tau != 0;
    r.seed_lo = static_cast<uint32_t>(s.seed);
    r.seed_hi = static_cast<uint32_t>(s.seed >> 32);
    r.stream = s.stream;
    r.epoch = epoch;
    r.nu_tau = s.nu_tau;
    r.sigma_tau = s.sigma_tau;
    r.g_max = s.g_max;
    const double sg = s.sigma_tau * s.g_max;
    r.x_max = s.nu_tau + sg;
    const double p_max = -std::expm1(-r.x_max);
    r.K = std::isinf(r.x_max) ? uint64_t(1) << 32 : static_cast<uint64_t>(std::ldexp(p_max, 32));
    r.M = std::isinf(s.mass_ratio) ? 1.0 : s.mass_ratio / (1.0 + s.mass_ratio);
    r.decay = std::exp(-s.nu_tau);
    const double spread = std::sqrt(-std::expm1(-2.0 * s.nu_tau));
    for (int a = 0; a < 3; ++a) {
        r.drift[a] = s.drift[a];
        r.vth[a] = s.vth[a];
        r.sv[a] = spread * s.vth[a];
    }
    return r;
}

} // namespace fescoll
#endif
