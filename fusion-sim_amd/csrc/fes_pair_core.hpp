// fes_pair_core.hpp — the rule of the binary Coulomb collision operator of a CART3D handle (fpic_pair; Takizuka & Abe 1977;
// the kernels are fes_pair_kernels.hpp, the orchestration fes_pair.inc.hpp): the host-side numbers of a request, the sort
// key, who pairs with whom in a cell, the update of one pair, and the checks of a request.  Plain C++ that compiles for the
// host and the device, shared with a host test (tests/native/pair_core_test.cpp, g++).
//
// The result depends on the request, the epoch, the particles' ids, their cells and their stored velocities alone.  All
// arithmetic is double, every operation rounded once (build with -ffp-contract=off, as the library is); a stored T velocity
// is converted to double, and AFTER EVERY PAIR both velocities are cast back to T (settle<T>): a particle's next pair starts
// from the cast value.  Velocities are in units of c.
//
//   words      P(b) = Philox4x32-10(counter (id, epoch, stream, 0xC0120 + b), key (seed_lo, seed_hi)) — fesload::philox.
//   order      the particles of one species in a cell ascending by (P(0)[0] of their own id, id): before().
//   numbers    (rule_of, on the host) m_ab = (m_a m_b) / (m_a + m_b); qq = q_a q_b;
//              kappa = ((((qq qq) log_lambda) tau) W) / (((((8 pi) (eps0 eps0)) (m_ab m_ab)) ((c c) c)) dV);
//              fa = m_ab / m_a, fb = m_ab / m_b.
//   unlike     Nm >= Nf the counts of the cell, `many` the species with more (a tie: species_a: many_is_a).  Nf = 0: nothing.
//              many[j] pairs with few[j mod Nf]; few[q] takes j = q, q + Nf, ... in ascending order; the owner of a pair is
//              the many particle; N_L = Nf.
//   like       N < 2: nothing.  N even: (s[2t], s[2t+1]), N_L = N.  N odd: (s0,s1), (s1,s2), (s2,s0) with N_L = N / 2, then
//              (s[3+2t], s[4+2t]) with N_L = N.  The owner is the first member.  like_lead(N, q) says what starts at s[q].
//   one pair   collide(): see the operation order there; it is restated identically in tests/pair_reference.py.
#ifndef FES_PAIR_CORE_HPP
#define FES_PAIR_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_load_core.hpp"

namespace fespair {

constexpr uint32_t kTag = 0xC0120u;       // the fourth counter word of block 0; block b has kTag + b
constexpr int kCounted = 1, kStrong = 2;  // what a pair reports
constexpr double kEps0 = 8.8541878128e-12, kC = 2.998e8;   // the constants of the box (fes_host_push.inc.hpp)
constexpr double kPi = 3.14159265358979323846;
enum { kNothing = 0, kPairLead = 1, kTripleLead = 3 };      // like_lead()

// a request as the kernels read it
struct Rule {
    uint32_t seed_lo, seed_hi, stream, epoch;
    int like;                          // species_a == species_b
    double kappa, fa, fb;
};

FES_HIST_HD void words(const Rule& r, uint32_t id, uint32_t block, uint32_t (&w)[4])
{
    fesload::philox(id, r.epoch, r.stream, kTag + block, r.seed_lo, r.seed_hi, w);
}

// the sort key of a particle
FES_HIST_HD uint32_t key_of(const Rule& r, uint32_t id)
{
    uint32_t w[4];
    words(r, id, 0u, w);
    return w[0];
}
FES_HIST_HD bool before(uint32_t key_x, uint32_t id_x, uint32_t key_y, uint32_t id_y)
{
    return key_x < key_y || (key_x == key_y && id_x < id_y);
}

// unlike species: whether species_a is the `many` one of a cell with na and nb particles
FES_HIST_HD bool many_is_a(uint32_t na, uint32_t nb) { return na >= nb; }

// like species: what starts at s[q] of a cell's n sorted particles — nothing, a pair (s[q], s[q+1]) or the triple (s0, s1, s2)
FES_HIST_HD int like_lead(uint32_t n, uint32_t q)
{
    if (n < 2u) return kNothing;
    if (!(n & 1u)) return (q & 1u) ? kNothing : kPairLead;
    if (q == 0u) return kTripleLead;
    return (q >= 3u && (q & 1u)) ? kPairLead : kNothing;
}
FES_HIST_HD double like_nl(uint32_t n, int lead) { return lead == kTripleLead ? static_cast<double>(n) * 0.5 : static_cast<double>(n); }

// the cast back to the stored type after a pair
template <typename T>
FES_HIST_HD void settle(double (&v)[3])
{
    for (int a = 0; a < 3; ++a) v[a] = static_cast<double>(static_cast<T>(v[a]));
}

// One pair: the owner's id, N_L, the mass factors of the owner and of the partner, the two velocities (rewritten unless
// g == 0).  Returns kCounted | kStrong bits.  The caller settles both velocities afterwards.
FES_HIST_HD int collide(const Rule& r, uint32_t owner, double n_l, double fo, double fp, double (&vo)[3], double (&vp)[3])
{
    const double ux = vo[0] - vp[0], uy = vo[1] - vp[1], uz = vo[2] - vp[2];
    const double uxx = ux * ux, uyy = uy * uy, uzz = uz * uz;
    const double up2 = uxx + uyy;
    const double up = sqrt(up2);
    const double g = sqrt(up2 + uzz);
    if (g == 0) return 0;
    const double kn = r.kappa * n_l;
    const double g2 = g * g;
    const double g3 = g2 * g;
    const double var = kn / g3;
    uint32_t w0[4], w1[4];
    words(r, owner, 0u, w0);
    words(r, owner, 1u, w1);
    double n[3];
    fesload::normals_from(w1, n);
    const double delta = sqrt(var) * n[0];
    const double d2 = delta * delta;
    const double den = 1.0 + d2;
    const double sinT = (2.0 * delta) / den;
    const double omc = (2.0 * d2) / den;
    const double phi2 = 2.0 * fesload::fraction_of(w0[1]);
    const double cs = fesload::cospi_(phi2), sn = fesload::sinpi_(phi2);
    double du[3];
    if (up > 0) {
        const double ex = ux / up, ey = uy / up;
        const double a1 = ex * uz, a2 = a1 * sinT, a3 = a2 * cs;
        const double b1 = ey * g, b2 = b1 * sinT, b3 = b2 * sn;
        const double c1 = ux * omc;
        const double ab = a3 - b3;
        du[0] = ab - c1;
        const double d1 = ey * uz, d2_ = d1 * sinT, d3 = d2_ * cs;
        const double e1 = ex * g, e2 = e1 * sinT, e3 = e2 * sn;
        const double f1 = uy * omc;
        const double de = d3 + e3;
        du[1] = de - f1;
        const double h1 = up * sinT, h2 = h1 * cs;
        const double i1 = uz * omc;
        du[2] = (-h2) - i1;
    } else {
        const double gs = g * sinT;
        du[0] = gs * cs;
        du[1] = gs * sn;
        du[2] = -(g * omc);
    }
    for (int a = 0; a < 3; ++a) {
        const double to = fo * du[a], tp = fp * du[a];
        vo[a] = vo[a] + to;
        vp[a] = vp[a] - tp;
    }
    return kCounted | (var > 1.0 ? kStrong : 0);
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style,
// ".property <- what is wrong").  nspecies: the species the handle has.
inline const char* check(const fpic_pair_spec* p, int nspecies)
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    const fpic_pair_spec& s = *p;
    if (s.species_a < 0 || s.species_a >= nspecies) return ".species_a <- no such species";
    if (s.species_b < 0 || s.species_b >= nspecies) return ".species_b <- no such species";
    for (double z : s.reserved)
        if (!(z == 0)) return ".reserved <- must be zero";
    if (std::isnan(s.log_lambda)) return ".log_lambda <- must not be NaN";
    if (std::isnan(s.tau)) return ".tau <- must not be NaN";
    if (!(s.log_lambda > 0) || std::isinf(s.log_lambda)) return ".log_lambda <- must be positive and finite";
    if (!(s.tau > 0) || std::isinf(s.tau)) return ".tau <- must be positive and finite";
    return nullptr;
}

// the kernels' form of a checked request, at `epoch`: the masses (kg) and charges (C) of the two species, the macro weight,
// the cell volume (m^3)
inline Rule rule_of(const fpic_pair_spec& s, uint32_t epoch, double ma, double qa, double mb, double qb, double W, double dV)
{
    Rule r{};
    r.seed_lo = static_cast<uint32_t>(s.seed);
    r.seed_hi = static_cast<uint32_t>(s.seed >> 32);
    r.stream = s.stream;
    r.epoch = epoch;
    r.like = s.species_a == s.species_b;
    const double mm = ma * mb, ms = ma + mb;
    const double mab = mm / ms;
    const double qq = qa * qb;
    const double n1 = qq * qq, n2 = n1 * s.log_lambda, n3 = n2 * s.tau, num = n3 * W;
    const double e2 = kEps0 * kEps0, m2 = mab * mab, c2 = kC * kC, c3 = c2 * kC;
    const double d1 = 8.0 * kPi, d2 = d1 * e2, d3 = d2 * m2, d4 = d3 * c3, den = d4 * dV;
    r.kappa = num / den;
    r.fa = mab / ma;
    r.fb = mab / mb;
    return r;
}

} // namespace fespair
#endif
