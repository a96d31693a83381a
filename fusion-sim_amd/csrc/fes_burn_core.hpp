// fes_burn_core.hpp — the rule of the fusion burn of a CART3D handle (fpic_burn; the passes are fes_burn_kernels.hpp, the
// orchestration fes_burn.inc.hpp): the host-side numbers of a request, the sort key, the probability and the acceptance of one
// pair, who wins a chain, the outcome of an event, whether the events fit their targets, the checks of a request and the
// totals' conversion to the result.  Plain C++ that compiles for the host and the device, shared with a host test
// (tests/native/burn_core_test.cpp, g++); restated independently in numpy float64 and Python integers by
// tests/burn_reference.py.  It joins pieces that exist: the cells, the order, the pair sets, N_L and the table lookup are
// fpic_fusion's (fes_fusion_core.hpp: like_pair, many_is_a, sigma_at, the checks of the shared fields and of the bound), the
// host numbers and the exact isotropic try fpic_fusion_spectrum's (fesfspec::rule_of, try_direction), the fit of a target
// fes_inject_core.hpp's (fesinj::fits), the tally term of a particle fes_ionize_core.hpp's (fesion::gain).
//
// What an application does depends on the request, the epoch, the ids, the cells and the stored state alone.  All arithmetic
// is double, every operation one of + - x / sqrt and rounded once (build with -ffp-contract=off, as the library is);
// include/fusionpic.h states the rule in full.  In short, with B(t) = Philox4x32-10((id, epoch, stream, t), (seed_lo, seed_hi)):
//   key        B(0xB0510)[0] of every particle; the order in a cell ascending by (key, id).
//   one pair   g, below / above and sigma as fesfusion::tally; y = ((((W W) N_L) tau) / dV) (sigma (g c)); P = y / W.
//   accepted   iff (u + 0.5) 2^-32 < P with u = B(0xB0511 + side)[0] of the OWNER, side = 1 iff the owner is of species_b of
//              an unlike request.  P >= 1: always, `saturated`.
//   chains     unlike: the `many` places p with the same p mod Nf share few[p mod Nf]; like: the three pairs of an odd cell's
//              triple share one chain.  The accepted pair of a chain with the lowest place (pair number) REACTS; the others are
//              `blocked`.  The kernel takes that minimum with an integer atomicMin in LDS; wins() is the comparison.
//   outcome    with a, b the reactants of species_a, species_b (like: owner, partner): K = hk (g g); Et = q_value + K held to 0
//              from below; u3 = sqrt(Et kf); u4 = r34 u3; V = f_a v_a + f_b v_b; n from the blocks B(0xB0520 + k) of a's id;
//              w3 = V + u3 n; w4 = V - u4 n.
#ifndef FES_BURN_CORE_HPP
#define FES_BURN_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_fusion_spectrum_core.hpp"
#include "fes_ionize_core.hpp"

namespace fesburn {

constexpr uint32_t kTag = 0xB0510u;       // the fourth counter word of the key's block
constexpr uint32_t kAcceptTag = 0xB0511u; // ... of the acceptance block; + 1: the owner is of species_b of an unlike request
constexpr uint32_t kDirTag = 0xB0520u;    // ... of the first direction block of the species_a reactant
constexpr uint32_t kNoPlace = 0xFFFFFFFFu;   // a chain's word before any accepted pair has written it
enum { kInside = fesfusion::kInside, kBelow = fesfusion::kBelow, kAbove = fesfusion::kAbove };

// The device words of a request, four tallies one behind the other (Tally<NC, NS> of fes_pass.hpp: counts | sums (lo, hi) |
// the out-of-range bits):
//   [0, 9)     the deciding pass: pairs, below, above, cells, overfull_cells, overfull_particles, accepted, blocked, saturated
//   [9, 27)    the generation pass: burnt | product_a, product_b: energy, momentum x, y, z | bits (4 group + quantity)
//   [27, 37)   species_a's compaction: left | energy, momentum x, y, z | bits
//   [37, 47)   species_b's compaction likewise (like species: zeros)
constexpr int kDecideCounts = 9;
constexpr int kGenAt = kDecideCounts, kGenSums = 8, kGenWords = 1 + 2 * kGenSums + 1;
constexpr int kLostSums = 4, kLostWords = 1 + 2 * kLostSums + 1;
constexpr int kLostAt = kGenAt + kGenWords;                 // + kLostWords: species_b's
constexpr int kWords = kLostAt + 2 * kLostWords;
// what a word is to the add of an application's row to the totals: a count, the low word of a 128-bit sum (its high word
// follows), or bits that are ORed
enum { kCount = 0, kSumLo = 1, kSumHi = 2, kBits = 3 };
FES_HIST_HD int word_kind(int k)
{
    if (k < kGenAt) return kCount;
    int at = k - kGenAt, sums = kGenSums;
    if (k >= kLostAt) {
        at = (k - kLostAt) % kLostWords;
        sums = kLostSums;
    }
    if (at == 0) return kCount;
    if (at == 1 + 2 * sums) return kBits;
    return (at - 1) & 1 ? kSumHi : kSumLo;
}

// a request as the kernels read it (the table itself is passed beside it): fpic_fusion's form of the shared fields — its
// exponent and unit are not read — and the outcome's host numbers
struct Rule {
    fesfusion::Rule f;
    double w;                          // the macro weight W
    double hk, kf, f_a, f_b, r34, q_value;
    int tracked_b;                     // product_b is a species of the handle
};

FES_HIST_HD uint32_t key_of(const Rule& r, uint32_t id)
{
    uint32_t w[4];
    fesload::philox(id, r.f.epoch, r.f.stream, kTag, r.f.seed_lo, r.f.seed_hi, w);
    return w[0];
}

// the acceptance word of the pair whose owner has the id `id`
FES_HIST_HD uint32_t accept_word(const Rule& r, uint32_t id, bool side_b)
{
    uint32_t w[4];
    fesload::philox(id, r.f.epoch, r.f.stream, kAcceptTag + (side_b ? 1u : 0u), r.f.seed_lo, r.f.seed_hi, w);
    return w[0];
}

// One pair: N_L and the two stored velocities.  kInside: *p is the pair's probability; kBelow, kAbove: nothing happens.
// fesfusion::tally operation for operation up to its y, and one division
FES_HIST_HD int probability(const Rule& r, const double* S, double n_l, const double (&vo)[3], const double (&vp)[3], double* p)
{
    *p = 0;
    const double g = fesfspec::speed_of(vo, vp);
    if (g < r.f.g_lo) return kBelow;
    if (!(g < r.f.g_hi)) return kAbove;  // (a NaN velocity: above)
    const double sigma = fesfusion::sigma_at(r.f, S, g);
    const double w1 = r.f.ww * n_l, w2 = w1 * r.f.tau, w3 = w2 / r.f.dv;
    const double gc = g * fesfusion::kC, sv = sigma * gc;
    const double y = w3 * sv;
    *p = y / r.w;
    return kInside;
}

FES_HIST_HD bool accepts(uint32_t u, double p)
{
    const double x = (static_cast<double>(u) + 0.5) * fesload::kTwoM32;
    return x < p;
}

using fesfusion::few_of;   // the chain a `many` place belongs to
// whether the accepted pair of place (pair number) p reacts, given the least accepted place of its chain
FES_HIST_HD bool wins(uint32_t least, uint32_t p) { return least == p; }

// the isotropic direction of the event whose species_a reactant has the id `id`: fesfspec::direction_of on this family's blocks
FES_HIST_HD int direction_of(const Rule& r, uint32_t id, double (&n)[3])
{
    for (int a = 0; a < fesfspec::kBlocks; ++a) {
        uint32_t w[4];
        fesload::philox(id, r.f.epoch, r.f.stream, kDirTag + static_cast<uint32_t>(a), r.f.seed_lo, r.f.seed_hi, w);
        if (fesfspec::try_direction(w[0], w[1], n)) return 2 * a;
        if (fesfspec::try_direction(w[2], w[3], n)) return 2 * a + 1;
    }
    n[0] = 0.0;
    n[1] = 0.0;
    n[2] = 1.0;
    return fesfspec::kTries;
}

// the outcome of an event: va, vb the stored velocities of the species_a and the species_b reactant, n the direction
FES_HIST_HD void outcome(const Rule& r, const double (&va)[3], const double (&vb)[3], const double (&n)[3], double (&w3)[3], double (&w4)[3])
{
    const double g = fesfspec::speed_of(va, vb);
    const double gg = g * g;
    const double K = r.hk * gg;
    double et = r.q_value + K;
    if (!(et > 0)) et = 0;
    const double u3 = sqrt(et * r.kf);
    const double u4 = r.r34 * u3;
    for (int i = 0; i < 3; ++i) {
        const double a = r.f_a * va[i], b = r.f_b * vb[i];
        const double v = a + b;
        const double n3 = u3 * n[i], n4 = u4 * n[i];
        w3[i] = v + n3;
        w4[i] = v - n4;
    }
}

using fesion::Fix;
using fesion::gain;       // the tally term of one particle of stored velocity w

// whether M events fit their targets: product_a's (n, capacity, id span) and, if it is tracked, product_b's; kFits, or which does not
enum Fit { kFits = 0, kNoRoomA = 1, kNoRoomB = 2 };
inline Fit fit(uint64_t m, uint64_t n_3, uint64_t cap_3, uint64_t span_3, bool tracked_b, uint64_t n_4, uint64_t cap_4, uint64_t span_4)
{
    if (!fesinj::fits(n_3, cap_3, span_3, m)) return kNoRoomA;
    if (tracked_b && !fesinj::fits(n_4, cap_4, span_4, m)) return kNoRoomB;
    return kFits;
}
// the request's field a refusal names
inline const char* fit_field(Fit f) { return f == kNoRoomA ? "product_a" : "product_b"; }

// the shared fields as fpic_fusion's request
inline fpic_fusion_spec fusion_of(const fpic_burn_spec& s)
{
    fpic_fusion_spec q{};
    q.species_a = s.species_a;
    q.species_b = s.species_b;
    q.seed = s.seed;
    q.stream = s.stream;
    q.epoch = s.epoch;
    q.tau = s.tau;
    q.g_lo = s.g_lo;
    q.g_hi = s.g_hi;
    q.n = s.n;
    q.sigma = s.sigma;
    return q;
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style).  The
// shared fields are held by fesfusion::check itself; fusion_of leaves that request's reserved words zero, so this one's are
// held here
inline const char* check(const fpic_burn_spec* p, int nspecies)
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    const fpic_burn_spec& s = *p;
    if (s.reserved_i != 0) return ".reserved <- must be zero";
    for (double z : s.reserved)
        if (!(z == 0)) return ".reserved <- must be zero";
    const fpic_fusion_spec q = fusion_of(s);
    if (const char* why = fesfusion::check(&q, nspecies)) return why;
    if (s.product_a < 0 || s.product_a >= nspecies) return ".product_a <- no such species";
    if (s.product_b < -1 || s.product_b >= nspecies) return ".product_b <- must be -1 (not tracked) or a species of the handle";
    if (s.product_a == s.species_a || s.product_a == s.species_b) return ".product_a <- must differ from the reactants";
    if (s.product_b == s.species_a || s.product_b == s.species_b) return ".product_b <- must differ from the reactants";
    if (s.product_b == s.product_a) return ".product_b <- must differ from product_a";
    if (s.product_b == -1) {
        if (!(s.other_mass > 0) || std::isinf(s.other_mass)) return ".other_mass <- must be positive and finite when product_b is -1";
    } else if (!(s.other_mass == 0)) {
        return ".other_mass <- must be zero when product_b is a species: its mass is the species'";
    }
    if (std::isnan(s.q_value) || std::isinf(s.q_value)) return ".q_value <- must be finite";
    return nullptr;
}
inline const char* check_bound(const fpic_burn_spec& s, double W, double dV) { return fesfusion::check_bound(fusion_of(s), W, dV); }

// the kernels' form of a checked request at `epoch`: the macro weight, the cell volume (m^3), the masses of species_a,
// species_b, product_a and of product_b (or other_mass)
inline Rule rule_of(const fpic_burn_spec& s, uint32_t epoch, double W, double dV, double m_a, double m_b, double m3, double m4)
{
    Rule r{};
    r.f = fesfusion::rule_of(fusion_of(s), epoch, W, dV);
    r.w = W;
    fpic_fusion_spectrum_spec q{};
    q.axis = FPIC_FSPEC_PRODUCT;
    q.bins = 1;
    q.lo = 0;
    q.hi = 1;
    q.q_value = s.q_value;
    q.product_mass = m3;
    q.other_mass = m4;
    const fesfspec::Rule k = fesfspec::rule_of(q, m_a, m_b);
    r.hk = k.hk;
    r.kf = k.kf;
    r.f_a = k.f_a;
    r.f_b = k.f_b;
    r.r34 = m3 / m4;
    r.q_value = s.q_value;
    r.tracked_b = s.product_b >= 0;
    return r;
}

// one tally's sums -> a gain: s the first sum's low word, bits its four out-of-range bits, count the particles
inline void gain_of(const uint64_t* s, uint64_t bits, uint64_t count, double mass, double charge, double W, fpic_ionize_gain* g)
{
    const double ke = 0.5 * mass * W * fesforce::kC * fesforce::kC, pm = mass * W * fesforce::kC;   // the scales of the energy diagnostics
    g->energy_fixed[0] = s[0];
    g->energy_fixed[1] = s[1];
    g->energy = (bits & 1u) ? std::nan("") : ke * fesforce::fixed_to_double(s[0], s[1]);
    for (int a = 0; a < 3; ++a) {
        g->momentum_fixed[a][0] = s[2 + 2 * a];
        g->momentum_fixed[a][1] = s[3 + 2 * a];
        g->momentum[a] = (bits >> (1 + a) & 1u) ? std::nan("") : pm * fesforce::fixed_to_double(s[2 + 2 * a], s[3 + 2 * a]);
    }
    const double q = static_cast<double>(count) * charge;
    g->charge = q * W;
}

// the device words of a request -> the result but `applications`; mass, charge: of species_a, species_b, product_a and
// product_b (not tracked: other_mass, 0); W: the box's
inline void result_of(const uint64_t* w, const double (&mass)[4], const double (&charge)[4], double W, fpic_burn_result* out)
{
    out->pairs = w[0];
    out->below = w[1];
    out->above = w[2];
    out->cells = w[3];
    out->overfull_cells = w[4];
    out->overfull_particles = w[5];
    out->accepted = w[6];
    out->blocked = w[7];
    out->saturated = w[8];
    out->burnt = w[kGenAt];
    const uint64_t gen_bits = w[kGenAt + kGenWords - 1];
    gain_of(w + kLostAt + 1, w[kLostAt + kLostWords - 1], w[kLostAt], mass[0], charge[0], W, &out->reactant_a);
    gain_of(w + kLostAt + kLostWords + 1, w[kLostAt + 2 * kLostWords - 1], w[kLostAt + kLostWords], mass[1], charge[1], W, &out->reactant_b);
    gain_of(w + kGenAt + 1, gen_bits, w[kGenAt], mass[2], charge[2], W, &out->product_a);
    gain_of(w + kGenAt + 1 + 2 * kLostSums, gen_bits >> 4, w[kGenAt], mass[3], charge[3], W, &out->product_b);
}

} // namespace fesburn
#endif
