// fes_fusion_spectrum_core.hpp — the rule of the fusion product spectrum of a CART3D handle (fpic_fusion_spectrum; the kernel
// is fes_fusion_spectrum_kernels.hpp, the orchestration fes_fusion_spectrum.inc.hpp): the host-side numbers of a request, the
// kinematics of one pair, the emission direction, the bin of a value and the checks of a request.  It builds on
// fes_fusion_core.hpp: the cells, the key (tag 0xF0510), the order, the pair sets, the table and the integer q of a pair are
// exactly fpic_fusion's, so the words of a spectrum add to the yield fpic_fusion reports for the embedded request and epoch.
// Plain C++ that compiles for the host and the device, shared with a host test (tests/native/fusion_spectrum_core_test.cpp,
// g++); restated independently in numpy float64 and Python integers by tests/fusion_spectrum_reference.py.
//
// It is a tally: it reads the stored velocities and writes nothing to any particle.  All arithmetic is double, every operation
// is one of + - x / sqrt and rounded once (build with -ffp-contract=off, as the library is); velocities are in units of c.
//
//   host numbers (rule_of), m_a, m_b the species' masses, m3 = product_mass, m4 = other_mass:
//              M = m_a + m_b; f_a = m_a / M, f_b = m_b / M; m_ab = (m_a m_b) / M; cc = c c with c = fesfusion::kC;
//              hk = (0.5 m_ab) cc; kf = ((2 m4) / (m3 (m3 + m4))) / cc; h3 = (0.5 m3) cc; inv_w = bins / (hi - lo);
//              with a line of sight n = los / sqrt((lx lx + ly ly) + lz lz), component by component.
//   one pair   inside the table, with q from fesfusion::tally, owner o, partner p and g as there:
//              K = hk (g g).
//              axis CM:       x = K.
//              axis PRODUCT:  Et = q_value + K; if !(Et > 0) then Et = 0.  u3 = sqrt(Et kf).
//                             V_i = (f_o v_o,i) + (f_p v_p,i), f_o the mass fraction of the owner's species (like species:
//                             both fractions are equal).  w_i = V_i + (u3 n_i).  x = h3 ((w_x w_x + w_y w_y) + w_z w_z).
//   isotropic  n is exact, with no trigonometry (Marsaglia): blocks D(a) = Philox4x32-10(counter (id_o, epoch, stream,
//              0xF0520 + 16 [the owner is of species_b and a != b] + a), key seed), a = 0 .. 7; each block gives two tries,
//              (w0, w1) then (w2, w3): x1 = ((w + 0.5) 2^-31) - 1 and x2 likewise, s = x1 x1 + x2 x2; the first try with
//              s < 1 is taken: r = sqrt(1 - s), n = ((2 x1) r, (2 x2) r, 1 - (2 s)).  Sixteen rejections have the
//              probability 2e-11; the result is then n = (0, 0, 1).  try_direction() is one try.
//   binning    x < lo adds q to `under`; !(x < hi) adds q to `over` (a NaN included); otherwise t = (x - lo) inv_w,
//              k = min((int) t, bins - 1) and bin k gets q.
//   the words  a bin can receive every pair of the box, so one word per bin is not enough: q < 2^40 times 2^31 pairs
//              overflows it.  Every bin, `under` and `over` are two uint64 words, q >> 32 and q & 0xFFFFFFFF; a workgroup
//              carries its low word into its high word before it adds to global memory, and the host joins them as
//              fesfusion::join does: each entry is reported as (hi, lo) with lo < 2^32, in units of 2^e reactions.
//   the bound  a workgroup's low word is below 2^32 when it is added, and at most 512 workgroups add per application: the low
//              word of an entry grows by less than 2^41 per application.  The high word receives the pairs' q >> 32 < 2^8
//              (fewer than 2^31 pairs: below 2^39 in all) and the workgroups' carries (below 2^31 each): less than 2^41 per
//              application as well.  A registered operator is therefore exact for at least 2^23 = 8388608 applications between
//              two drains (fpic_fusion_spectrum_read with reset).  NOTHING DETECTS AN OVERFLOW BEYOND THAT: the words wrap
//              silently.
#ifndef FES_FUSION_SPECTRUM_CORE_HPP
#define FES_FUSION_SPECTRUM_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_fusion_core.hpp"

namespace fesfspec {

constexpr uint32_t kDirTag = 0xF0520u;    // the fourth counter word of the first direction block
constexpr uint32_t kDirSide = 16u;        // added when the owner is of species_b of an unlike request
constexpr int kBlocks = 8;                // direction blocks, two tries each
constexpr int kTries = 2 * kBlocks;       // the value direction_of returns on the fallback
constexpr double kTwoM31 = 1.0 / 2147483648.0;

// a request as the kernel reads it, beside the fesfusion::Rule of its tally
struct Rule {
    int axis, bins;
    int sight;                         // a line of sight is given (n below), else isotropic emission
    double lo, hi, inv_w;
    double hk;                         // K = hk (g g)
    double q_value, kf, h3;
    double f_a, f_b;                   // the mass fractions of species_a and species_b
    double n[3];
};

FES_HIST_HD double unit_of(uint32_t w) { return ((static_cast<double>(w) + 0.5) * kTwoM31) - 1.0; }

// one try of the isotropic direction: false if the point is outside the unit disc
FES_HIST_HD bool try_direction(uint32_t wa, uint32_t wb, double (&n)[3])
{
    const double x1 = unit_of(wa), x2 = unit_of(wb);
    const double x11 = x1 * x1, x22 = x2 * x2;
    const double s = x11 + x22;
    if (!(s < 1.0)) return false;
    const double r = sqrt(1.0 - s);
    n[0] = (2.0 * x1) * r;
    n[1] = (2.0 * x2) * r;
    n[2] = 1.0 - (2.0 * s);
    return true;
}

// the isotropic direction of the pair whose owner has the id `id`; side_b: the owner is of species_b of an unlike request.
// Returns the try that was taken, 0 .. kTries - 1, or kTries: the fallback (0, 0, 1).
FES_HIST_HD int direction_of(const fesfusion::Rule& r, uint32_t id, bool side_b, double (&n)[3])
{
    const uint32_t tag = kDirTag + (side_b ? kDirSide : 0u);
    for (int a = 0; a < kBlocks; ++a) {
        uint32_t w[4];
        fesload::philox(id, r.epoch, r.stream, tag + static_cast<uint32_t>(a), r.seed_lo, r.seed_hi, w);
        if (try_direction(w[0], w[1], n)) return 2 * a;
        if (try_direction(w[2], w[3], n)) return 2 * a + 1;
    }
    n[0] = 0.0;
    n[1] = 0.0;
    n[2] = 1.0;
    return kTries;
}

// g of a pair, as fesfusion::tally computes it
FES_HIST_HD double speed_of(const double (&vo)[3], const double (&vp)[3])
{
    const double ux = vo[0] - vp[0], uy = vo[1] - vp[1], uz = vo[2] - vp[2];
    const double uxx = ux * ux, uyy = uy * uy, uzz = uz * uz;
    const double up2 = uxx + uyy;
    return sqrt(up2 + uzz);
}

// K, the centre-of-mass kinetic energy of a pair (J)
FES_HIST_HD double cm_energy(const Rule& s, double g)
{
    const double gg = g * g;
    return s.hk * gg;
}

// the product's laboratory energy (J): f_o, f_p the mass fractions of the owner's and the partner's species, n the direction
FES_HIST_HD double product_energy(const Rule& s, double K, double f_o, double f_p, const double (&vo)[3], const double (&vp)[3], const double (&n)[3])
{
    double et = s.q_value + K;
    if (!(et > 0)) et = 0;
    const double u3 = sqrt(et * s.kf);
    double w[3];
    for (int i = 0; i < 3; ++i) {
        const double a = f_o * vo[i], b = f_p * vp[i];
        const double v = a + b;
        const double un = u3 * n[i];
        w[i] = v + un;
    }
    const double wxx = w[0] * w[0], wyy = w[1] * w[1], wzz = w[2] * w[2];
    const double wp2 = wxx + wyy;
    return s.h3 * (wp2 + wzz);
}

// the entry a value adds to: 0 .. bins - 1 the bins, bins: `under`, bins + 1: `over`
FES_HIST_HD int entry_of(const Rule& s, double x)
{
    if (x < s.lo) return s.bins;
    if (!(x < s.hi)) return s.bins + 1;
    const double t = (x - s.lo) * s.inv_w;
    const int k = static_cast<int>(t);
    return k > s.bins - 1 ? s.bins - 1 : k;
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message.
inline const char* check(const fpic_fusion_spectrum_spec* p, int nspecies)
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    const fpic_fusion_spectrum_spec& s = *p;
    if (const char* why = fesfusion::check(&s.tally, nspecies)) return why;
    for (double z : s.reserved)
        if (!(z == 0)) return ".reserved <- must be zero";
    if (s.axis != FPIC_FSPEC_CM && s.axis != FPIC_FSPEC_PRODUCT) return ".axis <- must be FPIC_FSPEC_CM (0) or FPIC_FSPEC_PRODUCT (1)";
    if (s.bins < 1 || s.bins > FPIC_FUSION_SPECTRUM_BINS_MAX) return ".bins <- must be 1 .. FPIC_FUSION_SPECTRUM_BINS_MAX (256)";
    if (std::isnan(s.lo) || std::isinf(s.lo)) return ".lo <- must be finite";
    if (!(s.hi > s.lo) || std::isinf(s.hi)) return ".hi <- must be finite and above lo";
    if (std::isnan(s.q_value) || std::isinf(s.q_value)) return ".q_value <- must be finite";
    if (s.axis == FPIC_FSPEC_PRODUCT) {
        if (!(s.product_mass > 0) || std::isinf(s.product_mass)) return ".product_mass <- must be positive and finite";
        if (!(s.other_mass > 0) || std::isinf(s.other_mass)) return ".other_mass <- must be positive and finite";
    }
    bool any = false;
    for (double z : s.los) {
        if (std::isnan(z) || std::isinf(z)) return ".los <- must be finite";
        any = any || z != 0;
    }
    if (any) {
        const double n2 = (s.los[0] * s.los[0] + s.los[1] * s.los[1]) + s.los[2] * s.los[2];
        if (!(n2 > 0) || std::isinf(n2)) return ".los <- must be all zero (isotropic) or have a non-zero, finite norm";
    }
    return nullptr;
}

// the kernel's form of a checked request: m_a, m_b the masses of species_a and species_b (kg)
inline Rule rule_of(const fpic_fusion_spectrum_spec& s, double m_a, double m_b)
{
    Rule r{};
    r.axis = s.axis;
    r.bins = s.bins;
    r.lo = s.lo;
    r.hi = s.hi;
    r.inv_w = static_cast<double>(s.bins) / (s.hi - s.lo);
    const double M = m_a + m_b;
    r.f_a = m_a / M;
    r.f_b = m_b / M;
    const double m_ab = (m_a * m_b) / M;
    const double cc = fesfusion::kC * fesfusion::kC;
    r.hk = (0.5 * m_ab) * cc;
    r.q_value = s.q_value;
    if (s.axis == FPIC_FSPEC_PRODUCT) {
        const double m3 = s.product_mass, m4 = s.other_mass;
        r.kf = ((2.0 * m4) / (m3 * (m3 + m4))) / cc;
        r.h3 = (0.5 * m3) * cc;
    }
    const double lx = s.los[0], ly = s.los[1], lz = s.los[2];
    r.sight = lx != 0 || ly != 0 || lz != 0;
    if (r.sight) {
        const double norm = std::sqrt((lx * lx + ly * ly) + lz * lz);
        r.n[0] = lx / norm;
        r.n[1] = ly / norm;
        r.n[2] = lz / norm;
    }
    return r;
}

} // namespace fesfspec
#endif
