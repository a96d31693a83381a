// fes_load_core.hpp — the rule of the particle loader of a CART3D handle (fpic_load; the kernels are fes_load_kernels.hpp, the
// orchestration fes_load.inc.hpp): the random words, the unit fractions, the position and the velocity of particle i, and
// the checks of a request.  Plain C++ that compiles for the host and the device, shared with a host test
// (tests/native/load_core_test.cpp, g++).
//
// The state of particle i (the caller's index = the id the box carries) depends on the request and on i alone: not on the
// slot, the rank, the precision of the handle or the time of the call.  All arithmetic is double, every operation rounded
// once (build with -ffp-contract=off, as the library is: p = lo + f w is one rounded multiply and one rounded add, never
// a fused one); an fp32 handle stores the float rounding of the same double result.
//
//   words      W(b) = Philox4x32-10(counter (i, stream, b, 0x10AD), key (seed_lo, seed_hi)) — the round function and the
//              constants of counter_rand (fpic_push.hpp).  b = 0: positions, b = 1: velocities; the lattice shifts of a
//              request are the block with counter (0, stream, 2, 0x10AD).
//   fractions  RANDOM   f_a = W(0)[a] 2^-32
//              LATTICE  f_a = ((i mult_a + shift_a) mod 2^32) 2^-32, mult = the three R3 multipliers of bench.py's lattice
//              — exact integers scaled by a power of two.
//   position   (box fractions) p_a = lo_f[a] + f_a w_f[a]; the phase in turns theta = (m_x p_x + m_y p_y) + m_z p_z;
//              p_a += xamp_f[a] sinpi(2 (theta + xphase)); stored: wrap01(T(p_a)), as the upload does.
//   velocity   (units of c) Box-Muller on W(1): u1 = (w0 + 0.5) 2^-32, u2 = w1 2^-32, n0 = sqrt(-2 ln u1) cospi(2 u2),
//              n1 = sqrt(-2 ln u1) sinpi(2 u2), n2 = sqrt(-2 ln((w2 + 0.5) 2^-32)) cospi(2 w3 2^-32);
//              v_a = (drift[a] + vth[a] n_a) + vamp[a] sinpi(2 (theta + vphase)), theta from the UNDISPLACED p.
//              The largest normal this can draw is sqrt(-2 ln 2^-33) = 6.76.
//   PAIRED     the velocity block is taken at i & ~1 and the thermal term of odd i is negated: with zero drift and zero vamp
//              the two velocities of a pair are exact negatives.
#ifndef FES_LOAD_CORE_HPP
#define FES_LOAD_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_hist_core.hpp"

namespace fesload {

constexpr uint32_t kTag = 0x10ADu;                       // the fourth counter word of every block of the loader
constexpr uint32_t kMult0 = 3518319155u, kMult1 = 2882110345u, kMult2 = 2360945575u;   // round(2^32 / phi3^k), phi3 = 1.2207440846
constexpr uint32_t kKnownFlags = FPIC_LOAD_POS | FPIC_LOAD_VEL | FPIC_LOAD_LATTICE | FPIC_LOAD_PAIRED | FPIC_LOAD_APPEND;
constexpr double kTwoM32 = 1.0 / 4294967296.0;
constexpr double kPi = 3.14159265358979323846;

FES_HIST_HD void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4])
{
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n1 = static_cast<uint32_t>(p1);
        const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1, n3 = static_cast<uint32_t>(p0);
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// sin(pi x), cos(pi x): the device's own functions in a kernel; on the host an exact reduction to [0, 1/2] and the libm
// function of the nearer axis (the host never generates a population: its tests read the exact parts)
FES_HIST_HD double sinpi_(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ::sinpi(x);
#else
    double s = x < 0 ? -1.0 : 1.0, r = std::fmod(std::fabs(x), 2.0);
    if (r >= 1.0) { r -= 1.0; s = -s; }
    if (r > 0.5) r = 1.0 - r;
    return s * (r <= 0.25 ? std::sin(kPi * r) : std::cos(kPi * (0.5 - r)));
#endif
}
FES_HIST_HD double cospi_(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ::cospi(x);
#else
    double s = 1.0, r = std::fmod(std::fabs(x), 2.0);
    if (r >= 1.0) r = 2.0 - r;
    if (r > 0.5) { r = 1.0 - r; s = -1.0; }
    return s * (r <= 0.25 ? std::cos(kPi * r) : std::sin(kPi * (0.5 - r)));
#endif
}

// a request as the kernels read it: the host has resolved the range, divided the lengths by the box and drawn the shifts
struct Rule {
    uint32_t flags, seed_lo, seed_hi, stream;
    uint64_t first, count;             // the indices [first, first + count)
    double lo_f[3], w_f[3];            // lo / L, (hi - lo) / L
    double drift[3], vth[3];
    double m[3];                       // the integer mode vector
    double xamp_f[3], xphase;          // xamp / L
    double vamp[3], vphase;
    uint32_t mult[3], shift[3];        // LATTICE
    int displaced, waved;              // any xamp != 0; any vamp != 0
};

FES_HIST_HD double fraction_of(uint32_t w) { return static_cast<double>(w) * kTwoM32; }
FES_HIST_HD uint32_t lattice_word(uint32_t i, uint32_t mult, uint32_t shift) { return i * mult + shift; }   // mod 2^32

// the undisplaced position of particle i and its phase in turns
FES_HIST_HD void base_of(const Rule& r, uint32_t i, double (&p)[3], double& theta)
{
    uint32_t w[4];
    if (r.flags & FPIC_LOAD_LATTICE) {
        for (int a = 0; a < 3; ++a) w[a] = lattice_word(i, r.mult[a], r.shift[a]);
    } else {
        philox(i, r.stream, 0u, kTag, r.seed_lo, r.seed_hi, w);
    }
    for (int a = 0; a < 3; ++a) {
        const double t = fraction_of(w[a]) * r.w_f[a];
        p[a] = r.lo_f[a] + t;
    }
    const double tx = r.m[0] * p[0], ty = r.m[1] * p[1], tz = r.m[2] * p[2];
    const double txy = tx + ty;
    theta = txy + tz;
}

// the position as it is stored (before the cast to T and wrap01)
FES_HIST_HD void displace(const Rule& r, double theta, double (&p)[3])
{
    if (!r.displaced) return;
    const double s = sinpi_(2.0 * (theta + r.xphase));
    for (int a = 0; a < 3; ++a) {
        const double d = r.xamp_f[a] * s;
        p[a] = p[a] + d;
    }
}

// three normals from four words: the Box-Muller step (shared with the collision operator, fes_collide_core.hpp)
FES_HIST_HD void normals_from(const uint32_t (&w)[4], double (&n)[3])
{
    const double u1 = (static_cast<double>(w[0]) + 0.5) * kTwoM32, u3 = (static_cast<double>(w[2]) + 0.5) * kTwoM32;
    const double r1 = sqrt(-2.0 * log(u1)), r3 = sqrt(-2.0 * log(u3));
    n[0] = r1 * cospi_(2.0 * fraction_of(w[1]));
    n[1] = r1 * sinpi_(2.0 * fraction_of(w[1]));
    n[2] = r3 * cospi_(2.0 * fraction_of(w[3]));
}

FES_HIST_HD void normals_of(const Rule& r, uint32_t i, double (&n)[3])
{
    uint32_t w[4];
    philox(r.flags & FPIC_LOAD_PAIRED ? i & ~1u : i, r.stream, 1u, kTag, r.seed_lo, r.seed_hi, w);
    normals_from(w, n);
}

FES_HIST_HD void velocity_of(const Rule& r, uint32_t i, double theta, double (&v)[3])
{
    double n[3];
    normals_of(r, i, n);
    const bool flip = (r.flags & FPIC_LOAD_PAIRED) && (i & 1u);
    const double s = r.waved ? sinpi_(2.0 * (theta + r.vphase)) : 0.0;
    for (int a = 0; a < 3; ++a) {
        const double th = r.vth[a] * n[a];
        const double dt = r.drift[a] + (flip ? -th : th);
        const double wv = r.vamp[a] * s;
        v[a] = dt + wv;
    }
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style,
// ".property <- what is wrong").  nspecies: the species the handle has; have: the particles of the species (an undecomposed
// handle), or ~0 on a rank of a decomposition (the indices are global ids: count must be given); L: the box in metres.
inline const char* check(const fpic_load_spec& s, int nspecies, uint64_t have, const double (&L)[3], bool decomposed)
{
    if (s.species < 0 || s.species >= nspecies) return ".species <- no such species";
    if (s.flags & ~kKnownFlags) return ".flags <- unknown bits";
    if (!(s.flags & (FPIC_LOAD_POS | FPIC_LOAD_VEL))) return ".flags <- at least one of FPIC_LOAD_POS and FPIC_LOAD_VEL";
    if (s.reserved != 0 || s.reserved2 != 0) return ".reserved <- must be zero";
    if (decomposed) {
        if ((s.flags & (FPIC_LOAD_POS | FPIC_LOAD_VEL)) != (FPIC_LOAD_POS | FPIC_LOAD_VEL))
            return ".flags <- a rank of a decomposition needs FPIC_LOAD_POS and FPIC_LOAD_VEL both";
        if (s.count == ~0ull) return ".count <- a rank of a decomposition does not know the whole population: give the count";
        if (s.first > 0xFFFFFFFFull || s.count > 0xFFFFFFFFull - s.first) return ".first <- the indices are 32-bit ids";
    } else {
        if (s.flags & FPIC_LOAD_APPEND) return ".flags <- FPIC_LOAD_APPEND is for a rank of a decomposition";
        if (s.first > have) return ".first <- beyond the species' particles";
        if (s.count != ~0ull && s.count > have - s.first) return ".count <- the range does not lie within the species' particles";
    }
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(s.lo[a]) || !std::isfinite(s.hi[a])) return ".lo <- lo and hi must be finite";
        if (!(s.lo[a] >= 0) || !(s.lo[a] < s.hi[a]) || !(s.hi[a] <= L[a])) return ".lo <- must be 0 <= lo < hi <= the box length";
        if (!std::isfinite(s.drift[a])) return ".drift <- must be finite";
        if (!std::isfinite(s.vth[a]) || s.vth[a] < 0) return ".vth <- must be finite and not negative";
        if (s.mode[a] > 32768 || s.mode[a] < -32768) return ".mode <- components must lie within +-2^15";
        if (!std::isfinite(s.xamp[a])) return ".xamp <- must be finite";
        if (!std::isfinite(s.vamp[a])) return ".vamp <- must be finite";
    }
    if (!std::isfinite(s.xphase)) return ".xphase <- must be finite";
    if (!std::isfinite(s.vphase)) return ".vphase <- must be finite";
    return nullptr;
}

// the kernels' form of a checked request
inline Rule rule_of(const fpic_load_spec& s, uint64_t have, const double (&L)[3])
{
    Rule r{};
    r.flags = s.flags;
    r.seed_lo = static_cast<uint32_t>(s.seed);
    r.seed_hi = static_cast<uint32_t>(s.seed >> 32);
    r.stream = s.stream;
    r.first = s.first;
    r.count = s.count == ~0ull ? have - s.first : s.count;
    for (int a = 0; a < 3; ++a) {
        r.lo_f[a] = s.lo[a] / L[a];
        r.w_f[a] = (s.hi[a] - s.lo[a]) / L[a];
        r.drift[a] = s.drift[a] + 0.0;   // (a drift of -0 is +0: the sum below then never sees a negative zero)
        r.vth[a] = s.vth[a];
        r.m[a] = static_cast<double>(s.mode[a]);
        r.xamp_f[a] = s.xamp[a] / L[a];
        r.vamp[a] = s.vamp[a];
        r.displaced |= s.xamp[a] != 0;
        r.waved |= s.vamp[a] != 0;
    }
    r.xphase = s.xphase;
    r.vphase = s.vphase;
    uint32_t w[4];
    philox(0u, s.stream, 2u, kTag, r.seed_lo, r.seed_hi, w);
    r.mult[0] = kMult0; r.mult[1] = kMult1; r.mult[2] = kMult2;
    for (int a = 0; a < 3; ++a) r.shift[a] = w[a];
    return r;
}

} // namespace fesload
#endif
