// fes_mom_core.hpp — the rule of the fluid moment grids (fpic_moments; the kernels are fes_mom_kernels.hpp, the
// orchestration fes_mom.inc.hpp): a particle's value of a moment, the rejection test, the fixed-point conversion, the split
// of one value over the eight nodes of its cell, and the checks of a request.  Plain C++ that compiles for the host and the
// device, shared with a host test (tests/native/mom_core_test.cpp, g++) and mirrored in numpy (tests/moments_reference.py).
// Every floating-point operation is a double operation rounded once: build with -ffp-contract=off, as the library is.
//
// Accumulators are int64 per node and moment.  N adds wx wy wz (14-bit weights: 2^42 per particle), so a node holds 2^21
// unit-weight particles before overflow — the bound rho_fixed has with Z = 1.  Every other moment adds the parts of
// t = floor(m 2^32) with |m| < 2^14 (|v| < 128), |t| < 2^46: 2^17 particles of the largest value per node at the least.
#ifndef FES_MOM_CORE_HPP
#define FES_MOM_CORE_HPP
#include <cmath>
#include <cstdint>

#include "../../include/fusionpic.h"

#if defined(__HIPCC__)
#define FES_MOM_HD __host__ __device__ __forceinline__
#else
#define FES_MOM_HD inline
#endif

namespace fesmom {

constexpr int kMoments = 10;               // N, FX FY FZ, SXX SYY SZZ, SXY SXZ SYZ: bits 0 .. 9 of a mask
constexpr double kVelocityLimit = 128.0;   // a particle with a component that is not finite or |v| >= 128 adds to no moment

// a particle that adds to no moment (and 1 to `rejected`): plain comparisons, so a NaN rejects
FES_MOM_HD bool rejected(double vx, double vy, double vz)
{
    return !(fabs(vx) < kVelocityLimit && fabs(vy) < kVelocityLimit && fabs(vz) < kVelocityLimit);
}

// the particle value of moment `bit` (1 .. 9); one multiplication in double for the second-order ones
FES_MOM_HD double value(int bit, double vx, double vy, double vz)
{
    switch (bit) {
    case 1: return vx;
    case 2: return vy;
    case 3: return vz;
    case 4: return vx * vx;
    case 5: return vy * vy;
    case 6: return vz * vz;
    case 7: return vx * vy;
    case 8: return vx * vz;
    default: return vy * vz;
    }
}

// t = floor(m 2^32): the scaling is exact (|m| < 2^14), one floor — also for a negative m
FES_MOM_HD int64_t fixed(double m) { return static_cast<int64_t>(floor(m * 4294967296.0)); }

// split with remainder by the upper weight w1 (0 .. 16384): upper = (w1 t + 8192) >> 14 (a flooring shift), lower = t - upper
FES_MOM_HD void split(int64_t t, int w1, int64_t& lower, int64_t& upper)
{
    upper = (static_cast<int64_t>(w1) * t + 8192) >> 14;
    lower = t - upper;
}

// The eight node terms of one particle for one moment other than N: t split along z, then y, then x.  out[a + 2 b + 4 c] goes
// to node (i + a, j + b, k + c); index 1 is the upper part.  The eight terms add up to t exactly.
FES_MOM_HD void mom_terms(int64_t t, int wx1, int wy1, int wz1, int64_t (&out)[8])
{
    int64_t tz[2];
    split(t, wz1, tz[0], tz[1]);
    for (int c = 0; c < 2; ++c) {
        int64_t ty[2];
        split(tz[c], wy1, ty[0], ty[1]);
        for (int b = 0; b < 2; ++b) split(ty[b], wx1, out[2 * b + 4 * c], out[1 + 2 * b + 4 * c]);
    }
}

// N: the charge deposit's integer with Z = 1, wx[a] wy[b] wz[c] with w[0] = 16384 - w[1]
FES_MOM_HD void n_terms(int wx1, int wy1, int wz1, int64_t (&out)[8])
{
    const int64_t wx[2] = { 16384 - wx1, wx1 }, wy[2] = { 16384 - wy1, wy1 }, wz[2] = { 16384 - wz1, wz1 };
    for (int c = 0; c < 2; ++c)
        for (int b = 0; b < 2; ++b)
            for (int a = 0; a < 2; ++a) out[a + 2 * b + 4 * c] = wx[a] * wy[b] * wz[c];
}

FES_MOM_HD int popcount(uint32_t mask)
{
    int n = 0;
    for (; mask; mask &= mask - 1) ++n;
    return n;
}

// A request's checks: nullptr if it is good, else the message (house style, ".property <- what is wrong").
// nspecies: the species the handle has.
inline const char* check(const fpic_moments_spec& s, int nspecies)
{
    if (s.species < 0 || s.species >= nspecies) return ".species <- no such species";
    if (s.mask == 0) return ".mask <- no moment asked for";
    if (s.mask & ~static_cast<uint32_t>(FPIC_MOM_ORDER2)) return ".mask <- bits above 9 (FPIC_MOM_N .. FPIC_MOM_SYZ are bits 0 .. 9)";
    for (double r : s.reserved)
        if (r != 0) return ".reserved <- must be zero";
    return nullptr;
}

} // namespace fesmom
#endif
