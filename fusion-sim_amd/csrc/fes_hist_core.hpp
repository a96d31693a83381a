// fes_hist_core.hpp — the bin rule of the phase-space histograms (fpic_histogram; the kernels are fes_hist_kernels.hpp, the
// orchestration fes_hist.inc.hpp): the value of an axis, the inside test, the index, and the checks of a request.  Plain
// C++ that compiles for the host and the device, shared with a host test (tests/native/hist_core_test.cpp, g++).  Every
// operation is a double operation rounded once: build with -ffp-contract=off, as the library is.
#ifndef FES_HIST_CORE_HPP
#define FES_HIST_CORE_HPP
#include <cmath>
#include <cstdint>

#include "../../include/fusionpic.h"

#if defined(__HIPCC__)
#define FES_HIST_HD __host__ __device__ __forceinline__
#else
#define FES_HIST_HD inline
#endif

namespace feshist {

// one axis of a request: q is inside iff lo <= q < hi; scale = bins / (hi - lo), computed once on the host
struct Axis {
    double lo, hi, scale;
    int64_t bins;
};

FES_HIST_HD double scale_of(int64_t bins, double lo, double hi) { return static_cast<double>(bins) / (hi - lo); }

// |v|^2 as diag_add (fes_diag_kernels.hpp) forms it: added left to right
FES_HIST_HD double v2_of(double x, double y, double z) { return x * x + y * y + z * z; }

// plain comparisons: a NaN is not inside
FES_HIST_HD bool inside(double q, const Axis& a) { return q >= a.lo && q < a.hi; }

// the bin of a q that is inside: floor((q - lo) scale), the subtraction and the product each rounded once; the product of
// the largest q below hi may round up to `bins`, which the min catches
FES_HIST_HD int64_t index_of(double q, const Axis& a)
{
    const double d = q - a.lo;
    const double t = d * a.scale;
    const int64_t k = static_cast<int64_t>(floor(t));
    return k < a.bins - 1 ? k : a.bins - 1;
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style,
// ".property <- what is wrong").  nspecies: the species the handle has.
inline const char* check(const fpic_hist_spec& s, int nspecies)
{
    if (s.naxes != 1 && s.naxes != 2) return ".naxes <- must be 1 or 2";
    if (s.species < 0 || s.species >= nspecies) return ".species <- no such species";
    uint64_t total = 1;
    for (int a = 0; a < s.naxes; ++a) {
        if (s.axis[a] < FPIC_AXIS_X || s.axis[a] > FPIC_AXIS_V2) return ".axis <- must be 0 .. 6 (x, y, z, vx, vy, vz, v2)";
        if (s.bins[a] < 1) return ".bins <- must be at least 1";
        if (!std::isfinite(s.lo[a]) || !std::isfinite(s.hi[a])) return ".range <- lo and hi must be finite";
        if (!(s.lo[a] < s.hi[a])) return ".range <- lo must be below hi";
        // (a width that overflows, or so narrow that bins / width does: the index could not be formed)
        if (!std::isfinite(s.hi[a] - s.lo[a]) || !std::isfinite(scale_of(s.bins[a], s.lo[a], s.hi[a]))) return ".range <- bins / (hi - lo) must be finite";
        total *= static_cast<uint64_t>(s.bins[a]);     // (each below 2^31: no overflow)
    }
    if (s.naxes == 2 && s.axis[0] == s.axis[1]) return ".axis <- the same axis twice";
    if (total > FPIC_HIST_MAX_BINS) return ".bins <- more than FPIC_HIST_MAX_BINS (2^22) bins in all";
    for (double r : s.reserved)
        if (r != 0) return ".reserved <- must be zero";
    return nullptr;
}

inline Axis axis_of(const fpic_hist_spec& s, int a) { return Axis{ s.lo[a], s.hi[a], scale_of(s.bins[a], s.lo[a], s.hi[a]), s.bins[a] }; }

} // namespace feshist
#endif
