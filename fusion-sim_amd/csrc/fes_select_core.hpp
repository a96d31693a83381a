// fes_select_core.hpp — the rule of the particle selection (fpic_select; the pass is fes_select_kernels.hpp, the orchestration
// fes_select.inc.hpp): the inside test of a term, the id rule, the arrays a request reads, and the checks of a request.
// Plain C++ that compiles for the host and the device, shared with a host test (tests/native/select_core_test.cpp, g++).
// The value of an axis is the histogram's (feshist::v2_of, fes_hist_core.hpp): build with -ffp-contract=off, as the
// library is.
#ifndef FES_SELECT_CORE_HPP
#define FES_SELECT_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_hist_core.hpp"

namespace fessel {

// plain comparisons in double: a NaN is not inside; lo may be -inf, hi +inf
FES_HIST_HD bool inside(double q, double lo, double hi) { return q >= lo && q < hi; }

// id_mod 0 or 1: every id
FES_HIST_HD bool id_passes(uint32_t id, uint32_t id_mod, uint32_t id_rem) { return id_mod < 2 || id % id_mod == id_rem; }

// the slab's arrays (bit c: x, y, z, vx, vy, vz) a request's terms read: one per position or velocity term, vx vy vz for V2
inline uint32_t arrays_of(const fpic_select_spec& s)
{
    uint32_t m = 0;
    for (int t = 0; t < s.nterms; ++t) m |= s.axis[t] == FPIC_AXIS_V2 ? 0x38u : 1u << s.axis[t];
    return m;
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style,
// ".property <- what is wrong").  nspecies: the species the handle has; outputs: whether any of the three output pointers
// is given.
inline const char* check(const fpic_select_spec& s, int nspecies, uint64_t capacity, bool outputs, int dtype)
{
    if (s.nterms < 0 || s.nterms > FPIC_SELECT_MAX_TERMS) return ".nterms <- must be 0 .. 7";
    if (s.species < 0 || s.species >= nspecies) return ".species <- no such species";
    uint32_t seen = 0;
    for (int t = 0; t < s.nterms; ++t) {
        if (s.axis[t] < FPIC_AXIS_X || s.axis[t] > FPIC_AXIS_V2) return ".axis <- must be 0 .. 6 (x, y, z, vx, vy, vz, v2)";
        if (seen >> s.axis[t] & 1u) return ".axis <- the same axis twice";
        seen |= 1u << s.axis[t];
        if (std::isnan(s.lo[t]) || std::isnan(s.hi[t])) return ".range <- lo and hi must not be NaN";
        if (!(s.lo[t] < s.hi[t])) return ".range <- lo must be below hi";
    }
    for (int t = s.nterms; t < 8; ++t)
        if (s.axis[t] != 0 || s.lo[t] != 0 || s.hi[t] != 0) return ".axis <- entries past nterms must be zero";   // (a NaN is not zero)
    if (s.id_mod > 1 && s.id_rem >= s.id_mod) return ".id_rem <- must be below id_mod";
    for (double r : s.reserved)
        if (r != 0) return ".reserved <- must be zero";
    if (capacity > FPIC_SELECT_MAX_ROWS) return ".capacity <- more than FPIC_SELECT_MAX_ROWS (2^24) rows";
    if (capacity > 0 && !outputs) return ".capacity <- rows asked for, but ids, pos_aos and vel_aos are all undefined";
    if (dtype != FPIC_F32 && dtype != FPIC_F64) return ".dtype <- must be FPIC_F32 or FPIC_F64";
    return nullptr;
}

} // namespace fessel
#endif
