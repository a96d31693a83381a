// fes_series_core.hpp — the host rules of the series diagnostic (fpic_series_*: the field at chosen points and the state of
// chosen particles, as rows; the kernels are fes_series_kernels.hpp, the orchestration fes_series.inc.hpp): the checks of a
// request, the normalised coordinate of a point, the tracers' sorted tables and bitmap filter (and the lookups the kernel
// makes in them), the owner of a point in a z-slab decomposition, and the selection by flag of the ranks' rows.  Plain C++
// that compiles for the host and the device, shared with a host test (tests/native/series_core_test.cpp, g++).  The recording
// ring is fesdiag::Ring (fes_diag_core.hpp).
#ifndef FES_SERIES_CORE_HPP
#define FES_SERIES_CORE_HPP
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/fusionpic.h"
#include "fes_diag_core.hpp"

#if defined(__HIPCC__)
#define FES_SERIES_HD __host__ __device__ __forceinline__
#else
#define FES_SERIES_HD inline
#endif

namespace fesser {

constexpr int kEntry = 8;          // doubles per entry of a row (a point or a tracer)
constexpr int kPointFlag = 7;      // `present`
constexpr int kTracerFlag = 6;     // `found`

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style).
// counts: the species' particle numbers of an undecomposed handle (ids are checked against them), nullptr on a decomposed one.
inline const char* check(const fpic_series_spec& s, int nspecies, const uint64_t* counts)
{
    if (!s.npoints && !s.ntracers) return ".points <- points and tracers are both empty";
    if (s.npoints > FPIC_SERIES_MAX_POINTS) return ".points <- more than FPIC_SERIES_MAX_POINTS (4096) points";
    if (s.ntracers > FPIC_SERIES_MAX_TRACERS) return ".tracers <- more than FPIC_SERIES_MAX_TRACERS (65536) tracers";
    if (s.npoints && !s.points) return ".points <- Non-optional property is undefined!";
    if (s.ntracers && (!s.tracer_species || !s.tracer_id)) return ".tracers <- Non-optional property is undefined!";
    for (uint32_t p = 0; p < 3 * s.npoints; ++p)
        if (!std::isfinite(s.points[p])) return ".points <- must be finite";
    std::vector<uint64_t> keys(s.ntracers);
    for (uint32_t t = 0; t < s.ntracers; ++t) {
        const int32_t sp = s.tracer_species[t];
        if (sp < 0 || sp >= nspecies) return ".tracers <- no such species";
        if (counts && s.tracer_id[t] >= counts[sp]) return ".tracers <- an id is not below the species' particle count";
        keys[t] = static_cast<uint64_t>(sp) << 32 | s.tracer_id[t];
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return ".tracers <- the same (species, id) twice";
    for (double r : s.reserved)
        if (r != 0) return ".reserved <- must be zero";
    return nullptr;
}

// step 1 of the point rule: the fraction of the box, in double, wrapped periodically into [0, 1)
inline double unit_of(double p, double L)
{
    double u = p / L;
    u -= std::floor(u);
    return u < 1 ? u : 0;
}

// ---- the tracers of one species: ids sorted ascending, index[k] = the entry of the request that sorted[k] is, and a bitmap
// filter of 2^log2bits bits.  A multiplicative hash of the id picks one 32-bit word (its top bits) and three bits of that
// word (the three 5-bit fields below them): an id passes iff all three are set — one read per id.  A member's bits are
// always set (no false negative).  A wave looks at 512 or more slots between two branches, so what matters is that a slot
// that is no tracer rarely passes: 256 bits per id (one id per eight words: about 1 in 10^4 passes), at least 2^10 bits
// (128 bytes), at most 2^19 (64 KiB of LDS: two workgroups still share a CU; 65536 ids then fill it four to a word and
// about 1 slot in 20 passes).
constexpr uint32_t kFilterMinLog2 = 10, kFilterMaxLog2 = 19;
inline uint32_t filter_log2(uint32_t m)
{
    uint32_t l = kFilterMinLog2;
    while (l < kFilterMaxLog2 && (1ull << l) < 256ull * m) ++l;
    return l;
}
// the word of an id and its three bits as a mask
FES_SERIES_HD void filter_place(uint32_t id, uint32_t log2bits, uint32_t& word, uint32_t& mask)
{
    const uint32_t h = id * 0x9E3779B1u, shift = 32 - (log2bits - 5);   // (shift >= 18: the fields lie below the word's bits)
    word = h >> shift;
    mask = 1u << (h >> (shift - 5) & 31) | 1u << (h >> (shift - 10) & 31) | 1u << (h >> (shift - 15) & 31);
}
FES_SERIES_HD bool filter_hit(const uint32_t* words, uint32_t id, uint32_t log2bits)
{
    uint32_t w, mask;
    filter_place(id, log2bits, w, mask);
    return (words[w] & mask) == mask;
}
// the place of `id` in sorted[0 .. m), or -1
FES_SERIES_HD int64_t lookup(const uint32_t* sorted, uint32_t m, uint32_t id)
{
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < m && sorted[lo] == id ? static_cast<int64_t>(lo) : -1;
}

struct Table {
    int species = 0;
    uint32_t log2bits = kFilterMinLog2;
    std::vector<uint32_t> sorted, index, filter;
};
// the tables of a (checked) request, one per species that has tracers, in ascending species order
inline std::vector<Table> build(const fpic_series_spec& s)
{
    std::vector<std::pair<uint64_t, uint32_t>> keyed(s.ntracers);
    for (uint32_t t = 0; t < s.ntracers; ++t) keyed[t] = { static_cast<uint64_t>(s.tracer_species[t]) << 32 | s.tracer_id[t], t };
    std::sort(keyed.begin(), keyed.end());
    std::vector<Table> out;
    for (size_t a = 0; a < keyed.size();) {
        size_t b = a;
        while (b < keyed.size() && keyed[b].first >> 32 == keyed[a].first >> 32) ++b;
        Table t;
        t.species = static_cast<int>(keyed[a].first >> 32);
        t.log2bits = filter_log2(static_cast<uint32_t>(b - a));
        t.filter.assign(size_t(1) << (t.log2bits - 5), 0u);
        for (size_t k = a; k < b; ++k) {
            const uint32_t id = static_cast<uint32_t>(keyed[k].first);
            t.sorted.push_back(id);
            t.index.push_back(keyed[k].second);
            uint32_t w, mask;
            filter_place(id, t.log2bits, w, mask);
            t.filter[w] |= mask;
        }
        out.push_back(std::move(t));
        a = b;
    }
    return out;
}

// a point whose cell plane (step 2 of the rule) is k belongs to the handle that owns that plane
FES_SERIES_HD bool owns_plane(int k, int k0, int nk) { return k >= k0 && k < k0 + nk; }

// Selection by flag: entry i of `out` is entry i of the one part whose flag (column `flag` of the entry) is set, zeros if
// none has it set — a selection, not a sum: -0.0 + 0.0 would change bits.  part r starts at parts + r * stride (doubles).
// Returns -1, or the first entry that two parts flag (an internal error: nothing is resolved silently).
inline int64_t select(const double* parts, size_t stride, int nparts, size_t entries, int flag, double* out)
{
    for (size_t i = 0; i < entries; ++i) {
        const double* from = nullptr;
        for (int r = 0; r < nparts; ++r) {
            const double* e = parts + static_cast<size_t>(r) * stride + i * kEntry;
            if (e[flag] != 0) {
                if (from) return static_cast<int64_t>(i);
                from = e;
            }
        }
        for (int c = 0; c < kEntry; ++c) out[i * kEntry + c] = from ? from[c] : 0.0;
    }
    return -1;
}

} // namespace fesser
#endif
