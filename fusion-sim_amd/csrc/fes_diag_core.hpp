// fes_diag_core.hpp — the host rules of the energy diagnostics (fpic_energy_*; the kernels are fes_diag_kernels.hpp, the
// orchestration fes_diag.inc.hpp) and of what the box diagnostics share (fes_record.inc.hpp): which planes a handle reduces
// and where it holds them, the recording ring's indexing, drop count, commit and drain, the ranks' agreement on a drain, the
// ranks' integer sum, and the fixed-order combination of several handles' rows.  Plain C++, shared with a host test
// (tests/native/diag_core_test.cpp, g++).
#ifndef FES_DIAG_CORE_HPP
#define FES_DIAG_CORE_HPP
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/fusionpic.h"
#include "fes_groups.hpp"

namespace fesdiag {

// the planes [k0, k0 + nk) a handle reduces: all nz of an undecomposed handle, the slab of rank `rank` of `world`
// (nz / world planes each, as fpic_domain_init) — in non-compact decomposed mode too, where every rank holds the whole grid,
// so that the ranks' sum counts every node once
struct Owned {
    int k0, nk;
};
inline Owned owned_planes(int nz, int world, int rank)
{
    if (world <= 1) return Owned{ 0, nz };
    const int nzl = nz / world;
    return Owned{ rank * nzl, nzl };
}

// every owned plane is held (fes::held_plane of the global plane is not -1), and with `next` also the plane above each of
// them (the curl that forms B of the integer time from the half-time B reads E one plane up)
inline bool owned_are_held(Owned o, fes::Held held, int nz, bool next)
{
    for (int k = o.k0; k < o.k0 + o.nk + (next ? 1 : 0); ++k)
        if (fes::held_plane(k % nz, held, nz) < 0) return false;
    return true;
}

// The recording ring: row number s (0, 1, 2, ... in the order the sub-steps enqueued them) goes to slot s % cap.  The host
// counts the rows it has enqueued (seq) and drained (drained), so it needs no read-back to index the ring.
struct Ring {
    uint64_t cap = 0, seq = 0, drained = 0;
    uint64_t slot(uint64_t s) const { return s % cap; }
    // the rows a drain returns: [first, first + n) of the sequence — the newest cap of those not yet drained — and how many
    // older ones the ring has overwritten
    void pending(uint64_t& first, uint64_t& n, uint64_t& dropped) const
    {
        const uint64_t avail = seq - drained;
        n = std::min(avail, cap);
        dropped = avail - n;
        first = seq - n;
    }
    // rows [first, first + n) as at most two runs of slots: (slot[k], len[k]), k < the returned count
    int runs(uint64_t first, uint64_t n, uint64_t slot_out[2], uint64_t len_out[2]) const
    {
        if (!n) return 0;
        const uint64_t s0 = slot(first), head = std::min(n, cap - s0);
        slot_out[0] = s0;
        len_out[0] = head;
        if (head == n) return 1;
        slot_out[1] = 0;
        len_out[1] = n - head;
        return 2;
    }
    void commit() { ++seq; }                  // the row enqueued into slot(seq) counts from now on
    void mark_drained() { drained = seq; }    // the rows pending() named have been delivered
};

// the ranks' agreement before a collective drain: pairs = [world][2], every rank's (pending rows, dropped rows) as doubles in
// rank order; the first rank whose pair differs from (n, dropped), or -1
inline int disagreeing_rank(const double* pairs, int world, double n, double dropped)
{
    for (int r = 0; r < world; ++r)
        if (pairs[2 * r] != n || pairs[2 * r + 1] != dropped) return r;
    return -1;
}

// out[i] = parts[i] + parts[m + i] + ... + parts[(world - 1) m + i]: `world` parts of m words, added in rank order
inline void add_words(const uint64_t* parts, size_t m, int world, uint64_t* out)
{
    for (size_t i = 0; i < m; ++i) out[i] = 0;
    for (int r = 0; r < world; ++r)
        for (size_t i = 0; i < m; ++i) out[i] += parts[static_cast<size_t>(r) * m + i];
}

// out = the rows part[0], part[stride], ..., part[(nparts - 1) stride] combined in that order: sums left to right (counts,
// energies, momenta), speed_max the largest (NaN if any part's is); substep and nspecies are part[0]'s (the parts are one sub-step of one box)
inline void combine(const fpic_energy* part, size_t stride, int nparts, fpic_energy* out)
{
    fpic_energy r = part[0];
    for (int p = 1; p < nparts; ++p) {
        const fpic_energy& q = part[static_cast<size_t>(p) * stride];
        r.field_e += q.field_e;
        r.field_b += q.field_b;
        r.field_b_external += q.field_b_external;
        for (int s = 0; s < FPIC_ENERGY_SPECIES; ++s) {
            r.count[s] += q.count[s];
            r.kinetic[s] += q.kinetic[s];
            for (int a = 0; a < 3; ++a) r.momentum[s][a] += q.momentum[s][a];
            if (q.speed_max[s] > r.speed_max[s] || q.speed_max[s] != q.speed_max[s]) r.speed_max[s] = q.speed_max[s]; // (NaN kept)
        }
    }
    *out = r;
}

} // namespace fesdiag
#endif
