// fes_fusion_kernels.hpp — the pass of the fusion yield tally of a CART3D handle (fpic_fusion; host side
// fes_fusion.inc.hpp, the rule fes_fusion_core.hpp).  The cell index is fpic_pair's, built by the same three passes
// (pair_count*, pair_scan, pair_fill* of fes_pair_kernels.hpp) into the same buffers; this header adds
//   pair_of<LIKE>   the pair that a place of a sorted run owns; the spectrum and the burn take it from here.
//   fusion_tally_kernel<T, LIKE>   The runs of sorted cells are those of pair_walk (fes_pair_kernels.hpp) with this family's
//       key, but this kernel KEEPS ITS OWN COPY of the walk and of the pair's derivation: with the shared ones its like
//       instance in fp32 measured 1.2 - 2 % slower, in every form that was tried (DESIGN 4.30 has the numbers).  A change
//       to pair_walk's planning or sort has to be made here as well.
//       Per run EVERY PAIR HAS A LANE OF ITS OWN: nothing is written back, so the chain of a `few` particle has no sequential
//       dependence; the lane of a `many` entry (unlike species) or of a pair's owner (like species; the three places of an odd
//       cell's triple own one pair each) gathers the two velocities, interpolates the table and floors the yield.
//       The table (at most 32 KiB of doubles) is gathered from global memory: beside the run's 56.5 KiB it would leave one
//       workgroup on a CU's 160 KiB of LDS, not two, and the sort is what the LDS is for; a table is read by every
//       workgroup of the pass at neighbouring entries (the relative speeds of a thermal plasma fill a small part of it), so
//       it lives in the CU's 32 KiB vector cache and the XCD's 4 MiB L2.
//       Per-cell sums: the lanes of a wave whose pairs are all of one cell (every wave of a cell above 64 pairs) add their q
//       across the wave and lane 0 keeps the sum in a register until the wave's cell changes; then, and for the mixed waves
//       of small cells lane by lane, the sum goes to the cell's 64-bit word of the run in LDS.  After the run one lane per
//       cell with a non-zero sum issues ONE 64-bit vector atomic add on the cell's word of the grid.
//       The counts (pairs, below, above, cells, overfull_cells, overfull_particles, yield_hi, yield_lo) are kept per lane —
//       a lane carries its low word into its high one — and added with collide_counts.  No scratch.
#pragma once

#include "fes_fusion_core.hpp"
#include "fes_pair_kernels.hpp"

namespace fes {

constexpr int kFusionCounts = 8;
constexpr size_t kFusionLdsBytes = kPairChunk * sizeof(unsigned long long) + kPairLdsBytes;
static_assert(kFusionLdsBytes <= 64 * 1024, "two workgroups per CU");
static_assert(fesfusion::kCellMax == kPairCellMax, "the bound's N_L is the cap");

template <typename T>
struct FusionArgs : PairHead<const T> {
    unsigned long long* counts;       // pairs, below, above, cells, overfull_cells, overfull_particles, yield_hi, yield_lo
    unsigned long long* grid;         // ncells words (int64 in two's complement)
    const double* table;              // r.n cross-sections
    fesfusion::Rule r;
};

// The pair that the place e of a sorted run owns (the tally, the spectrum and the burn: every pair has a lane of its own).
// Unlike species: the owner is the `many` particle, its partner few[p mod Nf]; like species: fesfusion::like_pair.
constexpr uint32_t kPairAlone = 0xFFFFFFFFu;
struct PairOf {
    bool has, isb, first;             // it owns one; unlike species: the owner is of species_b; the owner is the first of its cell
    uint32_t cell;                    // the run's cell of the place, whether it owns a pair or not
    uint32_t pp;                      // the partner's place: the owner's entry is sorted[e], the partner's sorted[pp]
    uint32_t chain, p;                // the place of the particle the pair shares with others — the `few` particle, the first of an
                                      // odd like cell's triple; kPairAlone: it shares none — and the owner's place in its segment
    double nl;
};
template <bool LIKE>
__device__ __forceinline__ PairOf pair_of(const PairRun& t, uint32_t e, uint32_t na, uint32_t len)
{
    PairOf q{};
    q.chain = kPairAlone;
    q.isb = !LIKE && e >= na;
    const uint32_t local = q.isb ? e - na : e;
    const uint32_t l = pair_segment_of(q.isb ? t.seg_b : t.seg_a, len, local);
    q.cell = l;
    if (LIKE) {
        const uint32_t lo = t.seg_a[l], n = t.seg_a[l + 1] - lo, p = e - lo;
        uint32_t partner;
        q.has = fesfusion::like_pair(n, p, partner, q.nl);
        if (q.has) {
            q.first = p == 0;
            q.pp = lo + partner;
            if ((n & 1u) && p < 3u) q.chain = lo;       // the triple
            q.p = p;
        }
    } else {
        const uint32_t alo = t.seg_a[l], blo = t.seg_b[l];
        const uint32_t ca = t.seg_a[l + 1] - alo, cb = t.seg_b[l + 1] - blo;
        const bool a_many = fesfusion::many_is_a(ca, cb);
        const uint32_t nf = a_many ? cb : ca;
        q.has = q.isb != a_many && nf > 0;              // (this entry is of the `many` species)
        if (q.has) {
            const uint32_t p = local - (q.isb ? blo : alo);
            q.first = p == 0;
            q.nl = static_cast<double>(nf);
            q.pp = q.chain = (a_many ? na + blo : alo) + fesfusion::few_of(p, nf);
            q.p = p;
        }
    }
    return q;
}

template <typename T, bool LIKE>
__global__ __launch_bounds__(kPairThreads) void fusion_tally_kernel(FusionArgs<T> g)
{
    extern __shared__ unsigned long long fusion_lds[];
    unsigned long long* cell_sum = fusion_lds;       // [kPairChunk] the run's cells
    uint32_t* st_key = reinterpret_cast<uint32_t*>(cell_sum + kPairChunk);   // the entries as loaded: species a's of the run, then species b's
    uint32_t* st_id = st_key + kPairEntries;
    uint32_t* st_slot = st_id + kPairEntries;
    uint32_t* seg_a = st_slot + kPairEntries;        // [len + 1] the segments of the run's cells, from 0
    uint32_t* seg_b = seg_a + (kPairChunk + 1);
    uint32_t* plan = seg_b + (kPairChunk + 1);       // [0]: the cells of the run
    uint16_t* sorted = reinterpret_cast<uint16_t*>(plan + 2);   // the entries' places, sorted inside their cells' segments
    unsigned long long count[kFusionCounts] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    const int lane = threadIdx.x & 63;
    const uint32_t nchunks = (g.ncells + kPairChunk - 1) / kPairChunk;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        uint32_t c0 = chunk * kPairChunk;
        const uint32_t cend = min(c0 + static_cast<uint32_t>(kPairChunk), g.ncells);
        while (c0 < cend) {
            // the run [c0, c0 + len): the cells from c0 on that are not overfull and fit the LDS together (wave 0 decides)
            if (threadIdx.x < 64) {
                const uint32_t c = c0 + threadIdx.x;
                bool ok = false;
                uint32_t na = 0, nb = 0;
                if (c < cend) {
                    const uint32_t ae = g.seg_a[c + 1];
                    na = ae - g.seg_a[c];
                    unsigned long long tot = ae - g.seg_a[c0];
                    if (!LIKE) {
                        const uint32_t be = g.seg_b[c + 1];
                        nb = be - g.seg_b[c];
                        tot += be - g.seg_b[c0];
                    }
                    ok = na <= static_cast<uint32_t>(kPairCellMax) && nb <= static_cast<uint32_t>(kPairCellMax) && tot <= static_cast<unsigned long long>(kPairEntries);
                }
                const unsigned long long fits = __ballot(ok);
                const uint32_t len = fits == ~0ull ? 64u : static_cast<uint32_t>(__ffsll(~fits)) - 1u;
                if (threadIdx.x == 0) {
                    plan[0] = len;
                    if (len == 0) {      // (a cell that is not overfull fits alone: c0 is overfull)
                        count[4] += 1;
                        count[5] += static_cast<unsigned long long>(na) + nb;
                    }
                }
                cell_sum[threadIdx.x] = 0;
            }
            __syncthreads();
            const uint32_t len = plan[0];
            if (len == 0) {
                c0 += 1;
                __syncthreads();   // (plan is rewritten by the next turn)
                continue;
            }
            const uint32_t a0 = g.seg_a[c0], b0 = LIKE ? 0u : g.seg_b[c0];
            if (threadIdx.x <= len) {
                seg_a[threadIdx.x] = g.seg_a[c0 + threadIdx.x] - a0;
                if (!LIKE) seg_b[threadIdx.x] = g.seg_b[c0 + threadIdx.x] - b0;
            }
            __syncthreads();
            const uint32_t na = seg_a[len], nb = LIKE ? 0u : seg_b[len], total = na + nb;   // (total <= kPairEntries)
            for (uint32_t e = threadIdx.x; e < total; e += kPairThreads) {
                const bool isb = !LIKE && e >= na;
                const uint32_t slot = isb ? g.index_b[b0 + (e - na)] : g.index_a[a0 + e];
                const uint32_t* ids = isb ? g.id_b : g.id_a;
                const uint32_t id = ids ? ids[slot] : slot;
                st_key[e] = fesfusion::key_of(g.r, id);
                st_id[e] = id;
                st_slot[e] = slot;
            }
            __syncthreads();
            // the sort: an entry's place in its cell's segment is the number of entries of the segment before it
            for (uint32_t e = threadIdx.x; e < total; e += kPairThreads) {
                const bool isb = !LIKE && e >= na;
                const uint32_t base = isb ? na : 0u;
                const uint32_t* seg = isb ? seg_b : seg_a;
                const uint32_t l = pair_segment_of(seg, len, e - base);
                const uint32_t lo = base + seg[l], hi = base + seg[l + 1];
                if (hi - lo > g.rank_max) {        // (the network below sorts this segment)
                    sorted[e] = static_cast<uint16_t>(e);
                    continue;
                }
                const uint32_t key = st_key[e], id = st_id[e];
                uint32_t rank = 0;
                for (uint32_t j = lo; j < hi; ++j) rank += fespair::before(st_key[j], st_id[j], key, id) ? 1u : 0u;
                sorted[lo + rank] = static_cast<uint16_t>(e);
            }
            __syncthreads();
            for (uint32_t l = 0; l < len; ++l) {   // (the same segments for every lane: the tables are in LDS)
                if (seg_a[l + 1] - seg_a[l] > g.rank_max) pair_bitonic(sorted, st_key, st_id, seg_a[l], seg_a[l + 1] - seg_a[l]);
                if (!LIKE && seg_b[l + 1] - seg_b[l] > g.rank_max) pair_bitonic(sorted, st_key, st_id, na + seg_b[l], seg_b[l + 1] - seg_b[l]);
            }
            // the pairs: the place e owns at most one.  Every lane of a wave takes the same turns (the ballots below).
            unsigned long long held = 0;           // lane 0: the sum of the wave's last whole-wave cell
            uint32_t held_cell = ~0u;
            const uint32_t turns = (total + kPairThreads - 1) / kPairThreads;
            for (uint32_t turn = 0; turn < turns; ++turn) {
                const uint32_t e = turn * kPairThreads + threadIdx.x;
                uint32_t cell = ~0u;               // the run's cell of this lane's entry; ~0: no entry
                unsigned long long q = 0;
                if (e < total) {
                    const bool isb = !LIKE && e >= na;
                    const uint32_t local = isb ? e - na : e;
                    const uint32_t l = pair_segment_of(isb ? seg_b : seg_a, len, local);
                    cell = l;
                    uint32_t so = 0, sp = 0;       // the slots of the owner and of the partner
                    double nl = 0;
                    bool has = false;
                    if (LIKE) {
                        const uint32_t lo = seg_a[l], n = seg_a[l + 1] - lo, p = e - lo;
                        uint32_t partner;
                        has = fesfusion::like_pair(n, p, partner, nl);
                        if (has) {
                            if (p == 0) count[3] += 1;
                            so = st_slot[sorted[e]];
                            sp = st_slot[sorted[lo + partner]];
                        }
                    } else {
                        const uint32_t alo = seg_a[l], blo = seg_b[l];
                        const uint32_t ca = seg_a[l + 1] - alo, cb = seg_b[l + 1] - blo;
                        const bool a_many = fesfusion::many_is_a(ca, cb);
                        const uint32_t nf = a_many ? cb : ca;
                        has = isb != a_many && nf > 0;       // (this entry is of the `many` species)
                        if (has) {
                            const uint32_t p = local - (isb ? blo : alo);
                            if (p == 0) count[3] += 1;
                            nl = static_cast<double>(nf);
                            so = st_slot[sorted[e]];
                            sp = st_slot[sorted[(a_many ? na + blo : alo) + fesfusion::few_of(p, nf)]];
                        }
                    }
                    if (has) {
                        double vo[3], vp[3];
                        pair_load(!LIKE && isb ? g.slab_b : g.slab_a, !LIKE && isb ? g.n_pad_b : g.n_pad_a, so, vo);
                        pair_load(LIKE || isb ? g.slab_a : g.slab_b, LIKE || isb ? g.n_pad_a : g.n_pad_b, sp, vp);
                        int64_t qq;
                        const int what = fesfusion::tally(g.r, g.table, nl, vo, vp, qq);
                        count[0] += what == fesfusion::kInside ? 1 : 0;
                        count[1] += what == fesfusion::kBelow ? 1 : 0;
                        count[2] += what == fesfusion::kAbove ? 1 : 0;
                        q = static_cast<unsigned long long>(qq);
                        count[6] += q >> 32;
                        count[7] += q & 0xFFFFFFFFull;
                    }
                }
                // registers -> wave -> LDS (an entry that owns no pair adds 0: the wave of a large cell stays whole)
                const uint32_t first = __shfl(cell, 0, 64);
                const bool whole = first != ~0u && __ballot(cell == first) == ~0ull;
                if (whole) {
                    unsigned long long s = q;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
                    if (lane == 0) {
                        if (held_cell != first) {
                            if (held) atomicAdd(&cell_sum[held_cell], held);
                            held = 0;
                            held_cell = first;
                        }
                        held += s;
                    }
                } else if (q) {
                    atomicAdd(&cell_sum[cell], q);
                }
            }
            if (lane == 0 && held) atomicAdd(&cell_sum[held_cell], held);
            __syncthreads();
            if (threadIdx.x < len) {
                const unsigned long long s = cell_sum[threadIdx.x];
                if (s) atomicAdd(g.grid + c0 + threadIdx.x, s);
            }
            __syncthreads();   // (the run's tables are rewritten by the next)
            c0 += len;
        }
    }
    count[6] += count[7] >> 32;    // (a lane's low word is carried: the workgroups' adds stay below 2^49 per application)
    count[7] &= 0xFFFFFFFFull;
    collide_counts<kFusionCounts>(count, g.counts);
}

} // namespace fes
