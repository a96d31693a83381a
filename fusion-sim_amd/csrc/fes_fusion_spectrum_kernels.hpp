// fes_fusion_spectrum_kernels.hpp — the pass of the fusion product spectrum of a CART3D handle (fpic_fusion_spectrum; host side
// fes_fusion_spectrum.inc.hpp, the rule fes_fusion_spectrum_core.hpp on top of fes_fusion_core.hpp).  The cell index is
// fpic_pair's (pair_index<T>, unchanged); this header adds
//   fusion_spectrum_kernel<T, LIKE, AXIS>   A workgroup takes chunks of kPairChunk consecutive cells, cuts each into runs that
//       fit kPairEntries places of LDS, loads (key, id, slot) per entry and sorts every cell's segment in (key, id) exactly as
//       fusion_tally_kernel does, with the same helpers (pair_segment_of, pair_bitonic, pair_load) and the same key, so the
//       pairs and their q are the tally's.  EVERY PAIR HAS A LANE OF ITS OWN: the lane gathers the two velocities, floors the
//       yield (fesfusion::tally), computes the pair's place on the axis (AXIS = FPIC_FSPEC_CM: K; FPIC_FSPEC_PRODUCT: the
//       product's laboratory energy, with a line of sight or a direction of its own from at most 8 Philox blocks) and adds
//       q >> 32 and q & 0xFFFFFFFF to the entry's two words of the workgroup's histogram with LDS 64-bit atomics.
//       The histogram is (bins + 2) x 2 words of LDS (at most 4128 B) in front of the run's 56.5 KiB: zeroed ONCE PER
//       WORKGROUP, carried across all its chunks and runs, and flushed once at the end — a lane per entry carries the low
//       word into the high one and issues one 64-bit vector atomic per non-zero word.  The total stays below the 64 KiB a
//       launch may ask for without an attribute, so two workgroups share a CU as in the tally: this is why the bin cap is 256.
//       The per-cell words of the tally are not needed.  The counts (pairs, below, above, cells, overfull_cells,
//       overfull_particles, yield_hi, yield_lo) are kept per lane as in the tally and added with collide_counts.  No scratch.
#pragma once

#include "fes_fusion_spectrum_core.hpp"
#include "fes_fusion_kernels.hpp"

namespace fes {

constexpr int kFspecEntriesMax = FPIC_FUSION_SPECTRUM_BINS_MAX + 2;      // the bins, `under`, `over`
constexpr size_t kFspecHistBytesMax = kFspecEntriesMax * 2 * sizeof(unsigned long long);
constexpr size_t kFspecLdsBytesMax = kFspecHistBytesMax + kPairLdsBytes;
static_assert(kFspecLdsBytesMax <= 64 * 1024, "two workgroups per CU, and no launch attribute");

template <typename T>
struct FspecArgs {
    const T *slab_a, *slab_b;         // six arrays of n_pad each; like species: b = a
    const uint32_t *id_a, *id_b;      // nullptr: slot = id
    size_t n_pad_a, n_pad_b;
    const uint32_t *seg_a, *seg_b;    // cells + 1 words: cell c is index[seg[c] .. seg[c + 1])
    const uint32_t *index_a, *index_b;
    uint32_t ncells;
    uint32_t rank_max;                // a segment of more entries is sorted by the bitonic network, not by counting
    unsigned long long* counts;       // pairs, below, above, cells, overfull_cells, overfull_particles, yield_hi, yield_lo
    unsigned long long* words;        // (bins + 2) x 2: per entry the high and the low word
    const double* table;              // r.n cross-sections
    fesfusion::Rule r;
    fesfspec::Rule s;
};

// the dynamic LDS of a launch with `bins` bins
inline size_t fspec_lds_bytes(int bins) { return static_cast<size_t>(bins + 2) * 2 * sizeof(unsigned long long) + kPairLdsBytes; }

template <typename T, bool LIKE, int AXIS>
__global__ __launch_bounds__(kPairThreads) void fusion_spectrum_kernel(FspecArgs<T> g)
{
    extern __shared__ unsigned long long fspec_lds[];
    const uint32_t entries = static_cast<uint32_t>(g.s.bins) + 2u;
    unsigned long long* hist = fspec_lds;            // [entries][2] the workgroup's histogram: high word, low word
    uint32_t* st_key = reinterpret_cast<uint32_t*>(hist + 2 * entries);   // the entries as loaded: species a's of the run, then species b's
    uint32_t* st_id = st_key + kPairEntries;
    uint32_t* st_slot = st_id + kPairEntries;
    uint32_t* seg_a = st_slot + kPairEntries;        // [len + 1] the segments of the run's cells, from 0
    uint32_t* seg_b = seg_a + (kPairChunk + 1);
    uint32_t* plan = seg_b + (kPairChunk + 1);       // [0]: the cells of the run
    uint16_t* sorted = reinterpret_cast<uint16_t*>(plan + 2);   // the entries' places, sorted inside their cells' segments
    unsigned long long count[kFusionCounts] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (uint32_t w = threadIdx.x; w < 2 * entries; w += kPairThreads) hist[w] = 0;
    __syncthreads();
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
            // the pairs: the place e owns at most one
            for (uint32_t e = threadIdx.x; e < total; e += kPairThreads) {
                const bool isb = !LIKE && e >= na;
                const uint32_t local = isb ? e - na : e;
                const uint32_t l = pair_segment_of(isb ? seg_b : seg_a, len, local);
                uint32_t eo = 0, so = 0, sp = 0;   // the owner's entry, the slots of the owner and of the partner
                double nl = 0;
                bool has = false;
                if (LIKE) {
                    const uint32_t lo = seg_a[l], n = seg_a[l + 1] - lo, p = e - lo;
                    uint32_t partner;
                    has = fesfusion::like_pair(n, p, partner, nl);
                    if (has) {
                        if (p == 0) count[3] += 1;
                        eo = sorted[e];
                        so = st_slot[eo];
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
                        eo = sorted[e];
                        so = st_slot[eo];
                        sp = st_slot[sorted[(a_many ? na + blo : alo) + p % nf]];
                    }
                }
                if (!has) continue;
                double vo[3], vp[3];
                pair_load(!LIKE && isb ? g.slab_b : g.slab_a, !LIKE && isb ? g.n_pad_b : g.n_pad_a, so, vo);
                pair_load(LIKE || isb ? g.slab_a : g.slab_b, LIKE || isb ? g.n_pad_a : g.n_pad_b, sp, vp);
                int64_t qq;
                const int what = fesfusion::tally(g.r, g.table, nl, vo, vp, qq);
                count[0] += what == fesfusion::kInside ? 1 : 0;
                count[1] += what == fesfusion::kBelow ? 1 : 0;
                count[2] += what == fesfusion::kAbove ? 1 : 0;
                if (what != fesfusion::kInside) continue;
                const unsigned long long q = static_cast<unsigned long long>(qq);
                count[6] += q >> 32;
                count[7] += q & 0xFFFFFFFFull;
                if (!q) continue;                  // (nothing to add: the pair's place does not matter)
                const double K = fesfspec::cm_energy(g.s, fesfspec::speed_of(vo, vp));
                double x = K;
                if (AXIS == FPIC_FSPEC_PRODUCT) {
                    double n[3] = { g.s.n[0], g.s.n[1], g.s.n[2] };
                    if (!g.s.sight) (void)fesfspec::direction_of(g.r, st_id[eo], !LIKE && isb, n);
                    const double f_o = !LIKE && isb ? g.s.f_b : g.s.f_a, f_p = LIKE || isb ? g.s.f_a : g.s.f_b;
                    x = fesfspec::product_energy(g.s, K, f_o, f_p, vo, vp, n);
                }
                const uint32_t k = static_cast<uint32_t>(fesfspec::entry_of(g.s, x));   // (0 <= k < entries by construction)
                if (q >> 32) atomicAdd(&hist[2 * k], q >> 32);
                atomicAdd(&hist[2 * k + 1], q & 0xFFFFFFFFull);
            }
            __syncthreads();   // (the run's tables are rewritten by the next)
            c0 += len;
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < entries; k += kPairThreads) {
        const unsigned long long lo = hist[2 * k + 1], hi = hist[2 * k] + (lo >> 32);
        if (hi) atomicAdd(g.words + 2 * k, hi);
        if (lo & 0xFFFFFFFFull) atomicAdd(g.words + 2 * k + 1, lo & 0xFFFFFFFFull);
    }
    count[6] += count[7] >> 32;    // (a lane's low word is carried: the workgroups' adds stay below 2^49 per application)
    count[7] &= 0xFFFFFFFFull;
    collide_counts<kFusionCounts>(count, g.counts);
}

} // namespace fes
