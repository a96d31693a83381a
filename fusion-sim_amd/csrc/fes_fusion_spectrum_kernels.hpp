// fes_fusion_spectrum_kernels.hpp — the pass of the fusion product spectrum of a CART3D handle (fpic_fusion_spectrum; host side
// fes_fusion_spectrum.inc.hpp, the rule fes_fusion_spectrum_core.hpp on top of fes_fusion_core.hpp).  The cell index is
// fpic_pair's (pair_index<T>, unchanged); this header adds
//   fusion_spectrum_kernel<T, LIKE, AXIS>   The runs of sorted cells are pair_walk's (fes_pair_kernels.hpp) with the tally's key,
//       the pair of a place is pair_of's (fes_fusion_kernels.hpp), so the pairs and their q are the tally's.
//       EVERY PAIR HAS A LANE OF ITS OWN: the lane gathers the two velocities, floors the
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
// (this pass has no sort and no lookup of a place's cell of its own: it reaches the pair pass's through pair_walk and pair_of)
using fes::pair_bitonic;
using fes::pair_segment_of;

template <typename T>
struct FspecArgs : PairHead<const T> {
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
    unsigned long long* hist = fspec_lds;            // [entries][2] the workgroup's histogram: high word, low word; in front of the run's tables
    const PairRun t(hist + 2 * entries);
    unsigned long long count[kFusionCounts] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (uint32_t w = threadIdx.x; w < 2 * entries; w += kPairThreads) hist[w] = 0;
    __syncthreads();
    pair_walk<LIKE>(
        g, t, [&](uint32_t id) { return fesfusion::key_of(g.r, id); },
        [&](unsigned long long particles) {
            count[4] += 1;
            count[5] += particles;
        },
        [&](uint32_t, uint32_t len, uint32_t na, uint32_t, uint32_t total) {
            // the pairs: the place e owns at most one
            for (uint32_t e = threadIdx.x; e < total; e += kPairThreads) {
                const PairOf pair = pair_of<LIKE>(t, e, na, len);
                if (!pair.has) continue;
                if (pair.first) count[3] += 1;
                const uint32_t eo = t.sorted[e];   // the owner's entry
                double vo[3], vp[3];
                pair_load(pair.isb ? g.slab_b : g.slab_a, pair.isb ? g.n_pad_b : g.n_pad_a, t.st_slot[eo], vo);
                pair_load(LIKE || pair.isb ? g.slab_a : g.slab_b, LIKE || pair.isb ? g.n_pad_a : g.n_pad_b, t.st_slot[t.sorted[pair.pp]], vp);
                int64_t qq;
                const int what = fesfusion::tally(g.r, g.table, pair.nl, vo, vp, qq);
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
                    if (!g.s.sight) (void)fesfspec::direction_of(g.r, t.st_id[eo], pair.isb, n);
                    const double f_o = pair.isb ? g.s.f_b : g.s.f_a, f_p = LIKE || pair.isb ? g.s.f_a : g.s.f_b;
                    x = fesfspec::product_energy(g.s, K, f_o, f_p, vo, vp, n);
                }
                const uint32_t k = static_cast<uint32_t>(fesfspec::entry_of(g.s, x));   // (0 <= k < entries by construction)
                if (q >> 32) atomicAdd(&hist[2 * k], q >> 32);
                atomicAdd(&hist[2 * k + 1], q & 0xFFFFFFFFull);
            }
        });
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
