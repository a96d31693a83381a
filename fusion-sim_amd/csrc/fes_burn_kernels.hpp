// fes_burn_kernels.hpp — the passes of the fusion burn of a CART3D handle (fpic_burn; host side fes_burn.inc.hpp, the rule
// fes_burn_core.hpp).  The cell index is fpic_pair's (pair_index<T>), the ranks of the events come from fpic_renumber's
// popcount scan (renumber_count_kernel, load_scan_kernel); this header adds
//   burn_decide_kernel<T, LIKE>   the runs of sorted cells are pair_walk's (fes_pair_kernels.hpp) with this family's key, the
//       pair of a place pair_of's (fes_fusion_kernels.hpp); per run two sweeps over its places, a lane per pair.  FIRST sweep: the
//       lookup, P and the acceptance; an accepted pair that shares a particle with others — the chain of a `few` particle,
//       the triple of an odd like cell — takes an integer atomicMin with its place on the chain's word in LDS.  The words lie
//       where the sort keys lay (a key is dead once its segment is sorted), one per place, so a chain's word is the place of
//       its `few` particle (of the triple's first particle).  A lane remembers its accepted pairs as a bit per turn.  SECOND
//       sweep, behind a barrier: an accepted pair whose place is the chain's minimum reacts, every other one is `blocked`.
//       For a reacting pair the lane sets the reactants' bits in the slot bitmap of their species and the species_a
//       reactant's bit in the bitmap over that species' id span (integer atomicOr), and keeps the row (slot_a, slot_b,
//       id_a).  The waves put their rows into a stage in the workgroup's LDS (a ballot, one LDS atomic per wave), and the
//       workgroup empties the stage into the event list when another turn might not fit: ONE 64-bit atomic on the cursor per
//       emptying (DESIGN 4.28 has what one per wave costs).  The cursor is the event count the host reads.  The pass writes
//       NO particle: the host may still refuse the application.  The tally's cell sums are not needed; the stage takes
//       their room and what the 64 KiB leave.
//   burn_generate_kernel<T>   over the M events, one per lane: the rank of the event = the marked ids below id_a's, the
//       outcome from the stored state (the same operations on the same values as the deciding pass: the same g), the
//       products' six state words and ids at n + rank of their species, the exact gained sums.
//   burn_count_kernel, burn_move_kernel<T>   the compaction of a reactant species, the sibling of fpic_remove's passes with
//       the predicate "my slot's bit": a wave owns a chunk of kRemoveChunk slots; the count pass stores the chunk's survivors
//       (the popcount of its 64 bitmap words), (load_scan_kernel), the move pass writes the survivors — six state words and
//       the id — to offset[chunk] + (the survivors below me: ballots and mbcnt) of the other particle set and tallies what left.
//   burn_add_kernel   one thread: the row of this application added to the burner's totals.
// No float atomics, no inline assembly, no scratch.
#pragma once

#include "fes_burn_core.hpp"
#include "fes_fusion_kernels.hpp"
#include "fes_remove_kernels.hpp"

namespace fes {

struct BurnEvent {
    uint32_t slot_a, slot_b, id_a;
};

constexpr uint32_t kBurnStage = 512;       // rows of the stage: a turn adds at most kPairThreads
constexpr int kBurnTurnsMax = kPairEntries / kPairThreads;   // the turns of a run: a bit each in a lane's register
struct BurnStageHead {
    unsigned long long base;      // the rows taken of the list
    uint32_t n;                   // rows staged
    uint32_t flush;               // this turn's decision, written by one lane between two barriers
};
using BurnDecideCounts = Tally<fesburn::kDecideCounts, 0>;
using BurnGenSums = Tally<1, fesburn::kGenSums>;
using BurnLostSums = Tally<1, fesburn::kLostSums>;
static_assert(BurnGenSums::kWords == fesburn::kGenWords && BurnLostSums::kWords == fesburn::kLostWords, "the tallies' words are the request's");
constexpr size_t kBurnLdsBytes = kPairLdsBytes + sizeof(BurnStageHead) + kBurnStage * sizeof(BurnEvent);
// (beside the launch's bytes: the part[][] of tally_commit, a row per wave)
static_assert(kBurnLdsBytes + (kPassThreads / 64) * BurnDecideCounts::kWords * sizeof(unsigned long long) <= 64 * 1024, "two workgroups per CU");
static_assert(kPairLdsBytes % alignof(BurnStageHead) == 0, "the stage's head lies behind the run's tables");
static_assert(kBurnTurnsMax <= 32 && kBurnStage >= 2 * kPairThreads, "a lane's accepted turns fit a word; the stage holds a turn beside what stayed");
static_assert(kPairThreads == kPassThreads, "tally_commit reduces a workgroup of kPassThreads");

template <typename T>
struct BurnDecideArgs : PairHead<const T> {
    unsigned long long* words;        // fesburn::kDecideCounts of them are added here
    unsigned long long* cursor;       // the rows taken of `events`: the event count
    BurnEvent* events;                // room for max_events rows
    unsigned long long max_events;    // (a particle burns once: the rule never passes it; a row beyond it is not written)
    uint32_t *gone_a, *gone_b;        // a bit per slot of the species, zeroed; like species: b = a
    uint32_t* marked;                 // a bit per id below species_a's id span, zeroed
    const double* table;              // r.f.n cross-sections
    fesburn::Rule r;
};
static_assert(fesburn::kNoPlace == kPairAlone, "a chain's untouched word is the chain of a pair that shares no particle");

// The lanes' rows of this turn -> the workgroup's stage, and the stage -> rows of the list when another turn might not fit
// (last: whatever it holds).  EVERY lane of the workgroup calls it, once per turn and once after the loop
template <typename T>
__device__ __forceinline__ void burn_stage(const BurnDecideArgs<T>& g, BurnStageHead& st, BurnEvent* rows, bool keep, const BurnEvent& mine, bool last)
{
    const unsigned long long held = __ballot(keep);
    if (held) {                          // (wave-uniform)
        uint32_t at = 0;
        if ((threadIdx.x & 63) == 0) at = atomicAdd(&st.n, static_cast<uint32_t>(__popcll(held)));   // (st.n <= kBurnStage - kPairThreads before the turn)
        at = __shfl(at, 0, 64);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(held >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(held), 0u));
        if (keep) rows[at + below] = mine;
    }
    __syncthreads();                     // (every wave's rows and its add to st.n are in)
    if (threadIdx.x == 0) {
        st.flush = (st.n > kBurnStage - kPairThreads || (last && st.n != 0)) ? 1u : 0u;
        if (st.flush) st.base = atomicAdd(g.cursor, static_cast<unsigned long long>(st.n));
    }
    __syncthreads();
    if (st.flush) {                      // (workgroup-uniform)
        const uint32_t n = st.n;
        for (uint32_t k = threadIdx.x; k < n; k += kPairThreads)
            if (st.base + k < g.max_events) g.events[st.base + k] = rows[k];
        __syncthreads();
        if (threadIdx.x == 0) st.n = 0;
        __syncthreads();                 // (the next turn adds to an empty stage)
    }
}

template <typename T, bool LIKE>
__global__ __launch_bounds__(kPairThreads) void burn_decide_kernel(BurnDecideArgs<T> g)
{
    extern __shared__ unsigned long long burn_lds[];
    const PairRun t(burn_lds);                       // the run's tables, and behind them the stage
    BurnStageHead& stage = *reinterpret_cast<BurnStageHead*>(reinterpret_cast<unsigned char*>(burn_lds) + kPairLdsBytes);
    BurnEvent* rows = reinterpret_cast<BurnEvent*>(&stage + 1);
    uint32_t* chain = t.st_key;                      // after the sort: the chains' words, a place each
    BurnDecideCounts acc;
    if (threadIdx.x == 0) { stage.n = 0; stage.flush = 0; }
    __syncthreads();
    pair_walk<LIKE>(
        g, t, [&](uint32_t id) { return fesburn::key_of(g.r, id); },
        [&](unsigned long long particles) {
            acc.count[4] += 1;
            acc.count[5] += particles;
        },
        [&](uint32_t, uint32_t len, uint32_t na, uint32_t, uint32_t total) {
            // (every read of a key lies before a barrier: the counting sort's, or the last step's of the network)
            for (uint32_t e = threadIdx.x; e < total; e += kPairThreads) chain[e] = fesburn::kNoPlace;
            __syncthreads();
            // the first sweep: the place e owns at most one pair; P, the acceptance, the chain's minimum
            const uint32_t turns = (total + kPairThreads - 1) / kPairThreads;   // (<= kBurnTurnsMax)
            uint32_t accepted = 0;                 // a bit per turn
            for (uint32_t turn = 0; turn < turns; ++turn) {
                const uint32_t e = turn * kPairThreads + threadIdx.x;
                if (e >= total) continue;
                const PairOf q = pair_of<LIKE>(t, e, na, len);
                if (!q.has) continue;
                if (q.first) acc.count[3] += 1;
                const uint32_t eo = t.sorted[e];   // the owner's entry
                double vo[3], vp[3];
                pair_load(q.isb ? g.slab_b : g.slab_a, q.isb ? g.n_pad_b : g.n_pad_a, t.st_slot[eo], vo);
                pair_load(LIKE || q.isb ? g.slab_a : g.slab_b, LIKE || q.isb ? g.n_pad_a : g.n_pad_b, t.st_slot[t.sorted[q.pp]], vp);
                double p;
                const int what = fesburn::probability(g.r, g.table, q.nl, vo, vp, &p);
                acc.count[0] += what == fesburn::kInside ? 1 : 0;
                acc.count[1] += what == fesburn::kBelow ? 1 : 0;
                acc.count[2] += what == fesburn::kAbove ? 1 : 0;
                if (what != fesburn::kInside) continue;
                if (!fesburn::accepts(fesburn::accept_word(g.r, t.st_id[eo], q.isb), p)) continue;
                acc.count[6] += 1;
                acc.count[8] += p >= 1.0 ? 1 : 0;
                accepted |= 1u << turn;
                if (q.chain != fesburn::kNoPlace) atomicMin(&chain[q.chain], q.p);
            }
            __syncthreads();
            // the second sweep: who reacts.  Every lane of the workgroup takes the same turns (the stage's barriers)
            for (uint32_t turn = 0; turn < turns; ++turn) {
                const uint32_t e = turn * kPairThreads + threadIdx.x;
                bool reacts = false;
                BurnEvent row{};
                if (accepted >> turn & 1u) {
                    const PairOf q = pair_of<LIKE>(t, e, na, len);
                    reacts = q.chain == fesburn::kNoPlace || fesburn::wins(chain[q.chain], q.p);
                    if (reacts) {
                        const uint32_t eo = t.sorted[e], ep = t.sorted[q.pp];
                        const uint32_t ea = q.isb ? ep : eo, eb = q.isb ? eo : ep;   // the entries of species_a's and of species_b's reactant
                        row.slot_a = t.st_slot[ea];
                        row.slot_b = t.st_slot[eb];
                        row.id_a = t.st_id[ea];
                        atomicOr(g.gone_a + (row.slot_a >> 5), 1u << (row.slot_a & 31u));
                        atomicOr(g.gone_b + (row.slot_b >> 5), 1u << (row.slot_b & 31u));
                        atomicOr(g.marked + (row.id_a >> 5), 1u << (row.id_a & 31u));
                    } else {
                        acc.count[7] += 1;
                    }
                }
                burn_stage(g, stage, rows, reacts, row, false);
            }
        });
    burn_stage(g, stage, rows, false, BurnEvent{}, true);
    tally_commit(acc, g.words);
}

constexpr int kBurnThreads = 256;         // the generation pass
constexpr int kBurnBlocks = 2048;
static_assert(kBurnThreads == kPassThreads, "tally_commit reduces a workgroup of kPassThreads");

template <typename T>
struct BurnGenerateArgs {
    const T *slab_a, *slab_b;     // the reactants' live sets: six arrays of n_pad each
    size_t n_pad_a, n_pad_b;
    const BurnEvent* events;
    uint32_t m;                   // the events
    const uint32_t *bitmap, *below, *offset;   // the marked ids, per word those below it in its chunk, the chunks' exclusive offsets
    T* slab_3;                    // product_a's live set, its stride, its ids; the first new slot and id
    size_t n_pad_3;
    uint32_t* id_3;
    size_t s0_3;
    uint32_t id0_3;
    T* slab_4;                    // product_b's; nullptr: not tracked
    size_t n_pad_4;
    uint32_t* id_4;
    size_t s0_4;
    uint32_t id0_4;
    unsigned long long* words;    // BurnGenSums::kWords of them are added here
    fesburn::Rule r;
};

template <typename T>
__global__ __launch_bounds__(kBurnThreads) void burn_generate_kernel(BurnGenerateArgs<T> g)
{
    BurnGenSums acc;
    const size_t stride = static_cast<size_t>(gridDim.x) * kBurnThreads;
    for (size_t e = static_cast<size_t>(blockIdx.x) * kBurnThreads + threadIdx.x; e < g.m; e += stride) {
        const BurnEvent ev = g.events[e];
        const uint32_t i = ev.id_a, w = i >> 5;
        const uint32_t rank = g.offset[w / kRenumberChunk] + g.below[w] + __popc(g.bitmap[w] & ((1u << (i & 31u)) - 1u));
        const T* pa = g.slab_a + ev.slot_a;
        const T* pb = g.slab_b + ev.slot_b;
        double va[3], vb[3], n[3], w3[3], w4[3];
        pair_load(g.slab_a, g.n_pad_a, ev.slot_a, va);
        pair_load(g.slab_b, g.n_pad_b, ev.slot_b, vb);
        (void)fesburn::direction_of(g.r, i, n);
        fesburn::outcome(g.r, va, vb, n, w3, w4);
        const size_t s3 = g.s0_3 + rank, s4 = g.s0_4 + rank;
        double t3[3], t4[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const T c3 = static_cast<T>(w3[a]);
            g.slab_3[a * g.n_pad_3 + s3] = pa[a * g.n_pad_a];
            g.slab_3[(3 + a) * g.n_pad_3 + s3] = c3;
            t3[a] = static_cast<double>(c3);
            t4[a] = w4[a];
            if (g.slab_4) {
                const T c4 = static_cast<T>(w4[a]);
                g.slab_4[a * g.n_pad_4 + s4] = pb[a * g.n_pad_b];
                g.slab_4[(3 + a) * g.n_pad_4 + s4] = c4;
                t4[a] = static_cast<double>(c4);
            }
        }
        g.id_3[s3] = g.id0_3 + rank;
        if (g.slab_4) g.id_4[s4] = g.id0_4 + rank;
        acc.count[0] += 1;
        fesburn::gain(t3, &acc.sum[0], acc.out, 0);
        fesburn::gain(t4, &acc.sum[4], acc.out, 4);
    }
    tally_commit(acc, g.words);
}

// the compaction of a reactant species
template <typename T>
struct BurnMoveArgs {
    const T* slab;                // the live set: six arrays of n_pad
    const uint32_t* id;
    size_t n, n_pad;              // slots [0, n)
    const uint32_t* gone;         // a bit per slot: it leaves
    uint32_t* chunk;              // [nchunks]: the count pass's survivor counts, for the move pass their exclusive offsets
    size_t nchunks;
    T* dst_slab;                  // the other set
    uint32_t* dst_id;
    unsigned long long* words;    // BurnLostSums::kWords of them are added here
};
static_assert(kRemoveChunk == 64 * 32, "a wave owns a chunk: a bitmap word per lane");

__global__ __launch_bounds__(kRemoveThreads) void burn_count_kernel(const uint32_t* __restrict__ gone, size_t n, uint32_t* __restrict__ chunk, size_t nchunks)
{
    const int lane = threadIdx.x & 63;
    const size_t waves = static_cast<size_t>(gridDim.x) * (kRemoveThreads / 64);
    for (size_t c = static_cast<size_t>(blockIdx.x) * (kRemoveThreads / 64) + (threadIdx.x >> 6); c < nchunks; c += waves) {
        const size_t s0 = c * kRemoveChunk + static_cast<size_t>(lane) * 32;   // the first slot of this lane's word
        uint32_t kept = 0;
        if (s0 < n) {
            const uint32_t live = n - s0 >= 32 ? ~0u : (1u << (n - s0)) - 1u;
            kept = __popc(live & ~gone[s0 >> 5]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) kept += __shfl_xor(kept, off, 64);
        if (lane == 0) chunk[c] = kept;
    }
}

template <typename T>
__global__ __launch_bounds__(kRemoveThreads) void burn_move_kernel(BurnMoveArgs<T> g)
{
    static_assert(kRemoveThreads == kPassThreads, "tally_commit reduces a workgroup of kPassThreads");
    const int lane = threadIdx.x & 63;
    BurnLostSums acc;
    const size_t waves = static_cast<size_t>(gridDim.x) * (kRemoveThreads / 64);
    for (size_t c = static_cast<size_t>(blockIdx.x) * (kRemoveThreads / 64) + (threadIdx.x >> 6); c < g.nchunks; c += waves) {
        size_t row0 = g.chunk[c];   // the target row of the next survivor of the chunk (wave-uniform)
        for (size_t s0 = c * kRemoveChunk; s0 < (c + 1) * kRemoveChunk && s0 < g.n; s0 += 64) {   // (wave-uniform)
            const size_t slot = s0 + lane;
            const bool live = slot < g.n;
            const bool leaves = live && (g.gone[slot >> 5] >> (slot & 31u) & 1u);
            const bool keep = live && !leaves;
            const unsigned long long b = __ballot(keep);
            if (keep) {
                const size_t row = row0 + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b), 0u));
#pragma unroll
                for (int a = 0; a < 6; ++a) g.dst_slab[a * g.n_pad + row] = g.slab[a * g.n_pad + slot];
                g.dst_id[row] = g.id[slot];
            } else if (leaves) {
                double v[3];
                pair_load(g.slab, g.n_pad, static_cast<uint32_t>(slot), v);
                acc.count[0] += 1;
                fesburn::gain(v, &acc.sum[0], acc.out, 0);
            }
            row0 += __popcll(b);
        }
    }
    tally_commit(acc, g.words);
}

// total[0 .. kWords) += last[0 .. kWords): the counts as they are, the sums with their carries, the bits ORed.  One thread
__global__ void burn_add_kernel(const unsigned long long* __restrict__ last, unsigned long long* __restrict__ total)
{
    for (int k = 0; k < fesburn::kWords; ++k) {
        const int kind = fesburn::word_kind(k);
        if (kind == fesburn::kCount) total[k] += last[k];
        else if (kind == fesburn::kBits) total[k] |= last[k];
        else if (kind == fesburn::kSumLo) {
            const Fix s = ((static_cast<Fix>(total[k + 1]) << 64) | total[k]) + ((static_cast<Fix>(last[k + 1]) << 64) | last[k]);
            total[k] = static_cast<unsigned long long>(s);
            total[k + 1] = static_cast<unsigned long long>(s >> 64);
        }
    }
}

} // namespace fes
