// fes_ionize_kernels.hpp — the passes of the electron-impact ionisation of a CART3D handle (fpic_ionize; host side
// fes_ionize.inc.hpp, the rule fes_ionize_core.hpp).  Launch shape, group access, the two hand-outs of candidates and the
// tally are the shared forms of fes_pass.hpp.
//   ionize_decide_kernel<T, WINDOW_FIRST, COMPACT>   the deciding pass over the projectile species, in gas_kernel's shape
//       (kGasBlocks x kGasThreads, groups of four slots, the same two orders of the candidate test and the same two hand-outs,
//       chosen by the same host rule).  It counts candidates, below and above, and for every EVENT it records (slot, id) in
//       the event list and sets the id's bit in a bitmap over the projectile's id span (integer atomicOr).  It writes NO
//       particle state: the host may still refuse the application.  Rows of the list: a lane keeps the events of its turn
//       (at most four: its group's slots, or its four places of the 1024-entry queue) in registers; after the hand-out the
//       waves put them into a stage of 2048 rows in the workgroup's LDS (ballots, one LDS atomic per wave), and the
//       workgroup empties the stage into the list when it holds more than a turn can add: ONE 64-bit atomic on the cursor
//       per emptying, not one per event nor per wave and turn.  The cursor is the event count the host reads.
//   (renumber_count_kernel, load_scan_kernel: the popcount scan of the bitmap, as fpic_renumber's)
//   ionize_generate_kernel<T>   over the M events, one per lane: the event's rank = the marked ids below its primary's
//       (offset[chunk] + below[word] + the bits of its word under its own).  It recomputes the partner and the relative
//       speed from the words and the stored state (the same operations on the same values: the same bits; the acceptance is
//       not repeated), forms the outcome, stores the primary's velocity, and writes the electron's and the ion's six state
//       words and id at slot n + rank of their species.  With electron == species the new rows lie at n + rank >= n, the
//       primaries below n: no lane reads what another writes.  The three groups of exact sums are a Tally<1, 12>.
//   ionize_add_kernel           one thread: the row of this application added to the ioniser's totals (128-bit adds).
// No float atomics, no inline assembly, no scratch.
#pragma once

#include "fes_gas_kernels.hpp"
#include "fes_ionize_core.hpp"
#include "fes_remove_kernels.hpp"

namespace fes {

constexpr int kIonizeThreads = 256;       // the generation pass; the deciding pass has gas_kernel's shape
constexpr int kIonizeBlocks = 2048;
static_assert(kIonizeThreads == kPassThreads, "tally_commit reduces a workgroup of kPassThreads");

struct IonizeEvent {
    uint32_t slot, id;
};

template <typename T>
struct IonizeDecideArgs : PassArgs<T> {
    unsigned long long* words;    // fesion::kCounts of them are added here
    unsigned long long* cursor;   // the rows taken of `events`: the event count
    IonizeEvent* events;          // room for s1 rows
    uint32_t* bitmap;             // a bit per id below the projectile's id span, zeroed
    fesion::Rule r;
};

using IonizeCounts = Tally<fesion::kCounts, 0>;    // candidates, below, above
using IonizeSums = Tally<1, fesion::kSums>;        // ionised | primary, electron, ion: energy, momentum x, y, z
static_assert(fesion::kCounts + IonizeSums::kWords == fesion::kWords, "the two tallies' words are the request's");

// a lane's events of one turn: scalars, placed by comparison, so that they stay in registers.  FOUR places, because either
// hand-out of fes_pass.hpp calls a lane at most four times per turn: take_pending serves the four slots of the lane's own
// group, take_queued the 4 kPassThreads entries of its queue over kPassThreads lanes.  A hand-out that gave a lane more
// would lose the fifth event's row (its bitmap bit is already set): the asserts below hold the two numbers together
constexpr int kIonizeKept = 4;
static_assert(kIonizeKept == 4 * kPassThreads / kGasThreads, "a lane takes at most (queue entries / lanes) candidates per turn of take_queued");
static_assert(kIonizeKept == 4, "take_pending hands a lane the slots of its group of four; IonizeKept has that many places");
struct IonizeKept {
    uint32_t n = 0;
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, i0 = 0, i1 = 0, i2 = 0, i3 = 0;
    __device__ __forceinline__ void keep(uint32_t slot, uint32_t id)
    {
        s0 = n == 0 ? slot : s0; i0 = n == 0 ? id : i0;
        s1 = n == 1 ? slot : s1; i1 = n == 1 ? id : i1;
        s2 = n == 2 ? slot : s2; i2 = n == 2 ? id : i2;
        s3 = n == 3 ? slot : s3; i3 = n == 3 ? id : i3;
        n += 1;
    }
    __device__ __forceinline__ uint32_t slot(uint32_t j) const { return j == 0 ? s0 : j == 1 ? s1 : j == 2 ? s2 : s3; }
    __device__ __forceinline__ uint32_t id(uint32_t j) const { return j == 0 ? i0 : j == 1 ? i1 : j == 2 ? i2 : i3; }
};

// One particle whose word has passed.  CHECK: the window is still to be tested (the word came first).
template <typename T, bool CHECK>
__device__ __forceinline__ void ionize_one(const IonizeDecideArgs<T>& g, const double* S, const double* const (&tab)[3], uint32_t i, size_t slot, IonizeCounts& acc, IonizeKept& kept)
{
    const fesion::Rule& r = g.r;
    const bool need_p = !r.g.win.whole || r.g.win.tapered;
    double p[3] = { 0, 0, 0 };
    if (need_p) {
        p[0] = static_cast<double>(g.slab[slot]);
        p[1] = static_cast<double>(g.slab[g.n_pad + slot]);
        p[2] = static_cast<double>(g.slab[2 * g.n_pad + slot]);
        if (CHECK && !r.g.win.whole && !fesforce::inside(r.g.win, p)) return;
    }
    const T* vel = g.slab + 3 * g.n_pad + slot;
    const double u[3] = { static_cast<double>(vel[0]), static_cast<double>(vel[g.n_pad]), static_cast<double>(vel[2 * g.n_pad]) };
    double vb[3], rel;
    const int what = fesion::decide(r, S, tab, i, p, u, vb, &rel);
    acc.count[0] += 1;
    acc.count[1] += what & fesion::kBelow ? 1 : 0;
    acc.count[2] += what & fesion::kAbove ? 1 : 0;
    if (what & fesion::kEvent) {
        atomicOr(g.bitmap + (i >> 5), 1u << (i & 31u));
        kept.keep(static_cast<uint32_t>(slot), i);   // (at most four per lane and turn)
    }
}

// The workgroup's staging of event rows in LDS: a turn adds at most 4 kGasThreads rows (kIonizeKept per lane), and the stage is
// emptied into the list once it holds more than that, so 8 kGasThreads places serve.  16 KiB.
constexpr uint32_t kIonizeTurnMost = kIonizeKept * kGasThreads, kIonizeStage = 2 * kIonizeTurnMost;
struct IonizeStage {
    IonizeEvent row[kIonizeStage];
    uint32_t n;                   // rows staged
    uint32_t flush;               // this turn's decision, written by one lane between two barriers
    unsigned long long base;      // the rows taken of the list
};

// The lanes' kept events of this turn -> the workgroup's stage, and the stage -> rows of the list when it has filled past one
// turn's most (last: whatever it holds).  EVERY lane of the workgroup calls it, once per turn and once after the loop.  A
// wave counts its events with ballots and takes its places in the stage with ONE LDS atomic; the list's cursor sees one
// 64-bit atomic per emptying — per some thousand events — instead of one per wave and turn: at 6e6 events among 5e8
// projectiles that cursor word took 1.9e6 atomics and the pass 1.86 x gas_kernel's time.
template <typename T>
__device__ __forceinline__ void ionize_stage(const IonizeDecideArgs<T>& g, IonizeStage& st, IonizeKept& kept, bool last)
{
    if (__any(kept.n != 0)) {            // (wave-uniform)
        unsigned long long held[kIonizeKept];
        uint32_t total = 0;
#pragma unroll
        for (uint32_t j = 0; j < kIonizeKept; ++j) {
            held[j] = __ballot(kept.n > j);
            total += __popcll(held[j]);
        }
        uint32_t at = 0;
        if ((threadIdx.x & 63) == 0) at = atomicAdd(&st.n, total);     // (st.n <= kIonizeTurnMost before the turn: at + total <= kIonizeStage)
        at = __shfl(at, 0, 64);
#pragma unroll
        for (uint32_t j = 0; j < kIonizeKept; ++j) {
            const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(held[j] >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(held[j]), 0u));
            if (kept.n > j) st.row[at + below] = IonizeEvent{ kept.slot(j), kept.id(j) };
            at += __popcll(held[j]);
        }
        kept.n = 0;
    }
    __syncthreads();                     // (every wave's rows and its add to st.n are in)
    if (threadIdx.x == 0) {
        st.flush = (st.n > kIonizeTurnMost || (last && st.n != 0)) ? 1u : 0u;
        if (st.flush) st.base = atomicAdd(g.cursor, static_cast<unsigned long long>(st.n));   // (rows below the cursor, which never passes the live slots s1)
    }
    __syncthreads();
    if (st.flush) {                      // (workgroup-uniform)
        const uint32_t n = st.n;
        for (uint32_t k = threadIdx.x; k < n; k += kGasThreads) g.events[st.base + k] = st.row[k];
        __syncthreads();
        if (threadIdx.x == 0) st.n = 0;
        __syncthreads();                 // (the next turn adds to an empty stage)
    }
}

template <typename T, bool WINDOW_FIRST, bool COMPACT>
__global__ __launch_bounds__(kGasThreads) void ionize_decide_kernel(IonizeDecideArgs<T> g)
{
    const fesion::Rule& r = g.r;
    const double* const S = r.g.sigma;
    const double* const tabs[3] = { r.g.win.tab[0], r.g.win.tab[1], r.g.win.tab[2] };
    const size_t g1 = (g.s1 + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kGasThreads;
    IonizeCounts acc;
    IonizeKept kept;
    __shared__ IonizeStage stage;
    if (threadIdx.x == 0) { stage.n = 0; stage.flush = 0; }
    __syncthreads();
    auto one = [&](uint32_t i, size_t slot) { ionize_one<T, !WINDOW_FIRST>(g, S, tabs, i, slot, acc, kept); };
    for (size_t vb = static_cast<size_t>(blockIdx.x) * kGasThreads; vb < g1; vb += stride) {   // (the same turns for every lane)
        const size_t v = vb + threadIdx.x;
        const size_t base = 4 * v;                        // (v < g1: base + 3 < n_pad, as s1 <= n_pad, a multiple of 4)
        uint32_t idx[4] = { 0, 0, 0, 0 }, pend = 0;
        if (v < g1) {
            uint32_t in = 0;
#pragma unroll
            for (int l = 0; l < 4; ++l) in |= base + l < g.s1 ? 1u << l : 0u;
            if constexpr (WINDOW_FIRST) {
                T pos[3][4];
#pragma unroll
                for (int a = 0; a < 3; ++a) load4(g.slab + a * g.n_pad + base, pos[a]);
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const double p[3] = { static_cast<double>(pos[0][l]), static_cast<double>(pos[1][l]), static_cast<double>(pos[2][l]) };
                    in &= fesforce::inside(r.g.win, p) ? ~0u : ~(1u << l);
                }
            }
            if (in) {
                ids4(g.id, base, idx);
#pragma unroll
                for (int l = 0; l < 4; ++l) pend |= ((in >> l & 1u) && fesion::drawn(r, idx[l])) ? 1u << l : 0u;
            }
        }
        if constexpr (COMPACT) take_queued([&](int l) { return (pend >> l & 1u) != 0; }, idx, vb, one);
        else take_pending(pend, idx, base, one);
        ionize_stage(g, stage, kept, false);
    }
    ionize_stage(g, stage, kept, true);
    tally_commit(acc, g.words);
}

template <typename T>
struct IonizeGenerateArgs {
    T* slab;                      // the projectile species' live set: six arrays of n_pad
    size_t n_pad;
    const IonizeEvent* events;
    uint32_t m;                   // the events
    const uint32_t *bitmap, *below, *offset;   // the marked ids, per word those below it in its chunk, the chunks' exclusive offsets
    T* slab_e;                    // the electrons' live set, its stride, its ids; the first new slot and id
    size_t n_pad_e;
    uint32_t* id_e;
    size_t s0_e;
    uint32_t id0_e;
    T* slab_i;                    // the ions'
    size_t n_pad_i;
    uint32_t* id_i;
    size_t s0_i;
    uint32_t id0_i;
    unsigned long long* words;    // IonizeSums::kWords of them are added here
    fesion::Rule r;
};

template <typename T>
__global__ __launch_bounds__(kIonizeThreads) void ionize_generate_kernel(IonizeGenerateArgs<T> g)
{
    const fesion::Rule& r = g.r;
    IonizeSums acc;
    const size_t stride = static_cast<size_t>(gridDim.x) * kIonizeThreads;
    for (size_t e = static_cast<size_t>(blockIdx.x) * kIonizeThreads + threadIdx.x; e < g.m; e += stride) {
        const IonizeEvent ev = g.events[e];
        const uint32_t i = ev.id, w = i >> 5;
        const uint32_t rank = g.offset[w / kRenumberChunk] + g.below[w] + __popc(g.bitmap[w] & ((1u << (i & 31u)) - 1u));
        const size_t slot = ev.slot;
        T* src = g.slab + slot;
        const T pos[3] = { src[0], src[g.n_pad], src[2 * g.n_pad] };
        const double u0[3] = { static_cast<double>(src[3 * g.n_pad]), static_cast<double>(src[4 * g.n_pad]), static_cast<double>(src[5 * g.n_pad]) };
        double vb[3], v1[3], vs[3];
        const double rel = fesion::partner(r, i, u0, vb);
        fesion::outcome(r, i, vb, rel, v1, vs);
        const size_t se = g.s0_e + rank, si = g.s0_i + rank;
        double w1[3], we[3], wi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const T t1 = static_cast<T>(v1[a]), te = static_cast<T>(vs[a]), ti = static_cast<T>(vb[a]);
            src[(3 + a) * g.n_pad] = t1;
            g.slab_e[a * g.n_pad_e + se] = pos[a];
            g.slab_e[(3 + a) * g.n_pad_e + se] = te;
            g.slab_i[a * g.n_pad_i + si] = pos[a];
            g.slab_i[(3 + a) * g.n_pad_i + si] = ti;
            w1[a] = static_cast<double>(t1);
            we[a] = static_cast<double>(te);
            wi[a] = static_cast<double>(ti);
        }
        g.id_e[se] = g.id0_e + rank;
        g.id_i[si] = g.id0_i + rank;
        acc.count[0] += 1;
        fesion::Fix(&primary)[4] = *reinterpret_cast<fesion::Fix(*)[4]>(&acc.sum[0]);
        fesion::tally(u0, w1, primary, acc.out);
        fesion::gain(we, &acc.sum[4], acc.out, 4);
        fesion::gain(wi, &acc.sum[8], acc.out, 8);
    }
    tally_commit(acc, g.words);
}

// total[0 .. kWords) += last[0 .. kWords): the counts as they are, the sums with their carries, the bits ORed.  One thread
__global__ void ionize_add_kernel(const unsigned long long* __restrict__ last, unsigned long long* __restrict__ total)
{
    for (int c = 0; c <= fesion::kCounts; ++c) total[c] += last[c];
    for (int k = 0; k < fesion::kSums; ++k) {
        const int at = fesion::kCounts + 1 + 2 * k;
        const Fix s = ((static_cast<Fix>(total[at + 1]) << 64) | total[at]) + ((static_cast<Fix>(last[at + 1]) << 64) | last[at]);
        total[at] = static_cast<unsigned long long>(s);
        total[at + 1] = static_cast<unsigned long long>(s >> 64);
    }
    total[fesion::kOutAt] |= last[fesion::kOutAt];
}

} // namespace fes
