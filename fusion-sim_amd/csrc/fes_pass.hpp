// fes_pass.hpp — the forms the particle passes of a CART3D handle share (collide, force, gas, inject, load).  Every such pass
// has one launch shape: kPassThreads lanes per workgroup, a fixed grid, and a grid-stride loop over groups of FOUR slots.
//   PassArgs      the head of a pass's arguments (the host fills it with pass_head, fes_ops.inc.hpp).
//   ids4, load4, store4, store4_masked   a group's access to its arrays: 16 bytes per load or store (twice 16 in double), or
//       scalar stores of the slots in a mask, so that a particle outside the mask keeps every bit.
//   take_pending, take_queued   the two hand-outs of a group's candidates to a per-candidate function.
//   Tally, tally_commit   counts and exact 128-bit fixed-point sums (Fix, fes_diag_kernels.hpp) kept per lane and added to a
//       request's device words with one set of 64-bit atomics per workgroup.
// No scratch, no float atomics: the same state gives the same bits.
#pragma once

#include <type_traits>

#include "fes_diag_kernels.hpp"

namespace fes {

constexpr int kPassThreads = 256;

template <typename T>
struct PassArgs {
    T* slab;                  // x, y, z, vx, vy, vz: six arrays of n_pad
    const uint32_t* id;       // n_pad words; nullptr: slot = id
    size_t n_pad;             // a multiple of 1024: a group of four slots stays inside the arrays
    size_t s1;                // the slots [0, s1) the pass visits
    int dead;                 // a rank of a decomposition: x < 0 marks a dead slot
};

using fpic::load4;

// the ids of the four slots from `base` on: one 16-byte load, or the slot numbers
__device__ __forceinline__ void ids4(const uint32_t* id, size_t base, uint32_t (&idx)[4])
{
    if (id) {
        const uint4 q = *reinterpret_cast<const uint4*>(id + base);
        idx[0] = q.x; idx[1] = q.y; idx[2] = q.z; idx[3] = q.w;
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l) idx[l] = static_cast<uint32_t>(base + l);
    }
}

// four values of one array (float, double or ids), p 16-byte aligned: one 16-byte store, or two
template <typename T>
__device__ __forceinline__ void store4(T* p, const T (&v)[4])
{
    if constexpr (sizeof(T) == 4) {
        using V = std::conditional_t<std::is_same_v<T, float>, float4, uint4>;
        *reinterpret_cast<V*>(p) = V(v[0], v[1], v[2], v[3]);
    } else {
        *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
        *reinterpret_cast<double2*>(p + 2) = make_double2(v[2], v[3]);
    }
}

// a group's values v[a][l] of NA arrays that lie `stride` apart, p the group's place in the first: store4 per array where
// all four slots are in the mask, else scalar stores of the slots in it only (one branch for the NA arrays)
template <int NA, typename T>
__device__ __forceinline__ void store4_masked(T* p, size_t stride, uint32_t in, const T (*v)[4])
{
    if (in == 0xFu) {
#pragma unroll
        for (int a = 0; a < NA; ++a) store4(p + a * stride, v[a]);
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (in >> l & 1u) {
#pragma unroll
                for (int a = 0; a < NA; ++a) p[a * stride + l] = v[a][l];
            }
    }
}

// The candidates `pend` (a bit per slot) of the group at `base`, ids idx, to one(id, slot).
// take_pending: one per turn of a loop the wave shares (the wave makes as many turns as its busiest lane has candidates).
template <typename F>
__device__ __forceinline__ void take_pending(uint32_t pend, const uint32_t (&idx)[4], size_t base, F&& one)
{
    while (pend) {
        const int l = __ffs(pend) - 1;
        pend &= pend - 1;
        one(l == 0 ? idx[0] : l == 1 ? idx[1] : l == 2 ? idx[2] : idx[3], base + l);
    }
}

// take_queued: the candidates of a workgroup's turn (the 1024 slots from 4 vb on; lane t holds the group at 4 (vb + t)) go
// into a queue in LDS (id and slot; LDS atomics give the places) and are then taken densely, one per lane, by as few waves
// as they fill.  cand(l): is slot l of the lane's group a candidate — asked once per slot, in order, between the queue's
// first two barriers, so a pass may make its test there (collide_kernel) or hand over bits it has (gas_kernel).  EVERY lane
// of the workgroup calls it, each turn.  8 KiB of LDS.  Like take_pending it calls one() at most FOUR times per lane and turn
// (4 kPassThreads entries over kPassThreads lanes): the ioniser's deciding pass keeps a lane's events of a turn in that many
// registers (fes_ionize_kernels.hpp, kIonizeKept).
template <typename C, typename F>
__device__ __forceinline__ void take_queued(C&& cand, const uint32_t (&idx)[4], size_t vb, F&& one)
{
    __shared__ uint32_t q_id[4 * kPassThreads], q_rel[4 * kPassThreads];
    __shared__ uint32_t q_n;
    if (threadIdx.x == 0) q_n = 0;
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 4; ++l)
        if (cand(l)) {
            const uint32_t at = atomicAdd(&q_n, 1u);         // (at most 1024 per turn: the queue's size)
            q_id[at] = idx[l];
            q_rel[at] = 4u * threadIdx.x + l;
        }
    __syncthreads();
    const uint32_t total = q_n;
    for (uint32_t k = threadIdx.x; k < total; k += kPassThreads) one(q_id[k], 4 * vb + q_rel[k]);
    __syncthreads();   // (the queue is rewritten by the next turn)
}

// A lane's tallies: NC counts, NS fixed-point sums and — with sums — the bits `out` of the sums that met a term outside the
// fixed-point range.  The device words: the counts | the sums (lo, hi) | out.
template <int NC, int NS>
struct Tally {
    static constexpr int kWords = NC + 2 * NS + (NS ? 1 : 0);
    unsigned long long count[NC] = {};
    unsigned long long out = 0;
    Fix sum[NS ? NS : 1] = {};
};

// the lanes' tallies -> the words: every lane of the workgroup calls it once, after its loop.  Reduced over the wave by
// shuffles and over the workgroup through LDS, then added by one lane (counts alone: by a lane per count), nothing where
// nothing is to add: a 128-bit sum as its low word, then its high word plus the carry the low word's add shows.
template <int NC, int NS>
__device__ __forceinline__ void tally_commit(Tally<NC, NS>& a, unsigned long long* words)
{
    constexpr int W = Tally<NC, NS>::kWords, kWaves = kPassThreads / 64;
    __shared__ unsigned long long part[kWaves][W];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < NC; ++c) a.count[c] += __shfl_xor(a.count[c], off, 64);
#pragma unroll
        for (int c = 0; c < NS; ++c) a.sum[c] += shfl_xor_fix(a.sum[c], off);
        if constexpr (NS > 0) a.out |= __shfl_xor(a.out, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* p = part[threadIdx.x >> 6];
#pragma unroll
        for (int c = 0; c < NC; ++c) p[c] = a.count[c];
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            p[NC + 2 * c] = static_cast<unsigned long long>(a.sum[c]);
            p[NC + 2 * c + 1] = static_cast<unsigned long long>(a.sum[c] >> 64);
        }
        if constexpr (NS > 0) p[W - 1] = a.out;
    }
    __syncthreads();
    auto add_count = [&](int c) {
        unsigned long long s = 0;
        for (int w = 0; w < kWaves; ++w) s += part[w][c];
        if (s) atomicAdd(words + c, s);
    };
    if constexpr (NS == 0) {   // counts alone: a lane each, their atomics side by side
        if (threadIdx.x < NC) add_count(threadIdx.x);
    } else if (threadIdx.x == 0) {
        for (int c = 0; c < NC; ++c) add_count(c);
        for (int c = 0; c < NS; ++c) {
            const int at = NC + 2 * c;
            Fix s = 0;
            for (int w = 0; w < kWaves; ++w) s += (static_cast<Fix>(part[w][at + 1]) << 64) | part[w][at];
            const unsigned long long lo = static_cast<unsigned long long>(s), hi = static_cast<unsigned long long>(s >> 64);
            unsigned long long carry = 0;
            if (lo) {
                const unsigned long long old = atomicAdd(words + at, lo);
                carry = old + lo < old ? 1ull : 0ull;
            }
            if (hi + carry) atomicAdd(words + at + 1, hi + carry);
        }
        unsigned long long out = 0;
        for (int w = 0; w < kWaves; ++w) out |= part[w][W - 1];
        if (out) atomicOr(words + W - 1, out);
    }
}

} // namespace fes
