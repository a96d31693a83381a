// fes_collide_kernels.hpp — the passes of the Monte Carlo collision operator of a CART3D handle (fpic_collide; host side
// fes_collide.inc.hpp, the rule fes_collide_core.hpp).  All have the launch shape of the loader and the selection (fixed
// grid, grid-stride) over groups of FOUR slots; a lane takes the four ids from id[slot] (one 16-byte load) or, while the
// species is in the caller's order, the slot numbers.
//   collide_kernel<T, KIND, NULLC>  EXCHANGE and ELASTIC.  Per particle the pass reads only the id, runs Philox block 0 and
//       makes the integer test w0 < K; the candidates of a lane are then taken one per turn of a loop the wave shares (the
//       wave makes as many turns as its busiest lane has candidates: one at small P_max, four at P_max = 1).  Only a
//       candidate gathers x (a rank of a decomposition: a dead slot, x < 0, is skipped and not counted) and its three
//       velocities, and only a particle that collides is stored: every other particle keeps its bits.
//   collide_compact_kernel<T, KIND, NULLC>  the same rule for the middle range of P_max, where most lanes of the plain pass
//       idle while one lane of their wave works: the candidates of a workgroup's turn (its 1024 slots) go into a queue in LDS
//       (id and slot; LDS atomics give the places) and are then taken densely, one per lane, by as few waves as they fill.
//       What a particle gets does not depend on its place in the queue.
//   relax_kernel<T>                 RELAX: every live particle.  Streams the three velocity arrays (and x on a rank) with
//       16-byte loads, and rewrites them with 16-byte stores where all four slots of a group are updated; a group at the
//       edge of the range or with a dead slot takes scalar stores of the updated slots only.
// The counts (candidates, collided, clipped) are kept per lane, reduced over the wave and the workgroup, and added to the
// three device words with one 64-bit atomic per workgroup and count.  No scratch; 8 KiB of LDS in the compacting pass.
#pragma once

#include "fes_collide_core.hpp"
#include "fes_hist_kernels.hpp"

namespace fes {

constexpr int kCollideThreads = 256;
constexpr int kCollideBlocks = 2048;     // 8 workgroups of 4 waves per CU of the 256, as kLoadBlocks
// collide_compact_kernel serves the requests with kCollideCompactMin <= K <= kCollideCompactMax (P_max from 2^-8 to 2^-3): below,
// its barriers cost more than the idle lanes of the plain pass; above, most lanes of the plain pass are busy anyway
constexpr unsigned long long kCollideCompactMin = 1ull << 24, kCollideCompactMax = 1ull << 29;
inline bool collide_compacts(unsigned long long K) { return K >= kCollideCompactMin && K <= kCollideCompactMax; }

template <typename T>
struct CollideArgs {
    T* slab;                  // x, y, z, vx, vy, vz: six arrays of n_pad
    const uint32_t* id;       // n_pad words; nullptr: slot = id
    size_t n_pad;             // a multiple of 1024: a group of four slots stays inside the arrays
    size_t s1;                // the slots [0, s1) the pass visits
    int dead;                 // a rank of a decomposition: x < 0 marks a dead slot
    unsigned long long* counts;   // candidates, collided, clipped
    fescoll::Rule r;
};

// the lanes' counts -> counts[0 .. NC): every lane of the workgroup calls it once, after its loop
template <int NC>
__device__ __forceinline__ void collide_counts(unsigned long long (&mine)[NC], unsigned long long* counts)
{
    __shared__ unsigned long long part[kCollideThreads / 64][NC];
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine[c] += __shfl_xor(mine[c], off, 64);
        if (lane == 0) part[threadIdx.x >> 6][c] = mine[c];
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        unsigned long long s = 0;
        for (int w = 0; w < kCollideThreads / 64; ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(counts + threadIdx.x, s);
    }
}

__device__ __forceinline__ void collide_ids(const uint32_t* id, size_t base, uint32_t (&idx)[4])
{
    if (id) {
        const uint4 q = *reinterpret_cast<const uint4*>(id + base);
        idx[0] = q.x; idx[1] = q.y; idx[2] = q.z; idx[3] = q.w;
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l) idx[l] = static_cast<uint32_t>(base + l);
    }
}

template <typename T, int KIND, bool NULLC>
__global__ __launch_bounds__(kCollideThreads) void collide_kernel(CollideArgs<T> g)
{
    const size_t g1 = (g.s1 + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kCollideThreads;
    unsigned long long count[3] = { 0, 0, 0 };
    for (size_t v = static_cast<size_t>(blockIdx.x) * kCollideThreads + threadIdx.x; v < g1; v += stride) {
        const size_t base = 4 * v;                        // (base + 3 < n_pad: s1 <= n_pad, a multiple of 4)
        uint32_t idx[4];
        collide_ids(g.id, base, idx);
        uint32_t pend = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l) pend |= (base + l < g.s1 && fescoll::candidate(g.r, idx[l])) ? 1u << l : 0u;
        while (pend) {
            const int l = __ffs(pend) - 1;
            pend &= pend - 1;
            const uint32_t i = l == 0 ? idx[0] : l == 1 ? idx[1] : l == 2 ? idx[2] : idx[3];
            const size_t slot = base + l;
            if (g.dead && g.slab[slot] < static_cast<T>(0)) continue;
            T* vel = g.slab + 3 * g.n_pad + slot;
            double u[3] = { static_cast<double>(vel[0]), static_cast<double>(vel[g.n_pad]), static_cast<double>(vel[2 * g.n_pad]) };
            const int what = fescoll::scatter<KIND, NULLC>(g.r, i, u);
            count[0] += 1;
            count[1] += what & fescoll::kCollided ? 1 : 0;
            count[2] += what & fescoll::kClipped ? 1 : 0;
            if (what & fescoll::kCollided) {
                vel[0] = static_cast<T>(u[0]);
                vel[g.n_pad] = static_cast<T>(u[1]);
                vel[2 * g.n_pad] = static_cast<T>(u[2]);
            }
        }
    }
    collide_counts<3>(count, g.counts);
}

// the same pass with the candidates of a workgroup's turn (its 1024 slots) compacted into LDS and taken densely, one per lane
template <typename T, int KIND, bool NULLC>
__global__ __launch_bounds__(kCollideThreads) void collide_compact_kernel(CollideArgs<T> g)
{
    __shared__ uint32_t q_id[4 * kCollideThreads], q_rel[4 * kCollideThreads];
    __shared__ uint32_t q_n;
    const size_t g1 = (g.s1 + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kCollideThreads;
    unsigned long long count[3] = { 0, 0, 0 };
    for (size_t vb = static_cast<size_t>(blockIdx.x) * kCollideThreads; vb < g1; vb += stride) {   // (the same turns for every lane)
        if (threadIdx.x == 0) q_n = 0;
        __syncthreads();
        const size_t v = vb + threadIdx.x;
        if (v < g1) {
            const size_t base = 4 * v;
            uint32_t idx[4];
            collide_ids(g.id, base, idx);
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (base + l < g.s1 && fescoll::candidate(g.r, idx[l])) {
                    const uint32_t at = atomicAdd(&q_n, 1u);             // (at most 1024 per turn: the queue's size)
                    q_id[at] = idx[l];
                    q_rel[at] = 4u * threadIdx.x + l;
                }
        }
        __syncthreads();
        const uint32_t total = q_n;
        for (uint32_t k = threadIdx.x; k < total; k += kCollideThreads) {
            const uint32_t i = q_id[k];
            const size_t slot = 4 * vb + q_rel[k];
            if (g.dead && g.slab[slot] < static_cast<T>(0)) continue;
            T* vel = g.slab + 3 * g.n_pad + slot;
            double u[3] = { static_cast<double>(vel[0]), static_cast<double>(vel[g.n_pad]), static_cast<double>(vel[2 * g.n_pad]) };
            const int what = fescoll::scatter<KIND, NULLC>(g.r, i, u);
            count[0] += 1;
            count[1] += what & fescoll::kCollided ? 1 : 0;
            count[2] += what & fescoll::kClipped ? 1 : 0;
            if (what & fescoll::kCollided) {
                vel[0] = static_cast<T>(u[0]);
                vel[g.n_pad] = static_cast<T>(u[1]);
                vel[2 * g.n_pad] = static_cast<T>(u[2]);
            }
        }
        __syncthreads();   // (the queue is rewritten by the next turn)
    }
    collide_counts<3>(count, g.counts);
}

template <typename T>
__global__ __launch_bounds__(kCollideThreads) void relax_kernel(CollideArgs<T> g)
{
    const size_t g1 = (g.s1 + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kCollideThreads;
    unsigned long long count[1] = { 0 };
    auto load4 = [](const T* src, T (&out)[4]) {
        if constexpr (sizeof(T) == 4) {
            const float4 q = *reinterpret_cast<const float4*>(src);
            out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
        } else {
            const double2 a = *reinterpret_cast<const double2*>(src), b = *reinterpret_cast<const double2*>(src + 2);
            out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y;
        }
    };
    for (size_t v = static_cast<size_t>(blockIdx.x) * kCollideThreads + threadIdx.x; v < g1; v += stride) {
        const size_t base = 4 * v;
        uint32_t idx[4];
        collide_ids(g.id, base, idx);
        T st[3][4];
#pragma unroll
        for (int a = 0; a < 3; ++a) load4(g.slab + (3 + a) * g.n_pad + base, st[a]);
        uint32_t in = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l) in |= base + l < g.s1 ? 1u << l : 0u;
        if (g.dead) {
            T x[4];
            load4(g.slab + base, x);
#pragma unroll
            for (int l = 0; l < 4; ++l) in &= x[l] < static_cast<T>(0) ? ~(1u << l) : ~0u;
        }
        if (!in) continue;
        count[0] += __popc(in);
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (in >> l & 1u) {
                double u[3] = { static_cast<double>(st[0][l]), static_cast<double>(st[1][l]), static_cast<double>(st[2][l]) };
                fescoll::relax(g.r, idx[l], u);
#pragma unroll
                for (int a = 0; a < 3; ++a) st[a][l] = static_cast<T>(u[a]);
            }
        if (in == 0xFu) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                T* dst = g.slab + (3 + a) * g.n_pad + base;
                if constexpr (sizeof(T) == 4) {
                    *reinterpret_cast<float4*>(dst) = make_float4(st[a][0], st[a][1], st[a][2], st[a][3]);
                } else {
                    *reinterpret_cast<double2*>(dst) = make_double2(st[a][0], st[a][1]);
                    *reinterpret_cast<double2*>(dst + 2) = make_double2(st[a][2], st[a][3]);
                }
            }
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (in >> l & 1u) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) g.slab[(3 + a) * g.n_pad + base + l] = st[a][l];
                }
        }
    }
    collide_counts<1>(count, g.counts + 1);
}

} // namespace fes
