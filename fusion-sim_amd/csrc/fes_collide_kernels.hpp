// fes_collide_kernels.hpp — the passes of the Monte Carlo collision operator of a CART3D handle (fpic_collide; host side
// fes_collide.inc.hpp, the rule fes_collide_core.hpp).  Launch shape, group access, the two hand-outs of candidates and the
// tally are the shared forms of fes_pass.hpp.
//   collide_kernel<T, KIND, NULLC, COMPACT>  EXCHANGE and ELASTIC.  Per particle the pass reads only the id, runs Philox block
//       0 and makes the integer test w0 < K.  Only a candidate gathers x (a rank of a decomposition: a dead slot, x < 0, is
//       skipped and not counted) and its three velocities, and only a particle that collides is stored: every other particle
//       keeps its bits.  COMPACT = false hands the candidates out by take_pending (one turn at small P_max, four at P_max = 1);
//       COMPACT = true, for the middle range of P_max where most lanes of that loop idle while one lane of their wave works,
//       by take_queued.  What a particle gets does not depend on its place in the queue.
//   relax_kernel<T>                 RELAX: every live particle.  Streams the three velocity arrays (and x on a rank) with
//       load4, and rewrites them with store4_masked.
// The counts (candidates, collided, clipped) are a Tally<3, 0>.  No scratch; 8 KiB of LDS in the compacting pass.
#pragma once

#include "fes_collide_core.hpp"
#include "fes_hist_kernels.hpp"
#include "fes_pass.hpp"

namespace fes {

constexpr int kCollideThreads = 256;
static_assert(kCollideThreads == kPassThreads, "the shared forms reduce and queue for a workgroup of kPassThreads");
constexpr int kCollideBlocks = 2048;     // 8 workgroups of 4 waves per CU of the 256, as kLoadBlocks
// the queue serves the requests with kCollideCompactMin <= K <= kCollideCompactMax (P_max from 2^-8 to 2^-3): below, its
// barriers cost more than the idle lanes of the plain pass; above, most lanes of the plain pass are busy anyway
constexpr unsigned long long kCollideCompactMin = 1ull << 24, kCollideCompactMax = 1ull << 29;
inline bool collide_compacts(unsigned long long K) { return K >= kCollideCompactMin && K <= kCollideCompactMax; }

template <typename T>
struct CollideArgs : PassArgs<T> {
    unsigned long long* counts;   // candidates, collided, clipped
    fescoll::Rule r;
};

// the pair and fusion passes keep their counts as a plain array: the same Tally without sums (a lane per count, as ever)
template <int NC>
__device__ __forceinline__ void collide_counts(const unsigned long long (&mine)[NC], unsigned long long* counts)
{
    Tally<NC, 0> a;
#pragma unroll
    for (int c = 0; c < NC; ++c) a.count[c] = mine[c];
    tally_commit(a, counts);
}

// one candidate
template <typename T, int KIND, bool NULLC>
__device__ __forceinline__ void collide_one(const CollideArgs<T>& g, uint32_t i, size_t slot, Tally<3, 0>& acc)
{
    if (g.dead && g.slab[slot] < static_cast<T>(0)) return;
    T* vel = g.slab + 3 * g.n_pad + slot;
    double u[3] = { static_cast<double>(vel[0]), static_cast<double>(vel[g.n_pad]), static_cast<double>(vel[2 * g.n_pad]) };
    const int what = fescoll::scatter<KIND, NULLC>(g.r, i, u);
    acc.count[0] += 1;
    acc.count[1] += what & fescoll::kCollided ? 1 : 0;
    acc.count[2] += what & fescoll::kClipped ? 1 : 0;
    if (what & fescoll::kCollided) {
        vel[0] = static_cast<T>(u[0]);
        vel[g.n_pad] = static_cast<T>(u[1]);
        vel[2 * g.n_pad] = static_cast<T>(u[2]);
    }
}

template <typename T, int KIND, bool NULLC, bool COMPACT>
__global__ __launch_bounds__(kCollideThreads) void collide_kernel(CollideArgs<T> g)
{
    const size_t g1 = (g.s1 + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kCollideThreads;
    Tally<3, 0> acc;
    auto one = [&](uint32_t i, size_t slot) { collide_one<T, KIND, NULLC>(g, i, slot, acc); };
    uint32_t idx[4] = { 0, 0, 0, 0 };
    if constexpr (COMPACT) {   // (the queue's barriers: the same turns for every lane of the workgroup)
        for (size_t vb = static_cast<size_t>(blockIdx.x) * kCollideThreads; vb < g1; vb += stride) {
            const size_t v = vb + threadIdx.x, base = 4 * v;
            if (v < g1) ids4(g.id, base, idx);
            take_queued([&](int l) { return v < g1 && base + l < g.s1 && fescoll::candidate(g.r, idx[l]); }, idx, vb, one);
        }
    } else {
        for (size_t v = static_cast<size_t>(blockIdx.x) * kCollideThreads + threadIdx.x; v < g1; v += stride) {
            const size_t base = 4 * v;                    // (base + 3 < n_pad: s1 <= n_pad, a multiple of 4)
            ids4(g.id, base, idx);
            uint32_t pend = 0;
#pragma unroll
            for (int l = 0; l < 4; ++l) pend |= (base + l < g.s1 && fescoll::candidate(g.r, idx[l])) ? 1u << l : 0u;
            take_pending(pend, idx, base, one);
        }
    }
    tally_commit(acc, g.counts);
}

template <typename T>
__global__ __launch_bounds__(kCollideThreads) void relax_kernel(CollideArgs<T> g)
{
    const size_t g1 = (g.s1 + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kCollideThreads;
    Tally<1, 0> acc;
    for (size_t v = static_cast<size_t>(blockIdx.x) * kCollideThreads + threadIdx.x; v < g1; v += stride) {
        const size_t base = 4 * v;
        uint32_t idx[4];
        ids4(g.id, base, idx);
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
        acc.count[0] += __popc(in);
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (in >> l & 1u) {
                double u[3] = { static_cast<double>(st[0][l]), static_cast<double>(st[1][l]), static_cast<double>(st[2][l]) };
                fescoll::relax(g.r, idx[l], u);
#pragma unroll
                for (int a = 0; a < 3; ++a) st[a][l] = static_cast<T>(u[a]);
            }
        store4_masked<3>(g.slab + 3 * g.n_pad + base, g.n_pad, in, st);
    }
    tally_commit(acc, g.counts + 1);
}

} // namespace fes
