// fes_mom_kernels.hpp — the fluid moment grids of one species of a CART3D handle (fpic_moments; host side fes_mom.inc.hpp,
// the rule fes_mom_core.hpp).  Two passes over the species' slots, both adding the same integers:
//   mom_tiles_kernel  a binned species, in the shape of em_rho_tiles_kernel: one work item of the species' own work list per
//                     workgroup; the tile's window (tile + 1 node per axis, no halo) of int64 accumulators in LDS, ONE WINDOW
//                     PER MOMENT OF THE SWEEP (the host sizes the dynamic LDS and splits a large mask into sweeps); eight
//                     ds_add_u64 per particle and moment; the non-zero accumulators flushed with 64-bit global atomics.  A
//                     particle whose cell has left the tile since the binning adds through global memory (`spilled`).
//   mom_flat_kernel   a range of slots of a species in any order (not binned yet; the arrivals of a migration in the tail):
//                     grid-stride, eight 64-bit global atomics per particle and moment.
// Both read x, y, z, vx, vy, vz of every slot — the velocities also for a request of N alone: a rejected particle adds to no
// moment, N included, whatever the mask.  `rejected` and `spilled` are counted per lane and added once per workgroup (per
// wave in the flat form) to two words behind the pass's own grids; the handle's spill counter, which the pushes read to
// decide when to re-bin, is not touched.  Integer adds commute: the same state gives the same bits.
#pragma once

#include "fes_kernels.hpp"
#include "fes_mom_core.hpp"

namespace fes {

constexpr int kMomThreads = 512;       // tiled form: 8 waves per workgroup (two workgroups of a three-moment 17x17x9 sweep share a CU: 16 waves)
constexpr int kMomFlatThreads = 256;
constexpr int kMomFlatBlocks = 4096;
constexpr size_t kMomLdsBudget = 64 * 1024;   // per workgroup: at least two workgroups on a CU's 160 KB

template <int LX, int LY, int LZ>
struct MomWin {
    static constexpr int TX = 1 << LX, TY = 1 << LY, TZ = 1 << LZ;
    static constexpr int WX = TX + 1, WY = TY + 1, WZ = TZ + 1;
    static constexpr int N = WX * WY * WZ;
    // moments of one sweep: what fits the budget beside the two counter words
    static constexpr int kSweep = static_cast<int>((kMomLdsBudget - 16) / (static_cast<size_t>(N) * 8)) < fesmom::kMoments
                                      ? static_cast<int>((kMomLdsBudget - 16) / (static_cast<size_t>(N) * 8)) : fesmom::kMoments;
    static_assert(kSweep >= 1, "one moment's window must fit");
};

template <typename T>
struct MomArgs {
    const T* slab;                 // x, y, z, vx, vy, vz, each `stride` elements
    size_t stride;
    size_t first, count;           // flat form: the slots [first, first + count)
    int nx, ny, nz;
    Held held;                     // the planes the grids hold
    int ntx, nty;
    const BlockWork* work;         // tiled form: the species' live work list
    const uint32_t* nwork;
    unsigned long long* grids;     // grid g: grid_words int64 accumulators, node i + nx (j + ny plane)
    size_t grid_words;
    unsigned long long* counters;  // rejected, spilled
    int nm;                        // moments of this sweep
    int bit[fesmom::kMoments];     // ... their bits
    int grid[fesmom::kMoments];    // ... and their grids in the buffer
    int counting;                  // the first sweep of a request counts rejected and spilled
};

// A stored position lies in [0, 1) and axis() gives a cell of the grid.  A slot whose position is no such number (nothing
// the library writes) is passed over like a dead one, so that no address is ever formed from it.
__device__ __forceinline__ bool mom_cell_ok(int i, int j, int k, int nx, int ny, int nz)
{
    return static_cast<unsigned>(i) < static_cast<unsigned>(nx) && static_cast<unsigned>(j) < static_cast<unsigned>(ny) && static_cast<unsigned>(k) < static_cast<unsigned>(nz);
}

// the eight terms of one particle for moment `bit`
__device__ __forceinline__ void mom_particle_terms(int bit, double vx, double vy, double vz, int wx1, int wy1, int wz1, int64_t (&t)[8])
{
    if (bit == 0) fesmom::n_terms(wx1, wy1, wz1, t);
    else fesmom::mom_terms(fesmom::fixed(fesmom::value(bit, vx, vy, vz)), wx1, wy1, wz1, t);
}

// a particle's terms of every moment of the sweep straight to the grids in global memory
template <typename T>
__device__ __forceinline__ void mom_global(const MomArgs<T>& a, int i, int j, int k, int wx1, int wy1, int wz1, double vx, double vy, double vz)
{
    size_t node[8];
    bool held[8];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int aa = 0; aa < 2; ++aa) {
                const int ii = (i + aa == a.nx) ? 0 : i + aa, jj = (j + b == a.ny) ? 0 : j + b, kk = held_plane((k + c == a.nz) ? 0 : k + c, a.held, a.nz);
                held[aa + 2 * b + 4 * c] = kk >= 0;
                node[aa + 2 * b + 4 * c] = static_cast<size_t>(ii) + static_cast<size_t>(a.nx) * (static_cast<size_t>(jj) + static_cast<size_t>(a.ny) * (kk >= 0 ? kk : 0));
            }
    for (int m = 0; m < a.nm; ++m) {
        int64_t t[8];
        mom_particle_terms(a.bit[m], vx, vy, vz, wx1, wy1, wz1, t);
        unsigned long long* g = a.grids + static_cast<size_t>(a.grid[m]) * a.grid_words;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (t[e] != 0 && held[e]) atomicAdd(g + node[e], static_cast<unsigned long long>(t[e]));
    }
}

template <typename T, int LX, int LY, int LZ>
__global__ __launch_bounds__(kMomThreads) void mom_tiles_kernel(MomArgs<T> a)
{
    using W = MomWin<LX, LY, LZ>;
    constexpr int PPT = Vec16<T>::N;
    constexpr int WX = W::WX, WY = W::WY, WN = W::N;
    extern __shared__ unsigned long long mom_lds[];   // nm windows of WN accumulators, then the two counters
    const BlockWork w = a.work[blockIdx.x];           // (the list has a slot for every workgroup of the launch)
    if (blockIdx.x >= *a.nwork) return;
    const int ti = static_cast<int>(w.tile % a.ntx), tj = static_cast<int>((w.tile / a.ntx) % a.nty), tk = static_cast<int>(w.tile / (a.ntx * a.nty));
    const int ox = ti * W::TX, oy = tj * W::TY, oz = tk * W::TZ;
    const int words = a.nm * WN;
    for (int s = threadIdx.x; s < words + 2; s += kMomThreads) mom_lds[s] = 0ull;
    __syncthreads();
    unsigned my_rejected = 0, my_spilled = 0;
    size_t g_begin, g_end;
    fesgrp::groups_exact(w.begin, w.end, PPT, g_begin, g_end);
    for (size_t g = g_begin + threadIdx.x; g < g_end; g += kMomThreads) {
        const size_t base = g * PPT;
        T p[6][PPT];
#pragma unroll
        for (int f = 0; f < 6; ++f) load_lane<T, PPT>(a.slab + f * a.stride, base, p[f]);
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
            if (!fesgrp::owns(w.begin, w.end, base + q) || p[0][q] < static_cast<T>(0)) continue; // (x < 0: a migrated slot)
            const double vx = static_cast<double>(p[3][q]), vy = static_cast<double>(p[4][q]), vz = static_cast<double>(p[5][q]);
            if (fesmom::rejected(vx, vy, vz)) { ++my_rejected; continue; }
            int i, j, k, wx1, wy1, wz1;
            axis(p[0][q], a.nx, i, wx1);
            axis(p[1][q], a.ny, j, wy1);
            axis(p[2][q], a.nz, k, wz1);
            if (!mom_cell_ok(i, j, k, a.nx, a.ny, a.nz)) continue;
            // the cell within the tile, or the particle has left it since the binning
            const unsigned l = wrap_near(i - ox, a.nx), m = wrap_near(j - oy, a.ny), n = wrap_near(k - oz, a.nz);
            if (!(l < static_cast<unsigned>(W::TX) && m < static_cast<unsigned>(W::TY) && n < static_cast<unsigned>(W::TZ))) {
                mom_global<T>(a, i, j, k, wx1, wy1, wz1, vx, vy, vz);
                ++my_spilled;
                continue;
            }
            const int s0 = static_cast<int>(__umul24(__umul24(n, WY) + m, WX) + l);
            for (int mi = 0; mi < a.nm; ++mi) {
                int64_t t[8];
                mom_particle_terms(a.bit[mi], vx, vy, vz, wx1, wy1, wz1, t);
                unsigned long long* win = mom_lds + mi * WN + s0;
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int aa = 0; aa < 2; ++aa)
                            __hip_atomic_fetch_add(win + (aa + WX * b + WX * WY * c), static_cast<unsigned long long>(t[aa + 2 * b + 4 * c]), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    if (a.counting) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            my_rejected += __shfl_xor(my_rejected, off, 64);
            my_spilled += __shfl_xor(my_spilled, off, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (my_rejected) __hip_atomic_fetch_add(mom_lds + words, static_cast<unsigned long long>(my_rejected), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (my_spilled) __hip_atomic_fetch_add(mom_lds + words + 1, static_cast<unsigned long long>(my_spilled), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < words; s += kMomThreads) {
        const unsigned long long val = mom_lds[s];
        if (val == 0ull) continue;
        const int mi = s / WN, r = s - mi * WN;
        const int n = r / (WX * WY), rem = r - n * (WX * WY);
        const int m = rem / WX, l = rem - m * WX;
        const int gi = wrap_window(ox + l, a.nx), gj = wrap_window(oy + m, a.ny), gk = wrap_window(oz - a.held.zs0 + n, a.nz); // gk: among the planes held
        if (gk < a.held.nzs)
            atomicAdd(a.grids + static_cast<size_t>(a.grid[mi]) * a.grid_words + (static_cast<size_t>(gi) + static_cast<size_t>(a.nx) * (static_cast<size_t>(gj) + static_cast<size_t>(a.ny) * gk)), val);
    }
    if (threadIdx.x < 2 && a.counting) {
        const unsigned long long c = mom_lds[words + threadIdx.x];
        if (c) atomicAdd(a.counters + threadIdx.x, c);
    }
}

template <typename T>
__global__ __launch_bounds__(kMomFlatThreads) void mom_flat_kernel(MomArgs<T> a)
{
    unsigned my_rejected = 0, my_spilled = 0;
    const size_t stride = static_cast<size_t>(gridDim.x) * kMomFlatThreads;
    for (size_t s = static_cast<size_t>(blockIdx.x) * kMomFlatThreads + threadIdx.x; s < a.count; s += stride) {
        const size_t at = a.first + s;
        const T x = a.slab[at], y = a.slab[a.stride + at], z = a.slab[2 * a.stride + at];
        if (x < static_cast<T>(0)) continue; // (a migrated slot)
        const double vx = static_cast<double>(a.slab[3 * a.stride + at]), vy = static_cast<double>(a.slab[4 * a.stride + at]), vz = static_cast<double>(a.slab[5 * a.stride + at]);
        if (fesmom::rejected(vx, vy, vz)) { ++my_rejected; continue; }
        int i, j, k, wx1, wy1, wz1;
        axis(x, a.nx, i, wx1);
        axis(y, a.ny, j, wy1);
        axis(z, a.nz, k, wz1);
        if (!mom_cell_ok(i, j, k, a.nx, a.ny, a.nz)) continue;
        mom_global<T>(a, i, j, k, wx1, wy1, wz1, vx, vy, vz);
        ++my_spilled;
    }
    if (!a.counting) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        my_rejected += __shfl_xor(my_rejected, off, 64);
        my_spilled += __shfl_xor(my_spilled, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (my_rejected) atomicAdd(a.counters, static_cast<unsigned long long>(my_rejected));
        if (my_spilled) atomicAdd(a.counters + 1, static_cast<unsigned long long>(my_spilled));
    }
}

} // namespace fes
