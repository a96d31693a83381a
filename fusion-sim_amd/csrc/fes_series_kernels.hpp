// fes_series_kernels.hpp — the two passes of the series diagnostic of a CART3D handle (fpic_series_*; host side
// fes_series.inc.hpp, the rules fes_series_core.hpp).  The row they write into has been zeroed on the stream before them.
//   series_points_kernel   one lane per point: the charge deposit's cell and weights of the point, eight gathers of the node
//                          records of E4 (and B4n), the sums of the rule in double, plain stores.  At most 4096 lanes.
//   series_tracers_kernel  finds the request's ids of one species among its slots, whose order the binning decides: a
//                          streaming pass in the shape of hist_kernel (fixed grid, grid-stride, 16-byte loads, four vectors
//                          per lane in flight, all loads before any arithmetic) over the id array alone — 4 bytes per slot
//                          in both precisions.  Each workgroup stages the request's bitmap filter into LDS; a slot costs one
//                          LDS read, and only on a filter hit a binary search of the sorted id table (global memory, L2
//                          resident).  On a match, and only then, the slot's six state words are read (a decomposed rank's
//                          dead slot, x < 0, does not match) and the row is written with plain stores.  An id matches at
//                          most one live slot, so no two lanes write one entry: no atomics.
#pragma once

#include "fes_hist_kernels.hpp"
#include "fes_kernels.hpp"
#include "fes_series_core.hpp"

namespace fes {

constexpr int kSeriesThreads = kHistThreads;
constexpr int kSeriesBlocks = kHistBlocks;   // 8 workgroups of 4 waves per CU of the 256, as hist_kernel

template <typename T>
__global__ __launch_bounds__(256) void series_points_kernel(const T* __restrict__ u, uint32_t npoints, const T* __restrict__ E4, const T* __restrict__ B4n,
                                                            int nx, int ny, int nz, Held held, int k0, int nk, double* __restrict__ rows)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npoints) return;
    int i, j, k, wx[2], wy[2], wz[2];
    axis(u[3 * p], nx, i, wx[1]); wx[0] = 16384 - wx[1];
    axis(u[3 * p + 1], ny, j, wy[1]); wy[0] = 16384 - wy[1];
    axis(u[3 * p + 2], nz, k, wz[1]); wz[0] = 16384 - wz[1];
    if (!fesser::owns_plane(k, k0, nk)) return;   // another rank's point: the entry stays zero
    const int kk[2] = { held_plane(k, held, nz), held_plane((k + 1 == nz) ? 0 : k + 1, held, nz) };
    if (kk[0] < 0 || kk[1] < 0) return;           // (the host refuses a handle that does not hold the plane above its slab)
    double acc[7] = { 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int a = e & 1, b = (e >> 1) & 1, c = e >> 2;
        const int ii = (i + a == nx) ? 0 : i + a, jj = (j + b == ny) ? 0 : j + b;
        const size_t node = static_cast<size_t>(ii) + static_cast<size_t>(nx) * (static_cast<size_t>(jj) + static_cast<size_t>(ny) * kk[c]);
        const double w = static_cast<double>(static_cast<long long>(wx[a]) * wy[b] * wz[c]);
        T f[4];
        fpic::load4(E4 + 4 * node, f);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double t = w * static_cast<double>(f[q]);
            acc[q] = e == 0 ? t : acc[q] + t;
        }
        if (B4n) {
            fpic::load4(B4n + 4 * node, f);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double t = w * static_cast<double>(f[q]);
                acc[4 + q] = e == 0 ? t : acc[4 + q] + t;
            }
        }
    }
    double* row = rows + static_cast<size_t>(p) * fesser::kEntry;
#pragma unroll
    for (int q = 0; q < 7; ++q) row[q] = acc[q] * 0x1p-42;
    row[fesser::kPointFlag] = 1.0;
}

template <typename T>
struct SeriesTracerArgs {
    const uint32_t* id;        // the species' id array: n_pad (a multiple of 1024) words, so the last 16-byte vector stays inside
    const T* slab;             // x, y, z, vx, vy, vz: six arrays of n_pad
    size_t n, n_pad;           // slots [0, n)
    const uint32_t* sorted;    // the request's ids of this species, ascending
    const uint32_t* index;     // ... and the entry of the request each of them is
    const uint32_t* filter;    // 2^log2bits bits
    uint32_t m, log2bits;
    int dead;                  // a decomposed rank: a slot with x < 0 is dead and its id stale
    double* rows;              // the tracer entries of the row
};

template <typename T>
__device__ __forceinline__ void series_match(const SeriesTracerArgs<T>& g, size_t slot, uint32_t id)
{
    const int64_t at = fesser::lookup(g.sorted, g.m, id);
    if (at < 0) return;        // (a false positive of the filter)
    const T x = g.slab[slot];
    if (g.dead && x < static_cast<T>(0)) return;
    double* row = g.rows + static_cast<size_t>(g.index[at]) * fesser::kEntry;
    row[0] = static_cast<double>(x);
#pragma unroll
    for (int c = 1; c < 6; ++c) row[c] = static_cast<double>(g.slab[c * g.n_pad + slot]);
    row[fesser::kTracerFlag] = 1.0;
    row[7] = 0.0;
}

template <typename T>
__global__ __launch_bounds__(kSeriesThreads) void series_tracers_kernel(SeriesTracerArgs<T> g)
{
    extern __shared__ uint32_t series_filter[];
    const uint32_t words = 1u << (g.log2bits - 5);
    for (uint32_t w = threadIdx.x; w < words; w += kSeriesThreads) series_filter[w] = g.filter[w];
    __syncthreads();
    const size_t n = g.n, nv = (n + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kSeriesThreads;
    const uint4* ids = reinterpret_cast<const uint4*>(g.id);
    // the filter's answers for the four slots of a vector, one bit each: four LDS reads issued together, no branch between them
    auto hits = [&](const uint4& q) {
        return (fesser::filter_hit(series_filter, q.x, g.log2bits) ? 1u : 0u) | (fesser::filter_hit(series_filter, q.y, g.log2bits) ? 2u : 0u) |
               (fesser::filter_hit(series_filter, q.z, g.log2bits) ? 4u : 0u) | (fesser::filter_hit(series_filter, q.w, g.log2bits) ? 8u : 0u);
    };
    // the rare path: the slots of vector v the filter let through
    auto take = [&](size_t v, const uint4& q, uint32_t mask) {
        const uint32_t id[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const size_t slot = 4 * v + l;
            if ((mask >> l & 1u) && slot < n) series_match<T>(g, slot, id[l]);
        }
    };
    size_t v = static_cast<size_t>(blockIdx.x) * kSeriesThreads + threadIdx.x;
    // four vectors per lane in flight, all loads before any arithmetic: a request with the full filter leaves a CU two
    // workgroups, and 64 bytes per lane keep the stream fed at that occupancy
    for (; v + 3 * stride < nv; v += 4 * stride) {
        const uint4 q0 = ids[v], q1 = ids[v + stride], q2 = ids[v + 2 * stride], q3 = ids[v + 3 * stride];
        const uint32_t m0 = hits(q0), m1 = hits(q1), m2 = hits(q2), m3 = hits(q3);
        if (m0 | m1 | m2 | m3) {
            take(v, q0, m0);
            take(v + stride, q1, m1);
            take(v + 2 * stride, q2, m2);
            take(v + 3 * stride, q3, m3);
        }
    }
    for (; v < nv; v += stride) {
        const uint4 q0 = ids[v];
        const uint32_t m0 = hits(q0);
        if (m0) take(v, q0, m0);
    }
}

} // namespace fes
