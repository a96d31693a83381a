// fes_hist_kernels.hpp — the phase-space histogram of one species of a CART3D handle (fpic_histogram; host side
// fes_hist.inc.hpp, the bin rule fes_hist_core.hpp).  One streaming pass in the shape of diag_particles_kernel (fixed grid,
// grid-stride, 16-byte loads, two vectors per lane in flight, all loads before any arithmetic) that reads only the arrays
// its axes need — plus x on a decomposed rank, whose dead slots have x < 0, when x is not an axis already:
//   LDS = true   up to kHistLdsBins bins: a private uint32 histogram per workgroup in LDS (no-return LDS atomics), whose
//                non-zero bins go to the uint64 counters in global memory with integer atomics at the end
//   LDS = false  up to FPIC_HIST_MAX_BINS bins: integer atomics on the global uint64 counters directly
// Before an atomic a wave whose active lanes all hold the same bin (a cold beam) lets one lane add their number.
// Integer adds commute: the same state gives the same bits; no float atomics.  counts[nbins] is the `outside` word; the
// host zeroes all nbins + 1 words on the stream before the launch.
#pragma once

#include "fes_diag_kernels.hpp"
#include "fes_hist_core.hpp"

namespace fes {

constexpr int kHistThreads = 256;
constexpr int kHistBlocks = 2048;       // 8 workgroups of 4 waves per CU of the 256, as kDiagBlocks
// The LDS path's limit: 16384 uint32 bins are 64 KiB of the CU's 160 KiB, so two such workgroups (8 waves) still share a CU;
// a 1024-bin histogram takes 4 KiB and does not limit the 8 workgroups per CU the grid is sized for.
constexpr uint32_t kHistLdsBins = 16384;
// A workgroup's share of a species: the vectors of its lanes at the grid's stride.  The private uint32 bins cannot
// overflow while this is below 2^32 — which it is for every species the library holds (particle ids are 32-bit: n <= 2^32
// gives at most 2^21 + 2048 per workgroup); the host checks it and takes the global path otherwise.
constexpr uint64_t hist_block_share(uint64_t n, int lanes_per_vec)
{
    const uint64_t nv = (n + lanes_per_vec - 1) / lanes_per_vec, stride = static_cast<uint64_t>(kHistBlocks) * kHistThreads;
    return (nv + stride - 1) / stride * kHistThreads * lanes_per_vec;
}

enum HistKind { HIST_NONE = 0, HIST_PLAIN = 1, HIST_V2 = 2 };   // no axis | one stored array | vx, vy, vz -> |v|^2

template <typename T>
struct HistArgs {
    const T* src[2][3];    // axis a: its array (PLAIN) or vx, vy, vz (V2)
    const T* x;            // dead_from == 2: the positions, read for the dead test alone
    int dead_from;         // -1: no dead slots (not decomposed); 0 / 1: axis 0 / 1 is x, a slot is dead when its q < 0; 2: x
    feshist::Axis ax[2];
    size_t n;              // slots [0, n); the arrays are n_pad long (a multiple of 1024): the last 16-byte vector stays inside
    uint32_t nbins;        // bins[0] (* bins[1])
};

template <bool LDS>
__device__ __forceinline__ void hist_add(uint32_t* lds, unsigned long long* counts, uint32_t bin, uint32_t by)
{
    if constexpr (LDS) atomicAdd(lds + bin, by);
    else atomicAdd(counts + bin, static_cast<unsigned long long>(by));
}

template <typename T, int K0, int K1, bool LDS>
__global__ __launch_bounds__(kHistThreads) void hist_kernel(HistArgs<T> g, unsigned long long* __restrict__ counts)
{
    extern __shared__ unsigned long long hist_shared[];   // LDS: nbins uint32; afterwards (and without LDS) one word per wave
    uint32_t* lds = reinterpret_cast<uint32_t*>(hist_shared);
    using V = typename Vec16<T>::type;
    constexpr int L = 16 / sizeof(T);
    constexpr int N0 = K0 == HIST_V2 ? 3 : 1, N1 = K1 == HIST_V2 ? 3 : (K1 == HIST_PLAIN ? 1 : 0);
    struct Vecs {
        V a[N0], b[N1 ? N1 : 1], x;
    };
    const size_t n = g.n, nv = (n + L - 1) / L, stride = static_cast<size_t>(gridDim.x) * kHistThreads;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (LDS) {
        for (uint32_t b = threadIdx.x; b < g.nbins; b += kHistThreads) lds[b] = 0;
        __syncthreads();
    }
    unsigned long long out = 0;
    auto load = [&](size_t v, Vecs& r) {
#pragma unroll
        for (int k = 0; k < N0; ++k) r.a[k] = reinterpret_cast<const V*>(g.src[0][k])[v];
#pragma unroll
        for (int k = 0; k < N1; ++k) r.b[k] = reinterpret_cast<const V*>(g.src[1][k])[v];
        if (g.dead_from == 2) r.x = reinterpret_cast<const V*>(g.x)[v];
    };
    auto take = [&](size_t v, const Vecs& r) {
        const T* a = reinterpret_cast<const T*>(r.a);
        const T* b = reinterpret_cast<const T*>(r.b);
        const T* xs = reinterpret_cast<const T*>(&r.x);
#pragma unroll
        for (int l = 0; l < L; ++l) {
            double q0, q1 = 0;
            if constexpr (K0 == HIST_V2) q0 = feshist::v2_of(static_cast<double>(a[l]), static_cast<double>(a[L + l]), static_cast<double>(a[2 * L + l]));
            else q0 = static_cast<double>(a[l]);
            if constexpr (K1 == HIST_V2) q1 = feshist::v2_of(static_cast<double>(b[l]), static_cast<double>(b[L + l]), static_cast<double>(b[2 * L + l]));
            else if constexpr (K1 == HIST_PLAIN) q1 = static_cast<double>(b[l]);
            bool live = v * L + l < n;
            if (g.dead_from == 0) live = live && !(q0 < 0);
            else if (g.dead_from == 1) live = live && !(q1 < 0);
            else if (g.dead_from == 2) live = live && !(xs[l] < static_cast<T>(0));
            bool in = live && feshist::inside(q0, g.ax[0]);
            if constexpr (K1 != HIST_NONE) in = in && feshist::inside(q1, g.ax[1]);
            out += live && !in ? 1 : 0;
            if (in) {
                uint32_t bin = static_cast<uint32_t>(feshist::index_of(q0, g.ax[0]));
                if constexpr (K1 != HIST_NONE) bin = bin * static_cast<uint32_t>(g.ax[1].bins) + static_cast<uint32_t>(feshist::index_of(q1, g.ax[1]));
                // the lanes here all in one bin (compared with the first of them): one lane adds their number
                const uint32_t first_bin = __builtin_amdgcn_readfirstlane(bin);
                const unsigned long long active = __ballot(1), same = __ballot(bin == first_bin);
                if (same == active) {
                    if (lane == __ffsll(active) - 1) hist_add<LDS>(lds, counts, first_bin, static_cast<uint32_t>(__popcll(active)));
                } else {
                    hist_add<LDS>(lds, counts, bin, 1u);
                }
            }
        }
    };
    size_t v = static_cast<size_t>(blockIdx.x) * kHistThreads + threadIdx.x;
    // two vectors per lane in flight: all loads of both before any arithmetic
    for (; v + stride < nv; v += 2 * stride) {
        Vecs r0, r1;
        load(v, r0);
        load(v + stride, r1);
        take(v, r0);
        take(v + stride, r1);
    }
    if (v < nv) {
        Vecs r0;
        load(v, r0);
        take(v, r0);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) out += __shfl_xor(out, off, 64);
    __syncthreads();
    if constexpr (LDS) {
        for (uint32_t b = threadIdx.x; b < g.nbins; b += kHistThreads) {
            const uint32_t c = lds[b];
            if (c) atomicAdd(counts + b, static_cast<unsigned long long>(c));
        }
        __syncthreads();
    }
    if (lane == 0) hist_shared[wave] = out;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < kHistThreads / 64; ++w) s += hist_shared[w];
        if (s) atomicAdd(counts + g.nbins, s);
    }
}

} // namespace fes
