// fes_select_kernels.hpp — the filter-and-compact pass of the particle selection of a CART3D handle (fpic_select; host side
// fes_select.inc.hpp, the rule fes_select_core.hpp).  One streaming pass in the shape of hist_kernel (fixed grid, grid-stride,
// 16-byte loads, two vectors per lane in flight, all loads before any arithmetic) that reads only the arrays the request
// names: one array per position or velocity term, vx vy vz for V2, x on a decomposed rank (a dead slot has x < 0), the ids
// when the request thins by id.  WHICH arrays is decided at run time — the host hands the pass a list of them, in slab
// order, and wave-uniform flags say what each is tested for —; HOW MANY (NA = 0 .. 6) is a template parameter, so that a lane
// holds registers for the vectors it loads and no others (a pass with room for all six held 82 VGPRs, ran 5 waves per SIMD
// and took twice the histogram's time over one fp32 array).  No instantiation per axis combination.
//   DELIVER = false  the count query: per-lane counts, summed over the wave and the workgroup, one 64-bit integer atomic per
//                    workgroup on the cursor
//   DELIVER = true   per vector a wave ballots its hits (one ballot per slot of the vector), one lane takes their number of
//                    rows from the 64-bit cursor with one atomic, every hit lane finds its row from the hits below it
//                    (mbcnt), and only a lane whose row is below `cap` reads the slot's six state words and its id and writes
//                    them to out_id[cap], out_state[6][cap] with plain stores.  The cursor keeps counting past cap: it is
//                    `matched` either way.
// Integer atomics only; the rows' order is the atomics' and the host sorts them by id.
#pragma once

#include "fes_hist_kernels.hpp"
#include "fes_select_core.hpp"

namespace fes {

constexpr int kSelectThreads = 256;
constexpr int kSelectBlocks = 2048;     // 8 workgroups of 4 waves per CU of the 256, as kHistBlocks

constexpr int kSelectMaxArrays = 6;

template <typename T>
struct SelectArgs {
    const T* slab;             // x, y, z, vx, vy, vz: six arrays of n_pad (the rows a hit lane copies)
    const uint32_t* id;        // n_pad words
    size_t n, n_pad;           // slots [0, n); n_pad is a multiple of 1024: the last 16-byte vector stays inside the arrays
    const T* src[kSelectMaxArrays];   // the NA arrays the pass streams, in slab order
    double lo[kSelectMaxArrays], hi[kSelectMaxArrays];   // ... and the term of each that has one
    uint32_t term;             // bit k: src[k] has a term
    int dead;                  // a decomposed rank: src[0] is x, and a slot with x < 0 is dead
    int v2;                    // the request has a term on V2: the last three of src are vx, vy, vz
    double v2_lo, v2_hi;
    uint32_t id_mod, id_rem;   // id_mod > 1: the pass streams the ids too
    unsigned long long cap;    // rows of the outputs
    uint32_t* out_id;          // [cap]
    T* out_state;              // [6][cap]
};

template <int L>
struct SelectIdVec;
template <>
struct SelectIdVec<4> { using type = uint4; };
template <>
struct SelectIdVec<2> { using type = uint2; };

template <typename T, int NA, bool DELIVER>
__global__ __launch_bounds__(kSelectThreads) void select_kernel(SelectArgs<T> g, unsigned long long* __restrict__ cursor)
{
    using V = typename Vec16<T>::type;
    constexpr int L = 16 / sizeof(T);
    using IV = typename SelectIdVec<L>::type;
    struct Vecs {
        V a[NA ? NA : 1];
        IV id;
    };
    const size_t n = g.n, nv = (n + L - 1) / L, stride = static_cast<size_t>(gridDim.x) * kSelectThreads;
    const int lane = threadIdx.x & 63;
    const bool by_id = g.id_mod > 1;
    unsigned long long count = 0;
    auto load = [&](size_t v, Vecs& r) {
#pragma unroll
        for (int k = 0; k < NA; ++k) r.a[k] = reinterpret_cast<const V*>(g.src[k])[v];
        if (by_id) r.id = reinterpret_cast<const IV*>(g.id)[v];
    };
    // the slots of vector v that are selected, one bit each; every branch is wave-uniform and taken once per vector
    auto hits = [&](size_t v, const Vecs& r) {
        const T* a = reinterpret_cast<const T*>(r.a);       // a[k * L + l]: slot l of array k
        const uint32_t* ids = reinterpret_cast<const uint32_t*>(&r.id);
        uint32_t mask = 0;
#pragma unroll
        for (int l = 0; l < L; ++l) mask |= v * L + l < n ? 1u << l : 0u;
        if constexpr (NA >= 1) {
            if (g.dead) {
#pragma unroll
                for (int l = 0; l < L; ++l) mask &= a[l] < static_cast<T>(0) ? ~(1u << l) : ~0u;
            }
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            if (g.term >> k & 1u) {
#pragma unroll
                for (int l = 0; l < L; ++l) mask &= fessel::inside(static_cast<double>(a[k * L + l]), g.lo[k], g.hi[k]) ? ~0u : ~(1u << l);
            }
        }
        if constexpr (NA >= 3) {
            if (g.v2) {
#pragma unroll
                for (int l = 0; l < L; ++l)
                    mask &= fessel::inside(feshist::v2_of(static_cast<double>(a[(NA - 3) * L + l]), static_cast<double>(a[(NA - 2) * L + l]), static_cast<double>(a[(NA - 1) * L + l])),
                                           g.v2_lo, g.v2_hi)
                                ? ~0u
                                : ~(1u << l);
            }
        }
        if (by_id) {
#pragma unroll
            for (int l = 0; l < L; ++l) mask &= fessel::id_passes(ids[l], g.id_mod, g.id_rem) ? ~0u : ~(1u << l);
        }
        return mask;
    };
    auto take = [&](size_t v, const Vecs& r) {
        const uint32_t mask = hits(v, r);
        if constexpr (!DELIVER) {
            count += __popc(mask);
        } else {
            // (a lane that has left the loop is in no ballot: the masks hold the active lanes only)
            unsigned long long b[L];
            uint32_t total = 0;
#pragma unroll
            for (int l = 0; l < L; ++l) {
                b[l] = __ballot(mask >> l & 1u);
                total += __popcll(b[l]);
            }
            if (total) {
                const int leader = __ffsll(__ballot(1)) - 1;   // the first active lane: what readfirstlane reads
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(cursor, static_cast<unsigned long long>(total));
                base = static_cast<unsigned long long>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base))) |
                       static_cast<unsigned long long>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base >> 32))) << 32;
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    if (mask >> l & 1u) {
                        const unsigned long long row =
                            base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b[l] >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b[l]), 0u));
                        if (row < g.cap) {
                            const size_t slot = v * L + l;
                            g.out_id[row] = g.id[slot];
#pragma unroll
                            for (int c = 0; c < 6; ++c) g.out_state[c * g.cap + row] = g.slab[c * g.n_pad + slot];
                        }
                    }
                    base += __popcll(b[l]);
                }
            }
        }
    };
    size_t v = static_cast<size_t>(blockIdx.x) * kSelectThreads + threadIdx.x;
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
    if constexpr (!DELIVER) {
        __shared__ unsigned long long part[kSelectThreads / 64];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
        if (lane == 0) part[threadIdx.x >> 6] = count;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long s = 0;
            for (int w = 0; w < kSelectThreads / 64; ++w) s += part[w];
            if (s) atomicAdd(cursor, s);
        }
    }
}

} // namespace fes
