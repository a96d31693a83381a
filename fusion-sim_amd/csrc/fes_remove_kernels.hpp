// fes_remove_kernels.hpp — the passes of the absorbing particle sinks of a CART3D handle (fpic_remove, fpic_renumber; host
// side fes_remove.inc.hpp, the rule fes_remove_core.hpp).
//   remove_mark_kernel<T, NA>   one streaming pass in select_kernel's form: NA streamed arrays as a template parameter, WHICH
//                               arrays as run-time data, 16-byte loads, two vectors per lane in flight, all loads before any
//                               arithmetic, wave-uniform branches per vector.  It reads only the arrays the request names, and
//                               the ids only when the request thins by id.  The slots are cut into chunks of kRemoveChunk; a
//                               WAVE owns a chunk at a time (a fixed grid, the waves stride over the chunks), so a chunk's
//                               survivor count needs no LDS and no barrier: one store per chunk.  A wave that saw a removed
//                               slot adds its number of them to one 64-bit counter (one integer atomic per such wave; the
//                               sinks' common case has none): the 8 bytes the host reads.  The pass holds no tally: with the
//                               diagnostics' accumulator (four 128-bit sums) alive across the loop it held 98 .. 142 VGPRs and ran
//                               3 .. 4 waves per SIMD, which is what made select_kernel's first form slow, and
//                               this is the pass a sink that absorbs nothing pays every time.
//   (load_scan_kernel, fes_load_kernels.hpp: the chunks' counts -> their exclusive offsets; only if something was removed)
//   remove_move_kernel<T, NA>   only if something was removed.  The same walk; a chunk RE-EVALUATES the predicate (the source
//                               set has not changed; a per-slot bit left by the mark pass would cost that pass a store per
//                               vector in the common case where nothing leaves) and writes its survivors, six state words and
//                               the id, to offset[chunk] + (the survivors below me in the chunk: ballots and mbcnt) of the
//                               OTHER particle set.  Plain stores, no atomics; nothing is written outside [0, n') of the target
//                               set.  A lane that holds a removed slot reads that slot's vx vy vz and adds their fixed-point
//                               terms (diag_add: the energy diagnostics' accumulator, its 128-bit sums and its out-of-range
//                               rule); the workgroup's are combined in the diagnostics' fixed order (diag_acc_combine) into one
//                               partial row.
//   remove_combine_kernel       one workgroup: the partial rows -> the row of this application (plain stores) and, added to it,
//                               the operator's running totals.
//   renumber_*_kernel           fpic_renumber: the live ids into a bitmap over the id span (integer atomicOr), per word the live
//                               ids below it within its chunk of 64 words and the chunks' counts, (load_scan_kernel), then every
//                               particle's id <- the number of live ids below it.
// No float atomics, no scratch.
#pragma once

#include "fes_diag_kernels.hpp"
#include "fes_load_kernels.hpp"
#include "fes_remove_core.hpp"
#include "fes_select_kernels.hpp"

namespace fes {

constexpr int kRemoveThreads = 256;
constexpr int kRemoveBlocks = 2048;      // 8 workgroups of 4 waves per CU of the 256, as kSelectBlocks
constexpr int kRemoveChunk = 2048;       // slots per chunk: 8 (fp32) / 16 (fp64) 16-byte vectors per lane of the wave that owns it
constexpr int kRenumberChunk = 64;       // bitmap words per chunk of the renumbering: one per lane of a wave

static_assert(fesrem::kRowWords == kDiagWords, "a row of totals is the energy diagnostics' partial row");

template <typename T>
struct RemoveArgs {
    const T* slab;             // x, y, z, vx, vy, vz: six arrays of n_pad (the live set)
    const uint32_t* id;        // n_pad words
    size_t n, n_pad;           // slots [0, n); n_pad is a multiple of 1024: the last 16-byte vector stays inside the arrays
    const T* src[kSelectMaxArrays];   // the NA arrays the passes stream, in slab order
    double lo[kSelectMaxArrays], hi[kSelectMaxArrays];   // ... and the term of each that has one
    uint32_t term;             // bit k: src[k] has a term
    int v2;                    // the request has a term on V2: the last three of src are vx, vy, vz
    double v2_lo, v2_hi;
    uint32_t id_mod, id_rem;   // id_mod > 1: the passes stream the ids too
    uint32_t flags;            // FPIC_REMOVE_OUTSIDE
    uint32_t* chunk;           // [nchunks]: the mark pass's survivor counts, for the move pass their exclusive offsets
    size_t nchunks;
    unsigned long long* gone;  // the mark pass: the removed slots, one integer atomic per wave that has any
    unsigned long long* partial;   // the move pass: [gridDim.x][kDiagWords], the workgroups' tallies of what left
    T* dst_slab;               // the move pass: the other set
    uint32_t* dst_id;
};

template <typename T, int NA>
struct RemoveVecs {
    typename Vec16<T>::type a[NA ? NA : 1];
    typename SelectIdVec<16 / sizeof(T)>::type id;
};

template <typename T, int NA>
__device__ __forceinline__ void remove_load(const RemoveArgs<T>& g, size_t v, RemoveVecs<T, NA>& r)
{
    using V = typename Vec16<T>::type;
    using IV = typename SelectIdVec<16 / sizeof(T)>::type;
#pragma unroll
    for (int k = 0; k < NA; ++k) r.a[k] = reinterpret_cast<const V*>(g.src[k])[v];
    if (g.id_mod > 1) r.id = reinterpret_cast<const IV*>(g.id)[v];
}

// the slots of vector v that exist (live) and those of them that leave, one bit each; every branch is wave-uniform and taken
// once per vector (select_kernel's `hits`, then fesrem::removes)
template <typename T, int NA>
__device__ __forceinline__ void remove_eval(const RemoveArgs<T>& g, size_t v, const RemoveVecs<T, NA>& r, uint32_t& live, uint32_t& gone)
{
    constexpr int L = 16 / sizeof(T);
    const T* a = reinterpret_cast<const T*>(r.a);       // a[k * L + l]: slot l of array k
    const uint32_t* ids = reinterpret_cast<const uint32_t*>(&r.id);
    live = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) live |= v * L + l < g.n ? 1u << l : 0u;
    uint32_t in = live, ok = live;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        if (g.term >> k & 1u) {
#pragma unroll
            for (int l = 0; l < L; ++l) in &= fessel::inside(static_cast<double>(a[k * L + l]), g.lo[k], g.hi[k]) ? ~0u : ~(1u << l);
        }
    }
    if constexpr (NA >= 3) {
        if (g.v2) {
#pragma unroll
            for (int l = 0; l < L; ++l)
                in &= fessel::inside(feshist::v2_of(static_cast<double>(a[(NA - 3) * L + l]), static_cast<double>(a[(NA - 2) * L + l]), static_cast<double>(a[(NA - 1) * L + l])),
                                     g.v2_lo, g.v2_hi)
                          ? ~0u
                          : ~(1u << l);
        }
    }
    if (g.id_mod > 1) {
#pragma unroll
        for (int l = 0; l < L; ++l) ok &= fessel::id_passes(ids[l], g.id_mod, g.id_rem) ? ~0u : ~(1u << l);
    }
    gone = 0;
#pragma unroll
    for (int l = 0; l < L; ++l) gone |= (live >> l & 1u) && fesrem::removes(in >> l & 1u, ok >> l & 1u, g.flags) ? 1u << l : 0u;
}

// The walk both passes share: wave w of the grid owns the chunks w, w + waves, ...; a chunk is walked in turns of two vectors
// per lane (vectors [v, v + 64) and [v + 64, v + 128) of the chunk, in slot order), all loads of a turn before its arithmetic.
// begin(chunk), take(vector, live, gone) — called by every lane of the wave, a lane past the species' end with live = 0 —,
// end(chunk).
template <typename T, int NA, typename Begin, typename Take, typename End>
__device__ __forceinline__ void remove_walk(const RemoveArgs<T>& g, Begin begin, Take take, End end)
{
    constexpr int L = 16 / sizeof(T);
    constexpr size_t kVectors = kRemoveChunk / L;        // per chunk
    const int lane = threadIdx.x & 63;
    const size_t nv = (g.n + L - 1) / L, waves = static_cast<size_t>(gridDim.x) * (kRemoveThreads / 64);
    for (size_t c = static_cast<size_t>(blockIdx.x) * (kRemoveThreads / 64) + (threadIdx.x >> 6); c < g.nchunks; c += waves) {
        begin(c);
        const size_t v0 = c * kVectors;
        for (size_t t = 0; t < kVectors && v0 + t < nv; t += 128) {   // (wave-uniform)
            const size_t va = v0 + t + lane, vb = va + 64;
            RemoveVecs<T, NA> r0, r1;
            if (va < nv) remove_load<T, NA>(g, va, r0);
            if (vb < nv) remove_load<T, NA>(g, vb, r1);
            uint32_t live0 = 0, gone0 = 0, live1 = 0, gone1 = 0;
            if (va < nv) remove_eval<T, NA>(g, va, r0, live0, gone0);
            if (vb < nv) remove_eval<T, NA>(g, vb, r1, live1, gone1);
            take(va, live0, gone0);
            take(vb, live1, gone1);
        }
        end(c);
    }
}

template <typename T, int NA>
__global__ __launch_bounds__(kRemoveThreads) void remove_mark_kernel(RemoveArgs<T> g)
{
    const int lane = threadIdx.x & 63;
    uint32_t kept = 0, gone_n = 0;   // (a lane visits fewer than 2^32 slots)
    remove_walk<T, NA>(
        g, [&](size_t) { kept = 0; },
        [&](size_t, uint32_t live, uint32_t gone) {
            kept += __popc(live & ~gone);
            gone_n += __popc(gone);
        },
        [&](size_t c) {
            uint32_t s = kept;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == 0) g.chunk[c] = s;
        });
    unsigned long long s = gone_n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0 && s) atomicAdd(g.gone, s);   // (the sinks' common case: no wave has one)
}

// nblk partial rows -> last[kDiagWords] = their sum (this application), total[kDiagWords] += it (the operator's totals; total
// may be null).  One workgroup; integers, so the order does not matter, and it is fixed anyway.
__global__ __launch_bounds__(kDiagThreads) void remove_combine_kernel(const unsigned long long* __restrict__ partial, int nblk, unsigned long long* __restrict__ last,
                                                                      unsigned long long* __restrict__ total)
{
    DiagAcc a;
    for (int b = threadIdx.x; b < nblk; b += kDiagThreads) diag_load_acc(a, partial + static_cast<size_t>(b) * kDiagWords);
    diag_acc_combine(a);
    if (threadIdx.x == 0) {
        diag_store_acc(a, last);
        if (total) {
            diag_load_acc(a, total);
            diag_store_acc(a, total);
        }
    }
}

template <typename T, int NA>
__global__ __launch_bounds__(kRemoveThreads) void remove_move_kernel(RemoveArgs<T> g)
{
    constexpr int L = 16 / sizeof(T);
    DiagAcc acc;
    uint32_t row0 = 0;   // the target row of the next survivor of the chunk (wave-uniform)
    remove_walk<T, NA>(
        g, [&](size_t c) { row0 = g.chunk[c]; },
        [&](size_t v, uint32_t live, uint32_t gone) {
            const uint32_t keep = live & ~gone;
            // slot order within the 64 vectors: by lane, then by slot of the lane's vector
            uint32_t below = 0, all = 0;
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const unsigned long long b = __ballot(keep >> l & 1u);
                below += __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b), 0u));
                all += __popcll(b);
            }
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const size_t slot = v * L + l;
                if (keep >> l & 1u) {
                    const size_t row = static_cast<size_t>(row0) + below + __popc(keep & ((1u << l) - 1u));
#pragma unroll
                    for (int c = 0; c < 6; ++c) g.dst_slab[c * g.n_pad + row] = g.slab[c * g.n_pad + slot];
                    g.dst_id[row] = g.id[slot];
                } else if (gone >> l & 1u) {
                    diag_add(acc, static_cast<double>(g.slab[3 * g.n_pad + slot]), static_cast<double>(g.slab[4 * g.n_pad + slot]),
                             static_cast<double>(g.slab[5 * g.n_pad + slot]));
                }
            }
            row0 += all;
        },
        [&](size_t) {});
    diag_acc_combine(acc);
    if (threadIdx.x == 0) diag_store_acc(acc, g.partial + static_cast<size_t>(blockIdx.x) * kDiagWords);
}

// ---- fpic_renumber

// bit (id & 31) of word (id >> 5) for every live id; the bitmap was zeroed
__global__ __launch_bounds__(256) void renumber_mark_kernel(const uint32_t* __restrict__ id, size_t n, uint32_t* __restrict__ bitmap)
{
    for (size_t s = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; s < n; s += static_cast<size_t>(gridDim.x) * 256) {
        const uint32_t i = id[s];
        atomicOr(bitmap + (i >> 5), 1u << (i & 31u));
    }
}

// a wave per chunk of kRenumberChunk words: below[w] = the live ids in the chunk's words before w, chunk[c] = those of the chunk
__global__ __launch_bounds__(256) void renumber_count_kernel(const uint32_t* __restrict__ bitmap, size_t nwords, uint32_t* __restrict__ below, uint32_t* __restrict__ chunk,
                                                             size_t nchunks)
{
    const int lane = threadIdx.x & 63;
    const size_t waves = static_cast<size_t>(gridDim.x) * 4;
    for (size_t c = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); c < nchunks; c += waves) {
        const size_t w = c * kRenumberChunk + lane;
        const uint32_t mine = w < nwords ? __popc(bitmap[w]) : 0u;
        uint32_t inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = __shfl_up(inc, off, 64);
            if (lane >= off) inc += up;
        }
        if (w < nwords) below[w] = inc - mine;
        if (lane == 63) chunk[c] = inc;
    }
}

// id <- the number of live ids below it: offset[chunk of its word] + below[its word] + the set bits of its word under its own
__global__ __launch_bounds__(256) void renumber_assign_kernel(uint32_t* __restrict__ id, size_t n, const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ below,
                                                              const uint32_t* __restrict__ offset)
{
    for (size_t s = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; s < n; s += static_cast<size_t>(gridDim.x) * 256) {
        const uint32_t i = id[s], w = i >> 5;
        id[s] = offset[w / kRenumberChunk] + below[w] + __popc(bitmap[w] & ((1u << (i & 31u)) - 1u));
    }
}

} // namespace fes
