// fes_inject_kernels.hpp — the pass of the particle sources of a CART3D handle (fpic_inject; host side fes_inject.inc.hpp,
// the rule fes_inject_core.hpp).
//   inject_kernel<T, FLUX>   one streaming generation pass in load_slots_kernel's form (fixed grid, grid-stride over groups
//                            of kInjectGroup = FOUR slots, a group per lane and turn) over the slots [n, n + count) of the
//                            live set: slot n + l holds sequence number first + l and the id id0 + l.  A lane generates the
//                            state of its slots (fesinj::state_of: the loader's functions), rounds it to T, and stores the six
//                            state words and the id with store4_masked (fes_pass.hpp): the groups at the two edges of the
//                            range — n need not be a multiple of four — take scalar stores of the new slots only: no slot below
//                            n or from n + count on is written.  Each lane adds the fixed-point terms of the STORED velocities to the
//                            energy diagnostics' accumulator (diag_add: its 128-bit sums, its out-of-range rule), held in
//                            registers across the loop; the workgroup's are combined in the diagnostics' fixed order
//                            (diag_acc_combine) into one partial row.  The kind is a template parameter: the volume instance
//                            carries none of the flux arithmetic.
//                            All four slots of a group are generated together: the accumulator beside their state costs the
//                            fourth wave per SIMD (131 .. 142 VGPRs against the loader's 121), and that is the cheaper side —
//                            the same group taken in two halves of two, one after the other, holds 105 .. 118 VGPRs and runs
//                            four waves, and was SLOWER (1.32 x / 1.68 x the loader's launch in fp32 / fp64 against 1.30 x /
//                            1.29 x): the four independent chains of Philox, log and sqrt in flight hide
//                            more latency than the fourth wave does.
//   (remove_combine_kernel, fes_remove_kernels.hpp: the partial rows -> the row of this application and, added to it, the
//   source's running totals; one workgroup.  The sinks' kernel as it is: the rows have one layout.)
// Plain vector stores, no atomics of any kind, no scratch, no LDS beyond the combine's few words; nothing is read back.
#pragma once

#include "fes_diag_kernels.hpp"
#include "fes_inject_core.hpp"
#include "fes_load_kernels.hpp"
#include "fes_remove_kernels.hpp"

namespace fes {

constexpr int kInjectThreads = 256;
constexpr int kInjectBlocks = 2048;      // 8 workgroups of 4 waves per CU of the 256, as kLoadBlocks
constexpr int kInjectGroup = 4;          // slots per lane and turn: one 16-byte vector of floats or ids, two of doubles

static_assert(fesinj::kRowWords == kDiagWords, "a row of totals is the energy diagnostics' partial row");
static_assert(kInjectThreads == kDiagThreads, "diag_acc_combine's LDS rows are per wave of a kDiagThreads workgroup");

template <typename T>
struct InjectArgs {
    T* slab;                   // x, y, z, vx, vy, vz: six arrays of n_pad (the live set)
    uint32_t* id;              // n_pad words
    size_t n_pad;              // a multiple of 1024: a group of four slots stays inside the arrays
    size_t s0, s1;             // the slots [s0, s1) = [n, n + count); s1 <= the capacity <= n_pad (the host has checked)
    uint32_t first, id0;       // slot s0 + l: sequence number first + l, id id0 + l (neither passes 2^32 - 1: the host has checked)
    unsigned long long* partial;   // [gridDim.x][kDiagWords]: the workgroups' tallies of what the species gained
    fesinj::Rule q;
};

template <typename T, bool FLUX>
__global__ __launch_bounds__(kInjectThreads) void inject_kernel(InjectArgs<T> g)
{
    DiagAcc acc;
    fesinj::Rule q = g.q;
    q.kind = FLUX ? FPIC_INJECT_FLUX : FPIC_INJECT_VOLUME;   // (a constant to the compiler: the other kind's arithmetic goes)
    const size_t g0 = g.s0 / kInjectGroup, g1 = (g.s1 + kInjectGroup - 1) / kInjectGroup, stride = static_cast<size_t>(gridDim.x) * kInjectThreads;
    for (size_t v = g0 + static_cast<size_t>(blockIdx.x) * kInjectThreads + threadIdx.x; v < g1; v += stride) {
        const size_t base = kInjectGroup * v;             // (base + 3 < n_pad: s1 <= n_pad, a multiple of four)
        uint32_t in = 0;
#pragma unroll
        for (int l = 0; l < kInjectGroup; ++l) in |= (base + l >= g.s0 && base + l < g.s1) ? 1u << l : 0u;
        T st[6][kInjectGroup];
        uint32_t ids[kInjectGroup];
#pragma unroll
        for (int l = 0; l < kInjectGroup; ++l) {
            // (a slot outside the range: its sequence number wraps; the state is computed and dropped, as load_slots_kernel does)
            const uint32_t off = static_cast<uint32_t>(base + l - g.s0);
            ids[l] = g.id0 + off;
            double p[3], w[3];
            fesinj::state_of(q, g.first + off, p, w);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                st[a][l] = wrap01(static_cast<T>(p[a]));
                st[3 + a][l] = static_cast<T>(w[a]);
            }
            if (in >> l & 1u) diag_add(acc, static_cast<double>(st[3][l]), static_cast<double>(st[4][l]), static_cast<double>(st[5][l]));
        }
        store4_masked<6>(g.slab + base, g.n_pad, in, st);
        store4_masked<1>(g.id + base, 0, in, &ids);
    }
    diag_acc_combine(acc);
    if (threadIdx.x == 0) diag_store_acc(acc, g.partial + static_cast<size_t>(blockIdx.x) * kDiagWords);
}

// fpic_reserve: the live particles [0, n) of a species' arrays of stride `from_pad` into arrays of stride `to_pad`, column
// by column, and their ids
template <typename T>
__global__ __launch_bounds__(256) void reserve_copy_kernel(const T* __restrict__ from, size_t from_pad, const uint32_t* __restrict__ from_id, T* __restrict__ to, size_t to_pad,
                                                           uint32_t* __restrict__ to_id, size_t n)
{
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int f = 0; f < 6; ++f) to[f * to_pad + i] = from[f * from_pad + i];
    to_id[i] = from_id[i];
}

} // namespace fes
