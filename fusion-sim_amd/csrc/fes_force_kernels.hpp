// fes_force_kernels.hpp — the pass of the prescribed external forces of a CART3D handle (fpic_force; host side
// fes_force.inc.hpp, the rule fes_force_core.hpp).  The launch shape of relax_kernel / collide_kernel: a fixed grid and a
// grid-stride loop over groups of FOUR slots.
//   force_kernel<T, PLAIN>  streams x, y, z, vx, vy, vz of a group with 16-byte loads; a slot takes part if it lies in the
//       range, is not dead (a rank of a decomposition: x < 0) and — PLAIN = false — lies in the window.  The kick of every
//       such slot is formed in double (fesforce::kick) and cast to T.  A group whose four slots are all kicked rewrites its
//       velocities with 16-byte stores; any other group stores the kicked slots only, with scalar stores: a particle outside
//       keeps every bit.  Positions are never written.
//       PLAIN = true is the instance of a whole-box request without a taper table: no window compare, no table code, no
//       LDS beyond the tallies' few words.  PLAIN = false stages the taper tables (up to 3 x 1025 doubles = 24 600 bytes)
//       in the workgroup's LDS before its first particle, as the profiled loader stages its tables.
// The tallies (kicked, work, impulse; exact fixed point, Fix of fes_diag_kernels.hpp) are kept per lane, reduced over the
// wave by shuffles and over the workgroup through LDS, and added to the request's device words by one lane with one set of
// 64-bit atomics per workgroup: a 128-bit sum as its low word, then its high word plus the carry the low word's add shows.
// No scratch, no float atomics: the same state gives the same bits.
#pragma once

#include "fes_diag_kernels.hpp"
#include "fes_force_core.hpp"

namespace fes {

constexpr int kForceThreads = 256;
constexpr int kForceBlocks = 2048;        // 8 workgroups of 4 waves per CU of the 256, as kCollideBlocks
constexpr size_t kForceLdsBytesMax = 3 * static_cast<size_t>(FPIC_FORCE_TABLE_MAX) * sizeof(double);
static_assert(kForceLdsBytesMax + 1024 <= 64 * 1024, "a launch may ask for 64 KiB of LDS without an attribute");

template <typename T>
struct ForceArgs {
    T* slab;                  // x, y, z, vx, vy, vz: six arrays of n_pad
    size_t n_pad;             // a multiple of 1024: a group of four slots stays inside the arrays
    size_t s1;                // the slots [0, s1) the pass visits
    int dead;                 // a rank of a decomposition: x < 0 marks a dead slot
    unsigned long long* words;    // fesforce::kWords of them
    fesforce::Rule r;
};

struct ForceAcc {
    unsigned long long kicked = 0, out = 0;   // out: bit 0 work, bits 1..3 impulse: a term outside the fixed-point range
    Fix work = 0, imp[3] = { 0, 0, 0 };
};

// after - before as fixed-point integers into `sum`, or — either outside the range — the bit into `out`
__device__ __forceinline__ void force_fix_diff(Fix& sum, unsigned long long& out, double before, double after, int bit)
{
    if (fabs(before) < kFixRange && fabs(after) < kFixRange) sum += to_fix(after) - to_fix(before);
    else out |= 1ull << bit;
}

// sum (128 bits) into the words (lo, hi) of a device sum
__device__ __forceinline__ void force_add128(unsigned long long* w, Fix sum)
{
    if (!sum) return;
    const unsigned long long lo = static_cast<unsigned long long>(sum), hi = static_cast<unsigned long long>(sum >> 64);
    unsigned long long carry = 0;
    if (lo) {
        const unsigned long long old = atomicAdd(w, lo);
        carry = old + lo < old ? 1ull : 0ull;
    }
    if (hi + carry) atomicAdd(w + 1, hi + carry);
}

// the lanes' tallies -> the request's words: every lane of the workgroup calls it once, after its loop
__device__ __forceinline__ void force_tally(ForceAcc& a, unsigned long long* words)
{
    __shared__ unsigned long long part[kForceThreads / 64][fesforce::kWords];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a.kicked += __shfl_xor(a.kicked, off, 64);
        a.out |= __shfl_xor(a.out, off, 64);
        a.work += shfl_xor_fix(a.work, off);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.imp[c] += shfl_xor_fix(a.imp[c], off);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        unsigned long long* p = part[wave];
        p[0] = a.kicked;
        p[1] = static_cast<unsigned long long>(a.work);
        p[2] = static_cast<unsigned long long>(a.work >> 64);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p[3 + 2 * c] = static_cast<unsigned long long>(a.imp[c]);
            p[4 + 2 * c] = static_cast<unsigned long long>(a.imp[c] >> 64);
        }
        p[9] = a.out;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long kicked = 0, out = 0;
        Fix sum[4] = { 0, 0, 0, 0 };
        for (int w = 0; w < kForceThreads / 64; ++w) {
            kicked += part[w][0];
            out |= part[w][9];
            for (int q = 0; q < 4; ++q) sum[q] += (static_cast<Fix>(part[w][2 + 2 * q]) << 64) | part[w][1 + 2 * q];
        }
        if (kicked) atomicAdd(words, kicked);
        for (int q = 0; q < 4; ++q) force_add128(words + 1 + 2 * q, sum[q]);
        if (out) atomicOr(words + 9, out);
    }
}

template <typename T, bool PLAIN>
__global__ __launch_bounds__(kForceThreads) void force_kernel(ForceArgs<T> g)
{
    const fesforce::Rule& r = g.r;
    const double* tab[3] = { nullptr, nullptr, nullptr };
    if constexpr (!PLAIN) {
        extern __shared__ double force_lds[];
        uint32_t at = 0;
        for (int a = 0; a < 3; ++a) {
            const uint32_t n = r.tk[a] ? r.tk[a] + 1 : 0;
            for (uint32_t k = threadIdx.x; k < n; k += kForceThreads) force_lds[at + k] = g.r.tab[a][k];
            if (n) tab[a] = force_lds + at;
            at += n;
        }
        __syncthreads();
    }
    const size_t g1 = (g.s1 + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kForceThreads;
    ForceAcc acc;
    auto load4 = [](const T* src, T (&out)[4]) {
        if constexpr (sizeof(T) == 4) {
            const float4 q = *reinterpret_cast<const float4*>(src);
            out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
        } else {
            const double2 a = *reinterpret_cast<const double2*>(src), b = *reinterpret_cast<const double2*>(src + 2);
            out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y;
        }
    };
    for (size_t v = static_cast<size_t>(blockIdx.x) * kForceThreads + threadIdx.x; v < g1; v += stride) {
        const size_t base = 4 * v;                        // (base + 3 < n_pad: s1 <= n_pad, a multiple of 4)
        T st[6][4];
#pragma unroll
        for (int a = 0; a < 6; ++a) load4(g.slab + a * g.n_pad + base, st[a]);
        uint32_t in = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            bool take = base + l < g.s1 && !(g.dead && st[0][l] < static_cast<T>(0));
            if constexpr (!PLAIN) {
                const double p[3] = { static_cast<double>(st[0][l]), static_cast<double>(st[1][l]), static_cast<double>(st[2][l]) };
                take = take && fesforce::inside(r, p);
            }
            in |= take ? 1u << l : 0u;
        }
        if (!in) continue;
        acc.kicked += __popc(in);
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (in >> l & 1u) {
                const double p[3] = { static_cast<double>(st[0][l]), static_cast<double>(st[1][l]), static_cast<double>(st[2][l]) };
                const double u0[3] = { static_cast<double>(st[3][l]), static_cast<double>(st[4][l]), static_cast<double>(st[5][l]) };
                double u[3] = { u0[0], u0[1], u0[2] };
                const double* const tabs[3] = { tab[0], tab[1], tab[2] };
                if (PLAIN || !r.tapered) fesforce::kick<false>(r, tabs, p, u);
                else fesforce::kick<true>(r, tabs, p, u);
                double w[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    st[3 + a][l] = static_cast<T>(u[a]);
                    w[a] = static_cast<double>(st[3 + a][l]);
                    force_fix_diff(acc.imp[a], acc.out, u0[a], w[a], 1 + a);
                }
                const double b00 = u0[0] * u0[0], b11 = u0[1] * u0[1], b22 = u0[2] * u0[2];
                const double a00 = w[0] * w[0], a11 = w[1] * w[1], a22 = w[2] * w[2];
                const double b01 = b00 + b11, a01 = a00 + a11;
                force_fix_diff(acc.work, acc.out, b01 + b22, a01 + a22, 0);
            }
        if (in == 0xFu) {
#pragma unroll
            for (int a = 3; a < 6; ++a) {
                T* dst = g.slab + a * g.n_pad + base;
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
                    for (int a = 3; a < 6; ++a) g.slab[a * g.n_pad + base + l] = st[a][l];
                }
        }
    }
    force_tally(acc, g.words);
}

} // namespace fes
