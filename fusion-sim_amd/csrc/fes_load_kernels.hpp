// fes_load_kernels.hpp — the passes of the particle loader of a CART3D handle (fpic_load; host side fes_load.inc.hpp, the rule
// fes_load_core.hpp).
//   load_slots_kernel<T, POS, VEL>  an undecomposed handle.  A streaming pass in the launch shape of hist_kernel and
//       select_kernel (fixed grid, grid-stride) over groups of FOUR slots: a lane takes the four particle indices from
//       id[slot] or, while the species is in the caller's order, the slot numbers (ids4, fes_pass.hpp); generates the state
//       of each index inside [first, first + count); and stores it into the slots: a group whose four slots are all loaded
//       with store4, a group at the edge of the range, the tail of 1-3 slots and a group of a permuted species that holds
//       other particles with scalar stores of the loaded slots only: every other particle keeps its bits.  Identity order:
//       only the groups of [first, first + count) are visited.
//   load_keep_kernel<T, WRITE>      a rank of a decomposition, over the INDICES [first, first + count) in chunks of
//       kLoadChunk (one index per lane, one chunk per workgroup and turn).  WRITE = false generates the position only and
//       counts per chunk the particles whose cell plane (axis() of the stored z: cells3_kernel, the migration) lies in the
//       rank's planes [z0, z0 + nzl); load_scan_kernel turns the counts into exclusive offsets and the total; WRITE = true
//       regenerates, and a kept particle goes to slot base + offset[chunk] + (kept lanes below it): consecutive slots in
//       ascending index, the id beside it.
//   A profiled load (fpic_load_profile, the rule fes_load_profile_core.hpp) runs the same two kernels instantiated with
//   LoadProfileArgs / KeepProfileArgs, which add the tables; the instances of fpic_load take LoadArgs / KeepArgs and read no
//   table.  The tables are uploaded per call (at most 82 KB); a workgroup stages the SEARCHED ones - d and C of every axis
//   with a density table, at most 49 200 bytes - in its LDS before its first particle (stage_tables): a search is ten
//   dependent reads per axis, and the profiled instances hold two workgroups per CU by their registers, which 2 x 49 KB of
//   the CU's 160 KiB do not lower.  The thermal and shear tables are read once per particle, through the caches.
//   A radial load (fpic_load_radial, the rule fes_load_radial_core.hpp) is a third set of instances of the same two kernels,
//   with LoadRadialArgs / KeepRadialArgs.  Its tables - d and C of the density and up to four tables read once per particle,
//   at most 6 x 1025 doubles = 49 200 bytes, the profiled instances' bound - are ALL staged in the workgroup's LDS
//   (stage_radial).  The 52 halvings of the radius are the same straight line of fp64 operations in every lane.
// The plain instances: no LDS beyond a few words.  No atomics, no scratch in any instance.
#pragma once

#include "fes_hist_kernels.hpp"
#include "fes_load_profile_core.hpp"
#include "fes_load_radial_core.hpp"
#include "fes_pass.hpp"

namespace fes {

constexpr int kLoadThreads = 256;
constexpr int kLoadBlocks = 2048;       // 8 workgroups of 4 waves per CU of the 256, as kHistBlocks
constexpr int kLoadChunk = kLoadThreads;   // indices per chunk of load_keep_kernel: one per lane

template <typename T>
struct LoadArgs {
    T* slab;                  // x, y, z, vx, vy, vz: six arrays of n_pad
    const uint32_t* id;       // n_pad words; nullptr: slot = index
    size_t n_pad;             // a multiple of 1024: a group of four slots stays inside the arrays
    size_t s0, s1;            // the slots [s0, s1) the pass visits
    fesload::Rule r;
    static constexpr bool kProfile = false;
    static constexpr bool kRadial = false;
};
template <typename T>
struct LoadProfileArgs : LoadArgs<T> {
    fesload::Profile q;
    static constexpr bool kProfile = true;
};
template <typename T>
struct LoadRadialArgs : LoadArgs<T> {
    fesload::Radial q;
    static constexpr bool kRadial = true;
};

// Where the SEARCHED tables (d and C of every axis with a density table) are read from: 1 = staged once per workgroup in
// its LDS, 0 = through the caches (the placement the choice was measured against; build with
// EXTRA_HIPFLAGS=-DFES_LOAD_TABLES_LDS=0).  The thermal and shear tables are read once per particle and stay global.
#ifndef FES_LOAD_TABLES_LDS
#define FES_LOAD_TABLES_LDS 1
#endif
constexpr size_t kLoadLdsBytesMax = 3 * 2 * static_cast<size_t>(FPIC_LOAD_TABLE_MAX) * sizeof(double);
static_assert(kLoadLdsBytesMax + 64 <= 64 * 1024, "a launch may ask for 64 KiB of LDS without an attribute; two workgroups per CU fit the 160 KiB");

// the tables as the lanes read them: q with its searched tables copied to `lds` (q.lds_doubles doubles, the host's count)
__device__ __forceinline__ fesload::Profile stage_tables(const fesload::Profile& q, double* lds)
{
    fesload::Profile s = q;
#if FES_LOAD_TABLES_LDS
    uint32_t at = 0;
    for (int a = 0; a < 3; ++a) {
        const uint32_t n = q.dk[a] ? q.dk[a] + 1 : 0;       // d[0 .. n) and C[0 .. n) lie side by side (fesload::layout)
        for (uint32_t k = threadIdx.x; k < 2 * n; k += kLoadThreads) lds[at + k] = q.dens[a][k];
        s.dens[a] = lds + at;
        s.cum[a] = lds + at + n;
        at += 2 * n;
    }
    __syncthreads();
#endif
    return s;
}

static_assert(6 * static_cast<size_t>(FPIC_LOAD_TABLE_MAX) * sizeof(double) <= kLoadLdsBytesMax, "the tables of a radial load fit the same bound");

// the tables of a radial load as the lanes read them: the whole block (q.lds_doubles doubles from q.dens on) copied to `lds`
__device__ __forceinline__ fesload::Radial stage_radial(const fesload::Radial& q, double* lds)
{
    fesload::Radial s = q;
    for (uint32_t k = threadIdx.x; k < q.lds_doubles; k += kLoadThreads) lds[k] = q.dens[k];
    s.dens = lds;
    s.cum = lds + (q.cum - q.dens);
    if (q.tk) s.therm = lds + (q.therm - q.dens);
    if (q.rk) s.ur = lds + (q.ur - q.dens);
    if (q.zk) s.ut = lds + (q.ut - q.dens);
    if (q.ak) s.ua = lds + (q.ua - q.dens);
    __syncthreads();
    return s;
}

// the state of index i as the handle stores it
template <typename T, bool POS, bool VEL>
__device__ __forceinline__ void load_state(const fesload::Rule& r, uint32_t i, T (&out)[6])
{
    double p[3] = {}, theta = 0;
    if (POS || r.waved) fesload::base_of(r, i, p, theta);
    if constexpr (VEL) {
        double v[3];
        fesload::velocity_of(r, i, theta, v);
#pragma unroll
        for (int a = 0; a < 3; ++a) out[3 + a] = static_cast<T>(v[a]);
    }
    if constexpr (POS) {
        fesload::displace(r, theta, p);
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a] = wrap01(static_cast<T>(p[a]));
    }
}

// the same with the tables of a profile
template <typename T, bool POS, bool VEL>
__device__ __forceinline__ void load_state(const fesload::Rule& r, const fesload::Profile& q, uint32_t i, T (&out)[6])
{
    double p[3] = {}, fq[3] = {}, theta = 0;
    if (POS || r.waved || q.needs_pos) fesload::base_of(r, q, i, p, theta, fq);
    if constexpr (VEL) {
        double v[3];
        fesload::velocity_of(r, q, i, theta, fq, v);
#pragma unroll
        for (int a = 0; a < 3; ++a) out[3 + a] = static_cast<T>(v[a]);
    }
    if constexpr (POS) {
        fesload::displace(r, theta, p);
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a] = wrap01(static_cast<T>(p[a]));
    }
}

// the same with the tables of a radial load
template <typename T, bool POS, bool VEL>
__device__ __forceinline__ void load_state(const fesload::Rule& r, const fesload::Radial& q, uint32_t i, T (&out)[6])
{
    double p[3] = {}, dir[3] = {}, theta = 0, rho = 0;
    if (POS || r.waved || q.needs_pos) fesload::radial_base_of(r, q, i, p, theta, rho, dir);
    if constexpr (VEL) {
        double v[3];
        fesload::radial_velocity_of(r, q, i, theta, rho, dir, v);
#pragma unroll
        for (int a = 0; a < 3; ++a) out[3 + a] = static_cast<T>(v[a]);
    }
    if constexpr (POS) {
        fesload::displace(r, theta, p);
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a] = wrap01(static_cast<T>(p[a]));
    }
}

template <typename T, bool POS, bool VEL, typename Args = LoadArgs<T>>
__global__ __launch_bounds__(kLoadThreads) void load_slots_kernel(Args g)
{
    fesload::Profile tab{};
    if constexpr (Args::kProfile) {
        extern __shared__ double load_lds[];
        tab = stage_tables(g.q, load_lds);
    }
    fesload::Radial rad{};
    if constexpr (Args::kRadial) {
        extern __shared__ double load_lds[];
        rad = stage_radial(g.q, load_lds);
    }
    const size_t g0 = g.s0 / 4, g1 = (g.s1 + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kLoadThreads;
    const uint64_t first = g.r.first, count = g.r.count;
    for (size_t v = g0 + static_cast<size_t>(blockIdx.x) * kLoadThreads + threadIdx.x; v < g1; v += stride) {
        const size_t base = 4 * v;                        // (base + 3 < n_pad: s1 <= n <= n_pad, both multiples of 4 apart)
        uint32_t idx[4];
        ids4(g.id, base, idx);
        uint32_t in = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l)
            in |= (base + l >= g.s0 && base + l < g.s1 && static_cast<uint64_t>(idx[l]) - first < count) ? 1u << l : 0u;   // (idx < first wraps far beyond count)
        if (!in) continue;
        T st[4][6];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if constexpr (Args::kRadial) load_state<T, POS, VEL>(g.r, rad, idx[l], st[l]);
            else if constexpr (Args::kProfile) load_state<T, POS, VEL>(g.r, tab, idx[l], st[l]);
            else load_state<T, POS, VEL>(g.r, idx[l], st[l]);
        }
        constexpr int C0 = POS ? 0 : 3, C1 = VEL ? 6 : 3;
        // (not store4_masked per array: the profiled velocity-only instances then hold 179 VGPRs against 150 and lose a wave)
        if (in == 0xFu) {
#pragma unroll
            for (int c = C0; c < C1; ++c) {
                const T col[4] = { st[0][c], st[1][c], st[2][c], st[3][c] };
                store4(g.slab + c * g.n_pad + base, col);
            }
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (in >> l & 1u) {
#pragma unroll
                    for (int c = C0; c < C1; ++c) g.slab[c * g.n_pad + base + l] = st[l][c];
                }
        }
    }
}

template <typename T>
struct KeepArgs {
    T* slab;                  // WRITE: the rank's arrays
    uint32_t* id;
    size_t n_pad;
    size_t base, limit;       // WRITE: the kept particles go to slots [base, limit)
    uint32_t* chunk;          // [nchunks]: the kept particles per chunk (WRITE = false), their exclusive offsets (WRITE = true)
    size_t nchunks;
    int nz, z0, nzl;          // the rank owns the cell planes [z0, z0 + nzl)
    fesload::Rule r;
    static constexpr bool kProfile = false;
    static constexpr bool kRadial = false;
};
template <typename T>
struct KeepProfileArgs : KeepArgs<T> {
    fesload::Profile q;
    static constexpr bool kProfile = true;
};
template <typename T>
struct KeepRadialArgs : KeepArgs<T> {
    fesload::Radial q;
    static constexpr bool kRadial = true;
};

template <typename T, bool WRITE, typename Args = KeepArgs<T>>
__global__ __launch_bounds__(kLoadThreads) void load_keep_kernel(Args g)
{
    __shared__ uint32_t wave_kept[kLoadThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    fesload::Profile tab{};
    if constexpr (Args::kProfile) {
        extern __shared__ double load_lds[];
        tab = stage_tables(g.q, load_lds);
    }
    fesload::Radial rad{};
    if constexpr (Args::kRadial) {
        extern __shared__ double load_lds[];
        rad = stage_radial(g.q, load_lds);
    }
    for (size_t c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
        const uint64_t k = static_cast<uint64_t>(c) * kLoadChunk + threadIdx.x;
        const uint32_t i = static_cast<uint32_t>(g.r.first + k);
        T st[3] = {};
        double theta = 0, fq[3] = {}, rho = 0, dir[3] = {};
        bool keep = false;
        if (k < g.r.count) {
            double p[3];
            if constexpr (Args::kRadial) fesload::radial_base_of(g.r, rad, i, p, theta, rho, dir);
            else if constexpr (Args::kProfile) fesload::base_of(g.r, tab, i, p, theta, fq);
            else fesload::base_of(g.r, i, p, theta);
            fesload::displace(g.r, theta, p);
#pragma unroll
            for (int a = 0; a < 3; ++a) st[a] = wrap01(static_cast<T>(p[a]));   // (load_state's arithmetic)
            int plane, w1;
            axis(st[2], g.nz, plane, w1);
            keep = static_cast<unsigned>(plane - g.z0) < static_cast<unsigned>(g.nzl);
        }
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(b);
        __syncthreads();
        if constexpr (!WRITE) {
            if (threadIdx.x == 0) {
                uint32_t s = 0;
                for (int w = 0; w < kLoadThreads / 64; ++w) s += wave_kept[w];
                g.chunk[c] = s;
            }
        } else if (keep) {
            size_t slot = g.base + g.chunk[c] + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b), 0u));
            for (int w = 0; w < wave; ++w) slot += wave_kept[w];
            if (slot < g.limit) {   // (the host has checked the total against the capacity; the passes count alike)
                double v[3];
                if constexpr (Args::kRadial) fesload::radial_velocity_of(g.r, rad, i, theta, rho, dir, v);
                else if constexpr (Args::kProfile) fesload::velocity_of(g.r, tab, i, theta, fq, v);
                else fesload::velocity_of(g.r, i, theta, v);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    g.slab[a * g.n_pad + slot] = st[a];
                    g.slab[(3 + a) * g.n_pad + slot] = static_cast<T>(v[a]);
                }
                g.id[slot] = i;
            }
        }
        __syncthreads();   // (wave_kept is rewritten by the next chunk)
    }
}

// counts[0 .. n) -> their exclusive prefix sums in place, the total in *total: one workgroup, 1024 entries per turn
__global__ __launch_bounds__(1024) void load_scan_kernel(uint32_t* __restrict__ counts, size_t n, unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (size_t at = 0; at < n; at += 1024) {
        const size_t k = at + threadIdx.x;
        const uint32_t mine = k < n ? counts[k] : 0u;
        unsigned long long inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long up = __shfl_up(inc, off, 64);
            if (lane >= off) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        unsigned long long before = carry;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        if (k < n) counts[k] = static_cast<uint32_t>(before + inc - mine);   // (below the capacity the host checks, or unused)
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

} // namespace fes
