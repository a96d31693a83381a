// fes_diag_kernels.hpp — the energy and momentum diagnostics of a CART3D handle (fpic_energy_now / _record / _history;
// host side fes_diag.inc.hpp).  Two streaming passes write one partial row per workgroup, a combining pass reduces the
// partials of each species (one workgroup per species, one for the fields) and a last one-thread launch writes the row:
//   diag_particles_kernel  one launch per species: vx, vy, vz (and x on a decomposed rank, whose dead slots have x < 0) in
//                          16-byte loads; per lane the count, sum |v|^2 and sum v as EXACT fixed-point integers (Fix, units of
//                          2^-80 c^2 or c: each term floored once, the sums then independent of the particles' order — the
//                          binning lays a species out in an order its atomics decide, and two twin handles must agree bit
//                          for bit) and max |v|^2; combined by lane shuffles within the wave and through LDS across its waves
//   diag_field_kernel      the owned planes of the node E (electrostatic) or of the lattice E and B (full EM; B of the integer
//                          time formed from the half-time array in registers with em_half_curl when the chained step has left
//                          it open — nothing is written), summed in double: the node order is fixed
//   diag_combine_kernel    workgroup s < nsp: species s's partials; workgroup nsp: the field partials (fixed-order tree)
//   diag_row_kernel        the fpic_energy row, plain stores
// Fixed grids (kDiagBlocks, kDiagFieldBlocks) and no float atomics: the same state gives the same bits.
#pragma once

#include "fes_kernels.hpp"

namespace fes {

constexpr int kDiagThreads = 256;
constexpr int kDiagBlocks = 2048;      // partial rows per species: 8 workgroups of 4 waves per CU of the 256
constexpr int kDiagFieldBlocks = 512;
// partial row of a species pass, 64-bit words: count | sum |v|^2 (Fix: lo, hi) | sum vx, vy, vz (Fix) | max |v|^2 (double) |
// the sums that met a term outside the fixed-point range (bit 0: |v|^2, bits 1..3: vx, vy, vz)
constexpr int kDiagWords = 11;
constexpr int kDiagQuantities = 6;     // count, sum |v|^2, sum vx, sum vy, sum vz, max |v|^2 (as doubles after the combine)

// Fixed-point sums: value * 2^80, floored to an integer, in 128-bit two's complement.  A term below 2^15 (|v| < 181 c) times
// 2^32 particles stays below 2^127; the resolution 2^-80 is 1e-14 of the square of a speed of 1e-5 c.  A term outside that
// range, or not finite, adds nothing and marks its sum, which the species then reports as NaN (fix_add).
using Fix = unsigned __int128;
constexpr double kFixRange = 0x1p15;
// floor(d 2^80), exactly, for |d| < kFixRange.  y = |d| 2^80 is exact (a power-of-two scale, below 2^95); so are h = floor(y
// 2^-64) < 2^31 and r = y - h 2^64 in [0, 2^64) (the low bits of y), and the conversion of r truncates: floor(y) = h 2^64 + lo.
// A negative d floors to -ceil(y), one below -floor(y) when y has a fraction.  (Splitting a negative x = d 2^80 directly as
// h = -1, r = 2^64 + x instead rounds r to a multiple of 2^11 whenever |x| < 2^64.)
__device__ __forceinline__ Fix to_fix(double d)
{
    const double y = fabs(d) * 0x1p80;
    const double h = floor(y * 0x1p-64);
    const double r = y - h * 0x1p64;
    const unsigned long long lo = static_cast<unsigned long long>(r);
    const Fix mag = (static_cast<Fix>(static_cast<unsigned long long>(h)) << 64) + lo;
    if (!(d < 0)) return mag;
    return ~mag + (static_cast<double>(lo) != r ? 0 : 1);  // -(mag + 1) when y has a fraction, else -mag
}
// the double nearest to s 2^-80 (ties to even): the magnitude's top 64 bits, with a sticky bit for any set bit below them,
// converted in one rounding.  (Converting the two 64-bit words and adding them rounds twice: the low word of a small negative
// sum, 2^64 - |s|, lands on a multiple of 2^11.)
__device__ __forceinline__ double from_fix(Fix s)
{
    const bool neg = static_cast<__int128>(s) < 0;
    const Fix m = neg ? ~s + 1 : s;
    const unsigned long long hi = static_cast<unsigned long long>(m >> 64);
    double r;
    if (!hi) {
        r = static_cast<double>(static_cast<unsigned long long>(m));
    } else {
        const int sh = 64 - __clzll(static_cast<long long>(hi));                // bits of hi: m >> sh has its top bit set
        const unsigned long long top = static_cast<unsigned long long>(m >> sh) | ((m & ((static_cast<Fix>(1) << sh) - 1)) != 0 ? 1ull : 0ull);
        r = ldexp(static_cast<double>(top), sh);
    }
    return (neg ? -r : r) * 0x1p-80;
}
// the larger of two maxima, NaN if either is (fmax would drop it)
__device__ __forceinline__ double max_keep_nan(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ Fix shfl_xor_fix(Fix v, int off)
{
    const unsigned long long lo = __shfl_xor(static_cast<unsigned long long>(v), off, 64);
    const unsigned long long hi = __shfl_xor(static_cast<unsigned long long>(v >> 64), off, 64);
    return (static_cast<Fix>(hi) << 64) | lo;
}

struct DiagAcc {
    unsigned long long n = 0, out = 0;  // out: the sums that met a term outside the fixed-point range (bits as kDiagWords)
    Fix v2 = 0, vx = 0, vy = 0, vz = 0;
    double m2 = 0;                      // NaN once a |v|^2 is
};

// one term into its sum, or — outside the range, NaN and infinities included — its bit into `out`
__device__ __forceinline__ void fix_add(Fix& sum, unsigned long long& out, double d, int bit)
{
    if (fabs(d) < kFixRange) sum += to_fix(d);
    else out |= 1ull << bit;
}

__device__ __forceinline__ void diag_add(DiagAcc& a, double x, double y, double z)
{
    const double v2 = x * x + y * y + z * z;
    a.n += 1;
    fix_add(a.v2, a.out, v2, 0);
    fix_add(a.vx, a.out, x, 1);
    fix_add(a.vy, a.out, y, 2);
    fix_add(a.vz, a.out, z, 3);
    a.m2 = max_keep_nan(a.m2, v2);
}

__device__ __forceinline__ void diag_store_acc(const DiagAcc& a, unsigned long long* w)
{
    w[0] = a.n;
    const Fix f[4] = { a.v2, a.vx, a.vy, a.vz };
    for (int k = 0; k < 4; ++k) {
        w[1 + 2 * k] = static_cast<unsigned long long>(f[k]);
        w[2 + 2 * k] = static_cast<unsigned long long>(f[k] >> 64);
    }
    w[9] = __double_as_longlong(a.m2);
    w[10] = a.out;
}
__device__ __forceinline__ void diag_load_acc(DiagAcc& a, const unsigned long long* w)
{
    a.n += w[0];
    Fix* f[4] = { &a.v2, &a.vx, &a.vy, &a.vz };
    for (int k = 0; k < 4; ++k) *f[k] += (static_cast<Fix>(w[2 + 2 * k]) << 64) | w[1 + 2 * k];
    a.m2 = max_keep_nan(a.m2, __longlong_as_double(static_cast<long long>(w[9])));
    a.out |= w[10];
}

// the workgroup's accumulators combined (integers exactly, the maximum) -> lane 0 of wave 0 holds them on return
__device__ __forceinline__ void diag_acc_combine(DiagAcc& a)
{
    __shared__ unsigned long long lds[kDiagThreads / 64][kDiagWords];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a.n += __shfl_xor(a.n, off, 64);
        a.v2 += shfl_xor_fix(a.v2, off);
        a.vx += shfl_xor_fix(a.vx, off);
        a.vy += shfl_xor_fix(a.vy, off);
        a.vz += shfl_xor_fix(a.vz, off);
        a.m2 = max_keep_nan(a.m2, __shfl_xor(a.m2, off, 64));
        a.out |= __shfl_xor(a.out, off, 64);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) diag_store_acc(a, lds[wave]);
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kDiagThreads / 64; ++w) diag_load_acc(a, lds[w]);
}

// the workgroup's sums of `nq` doubles per lane, in a fixed order -> row[0 .. nq) by lane 0 of wave 0
template <int NQ>
__device__ __forceinline__ void diag_block_sum(double (&v)[NQ], double* __restrict__ row)
{
    __shared__ double lds[kDiagThreads / 64][NQ];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int q = 0; q < NQ; ++q) v[q] += __shfl_xor(v[q], off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < NQ; ++q) lds[wave][q] = v[q];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double s = lds[0][q];
            for (int w = 1; w < kDiagThreads / 64; ++w) s += lds[w][q];
            row[q] = s;
        }
    }
}

// slots [0, n) of one species; `x` non-null: skip a slot whose x < 0 (dead: fes_kernels.hpp, the migration's pack).
// Slot arrays are n_pad long (a multiple of 1024), so the 16-byte loads of the last vector stay inside them.
template <typename T>
__global__ __launch_bounds__(kDiagThreads) void diag_particles_kernel(const T* __restrict__ x, const T* __restrict__ vx, const T* __restrict__ vy,
                                                                      const T* __restrict__ vz, size_t n, unsigned long long* __restrict__ partial)
{
    using V = typename Vec16<T>::type;
    constexpr int L = 16 / sizeof(T);
    const size_t nv = (n + L - 1) / L, stride = static_cast<size_t>(gridDim.x) * kDiagThreads;
    const V* __restrict__ px = reinterpret_cast<const V*>(x);
    const V* __restrict__ pvx = reinterpret_cast<const V*>(vx);
    const V* __restrict__ pvy = reinterpret_cast<const V*>(vy);
    const V* __restrict__ pvz = reinterpret_cast<const V*>(vz);
    DiagAcc a;
    auto take = [&](size_t v, const V& ax, const V& ay, const V& az, const V& xx) {
        const T* sx = reinterpret_cast<const T*>(&ax);
        const T* sy = reinterpret_cast<const T*>(&ay);
        const T* sz = reinterpret_cast<const T*>(&az);
        const T* s0 = reinterpret_cast<const T*>(&xx);
#pragma unroll
        for (int l = 0; l < L; ++l)
            if (v * L + l < n && !(x && s0[l] < static_cast<T>(0))) diag_add(a, static_cast<double>(sx[l]), static_cast<double>(sy[l]), static_cast<double>(sz[l]));
    };
    size_t v = static_cast<size_t>(blockIdx.x) * kDiagThreads + threadIdx.x;
    // two vectors per lane in flight: all loads of both before any arithmetic
    for (; v + stride < nv; v += 2 * stride) {
        const V a0 = pvx[v], b0 = pvy[v], c0 = pvz[v], a1 = pvx[v + stride], b1 = pvy[v + stride], c1 = pvz[v + stride];
        V x0{}, x1{};
        if (x) { x0 = px[v]; x1 = px[v + stride]; }
        take(v, a0, b0, c0, x0);
        take(v + stride, a1, b1, c1, x1);
    }
    if (v < nv) {
        V x0{};
        if (x) x0 = px[v];
        take(v, pvx[v], pvy[v], pvz[v], x0);
    }
    diag_acc_combine(a);
    if (threadIdx.x == 0) diag_store_acc(a, partial + static_cast<size_t>(blockIdx.x) * kDiagWords);
}

// sum |E|^2 and sum |B|^2 over the nodes of the global planes [k0, k0 + nk) (all held): E = the node E (electrostatic) or
// the lattice E (full EM); B = By (full EM, B of the integer time), or — Bh non-null — Bh - half a step of curl E, which is
// what em_update_b_kernel would store in By (em_close); neither set: no B
template <typename T>
__global__ __launch_bounds__(kDiagThreads) void diag_field_kernel(const T* __restrict__ E, const T* __restrict__ B, const T* __restrict__ Bh, int nx, int ny, int nz,
                                                                  int k0, int nk, Held held, T cbx, T cby, T cbz, double* __restrict__ partial)
{
    const uint32_t plane = static_cast<uint32_t>(nx) * static_cast<uint32_t>(ny), total = plane * static_cast<uint32_t>(nk);
    const size_t sy = static_cast<size_t>(nx), sz = plane;
    double se = 0, sb = 0;
    for (uint32_t t = blockIdx.x * kDiagThreads + threadIdx.x; t < total; t += gridDim.x * kDiagThreads) {
        const int kg = k0 + static_cast<int>(t / plane);
        const uint32_t off = t % plane;
        const int k = held_plane(kg, held, nz);
        const size_t c = static_cast<size_t>(k) * plane + off;
        const double ex = E[4 * c], ey = E[4 * c + 1], ez = E[4 * c + 2];
        se += ex * ex + ey * ey + ez * ez;
        if (B) {
            const double bx = B[4 * c], by = B[4 * c + 1], bz = B[4 * c + 2];
            sb += bx * bx + by * by + bz * bz;
        } else if (Bh) {
            const int i = static_cast<int>(off % nx), j = static_cast<int>(off / nx);
            const int ip = (i + 1 == nx) ? 0 : i + 1, jp = (j + 1 == ny) ? 0 : j + 1, kp = held_plane((kg + 1 == nz) ? 0 : kg + 1, held, nz);
            T cx, cy, cz;
            em_half_curl(E, sy, sz, i, j, k, ip, jp, kp, cbx, cby, cbz, cx, cy, cz);
            const double bx = static_cast<T>(Bh[4 * c] - cx), by = static_cast<T>(Bh[4 * c + 1] - cy), bz = static_cast<T>(Bh[4 * c + 2] - cz);
            sb += bx * bx + by * by + bz * bz;
        }
    }
    double q[2] = { se, sb };
    diag_block_sum<2>(q, partial + static_cast<size_t>(blockIdx.x) * 2);
}

struct DiagScales {
    double ke[FPIC_ENERGY_SPECIES];  // 0.5 m W c^2
    double pm[FPIC_ENERGY_SPECIES];  // m W c
    double e, b, b_ext;              // 0.5 eps0 dV, 0.5 / mu0 dV, the external part of the field energy
    unsigned long long substep;
    int nsp, nblk, nblk_f;
};

// workgroup s < nsp: the nblk partial rows of species s ([nsp][nblk][kDiagWords]) -> sums[s][kDiagQuantities] as doubles;
// workgroup nsp: the nblk_f field partials ([nblk_f][2]) in a fixed order -> sums[FPIC_ENERGY_SPECIES][0 .. 2)
__global__ __launch_bounds__(kDiagThreads) void diag_combine_kernel(const unsigned long long* __restrict__ part, const double* __restrict__ fpart, int nsp,
                                                                    int nblk, int nblk_f, double* __restrict__ sums)
{
    const int s = blockIdx.x;
    if (s < nsp) {
        DiagAcc a;
        for (int b = threadIdx.x; b < nblk; b += kDiagThreads) diag_load_acc(a, part + (static_cast<size_t>(s) * nblk + b) * kDiagWords);
        diag_acc_combine(a);
        if (threadIdx.x == 0) {
            double* o = sums + s * kDiagQuantities;
            const Fix f[4] = { a.v2, a.vx, a.vy, a.vz };
            o[0] = static_cast<double>(a.n);
            for (int k = 0; k < 4; ++k) o[1 + k] = (a.out >> k & 1) ? __builtin_nan("") : from_fix(f[k]);
            o[5] = a.m2;
        }
        return;
    }
    double q[2] = { 0, 0 };
    for (int b = threadIdx.x; b < nblk_f; b += kDiagThreads) { q[0] += fpart[2 * b]; q[1] += fpart[2 * b + 1]; }
    diag_block_sum<2>(q, sums + FPIC_ENERGY_SPECIES * kDiagQuantities);
}

// the sums -> one fpic_energy row (one thread, plain stores)
__global__ void diag_row_kernel(const double* __restrict__ sums, DiagScales sc, fpic_energy* __restrict__ out)
{
    const double* f = sums + FPIC_ENERGY_SPECIES * kDiagQuantities;
    out->substep = sc.substep;
    out->nspecies = sc.nsp;
    out->reserved_i32 = 0;
    out->field_e = sc.e * f[0];
    out->field_b = sc.b * f[1];
    out->field_b_external = sc.b_ext;
    for (int s = 0; s < FPIC_ENERGY_SPECIES; ++s) {
        const bool on = s < sc.nsp;
        const double* v = sums + s * kDiagQuantities;
        out->count[s] = on ? static_cast<uint64_t>(v[0]) : 0;
        out->kinetic[s] = on ? sc.ke[s] * v[1] : 0.0;
        for (int a = 0; a < 3; ++a) out->momentum[s][a] = on ? sc.pm[s] * v[2 + a] : 0.0;
        out->speed_max[s] = on ? sqrt(v[5]) : 0.0;
    }
    for (int k = 0; k < 8; ++k) out->reserved[k] = 0.0;
}

} // namespace fes
