// fes_modes_core.hpp — the host rules of the modes diagnostic (fpic_modes_*: the complex Fourier amplitudes of the node fields
// at chosen wave vectors; the kernels are fes_modes_kernels.hpp, the orchestration fes_modes.inc.hpp): the checks of a
// request, the reduction of a wave number into [0, n), the twiddle tables with their two guaranteed properties, the place
// of a quantity in a row, and the launch shape, which fixes the order of the sum.  Plain C++ that compiles for the host and
// the device, shared with a host test (tests/native/modes_core_test.cpp, g++).  The recording ring is fesdiag::Ring.
#ifndef FES_MODES_CORE_HPP
#define FES_MODES_CORE_HPP
#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/fusionpic.h"

#if defined(__HIPCC__)
#define FES_MODES_HD __host__ __device__ __forceinline__
#else
#define FES_MODES_HD inline
#endif

namespace fesmod {

constexpr int kQuantities = 8;        // bits of a mask
constexpr int kThreads = 256;         // lanes of a workgroup of the partial pass
constexpr int kSegment = 256;         // nodes of a row staged at a time
constexpr unsigned kBlocks = 1024;    // at most this many workgroups (four per CU of the 256)
constexpr int kWxLdsMax = 2048;       // an x table of up to this many entries (32 KiB) is held in LDS; a longer one is read from memory

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style)
inline const char* check(const fpic_modes_spec& s, int nx, int ny, int nz)
{
    if (s.nmodes < 1 || s.nmodes > FPIC_MODES_MAX) return ".nmodes <- must lie in [1, FPIC_MODES_MAX (256)]";
    if (!s.modes) return ".modes <- Non-optional property is undefined!";
    if (!s.mask) return ".mask <- no quantity is selected";
    if (s.mask & ~FPIC_MODE_ALL) return ".mask <- unknown bits (bits 0 .. 7 are defined)";
    const int n[3] = { nx, ny, nz };
    std::vector<std::array<int32_t, 3>> seen(s.nmodes);
    for (uint32_t m = 0; m < s.nmodes; ++m)
        for (int a = 0; a < 3; ++a) {
            const int64_t c = s.modes[3 * m + a];
            if (2 * c > n[a] || 2 * c < -static_cast<int64_t>(n[a])) return ".modes <- a component lies outside [-n/2, n/2] of its axis";
            seen[m][a] = s.modes[3 * m + a];
        }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return ".modes <- the same wave vector twice";
    for (double r : s.reserved)
        if (r != 0) return ".reserved <- must be zero";
    return nullptr;
}

// m mod n in [0, n), for any m (integer arithmetic)
FES_MODES_HD int reduce(int64_t m, int n)
{
    const int64_t r = m % n;
    return static_cast<int>(r < 0 ? r + n : r);
}
// (m * i) mod n for a reduced m and i >= 0
FES_MODES_HD int index_of(int m_reduced, int64_t i, int n) { return static_cast<int>((static_cast<int64_t>(m_reduced) * i) % n); }

// w[t] = exp(-2 pi i t / n), t in [0, n), as (re, im) pairs.  Entries with 4 t divisible by n are exactly (1, 0), (0, -1),
// (-1, 0), (0, 1); the others with t < n / 2 are cos and -sin of the angle evaluated in long double and rounded once; those
// with t > n / 2 are the mirror: w[n - t] is bit for bit the conjugate of w[t] for every 0 < t < n / 2.  (t = n / 2 is its
// own mirror: (-1, 0).)
inline std::vector<double> table(int n)
{
    std::vector<double> w(2 * static_cast<size_t>(n));
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int t = 0; 2 * t <= n; ++t) {
        double re, im;
        if ((4 * static_cast<int64_t>(t)) % n == 0) {
            const int quarter = static_cast<int>(4 * static_cast<int64_t>(t) / n);     // 0, 1, 2
            re = quarter == 0 ? 1.0 : (quarter == 2 ? -1.0 : 0.0);
            im = quarter == 1 ? -1.0 : 0.0;
        } else {
            const long double a = two_pi * static_cast<long double>(t) / static_cast<long double>(n);
            re = static_cast<double>(std::cos(a));
            im = static_cast<double>(-std::sin(a));
        }
        w[2 * static_cast<size_t>(t)] = re;
        w[2 * static_cast<size_t>(t) + 1] = im;
        if (t > 0 && 2 * t < n) {
            w[2 * static_cast<size_t>(n - t)] = re;
            w[2 * static_cast<size_t>(n - t) + 1] = -im;
        }
    }
    return w;
}

// the place of each quantity (bit) in a row's nq entries, -1 for one that is not selected; returns nq
inline int places(uint32_t mask, int place[kQuantities])
{
    int nq = 0;
    for (int b = 0; b < kQuantities; ++b) place[b] = (mask >> b & 1u) ? nq++ : -1;
    return nq;
}

// The launch shape of the partial pass, a function of the number of modes and of the rows (k, j) the handle owns alone.
// A workgroup's 256 lanes are `slots` groups of `1 << log2p` lanes, lane = slot * p + mode: p is the smallest power of two
// that holds the modes; slot s takes the nodes i = s, s + slots, s + 2 slots, ... of every row of the workgroup.  The rows
// [0, rows) are cut into `blocks` contiguous shares of rows_per_block (the last one may be short).
struct Shape {
    int log2p, slots;
    unsigned blocks, rows_per_block;
};
inline Shape shape(uint32_t nmodes, uint64_t rows)
{
    Shape s{};
    while ((1u << s.log2p) < nmodes) ++s.log2p;
    s.slots = kThreads >> s.log2p;
    s.rows_per_block = static_cast<unsigned>(std::max<uint64_t>(1, (rows + kBlocks - 1) / kBlocks));
    s.blocks = static_cast<unsigned>(std::max<uint64_t>(1, (rows + s.rows_per_block - 1) / s.rows_per_block));
    return s;
}

// out[e] = part 0's + part 1's + ... in that order (part r at parts + r * stride): the ranks' rows combined on every rank
inline void add_parts(const double* parts, size_t stride, int nparts, size_t n, double* out)
{
    for (size_t e = 0; e < n; ++e) {
        double v = parts[e];
        for (int r = 1; r < nparts; ++r) v += parts[static_cast<size_t>(r) * stride + e];
        out[e] = v;
    }
}

} // namespace fesmod
#endif
