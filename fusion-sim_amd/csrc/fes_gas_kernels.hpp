// fes_gas_kernels.hpp — the pass of the windowed background collisions of a CART3D handle (fpic_gas; host side
// fes_gas.inc.hpp, the rule fes_gas_core.hpp).  Launch shape, group access, the two hand-outs of candidates and the tally
// are the shared forms of fes_pass.hpp.
//   gas_kernel<T, WINDOW_FIRST, COMPACT>  A candidate is a live particle inside the window whose word w0 < K: a set,
//       whichever test is made first.
//       WINDOW_FIRST = false  per particle the pass reads only the id, runs Philox block 0 and makes the integer test; a
//           particle whose word passes then gathers its position and is dropped if it is dead or outside.  The cheaper order
//           at small P_max and on the whole box (where an untapered request reads no position at all, as collide_kernel).
//       WINDOW_FIRST = true   the pass streams x, y, z of the group with load4 and runs Philox only for the live slots
//           inside; a group wholly outside loads no id.  The cheaper order when the window is a small part of a sorted box.
//       COMPACT = false  the candidates are handed out by take_pending, COMPACT = true by take_queued.
//       The cross-section table and the tapers are read through the caches: the lookups are indexed, not searched, and only
//       candidates make them.  A form that staged them in the workgroup's LDS first (up to 32 KiB + 24.6 KiB: two workgroups
//       per CU) lost the measurement and is not kept.
//       Only a candidate gathers its three velocities, and only a particle that collides is stored: every other particle
//       keeps its bits.  Positions are never written.
// The counts (candidates, below, above, collided) and the exact tallies (energy, momentum: fesgas::tally, the forces'
// before/after terms) are a Tally<4, 4>, whose device words are fesgas::kWords.  No scratch.
#pragma once

#include "fes_collide_kernels.hpp"
#include "fes_force_kernels.hpp"
#include "fes_gas_core.hpp"

namespace fes {

constexpr int kGasThreads = 256;
static_assert(kGasThreads == kPassThreads, "the shared forms reduce and queue for a workgroup of kPassThreads");
constexpr int kGasBlocks = 2048;          // 8 workgroups of 4 waves per CU of the 256, as kCollideBlocks
// The host's choices (gas_window_first, gas_compacts), per request.
// Window first when the window holds less than kGasWindowFirstMax of the box's volume: below, the Philox blocks the pass
// saves outweigh the three position arrays it streams (fp64 breaks even near 0.4, fp32 near 0.47: DESIGN 4.23).
constexpr double kGasWindowFirstMax = 0.4;
// The queue serves kGasCompactMin <= K <= kGasCompactMax (P_max from 2^-8 to 2^-3), the range collide_kernel's queue serves
// and for its reasons: below, the barriers cost more than the idle lanes; above, most lanes are busy anyway.
constexpr unsigned long long kGasCompactMin = 1ull << 24, kGasCompactMax = 1ull << 29;
inline double gas_window_volume(const fesgas::Rule& r) { return (r.win.w[0] * r.win.w[1]) * r.win.w[2]; }
inline bool gas_window_first(const fesgas::Rule& r) { return !r.win.whole && gas_window_volume(r) < kGasWindowFirstMax; }
inline bool gas_compacts(unsigned long long K) { return K >= kGasCompactMin && K <= kGasCompactMax; }

template <typename T>
struct GasArgs : PassArgs<T> {
    unsigned long long* words;    // fesgas::kWords of them
    fesgas::Rule r;
};

using GasAcc = Tally<4, 4>;               // candidates, below, above, collided | energy, momentum x, y, z
static_assert(GasAcc::kWords == fesgas::kWords, "the tally's words are the request's");

// One particle whose word has passed (S, tab: r.sigma and r.win.tab).  CHECK: the window and the dead mark are still to be
// tested (the word came first).
template <typename T, bool CHECK>
__device__ __forceinline__ void gas_one(const GasArgs<T>& g, const double* S, const double* const (&tab)[3], uint32_t i, size_t slot, GasAcc& acc)
{
    const fesgas::Rule& r = g.r;
    // the whole box without a taper reads no position (a stored position lies in [0, 1): every live particle is inside)
    const bool need_p = !r.win.whole || r.win.tapered;
    double p[3] = { 0, 0, 0 };
    if (need_p || (CHECK && g.dead)) {
        p[0] = static_cast<double>(g.slab[slot]);
        if (CHECK && g.dead && p[0] < 0) return;
    }
    if (need_p) {
        p[1] = static_cast<double>(g.slab[g.n_pad + slot]);
        p[2] = static_cast<double>(g.slab[2 * g.n_pad + slot]);
        if (CHECK && !r.win.whole && !fesforce::inside(r.win, p)) return;
    }
    T* vel = g.slab + 3 * g.n_pad + slot;
    const double u0[3] = { static_cast<double>(vel[0]), static_cast<double>(vel[g.n_pad]), static_cast<double>(vel[2 * g.n_pad]) };
    double u[3] = { u0[0], u0[1], u0[2] };
    const int what = fesgas::scatter(r, S, tab, i, p, u);
    acc.count[0] += 1;
    acc.count[1] += what & fesgas::kBelow ? 1 : 0;
    acc.count[2] += what & fesgas::kAbove ? 1 : 0;
    if (what & fesgas::kCollided) {
        acc.count[3] += 1;
        const T st[3] = { static_cast<T>(u[0]), static_cast<T>(u[1]), static_cast<T>(u[2]) };
        vel[0] = st[0];
        vel[g.n_pad] = st[1];
        vel[2 * g.n_pad] = st[2];
        const double w[3] = { static_cast<double>(st[0]), static_cast<double>(st[1]), static_cast<double>(st[2]) };
        fesgas::tally(u0, w, acc.sum, acc.out);
    }
}

template <typename T, bool WINDOW_FIRST, bool COMPACT>
__global__ __launch_bounds__(kGasThreads) void gas_kernel(GasArgs<T> g)
{
    const fesgas::Rule& r = g.r;
    const double* const S = r.sigma;
    const double* const tabs[3] = { r.win.tab[0], r.win.tab[1], r.win.tab[2] };
    const size_t g1 = (g.s1 + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kGasThreads;
    GasAcc acc;
    auto one = [&](uint32_t i, size_t slot) { gas_one<T, !WINDOW_FIRST>(g, S, tabs, i, slot, acc); };
    for (size_t vb = static_cast<size_t>(blockIdx.x) * kGasThreads; vb < g1; vb += stride) {   // (the same turns for every lane)
        const size_t v = vb + threadIdx.x;
        const size_t base = 4 * v;                        // (v < g1: base + 3 < n_pad, as s1 <= n_pad, a multiple of 4)
        uint32_t idx[4] = { 0, 0, 0, 0 }, pend = 0;
        if (v < g1) {
            uint32_t in = 0;
#pragma unroll
            for (int l = 0; l < 4; ++l) in |= base + l < g.s1 ? 1u << l : 0u;
            if constexpr (WINDOW_FIRST) {
                T pos[3][4];
#pragma unroll
                for (int a = 0; a < 3; ++a) load4(g.slab + a * g.n_pad + base, pos[a]);
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    const double p[3] = { static_cast<double>(pos[0][l]), static_cast<double>(pos[1][l]), static_cast<double>(pos[2][l]) };
                    const bool take = !(g.dead && pos[0][l] < static_cast<T>(0)) && fesforce::inside(r.win, p);
                    in &= take ? ~0u : ~(1u << l);
                }
            }
            if (in) {
                ids4(g.id, base, idx);
#pragma unroll
                for (int l = 0; l < 4; ++l) pend |= ((in >> l & 1u) && fesgas::drawn(r, idx[l])) ? 1u << l : 0u;
            }
        }
        if constexpr (COMPACT) take_queued([&](int l) { return (pend >> l & 1u) != 0; }, idx, vb, one);
        else take_pending(pend, idx, base, one);
    }
    tally_commit(acc, g.words);
}

} // namespace fes
