// fes_force_kernels.hpp — the pass of the prescribed external forces of a CART3D handle (fpic_force; host side
// fes_force.inc.hpp, the rule fes_force_core.hpp).  Launch shape, group access and the tally are the shared forms of
// fes_pass.hpp.
//   force_kernel<T, PLAIN>  streams x, y, z, vx, vy, vz of a group with load4; a slot takes part if it lies in the range, is
//       not dead (a rank of a decomposition: x < 0) and — PLAIN = false — lies in the window.  The kick of every such slot is
//       formed in double (fesforce::kick) and cast to T, and the velocities are rewritten with store4_masked: a particle
//       outside keeps every bit.  Positions are never written.
//       PLAIN = true is the instance of a whole-box request without a taper table: no window compare, no table code, no
//       LDS beyond the tallies' few words.  PLAIN = false stages the taper tables (up to 3 x 1025 doubles = 24 600 bytes)
//       in the workgroup's LDS before its first particle, as the profiled loader stages its tables.
// The tallies (kicked | work, impulse: fesforce::tally's exact before/after terms) are a Tally<1, 4>, whose device words are
// fesforce::kWords.
#pragma once

#include "fes_force_core.hpp"
#include "fes_pass.hpp"

namespace fes {

constexpr int kForceThreads = 256;
static_assert(kForceThreads == kPassThreads, "tally_commit reduces a workgroup of kPassThreads");
constexpr int kForceBlocks = 2048;        // 8 workgroups of 4 waves per CU of the 256, as kCollideBlocks
constexpr size_t kForceLdsBytesMax = 3 * static_cast<size_t>(FPIC_FORCE_TABLE_MAX) * sizeof(double);
static_assert(kForceLdsBytesMax + 1024 <= 64 * 1024, "a launch may ask for 64 KiB of LDS without an attribute");

template <typename T>
struct ForceArgs : PassArgs<T> {              // (id is not read: a kick does not depend on which particle it is)
    unsigned long long* words;    // fesforce::kWords of them
    fesforce::Rule r;
};

using ForceAcc = Tally<1, 4>;                 // kicked | work, impulse x, y, z; out: bit 0 work, bits 1..3 impulse
static_assert(ForceAcc::kWords == fesforce::kWords, "the tally's words are the request's");

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
        acc.count[0] += __popc(in);
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
                }
                fesforce::tally(u0, w, acc.sum, acc.out);
            }
        store4_masked<3>(g.slab + 3 * g.n_pad + base, g.n_pad, in, st + 3);
    }
    tally_commit(acc, g.words);
}

} // namespace fes
