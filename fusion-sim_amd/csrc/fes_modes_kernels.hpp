// fes_modes_kernels.hpp — the two passes of the modes diagnostic of a CART3D handle (fpic_modes_*; host side
// fes_modes.inc.hpp, the rules fes_modes_core.hpp).  The sum is separable: per row (k, j) the sum over i with the x twiddles,
// one multiplication of the row's sum by wy * wz, and the running total.
//   modes_partial_kernel  a fixed number of 256-lane workgroups (fesmod::shape), each over a fixed contiguous share of the
//                         owned rows.  A row is staged 256 nodes at a time into LDS as doubles, one array per selected
//                         quantity (coalesced 16- / 32-byte loads of the node records, 8-byte loads of the charge grid); the
//                         x table lies in LDS beside them.  Lanes map to modes: lane = slot * p + mode, and the slots share
//                         a staged segment node by node (slot s: nodes s, s + slots, ...), so a wave's reads of the staged
//                         values are broadcasts of at most 64 / p adjacent words.  A lane advances its table index by
//                         additions and one conditional subtraction (no division in the loops) and keeps its 8 complex row
//                         sums and 8 complex totals in registers.  At the end the slots of a mode are added in slot order
//                         through LDS and the workgroup's partial row is written with plain stores.  No atomics.
//   modes_combine_kernel  one wave per number of the row: the workgroups' partials added in a fixed two-level order, divided by N.
#pragma once

#include "fes_kernels.hpp"
#include "fes_modes_core.hpp"

namespace fes {

template <typename T>
struct ModesArgs {
    const T* E4;               // node records (held planes), nullptr if no quantity of it is selected
    const T* B4n;              // ... of the node-centred B; nullptr: not selected, or the box has none (its amplitudes are zero)
    const long long* rho;      // the integer charge grid, nullptr if not selected
    double rho_scale;          // q0 W / (2^42 dV)
    int nx, ny, nz;
    Held held;
    int k0, nk;                // the owned planes
    const double2 *wx, *wy, *wz;
    const int32_t* modes;      // [nmodes][3], reduced into [0, n)
    uint32_t nmodes;
    int nq;
    int place[fesmod::kQuantities];   // of quantity b in the nq entries of a mode, -1: not selected
    int log2p, slots;
    unsigned rows_per_block;
    double2* partial;          // [gridDim.x][nmodes][nq]
};

// a * b of two complex numbers, every operation rounded once: (a.x b.x - a.y b.y, a.x b.y + a.y b.x)
__device__ __forceinline__ double2 modes_cmul(double2 a, double2 b)
{
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

template <typename T, bool WX_LDS>
__global__ __launch_bounds__(fesmod::kThreads) void modes_partial_kernel(ModesArgs<T> g)
{
    constexpr int NQ = fesmod::kQuantities, SEG = fesmod::kSegment;
    extern __shared__ double2 modes_lds[];
    // [the x table, nx entries, if WX_LDS][the staged segment: nq arrays of SEG doubles; at the end 256 complex numbers]
    double2* const wx_lds = modes_lds;
    double* const stage = reinterpret_cast<double*>(modes_lds + (WX_LDS ? g.nx : 0));
    const int tid = static_cast<int>(threadIdx.x);
    if (WX_LDS)
        for (int t = tid; t < g.nx; t += fesmod::kThreads) wx_lds[t] = g.wx[t];
    const int p = 1 << g.log2p, mode = tid & (p - 1), slot = tid >> g.log2p;
    const bool active = static_cast<uint32_t>(mode) < g.nmodes;
    int mx = 0, my = 0, mz = 0;
    if (active) { mx = g.modes[3 * mode]; my = g.modes[3 * mode + 1]; mz = g.modes[3 * mode + 2]; }
    const int nx = g.nx, ny = g.ny, nz = g.nz, slots = g.slots;
    // the x index of the lane's first node of a row, and its step from one of its nodes to the next
    const int t_row = fesmod::index_of(mx, slot, nx), t_step = fesmod::index_of(mx, slots, nx);
    const uint64_t rows = static_cast<uint64_t>(g.nk) * ny;
    const uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * g.rows_per_block, r1 = r0 + g.rows_per_block < rows ? r0 + g.rows_per_block : rows;
    int j = 0, k = g.k0, ty = 0, tz = 0;
    if (r0 < rows) {
        j = static_cast<int>(r0 % ny);
        k = g.k0 + static_cast<int>(r0 / ny);
        ty = fesmod::index_of(my, j, ny);
        tz = fesmod::index_of(mz, k, nz);
    }
    double2 tot[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) tot[q] = make_double2(0.0, 0.0);
    for (uint64_t r = r0; r < r1; ++r) {
        const size_t row = static_cast<size_t>(nx) * (static_cast<size_t>(j) + static_cast<size_t>(ny) * held_plane(k, g.held, nz));
        double2 sum[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) sum[q] = make_double2(0.0, 0.0);
        int t = t_row;
        for (int i0 = 0; i0 < nx; i0 += SEG) {
            __syncthreads();   // (the lanes have finished with the segment before; the first time: the x table is in place)
            const int i = i0 + tid;
            if (i < nx) {
                const size_t node = row + i;
                if (g.E4) {
                    T f[4];
                    fpic::load4(g.E4 + 4 * node, f);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (g.place[c] >= 0) stage[g.place[c] * SEG + tid] = static_cast<double>(f[c]);
                }
                if (g.place[4] >= 0 || g.place[5] >= 0 || g.place[6] >= 0) {
                    T f[4] = { 0, 0, 0, 0 };
                    if (g.B4n) fpic::load4(g.B4n + 4 * node, f);
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (g.place[4 + c] >= 0) stage[g.place[4 + c] * SEG + tid] = static_cast<double>(f[c]);
                }
                if (g.rho) stage[g.place[7] * SEG + tid] = static_cast<double>(g.rho[node]) * g.rho_scale;
            }
            __syncthreads();
            if (active) {
                const int len = nx - i0 < SEG ? nx - i0 : SEG;
                for (int n = slot; n < len; n += slots) {
                    const double2 w = WX_LDS ? wx_lds[t] : g.wx[t];
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        if (q < g.nq) {
                            const double f = stage[q * SEG + n];
                            sum[q].x += f * w.x;
                            sum[q].y += f * w.y;
                        }
                    t += t_step;
                    if (t >= nx) t -= nx;
                }
            }
        }
        if (active) {
            const double2 w = modes_cmul(g.wy[ty], g.wz[tz]);
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (q < g.nq) {
                    const double2 v = modes_cmul(sum[q], w);
                    tot[q].x += v.x;
                    tot[q].y += v.y;
                }
        }
        // the next row: (k, j + 1), or (k + 1, 0)
        ty += my;
        if (ty >= ny) ty -= ny;
        if (++j == ny) {
            j = 0;
            ty = 0;
            ++k;
            tz += mz;
            if (tz >= nz) tz -= nz;
        }
    }
    // the slots of a mode, added in slot order
    double2* const red = reinterpret_cast<double2*>(stage);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (q >= g.nq) break;
        __syncthreads();
        red[tid] = tot[q];
        __syncthreads();
        if (active && slot == 0) {
            double2 v = red[mode];
            for (int s = 1; s < slots; ++s) {
                v.x += red[(s << g.log2p) + mode].x;
                v.y += red[(s << g.log2p) + mode].y;
            }
            g.partial[(static_cast<size_t>(blockIdx.x) * g.nmodes + mode) * g.nq + q] = v;
        }
    }
}

// row[e] = (the workgroups' partial[b][e] added up) / nodes, e < width (the numbers of a row: nmodes * nq * 2): one wave per
// number.  Lane l adds the partials of the workgroups [l * per, (l + 1) * per), per = ceil(blocks / 64), in workgroup order —
// independent loads, so the wave waits for memory once and not `blocks` times —, then lane 0 adds the 64 lane sums in lane
// order.  The order is a function of `blocks` alone.
__global__ __launch_bounds__(64) void modes_combine_kernel(const double* __restrict__ partial, unsigned blocks, unsigned width, double nodes, double* __restrict__ row)
{
    __shared__ double lane_sum[64];
    const unsigned e = blockIdx.x, lane = threadIdx.x, per = (blocks + 63u) / 64u;
    const unsigned b0 = lane * per < blocks ? lane * per : blocks, b1 = b0 + per < blocks ? b0 + per : blocks;
    double v = 0.0;
#pragma unroll 16
    for (unsigned b = b0; b < b1; ++b) v += partial[static_cast<size_t>(b) * width + e];
    lane_sum[lane] = v;
    __syncthreads();
    if (lane == 0) {
        double t = 0.0;
        for (int l = 0; l < 64; ++l) t += lane_sum[l];
        row[e] = t / nodes;
    }
}

} // namespace fes
