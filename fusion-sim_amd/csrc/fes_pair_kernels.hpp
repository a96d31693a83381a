// fes_pair_kernels.hpp — the passes of the binary Coulomb collision operator of a CART3D handle (fpic_pair; host side
// fes_pair.inc.hpp, the rule fes_pair_core.hpp).  The bin tables cannot serve this pass — an in-place push leaves particles
// in the slots of tiles they have left — so it builds a cell index of its own, per species:
//   pair_count_kernel<T>    streams the three position arrays; per live particle the deposit's cell (axis(), as the deposit
//       and fpic_moments) and one 32-bit atomic add on the cell's count.  Fixed grid, grid-stride.
//   pair_count_lds_kernel<T>   the same counts with a workgroup's adds privatised in LDS per tile: turns of 2048 consecutive
//       slots, a table of the cells of the tile of the turn's first slot, one global atomic per cell that was hit.  The form
//       the host uses (DESIGN 4.17 has the measurement); the plain one serves a tile larger than the table.
//   pair_scan_kernel        the exclusive scan of the counts in place: load_scan_kernel's form (one workgroup, a carry from
//       turn to turn), but a lane takes kPairScanPer = 16 consecutive counts with 16-byte loads and scans them in registers,
//       so a turn covers 16384 cells between its three barriers, not 1024 (256^3 cells: 1024 turns).
//   pair_fill_kernel<T>, pair_fill_lds_kernel<T>   the same stream; the particle's slot goes to index[cursor++] of its cell (the
//       scanned count is the cursor: afterwards it is the END of the cell's segment, and the word before it the beginning).
//       The LDS form gives the particles of the turn's tile their places inside the turn from the table and reserves a cell's
//       run with one global atomic.  The order inside a segment is arbitrary.
//   pair_walk<LIKE>   the walk over the index that this pass, the fusion tally, the fusion spectrum and the burn's deciding
//       pass share (PairHead: the head of their arguments; PairRun: the run's tables in LDS).  A workgroup takes chunks of
//       kPairChunk consecutive cells (fixed grid, grid-stride) and cuts each into runs of cells whose entries, both species
//       together, fit kPairEntries places of LDS.  It loads (key, id, slot) per entry, sorts every cell's segment in
//       (key, id) — up to kPairRankMax = 64 entries by counting the entries before each, longer ones by a bitonic network
//       (pair_bitonic) —, and hands the run to the pass's body.
//   pair_collide_kernel<T, LIKE>   per run one lane to every `few` particle (unlike species) or to every pair / triple (like
//       species).  The lane walks its chain sequentially with its own particle in registers and casts both velocities to T
//       after every pair; inside a cell no two lanes touch the same particle, so there are no atomics on velocities and no
//       barrier between rounds.  Only velocities that changed are stored.
// A cell with more than kPairCellMax = 2048 particles of either species is not collided and counted as overfull: two full
// species of a cell are the kPairEntries = 4096 places, 14 bytes each (the unsorted triple, and 16 bits for the place of the
// entry that is sorted to here) = 56.5 KiB with the run's tables: two workgroups on a CU's 160 KiB.
// The counts (pairs, strong, cells, overfull_cells, overfull_particles) are kept per lane, reduced over the wave and the
// workgroup, and added to the device words with one 64-bit atomic per workgroup and count (collide_counts).  No scratch.
#pragma once

#include "fes_collide_kernels.hpp"
#include "fes_kernels.hpp"
#include "fes_pair_core.hpp"

namespace fes {

constexpr int kPairThreads = 256;
constexpr int kPairBlocks = 2048;          // the index passes: the loader's shape
constexpr int kPairCollideBlocks = 512;    // the pairing pass: two workgroups of 56.5 KiB per CU of the 256
constexpr int kPairCellMax = 2048;         // particles of one species a cell may hold and still be collided
constexpr int kPairEntries = 2 * kPairCellMax;   // the entries of a run, both species together
constexpr int kPairChunk = 64;             // consecutive cells a workgroup claims at a time: one wave plans the runs
constexpr int kPairRankMax = 64;           // a cell's segment up to one wave's worth is ranked by counting, a longer one by the network
constexpr int kPairCounts = 5;
constexpr size_t kPairLdsBytes = (3 * static_cast<size_t>(kPairEntries) + 2 * (kPairChunk + 1) + 2) * sizeof(uint32_t) + kPairEntries * sizeof(uint16_t);
static_assert(kPairCellMax == FPIC_PAIR_CELL_MAX, "the header states the cap");
static_assert(kPairThreads == kCollideThreads, "collide_counts reduces a workgroup of kCollideThreads");
static_assert(kPairLdsBytes <= 64 * 1024 && kPairEntries <= 65536, "two workgroups per CU; a place fits 16 bits");

template <typename T>
struct PairIndexArgs {
    const T* slab;            // x, y, z, ...: arrays of n_pad
    size_t n_pad, n;          // the slots [0, n)
    int nx, ny, nz;
    int ltx, lty, ltz;        // log2 of the tile edges (pair_count_lds_kernel)
    uint32_t* cell;           // per cell: the count (pair_count_kernel), the cursor (pair_fill_kernel)
    uint32_t* index;          // the slots by cell
};

// the deposit's cell (i, j, k) of slot s; false: the stored position is no number of [0, 1)
template <typename T>
__device__ __forceinline__ bool pair_ijk(const PairIndexArgs<T>& a, size_t s, int& i, int& j, int& k)
{
    int w;
    axis(a.slab[s], a.nx, i, w);
    axis(a.slab[a.n_pad + s], a.ny, j, w);
    axis(a.slab[2 * a.n_pad + s], a.nz, k, w);
    return static_cast<unsigned>(i) < static_cast<unsigned>(a.nx) && static_cast<unsigned>(j) < static_cast<unsigned>(a.ny) &&
           static_cast<unsigned>(k) < static_cast<unsigned>(a.nz);
}
// the cell's number in the grid
template <typename T>
__device__ __forceinline__ uint32_t pair_cell_at(const PairIndexArgs<T>& a, uint32_t i, uint32_t j, uint32_t k)
{
    return i + static_cast<uint32_t>(a.nx) * (j + static_cast<uint32_t>(a.ny) * k);
}
template <typename T>
__device__ __forceinline__ bool pair_cell_of(const PairIndexArgs<T>& a, size_t s, uint32_t& c)
{
    int i, j, k;
    if (!pair_ijk(a, s, i, j, k)) return false;
    c = pair_cell_at(a, i, j, k);
    return true;
}
// lane 0 of the workgroup: the origin of the tile of the turn's first slot (-1: that slot holds no position of the box)
template <typename T>
__device__ __forceinline__ void pair_tile_origin(const PairIndexArgs<T>& a, size_t base, int mx, int my, int mz, int (&origin)[3])
{
    if (threadIdx.x != 0) return;
    int i, j, k;
    const bool ok = pair_ijk(a, base, i, j, k);
    origin[0] = ok ? i & ~mx : -1; origin[1] = ok ? j & ~my : -1; origin[2] = ok ? k & ~mz : -1;
}

template <typename T>
__global__ __launch_bounds__(kPairThreads) void pair_count_kernel(PairIndexArgs<T> a)
{
    const size_t stride = static_cast<size_t>(gridDim.x) * kPairThreads;
    for (size_t s = static_cast<size_t>(blockIdx.x) * kPairThreads + threadIdx.x; s < a.n; s += stride) {
        uint32_t c;
        if (pair_cell_of(a, s, c)) atomicAdd(a.cell + c, 1u);
    }
}

// The count with a workgroup's adds privatised in LDS: a turn takes kPairCountTurn consecutive slots, which in a binned species
// lie in one tile; the particles of the tile of the turn's first slot add to a table of the tile's cells in LDS, which is
// then flushed with one global atomic per cell that was hit; every other particle adds globally as pair_count_kernel does.
constexpr int kPairCountTurn = 2048;
constexpr int kPairTileCellsMax = 2048;    // 16 x 16 x 8 cells (electrostatic), 8 x 8 x 8 (full EM)
template <typename T>
__global__ __launch_bounds__(kPairThreads) void pair_count_lds_kernel(PairIndexArgs<T> a)
{
    __shared__ uint32_t table[kPairTileCellsMax];
    __shared__ int origin[3];
    const uint32_t tcells = 1u << (a.ltx + a.lty + a.ltz);
    const int mx = (1 << a.ltx) - 1, my = (1 << a.lty) - 1, mz = (1 << a.ltz) - 1;
    for (size_t base = static_cast<size_t>(blockIdx.x) * kPairCountTurn; base < a.n; base += static_cast<size_t>(gridDim.x) * kPairCountTurn) {
        for (uint32_t t = threadIdx.x; t < tcells; t += kPairThreads) table[t] = 0;
        pair_tile_origin(a, base, mx, my, mz, origin);
        __syncthreads();
        const int ox = origin[0], oy = origin[1], oz = origin[2];
#pragma unroll
        for (int q = 0; q < kPairCountTurn / kPairThreads; ++q) {
            const size_t s = base + static_cast<size_t>(q) * kPairThreads + threadIdx.x;
            int i, j, k;
            if (s >= a.n || !pair_ijk(a, s, i, j, k)) continue;
            if ((i & ~mx) == ox && (j & ~my) == oy && (k & ~mz) == oz)
                atomicAdd(&table[(i & mx) | ((j & my) << a.ltx) | ((k & mz) << (a.ltx + a.lty))], 1u);
            else
                atomicAdd(a.cell + pair_cell_at(a, i, j, k), 1u);
        }
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < tcells; t += kPairThreads) {
            const uint32_t c = table[t];
            if (!c) continue;     // (a cell that was hit lies inside the grid: a particle was there)
            const uint32_t i = ox + (t & mx), j = oy + ((t >> a.ltx) & my), k = oz + (t >> (a.ltx + a.lty));
            atomicAdd(a.cell + pair_cell_at(a, i, j, k), c);
        }
        __syncthreads();   // (the table is zeroed by the next turn)
    }
}

template <typename T>
__global__ __launch_bounds__(kPairThreads) void pair_fill_kernel(PairIndexArgs<T> a)
{
    const size_t stride = static_cast<size_t>(gridDim.x) * kPairThreads;
    for (size_t s = static_cast<size_t>(blockIdx.x) * kPairThreads + threadIdx.x; s < a.n; s += stride) {
        uint32_t c;
        if (pair_cell_of(a, s, c)) a.index[atomicAdd(a.cell + c, 1u)] = static_cast<uint32_t>(s);   // (below n: the counts' sum)
    }
}

constexpr int kPairScanPer = 16;           // counts a lane of pair_scan_kernel scans in registers

// counts[0 .. n) -> their exclusive prefix sums in place (below 2^32: the particles of a species); counts is 16-byte aligned
__global__ __launch_bounds__(1024) void pair_scan_kernel(uint32_t* __restrict__ counts, size_t n)
{
    __shared__ unsigned long long wave_sum[16];
    __shared__ unsigned long long carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (size_t at = 0; at < n; at += static_cast<size_t>(1024) * kPairScanPer) {
        const size_t k0 = at + static_cast<size_t>(kPairScanPer) * threadIdx.x;
        const bool whole = k0 + kPairScanPer <= n;
        uint32_t v[kPairScanPer];
        if (whole) {
#pragma unroll
            for (int q = 0; q < kPairScanPer / 4; ++q) {
                const uint4 t = *reinterpret_cast<const uint4*>(counts + k0 + 4 * q);
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kPairScanPer; ++j) v[j] = k0 + j < n ? counts[k0 + j] : 0u;
        }
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < kPairScanPer; ++j) mine += v[j];
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
        uint32_t run = static_cast<uint32_t>(before + inc - mine);
#pragma unroll
        for (int j = 0; j < kPairScanPer; ++j) {
            const uint32_t t = v[j];
            v[j] = run;
            run += t;
        }
        if (whole) {
#pragma unroll
            for (int q = 0; q < kPairScanPer / 4; ++q)
                *reinterpret_cast<uint4*>(counts + k0 + 4 * q) = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < kPairScanPer; ++j)
                if (k0 + j < n) counts[k0 + j] = v[j];
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + inc;
        __syncthreads();
    }
}

// The fill privatised the same way: the particles of the turn's tile take their places inside the turn from a table in LDS,
// every cell that was hit then reserves its run of the cell's segment with one global atomic, and the slots are written
// behind that base.  The order inside a segment stays arbitrary.
template <typename T>
__global__ __launch_bounds__(kPairThreads) void pair_fill_lds_kernel(PairIndexArgs<T> a)
{
    __shared__ uint32_t table[kPairTileCellsMax], first[kPairTileCellsMax];
    __shared__ int origin[3];
    constexpr int kPer = kPairCountTurn / kPairThreads;
    const uint32_t tcells = 1u << (a.ltx + a.lty + a.ltz);
    const int mx = (1 << a.ltx) - 1, my = (1 << a.lty) - 1, mz = (1 << a.ltz) - 1;
    for (size_t base = static_cast<size_t>(blockIdx.x) * kPairCountTurn; base < a.n; base += static_cast<size_t>(gridDim.x) * kPairCountTurn) {
        for (uint32_t t = threadIdx.x; t < tcells; t += kPairThreads) table[t] = 0;
        pair_tile_origin(a, base, mx, my, mz, origin);
        __syncthreads();
        const int ox = origin[0], oy = origin[1], oz = origin[2];
        uint32_t where[kPer], place[kPer];      // the cell within the tile (~0: none) and the place inside the turn
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const size_t s = base + static_cast<size_t>(q) * kPairThreads + threadIdx.x;
            int i, j, k;
            where[q] = ~0u;
            place[q] = 0;
            if (s >= a.n || !pair_ijk(a, s, i, j, k)) continue;
            if ((i & ~mx) == ox && (j & ~my) == oy && (k & ~mz) == oz) {
                where[q] = (i & mx) | ((j & my) << a.ltx) | ((k & mz) << (a.ltx + a.lty));
                place[q] = atomicAdd(&table[where[q]], 1u);
            } else {
                const uint32_t c = pair_cell_at(a, i, j, k);
                a.index[atomicAdd(a.cell + c, 1u)] = static_cast<uint32_t>(s);
            }
        }
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < tcells; t += kPairThreads) {
            const uint32_t c = table[t];
            if (!c) continue;
            const uint32_t i = ox + (t & mx), j = oy + ((t >> a.ltx) & my), k = oz + (t >> (a.ltx + a.lty));
            first[t] = atomicAdd(a.cell + pair_cell_at(a, i, j, k), c);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q)
            if (where[q] != ~0u) a.index[first[where[q]] + place[q]] = static_cast<uint32_t>(base + static_cast<size_t>(q) * kPairThreads + threadIdx.x);
        __syncthreads();   // (the tables are rewritten by the next turn)
    }
}

// The head of the arguments of every pass that walks the cell index (pair_walk); S is T where the pass writes velocities,
// const T where it only reads them.  pair_head (fes_pair.inc.hpp) fills it.
template <typename S>
struct PairHead {
    S *slab_a, *slab_b;               // six arrays of n_pad each; like species: b = a
    const uint32_t *id_a, *id_b;      // nullptr: slot = id
    size_t n_pad_a, n_pad_b;
    const uint32_t *seg_a, *seg_b;    // cells + 1 words: cell c is index[seg[c] .. seg[c + 1])
    const uint32_t *index_a, *index_b;
    uint32_t ncells;
    uint32_t rank_max;                // a segment of more entries is sorted by the bitonic network, not by counting
};

template <typename T>
struct PairArgs : PairHead<T> {
    unsigned long long* counts;       // pairs, strong, cells, overfull_cells, overfull_particles
    fespair::Rule r;
};

template <typename T>
__device__ __forceinline__ void pair_load(const T* slab, size_t n_pad, uint32_t slot, double (&v)[3])
{
    const T* p = slab + 3 * n_pad + slot;
    v[0] = static_cast<double>(p[0]);
    v[1] = static_cast<double>(p[n_pad]);
    v[2] = static_cast<double>(p[2 * n_pad]);
}
template <typename T>
__device__ __forceinline__ void pair_store(T* slab, size_t n_pad, uint32_t slot, const double (&v)[3])
{
    T* p = slab + 3 * n_pad + slot;
    p[0] = static_cast<T>(v[0]);
    p[n_pad] = static_cast<T>(v[1]);
    p[2 * n_pad] = static_cast<T>(v[2]);
}

// the cell of the run whose segment holds the place `local`: the largest l of [0, len) with seg[l] <= local
__device__ __forceinline__ uint32_t pair_segment_of(const uint32_t* seg, uint32_t len, uint32_t local)
{
    uint32_t lo = 0, hi = len;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg[mid] <= local) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The segment sorted[lo .. lo + n) of entry places -> ascending in (key, id): a bitonic network whose every exchange puts the
// smaller entry at the lower place (the first step of a merge pairs a place with its mirror in the block), so places beyond n
// count as +inf and n need not be a power of two.  Every lane of the workgroup calls it; a barrier ends each step.
__device__ __forceinline__ void pair_bitonic(uint16_t* sorted, const uint32_t* st_key, const uint32_t* st_id, uint32_t lo, uint32_t n)
{
    uint32_t p2 = 1;
    while (p2 < n) p2 <<= 1;
    for (uint32_t k = 2; k <= p2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t flip = j == (k >> 1) ? k - 1 : j;
            for (uint32_t i = threadIdx.x; i < n; i += kPairThreads) {
                const uint32_t l = i ^ flip;
                if (l > i && l < n) {
                    const uint16_t x = sorted[lo + i], y = sorted[lo + l];
                    if (fespair::before(st_key[y], st_id[y], st_key[x], st_id[x])) {
                        sorted[lo + i] = y;
                        sorted[lo + l] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// The tables of a run, kPairLdsBytes of LDS from `base` on (4-byte aligned).  A kernel's own LDS lies in front of or behind them.
struct PairRun {
    uint32_t *st_key, *st_id, *st_slot;   // [kPairEntries] the entries as loaded: species a's of the run, then species b's
    uint32_t *seg_a, *seg_b;              // [len + 1] the segments of the run's cells, from 0
    uint32_t* plan;                       // [0]: the cells of the run
    uint16_t* sorted;                     // [kPairEntries] the entries' places, sorted inside their cells' segments
    __device__ __forceinline__ explicit PairRun(void* base)
        : st_key(static_cast<uint32_t*>(base)), st_id(st_key + kPairEntries), st_slot(st_id + kPairEntries), seg_a(st_slot + kPairEntries),
          seg_b(seg_a + (kPairChunk + 1)), plan(seg_b + (kPairChunk + 1)), sorted(reinterpret_cast<uint16_t*>(plan + 2))
    {
    }
};

// The walk every pairing pass shares (pair_collide_kernel, fusion_tally_kernel, fusion_spectrum_kernel, burn_decide_kernel):
// a workgroup takes the chunks blockIdx.x, blockIdx.x + gridDim.x, ... of kPairChunk consecutive cells and cuts each into
// runs of cells that are not overfull and whose entries, both species together, fit kPairEntries places.  Per run it copies
// the segment tables to LDS, loads (key_of(id), id, slot) per entry, sorts every cell's segment in (key, id) and calls
// body(c0, len, na, nb, total) — the run is the cells [c0, c0 + len) with na + nb = total entries — between two barriers.
// A first cell that is overfull is skipped and reported: overfull(its particles), on lane 0 of the workgroup alone.
// EVERY lane of the workgroup calls it, and body runs on every lane: it may hold barriers of its own.
template <bool LIKE, typename S, typename Key, typename Overfull, typename Body>
__device__ __forceinline__ void pair_walk(const PairHead<S>& g, const PairRun& t, Key key_of, Overfull overfull, Body body)
{
    const uint32_t nchunks = (g.ncells + kPairChunk - 1) / kPairChunk;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        uint32_t c0 = chunk * kPairChunk;
        const uint32_t cend = min(c0 + static_cast<uint32_t>(kPairChunk), g.ncells);
        while (c0 < cend) {
            // the run [c0, c0 + len): the cells from c0 on that are not overfull and fit the LDS together (wave 0 decides)
            if (threadIdx.x < 64) {
                const uint32_t c = c0 + threadIdx.x;
                bool ok = false;
                uint32_t na = 0, nb = 0;
                if (c < cend) {
                    const uint32_t ae = g.seg_a[c + 1];
                    na = ae - g.seg_a[c];
                    unsigned long long tot = ae - g.seg_a[c0];
                    if (!LIKE) {
                        const uint32_t be = g.seg_b[c + 1];
                        nb = be - g.seg_b[c];
                        tot += be - g.seg_b[c0];
                    }
                    ok = na <= static_cast<uint32_t>(kPairCellMax) && nb <= static_cast<uint32_t>(kPairCellMax) && tot <= static_cast<unsigned long long>(kPairEntries);
                }
                const unsigned long long fits = __ballot(ok);
                const uint32_t len = fits == ~0ull ? 64u : static_cast<uint32_t>(__ffsll(~fits)) - 1u;
                if (threadIdx.x == 0) {
                    t.plan[0] = len;
                    if (len == 0) overfull(static_cast<unsigned long long>(na) + nb);   // (a cell that is not overfull fits alone: c0 is overfull)
                }
            }
            __syncthreads();
            const uint32_t len = t.plan[0];
            if (len == 0) {
                c0 += 1;
                __syncthreads();   // (plan is rewritten by the next turn)
                continue;
            }
            const uint32_t a0 = g.seg_a[c0], b0 = LIKE ? 0u : g.seg_b[c0];
            if (threadIdx.x <= len) {
                t.seg_a[threadIdx.x] = g.seg_a[c0 + threadIdx.x] - a0;
                if (!LIKE) t.seg_b[threadIdx.x] = g.seg_b[c0 + threadIdx.x] - b0;
            }
            __syncthreads();
            const uint32_t na = t.seg_a[len], nb = LIKE ? 0u : t.seg_b[len], total = na + nb;   // (total <= kPairEntries)
            for (uint32_t e = threadIdx.x; e < total; e += kPairThreads) {
                const bool isb = !LIKE && e >= na;
                const uint32_t slot = isb ? g.index_b[b0 + (e - na)] : g.index_a[a0 + e];
                const uint32_t* ids = isb ? g.id_b : g.id_a;
                const uint32_t id = ids ? ids[slot] : slot;
                t.st_key[e] = key_of(id);
                t.st_id[e] = id;
                t.st_slot[e] = slot;
            }
            __syncthreads();
            // the sort: an entry's place in its cell's segment is the number of entries of the segment before it
            for (uint32_t e = threadIdx.x; e < total; e += kPairThreads) {
                const bool isb = !LIKE && e >= na;
                const uint32_t base = isb ? na : 0u;
                const uint32_t* seg = isb ? t.seg_b : t.seg_a;
                const uint32_t l = pair_segment_of(seg, len, e - base);
                const uint32_t lo = base + seg[l], hi = base + seg[l + 1];
                if (hi - lo > g.rank_max) {        // (the network below sorts this segment)
                    t.sorted[e] = static_cast<uint16_t>(e);
                    continue;
                }
                const uint32_t key = t.st_key[e], id = t.st_id[e];
                uint32_t rank = 0;
                for (uint32_t j = lo; j < hi; ++j) rank += fespair::before(t.st_key[j], t.st_id[j], key, id) ? 1u : 0u;
                t.sorted[lo + rank] = static_cast<uint16_t>(e);
            }
            __syncthreads();
            for (uint32_t l = 0; l < len; ++l) {   // (the same segments for every lane: the tables are in LDS)
                if (t.seg_a[l + 1] - t.seg_a[l] > g.rank_max) pair_bitonic(t.sorted, t.st_key, t.st_id, t.seg_a[l], t.seg_a[l + 1] - t.seg_a[l]);
                if (!LIKE && t.seg_b[l + 1] - t.seg_b[l] > g.rank_max) pair_bitonic(t.sorted, t.st_key, t.st_id, na + t.seg_b[l], t.seg_b[l + 1] - t.seg_b[l]);
            }
            body(c0, len, na, nb, total);
            __syncthreads();   // (the run's tables are rewritten by the next)
            c0 += len;
        }
    }
}

template <typename T, bool LIKE>
__global__ __launch_bounds__(kPairThreads) void pair_collide_kernel(PairArgs<T> g)
{
    extern __shared__ uint32_t pair_lds[];
    const PairRun t(pair_lds);
    uint32_t *const st_id = t.st_id, *const st_slot = t.st_slot, *const seg_a = t.seg_a, *const seg_b = t.seg_b;
    uint16_t* const sorted = t.sorted;
    unsigned long long count[kPairCounts] = { 0, 0, 0, 0, 0 };
    pair_walk<LIKE>(
        g, t, [&](uint32_t id) { return fespair::key_of(g.r, id); },
        [&](unsigned long long particles) {
            count[3] += 1;
            count[4] += particles;
        },
        [&](uint32_t, uint32_t len, uint32_t na, uint32_t, uint32_t total) {
            for (uint32_t e = threadIdx.x; e < total; e += kPairThreads) {
                if (LIKE) {
                    const uint32_t l = pair_segment_of(seg_a, len, e);
                    const uint32_t lo = seg_a[l], n = seg_a[l + 1] - lo, q = e - lo;
                    const int lead = fespair::like_lead(n, q);
                    if (lead == fespair::kNothing) continue;
                    if (q == 0) count[2] += 1;
                    const double nl = fespair::like_nl(n, lead);
                    const uint32_t e0 = sorted[e], e1 = sorted[e + 1];
                    const uint32_t i0 = st_id[e0], i1 = st_id[e1], s0 = st_slot[e0], s1 = st_slot[e1];
                    double v0[3], v1[3];
                    pair_load(g.slab_a, g.n_pad_a, s0, v0);
                    pair_load(g.slab_a, g.n_pad_a, s1, v1);
                    if (lead == fespair::kPairLead) {
                        const int what = fespair::collide(g.r, i0, nl, g.r.fa, g.r.fa, v0, v1);
                        if (what & fespair::kCounted) {
                            count[0] += 1;
                            count[1] += what & fespair::kStrong ? 1 : 0;
                            pair_store(g.slab_a, g.n_pad_a, s0, v0);   // (the store is the cast to T)
                            pair_store(g.slab_a, g.n_pad_a, s1, v1);
                        }
                    } else {
                        const uint32_t e2 = sorted[e + 2];
                        const uint32_t i2 = st_id[e2], s2 = st_slot[e2];
                        double v2[3];
                        pair_load(g.slab_a, g.n_pad_a, s2, v2);
                        const int w01 = fespair::collide(g.r, i0, nl, g.r.fa, g.r.fa, v0, v1);
                        if (w01) { fespair::settle<T>(v0); fespair::settle<T>(v1); }
                        const int w12 = fespair::collide(g.r, i1, nl, g.r.fa, g.r.fa, v1, v2);
                        if (w12) { fespair::settle<T>(v1); fespair::settle<T>(v2); }
                        const int w20 = fespair::collide(g.r, i2, nl, g.r.fa, g.r.fa, v2, v0);
                        count[0] += (w01 & 1) + (w12 & 1) + (w20 & 1);
                        count[1] += ((w01 >> 1) & 1) + ((w12 >> 1) & 1) + ((w20 >> 1) & 1);
                        if (w01 | w20) pair_store(g.slab_a, g.n_pad_a, s0, v0);
                        if (w01 | w12) pair_store(g.slab_a, g.n_pad_a, s1, v1);
                        if (w12 | w20) pair_store(g.slab_a, g.n_pad_a, s2, v2);
                    }
                } else {
                    const bool isb = e >= na;
                    const uint32_t local = isb ? e - na : e;
                    const uint32_t l = pair_segment_of(isb ? seg_b : seg_a, len, local);
                    const uint32_t alo = seg_a[l], blo = seg_b[l];
                    const uint32_t ca = seg_a[l + 1] - alo, cb = seg_b[l + 1] - blo;
                    const bool a_many = fespair::many_is_a(ca, cb);
                    if (isb != a_many) continue;           // (this entry is of the `many` species: its lane is its partner's)
                    const uint32_t nf = a_many ? cb : ca, nm = a_many ? ca : cb;
                    const uint32_t q = local - (isb ? blo : alo);
                    if (q == 0) count[2] += 1;
                    T* slab_f = isb ? g.slab_b : g.slab_a;
                    T* slab_m = isb ? g.slab_a : g.slab_b;
                    const size_t pad_f = isb ? g.n_pad_b : g.n_pad_a, pad_m = isb ? g.n_pad_a : g.n_pad_b;
                    const double fo = a_many ? g.r.fa : g.r.fb, fp = a_many ? g.r.fb : g.r.fa, nl = static_cast<double>(nf);
                    const uint32_t many0 = a_many ? alo : na + blo;
                    const uint32_t sf = st_slot[sorted[e]];
                    double vf[3];
                    pair_load(slab_f, pad_f, sf, vf);
                    bool changed = false;
                    for (uint32_t j = q; j < nm; j += nf) {
                        const uint32_t em = sorted[many0 + j];
                        const uint32_t im = st_id[em], sm = st_slot[em];
                        double vm[3];
                        pair_load(slab_m, pad_m, sm, vm);
                        const int what = fespair::collide(g.r, im, nl, fo, fp, vm, vf);
                        if (what & fespair::kCounted) {
                            count[0] += 1;
                            count[1] += what & fespair::kStrong ? 1 : 0;
                            pair_store(slab_m, pad_m, sm, vm);
                            fespair::settle<T>(vf);
                            changed = true;
                        }
                    }
                    if (changed) pair_store(slab_f, pad_f, sf, vf);
                }
            }
        });
    collide_counts<kPairCounts>(count, g.counts);
}

} // namespace fes
