// Host test of fusion-sim_amd/csrc/fes_diag_core.hpp (the rules of the energy diagnostics): the planes a handle reduces and
// where it holds them, the recording ring's indexing, drop count, commit and drain, the ranks' agreement on a drain, the
// ranks' integer sum, the fixed-order combination of rows.  Built with g++
// by tests/test_energy_host.py; prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fusion-sim_amd/csrc/fes_diag_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static void owned_planes()
{
    // undecomposed: every plane; ranks: nz / world each, together every plane once
    CHECK(fesdiag::owned_planes(64, 1, 0).k0 == 0 && fesdiag::owned_planes(64, 1, 0).nk == 64);
    for (int world : { 2, 3, 4, 8 }) {
        const int nz = 24 * world;
        std::vector<int> seen(nz, 0);
        for (int r = 0; r < world; ++r) {
            const fesdiag::Owned o = fesdiag::owned_planes(nz, world, r);
            CHECK(o.k0 == r * (nz / world) && o.nk == nz / world);
            for (int k = o.k0; k < o.k0 + o.nk; ++k) seen[k]++;
        }
        for (int k = 0; k < nz; ++k) CHECK(seen[k] == 1);
    }
    // whole-grid arrays (an undecomposed handle, a non-compact rank): every plane held where it is
    const fes::Held all{ 0, 32 };
    for (int r = 0; r < 4; ++r) CHECK(fesdiag::owned_are_held(fesdiag::owned_planes(32, 4, r), all, 32, true));
    // a compact rank holds z0 - H .. z0 + nzl + H: its owned planes sit at held index H .. H + nzl - 1, the plane above too
    for (int world : { 2, 4 }) {
        const int nz = 64, nzl = nz / world, H = 4;
        for (int r = 0; r < world; ++r) {
            const fesdiag::Owned o = fesdiag::owned_planes(nz, world, r);
            const fes::Held held{ ((o.k0 - H) % nz + nz) % nz, nzl + 2 * H + 1 };
            CHECK(fesdiag::owned_are_held(o, held, nz, true));
            for (int k = o.k0; k < o.k0 + o.nk; ++k) CHECK(fes::held_plane(k, held, nz) == H + (k - o.k0));
            // a slab without its upper halo cannot form the curl of its last plane
            const fes::Held tight{ o.k0, nzl };
            CHECK(fesdiag::owned_are_held(o, tight, nz, false));
            CHECK(!fesdiag::owned_are_held(o, tight, nz, true));
        }
    }
}

static void ring()
{
    fesdiag::Ring r;
    r.cap = 4;
    uint64_t first, n, dropped, slot[2], len[2];
    r.pending(first, n, dropped);
    CHECK(n == 0 && dropped == 0 && r.runs(first, n, slot, len) == 0);
    // 3 rows: slots 0..2, one run
    r.seq = 3;
    r.pending(first, n, dropped);
    CHECK(first == 0 && n == 3 && dropped == 0);
    CHECK(r.runs(first, n, slot, len) == 1 && slot[0] == 0 && len[0] == 3);
    r.drained = 3;
    // 10 rows in all, 7 since the drain: the newest 4 (rows 6..9 at slots 2, 3, 0, 1), 3 dropped
    r.seq = 10;
    r.pending(first, n, dropped);
    CHECK(first == 6 && n == 4 && dropped == 3);
    CHECK(r.runs(first, n, slot, len) == 2 && slot[0] == 2 && len[0] == 2 && slot[1] == 0 && len[1] == 2);
    for (uint64_t s = first; s < first + n; ++s) CHECK(r.slot(s) == s % 4);
    // from a fresh ring: 10 rows into 4 slots drop 6
    fesdiag::Ring q;
    q.cap = 4;
    q.seq = 10;
    q.pending(first, n, dropped);
    CHECK(first == 6 && n == 4 && dropped == 6);
    // exactly full: no wrap, nothing dropped
    q.seq = 4;
    q.pending(first, n, dropped);
    CHECK(first == 0 && n == 4 && dropped == 0 && q.runs(first, n, slot, len) == 1 && len[0] == 4);
    // commit and mark_drained: a recorder's life in a ring of 3 — 13 rows committed one at a time, each into slot(seq)
    fesdiag::Ring c;
    c.cap = 3;
    uint64_t held[3] = { 0, 0, 0 };
    for (uint64_t row = 1; row <= 13; ++row) {
        held[c.slot(c.seq)] = row;
        c.commit();
        CHECK(c.seq == row && c.drained == 0);
    }
    c.pending(first, n, dropped);
    CHECK(first == 10 && n == 3 && dropped == 10);
    CHECK(c.runs(first, n, slot, len) == 2 && slot[0] == 1 && len[0] == 2 && slot[1] == 0 && len[1] == 1);
    for (uint64_t i = 0; i < n; ++i) CHECK(held[c.slot(first + i)] == 11 + i);
    // a delivery that failed marks nothing: the same rows are pending again; after mark_drained none are
    c.pending(first, n, dropped);
    CHECK(first == 10 && n == 3 && dropped == 10);
    c.mark_drained();
    c.pending(first, n, dropped);
    CHECK(n == 0 && dropped == 0 && c.drained == 13);
    c.commit();
    c.pending(first, n, dropped);
    CHECK(first == 13 && n == 1 && dropped == 0 && c.slot(first) == 1);
}

static void agreement()
{
    // world 1: a rank agrees with itself
    const double one[2] = { 3, 10 };
    CHECK(fesdiag::disagreeing_rank(one, 1, 3, 10) == -1);
    CHECK(fesdiag::disagreeing_rank(one, 1, 0, 0) == 0);
    // world 3, all the same (zero rows too)
    const double same[6] = { 3, 10, 3, 10, 3, 10 }, none[6] = { 0, 0, 0, 0, 0, 0 };
    CHECK(fesdiag::disagreeing_rank(same, 3, 3, 10) == -1);
    CHECK(fesdiag::disagreeing_rank(none, 3, 0, 0) == -1);
    // a mismatch on the first rank, on the last rank, and the first of two
    const double first[6] = { 2, 10, 3, 10, 3, 10 }, last[6] = { 3, 10, 3, 10, 4, 10 }, two[6] = { 3, 10, 5, 10, 4, 10 };
    CHECK(fesdiag::disagreeing_rank(first, 3, 3, 10) == 0);
    CHECK(fesdiag::disagreeing_rank(last, 3, 3, 10) == 2);
    CHECK(fesdiag::disagreeing_rank(two, 3, 3, 10) == 1);
    // the same number of rows, another number dropped
    const double drop[6] = { 3, 10, 3, 9, 3, 10 };
    CHECK(fesdiag::disagreeing_rank(drop, 3, 3, 10) == 1);
    CHECK(fesdiag::disagreeing_rank(drop, 3, 3, 9) == 0);
}

static void word_sum()
{
    // three parts of four words: plain sums, a carry past 2^32, the top of the 64-bit range
    const uint64_t big = 0xFFFFFFFFull;
    const uint64_t parts[12] = { 1, big, 0, 1ull << 63,   2, 1, 0, (1ull << 63) - 1,   3, big, 0, 0 };
    uint64_t out[4] = { 99, 99, 99, 99 };   // (overwritten, not added to)
    fesdiag::add_words(parts, 4, 3, out);
    CHECK(out[0] == 6 && out[1] == 2 * big + 1 && out[1] == 0x1FFFFFFFFull && out[2] == 0 && out[3] == ~0ull);
    // one part: a copy
    fesdiag::add_words(parts, 4, 1, out);
    CHECK(out[0] == 1 && out[1] == big && out[2] == 0 && out[3] == 1ull << 63);
    // in chunks of 4 words with a final short chunk, as the ranks' gather delivers them: chunk c of rank r is [r][m] of
    // that chunk's block.  10 words of 3 ranks -> chunks of 4, 4, 2
    const size_t n = 10, chunk = 4;
    const int world = 3;
    std::vector<uint64_t> mine[3], want(n, 0), got(n, 7);
    for (int r = 0; r < world; ++r)
        for (size_t i = 0; i < n; ++i) {
            mine[r].push_back((big - 1) * (r + 1) + 1000 * i + r);
            want[i] += mine[r].back();
        }
    size_t chunks = 0;
    for (size_t at = 0; at < n; at += chunk, ++chunks) {
        const size_t m = std::min(chunk, n - at);
        std::vector<uint64_t> block;
        for (int r = 0; r < world; ++r) block.insert(block.end(), mine[r].begin() + at, mine[r].begin() + at + m);
        fesdiag::add_words(block.data(), m, world, got.data() + at);
    }
    CHECK(chunks == 3 && got == want && want[9] > (1ull << 32));
    // no words: nothing is touched
    fesdiag::add_words(parts, 0, 3, out);
    CHECK(out[0] == 1);
}

static void combine()
{
    std::vector<fpic_energy> rows(3);
    std::memset(rows.data(), 0, rows.size() * sizeof(fpic_energy));
    for (int p = 0; p < 3; ++p) {
        fpic_energy& e = rows[p];
        e.substep = 42;
        e.nspecies = 2;
        e.field_e = 1.0 + p;
        e.field_b = p == 1 ? 1e-17 : 1.0;
        e.field_b_external = 0.25;
        for (int s = 0; s < 2; ++s) {
            e.count[s] = 10 * (p + 1) + s;
            e.kinetic[s] = 0.1 * (p + 1);
            e.momentum[s][0] = p == 2 ? -1.0 : 0.5;
            e.momentum[s][1] = 1e16;
            e.momentum[s][2] = p;
            e.speed_max[s] = p == 1 ? 0.9 : 0.1 * s;
        }
    }
    fpic_energy out;
    fesdiag::combine(rows.data(), 1, 3, &out);
    CHECK(out.substep == 42 && out.nspecies == 2);
    CHECK(out.count[0] == 60 && out.count[1] == 63 && out.count[2] == 0);
    CHECK(out.speed_max[0] == 0.9 && out.speed_max[1] == 0.9);
    // left to right, in double: (1 + 1e-17) + 1 is 2 (the middle term is lost), not 1 + (1e-17 + 1)
    volatile double b = 1.0;
    b = b + 1e-17;
    b = b + 1.0;
    CHECK(out.field_b == b);
    CHECK(out.field_e == 6.0 && out.field_b_external == 0.75);
    CHECK(out.momentum[0][0] == 0.0 && out.momentum[1][2] == 3.0);
    // a stride: rows of two sub-steps of two ranks, [rank][row]; row 1 combines elements 1 and 3
    std::vector<fpic_energy> block(4);
    std::memset(block.data(), 0, block.size() * sizeof(fpic_energy));
    for (int i = 0; i < 4; ++i) { block[i].substep = 3 * (i % 2 + 1); block[i].field_e = i; block[i].count[0] = 1u << i; }
    fesdiag::combine(block.data() + 1, 2, 2, &out);
    CHECK(out.substep == 6 && out.field_e == 4.0 && out.count[0] == 10);
    // a species with a NaN speed_max on one rank (a non-finite velocity) stays NaN, wherever that rank is; +inf stays +inf
    for (int at = 0; at < 3; ++at) {
        std::vector<fpic_energy> r3(rows);
        r3[at].speed_max[0] = std::nan("");
        r3[at].speed_max[1] = HUGE_VAL;
        fesdiag::combine(r3.data(), 1, 3, &out);
        CHECK(std::isnan(out.speed_max[0]) && out.speed_max[1] == HUGE_VAL);
    }
}

int main()
{
    owned_planes();
    ring();
    agreement();
    word_sum();
    combine();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
