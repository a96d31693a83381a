// Host test of fusion-sim_amd/csrc/fes_series_core.hpp (the host rules of the series diagnostic): every refusal of a request,
// the wrapped coordinate of a point, the sorted tables and the bitmap filter of the tracers (a member is never missed, over
// random id sets of 1 .. 65536 ids; the filter's size and load), the owner of a point's plane, the selection by flag of the
// ranks' rows (bits kept, zeros where nobody reports, two flags reported), and the ring the recorder reuses.  Built with g++
// -ffp-contract=off by tests/test_series_host.py; prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <string>

#include "../../fusion-sim_amd/csrc/fes_series_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static bool refused(const fpic_series_spec& s, int nspecies, const uint64_t* counts, const char* with)
{
    const char* why = fesser::check(s, nspecies, counts);
    return why && std::strncmp(why, with, std::strlen(with)) == 0;
}

static void checks()
{
    const double pts[6] = { 0.0, 1.0, -2.0, 1e30, 0.5, 0.25 };
    const int32_t sp[4] = { 0, 1, 1, 0 };
    const uint32_t id[4] = { 5, 5, 6, 9 };
    const uint64_t counts[2] = { 10, 7 };
    fpic_series_spec s{};
    CHECK(refused(s, 2, counts, ".points <- points and tracers are both empty"));
    s.npoints = 2; s.points = pts;
    CHECK(fesser::check(s, 2, counts) == nullptr);
    s.ntracers = 4; s.tracer_species = sp; s.tracer_id = id;
    CHECK(fesser::check(s, 2, counts) == nullptr);
    CHECK(fesser::check(s, 2, nullptr) == nullptr);
    s.npoints = FPIC_SERIES_MAX_POINTS + 1;
    CHECK(refused(s, 2, counts, ".points <- more than"));
    s.npoints = 2; s.points = nullptr;
    CHECK(refused(s, 2, counts, ".points <- Non-optional"));
    s.points = pts; s.tracer_id = nullptr;
    CHECK(refused(s, 2, counts, ".tracers <- Non-optional"));
    s.tracer_id = id; s.tracer_species = nullptr;
    CHECK(refused(s, 2, counts, ".tracers <- Non-optional"));
    s.tracer_species = sp; s.ntracers = FPIC_SERIES_MAX_TRACERS + 1;
    CHECK(refused(s, 2, counts, ".tracers <- more than"));
    s.ntracers = 4;
    const double bad[6] = { 0, 0, 0, 0, std::numeric_limits<double>::quiet_NaN(), 0 };
    s.points = bad;
    CHECK(refused(s, 2, counts, ".points <- must be finite"));
    const double inf[6] = { 0, 0, 0, 0, 0, -std::numeric_limits<double>::infinity() };
    s.points = inf;
    CHECK(refused(s, 2, counts, ".points <- must be finite"));
    s.points = pts;
    CHECK(refused(s, 1, counts, ".tracers <- no such species"));
    const int32_t neg[4] = { 0, -1, 1, 0 };
    s.tracer_species = neg;
    CHECK(refused(s, 2, counts, ".tracers <- no such species"));
    s.tracer_species = sp;
    const uint64_t few[2] = { 9, 7 };                   // id 9 of species 0 is not below its count
    CHECK(refused(s, 2, few, ".tracers <- an id is not below"));
    CHECK(fesser::check(s, 2, nullptr) == nullptr);     // a decomposed rank does not know the total
    const uint32_t dup[4] = { 5, 5, 6, 5 };             // (0, 5) twice; (1, 5) is another particle
    s.tracer_id = dup;
    CHECK(refused(s, 2, counts, ".tracers <- the same (species, id) twice"));
    s.tracer_id = id;
    s.reserved[2] = 1.0;
    CHECK(refused(s, 2, counts, ".reserved <- must be zero"));
    s.reserved[2] = 0.0;
    s.npoints = 0; s.points = nullptr;                  // tracers alone
    CHECK(fesser::check(s, 2, counts) == nullptr);
}

static void units()
{
    CHECK(fesser::unit_of(0.0, 2.0) == 0.0 && fesser::unit_of(2.0, 2.0) == 0.0 && fesser::unit_of(-2.0, 2.0) == 0.0);
    CHECK(fesser::unit_of(0.5, 2.0) == 0.25 && fesser::unit_of(4.5, 2.0) == 0.25 && fesser::unit_of(-3.5, 2.0) == 0.25);
    CHECK(fesser::unit_of(-1e-300, 1.0) == 0.0);        // (1 - 1e-300 rounds to 1: not < 1, so 0)
    CHECK(fesser::unit_of(-0.0, 1.0) == 0.0);
    std::mt19937_64 rng(1);
    std::uniform_real_distribution<double> d(-50.0, 50.0);
    for (int k = 0; k < 100000; ++k) {
        const double u = fesser::unit_of(d(rng), 0.37);
        CHECK(u >= 0.0 && u < 1.0);
    }
}

static void tables()
{
    std::mt19937_64 rng(7);
    const uint32_t sizes[] = { 1, 2, 3, 16, 100, 127, 128, 129, 4096, 30000, 65535, 65536 };
    for (uint32_t m : sizes) {
        // m distinct (species, id) pairs over three species: ids dense near zero, sparse over all of uint32, and clustered high
        std::set<uint64_t> keys;
        while (keys.size() < m) {
            const int sp = static_cast<int>(rng() % 3);
            const uint32_t id = sp == 0 ? static_cast<uint32_t>(rng() % (4ull * m)) : (sp == 1 ? static_cast<uint32_t>(rng()) : 0xFFFFFFFFu - static_cast<uint32_t>(rng() % (2ull * m)));
            keys.insert(static_cast<uint64_t>(sp) << 32 | id);
        }
        std::vector<int32_t> species;
        std::vector<uint32_t> ids;
        for (uint64_t k : keys) { species.push_back(static_cast<int32_t>(k >> 32)); ids.push_back(static_cast<uint32_t>(k)); }
        for (size_t k = ids.size(); k > 1; --k) {       // the caller's order is arbitrary
            const size_t j = rng() % k;
            std::swap(ids[k - 1], ids[j]);
            std::swap(species[k - 1], species[j]);
        }
        fpic_series_spec s{};
        s.ntracers = m; s.tracer_species = species.data(); s.tracer_id = ids.data();
        CHECK(fesser::check(s, 3, nullptr) == nullptr);
        const std::vector<fesser::Table> tabs = fesser::build(s);
        size_t total = 0;
        int last_species = -1;
        std::vector<char> seen(m, 0);
        for (const fesser::Table& t : tabs) {
            CHECK(t.species > last_species);
            last_species = t.species;
            const uint32_t n = static_cast<uint32_t>(t.sorted.size());
            total += n;
            CHECK(n > 0 && t.index.size() == n);
            CHECK(t.log2bits >= fesser::kFilterMinLog2 && t.log2bits <= fesser::kFilterMaxLog2 && t.log2bits == fesser::filter_log2(n));
            CHECK(t.filter.size() == (size_t(1) << t.log2bits) / 32);
            CHECK((1ull << t.log2bits) >= 256ull * n || t.log2bits == fesser::kFilterMaxLog2);
            for (uint32_t k = 0; k < n; ++k) {
                if (k) CHECK(t.sorted[k - 1] < t.sorted[k]);
                // a member is never missed: by the filter, by the search, and its entry is the caller's
                CHECK(fesser::filter_hit(t.filter.data(), t.sorted[k], t.log2bits));
                CHECK(fesser::lookup(t.sorted.data(), n, t.sorted[k]) == static_cast<int64_t>(k));
                const uint32_t e = t.index[k];
                CHECK(e < m && !seen[e] && species[e] == t.species && ids[e] == t.sorted[k]);
                if (e < m) seen[e] = 1;
            }
            // ids that are not members: the search says so whatever the filter said; the filter lets few through
            size_t set_bits = 0, passed = 0, tried = 0;
            for (uint32_t w : t.filter) set_bits += static_cast<size_t>(__builtin_popcount(w));
            CHECK(set_bits <= 3 * size_t(n) && set_bits >= 1);                      // up to three bits per id
            for (int k = 0; k < 20000; ++k) {
                const uint32_t q = static_cast<uint32_t>(rng());
                if (std::binary_search(t.sorted.begin(), t.sorted.end(), q)) continue;
                CHECK(fesser::lookup(t.sorted.data(), n, q) == -1);
                ++tried;
                passed += fesser::filter_hit(t.filter.data(), q, t.log2bits) ? 1 : 0;
            }
            // (a filter with room, 256 bits per id: about 1 in 10^4 passes; the full one at its densest, four ids per word: 1 in 20)
            CHECK(t.log2bits == fesser::kFilterMaxLog2 ? passed * 8 <= tried : passed * 500 <= tried);
        }
        CHECK(total == m);
    }
    CHECK(fesser::filter_log2(1) == 10 && fesser::filter_log2(4) == 10 && fesser::filter_log2(5) == 11 && fesser::filter_log2(16) == 12 &&
          fesser::filter_log2(2048) == 19 && fesser::filter_log2(65536) == 19);
    CHECK(fesser::lookup(nullptr, 0, 5) == -1);
}

static void owners()
{
    // four ranks of 32 planes: fesdiag::owned_planes gives the slab, owns_plane the test the kernel makes
    for (int r = 0; r < 4; ++r) {
        const fesdiag::Owned o = fesdiag::owned_planes(32, 4, r);
        for (int k = 0; k < 32; ++k) CHECK(fesser::owns_plane(k, o.k0, o.nk) == (k / 8 == r));
    }
    const fesdiag::Owned all = fesdiag::owned_planes(32, 1, 0);
    for (int k = 0; k < 32; ++k) CHECK(fesser::owns_plane(k, all.k0, all.nk));
    // a compact rank holds its slab and halo: the plane above the slab must be among them for a point row
    const fes::Held with_ghost{ 6, 13 }, bare{ 8, 8 };
    CHECK(fesdiag::owned_are_held(fesdiag::owned_planes(32, 4, 1), with_ghost, 32, true));
    CHECK(!fesdiag::owned_are_held(fesdiag::owned_planes(32, 4, 1), bare, 32, true));
}

static void selection()
{
    const int E = fesser::kEntry;
    const size_t entries = 5;
    // three parts of five entries; the flag is column 6
    std::vector<double> parts(3 * entries * E, 0.0), out(entries * E, -1.0);
    auto at = [&](int r, size_t i) { return parts.data() + (static_cast<size_t>(r) * entries + i) * E; };
    at(0, 0)[0] = -0.0; at(0, 0)[1] = 3.5; at(0, 0)[6] = 1.0;           // entry 0: part 0, with a negative zero
    at(2, 1)[0] = 7.0; at(2, 1)[6] = 1.0;                                // entry 1: part 2
    at(1, 3)[5] = std::numeric_limits<double>::quiet_NaN(); at(1, 3)[6] = 1.0;   // entry 3: part 1, with a NaN
    at(1, 4)[0] = 9.0;                                                   // entry 4: values without a flag are nobody's
    CHECK(fesser::select(parts.data(), entries * E, 3, entries, 6, out.data()) == -1);
    CHECK(std::memcmp(out.data(), at(0, 0), E * sizeof(double)) == 0 && std::signbit(out[0]));
    CHECK(std::memcmp(out.data() + E, at(2, 1), E * sizeof(double)) == 0);
    for (int c = 0; c < E; ++c) CHECK(out[2 * E + c] == 0.0 && !std::signbit(out[2 * E + c]) && out[4 * E + c] == 0.0);
    CHECK(std::memcmp(out.data() + 3 * E, at(1, 3), E * sizeof(double)) == 0);
    // the other flag column sees nothing set
    CHECK(fesser::select(parts.data(), entries * E, 3, entries, 7, out.data()) == -1);
    for (double v : out) CHECK(v == 0.0);
    // two flags for one entry: reported, with the entry
    at(1, 1)[6] = 1.0;
    CHECK(fesser::select(parts.data(), entries * E, 3, entries, 6, out.data()) == 1);
    // one part: the selection is that part where flagged
    CHECK(fesser::select(parts.data(), entries * E, 1, entries, 6, out.data()) == -1);
    CHECK(std::memcmp(out.data(), at(0, 0), E * sizeof(double)) == 0 && out[4 * E] == 0.0);
}

static void ring()
{
    fesdiag::Ring r;
    r.cap = 4;
    uint64_t first, n, dropped, slot[2], len[2];
    for (int k = 0; k < 10; ++k) r.seq++;
    r.pending(first, n, dropped);
    CHECK(first == 6 && n == 4 && dropped == 6);
    CHECK(r.runs(first, n, slot, len) == 2 && slot[0] == 2 && len[0] == 2 && slot[1] == 0 && len[1] == 2);
    r.drained = r.seq;
    r.pending(first, n, dropped);
    CHECK(n == 0 && dropped == 0);
}

int main()
{
    checks();
    units();
    tables();
    owners();
    selection();
    ring();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
