// Host test of fusion-sim_amd/csrc/fes_ionize_core.hpp (the rule of the electron-impact ionisation and the checks of a
// request): the request as the gas operator's, the words' tag, the decision and the outcome of hand-made projectiles, the
// tally terms and the result's conversion, the fit rule on both sides of every bound, and every refusal by its message.
// With two arguments it also reads cases from a file (tests/test_ionize_host.py writes them: a request, a precision,
// projectiles with their ids, the targets' populations) and writes what the rule gives, which the numpy reference must give
// bit for bit: the cases have vth = 0, so that no rounded function of the host's libm enters a decision, a rank, an id, an
// ion's velocity, a copied position or a count.  The ranks are formed as the passes form them: a bitmap over the id span and
// the set bits below the primary's.
// Built with g++ -ffp-contract=off by tests/test_ionize_host.py (also with -fsanitize=address,undefined, as a program of its
// own); prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../fusion-sim_amd/csrc/fes_ionize_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static const double kL[3] = { 0.015625, 0.015625, 0.03125 };
static const double kFlat[4] = { 2e-19, 2e-19, 2e-19, 2e-19 };
static const double* const kNoTaper[3] = { nullptr, nullptr, nullptr };

static fpic_ionize_spec good()
{
    fpic_ionize_spec s;
    std::memset(&s, 0, sizeof s);
    s.species = 0;
    s.electron = 0;
    s.ion = 1;
    s.seed = 0x1234567890ull;
    s.density = 1e21;
    s.tau = 1e-9;
    s.g_lo = 0.125;
    s.g_hi = 0.5;
    s.g_threshold = 0.125;
    s.n = 4;
    s.sigma = kFlat;
    for (int a = 0; a < 3; ++a) { s.lo[a] = 0; s.hi[a] = kL[a]; }
    return s;
}
static bool says(const char* msg, const char* text) { return msg && std::strcmp(msg, text) == 0; }

static void numbers()
{
    fpic_ionize_spec s = good();
    const fpic_gas_spec q = fesion::gas_of(s);
    CHECK(q.kind == FPIC_GAS_EXCHANGE && q.mass_ratio == 0 && q.species == 0 && q.seed == s.seed && q.density == s.density && q.tau == s.tau && q.g_lo == s.g_lo && q.g_hi == s.g_hi &&
          q.n == 4 && q.sigma == kFlat && q.hi[2] == kL[2] && q.reserved_i == 0 && q.reserved_u == 0);
    const fesion::Rule r = fesion::rule_of(s, kL, 7, kFlat, kFlat, kNoTaper);
    const fesgas::Rule g = fesgas::rule_of(q, kL, 7, kFlat, kFlat, kNoTaper);
    CHECK(r.g.K == g.K && r.g.x_max == g.x_max && r.g.column == g.column && r.g.epoch == 7 && r.thr2 == 0.125 * 0.125 && r.g.K > 0);
    CHECK(fesion::x_max_of(s) == g.x_max);
    // the tag is this operator's own
    uint32_t a[4], b[4];
    fesion::words(r, 5, 2, a);
    fesload::philox(5, r.g.epoch, r.g.stream, 0x1051E0u + 2u, r.g.seed_lo, r.g.seed_hi, b);
    CHECK(std::memcmp(a, b, sizeof a) == 0 && fesion::kTag == 0x1051E0u && fesion::kTag != fesgas::kTag && fesion::kTag != fesfusion::kTag);
    CHECK(fesion::kWords == 29 && fesion::kCounts == 3 && fesion::kOutAt == 28);
}

static void rule()
{
    // P_max = 1, a cold gas that drifts: every projectile is a candidate, vb = drift
    fpic_ionize_spec s = good();
    s.density = 1e30;
    s.drift[0] = 0.25;
    const fesion::Rule r = fesion::rule_of(s, kL, 0, kFlat, kFlat, kNoTaper);
    CHECK(r.g.K == uint64_t(1) << 32);
    const double p[3] = { 0.5, 0.5, 0.5 };
    double vb[3], g = 0;
    const double slow[3] = { 0.25, 0.0625, 0.0 };                              // g = 0.0625 < g_lo
    CHECK(fesion::decide(r, kFlat, kNoTaper, 1, p, slow, vb, &g) == fesion::kBelow && g == 0.0625 && vb[0] == 0.25 && vb[1] == 0 && vb[2] == 0);
    const double fast[3] = { 0.75, 0.0, 0.0 };                                 // g = 0.5 = g_hi
    CHECK(fesion::decide(r, kFlat, kNoTaper, 2, p, fast, vb, &g) == fesion::kAbove && g == 0.5);
    const double nan_v[3] = { kNan, 0.0, 0.0 };
    CHECK(fesion::decide(r, kFlat, kNoTaper, 3, p, nan_v, vb, &g) == fesion::kAbove);
    // at the threshold (g = g_lo = g_threshold): whoever has the event keeps no speed in the gas frame
    const double at[3] = { 0.25, 0.125, 0.0 };
    int events = 0;
    for (uint32_t i = 0; i < 64; ++i) {
        if (fesion::decide(r, kFlat, kNoTaper, i, p, at, vb, &g) != fesion::kEvent) continue;
        ++events;
        double v1[3], vs[3];
        fesion::outcome(r, i, vb, g, v1, vs);
        CHECK(g == 0.125 && v1[0] == 0.25 && v1[1] == 0 && v1[2] == 0 && vs[0] == 0.25 && vs[1] == 0 && vs[2] == 0);
    }
    CHECK(events > 0 && events < 64);                                          // (x / x_max = 0.25)
    // the outcome shares g^2 - thr^2
    const double mid[3] = { 0.25, 0.0, 0.375 };
    for (uint32_t i = 0; i < 16; ++i) {
        const double rel = fesion::partner(r, i, mid, vb);
        double v1[3], vs[3];
        fesion::outcome(r, i, vb, rel, v1, vs);
        double e = 0;
        for (int a = 0; a < 3; ++a) e += (v1[a] - vb[a]) * (v1[a] - vb[a]) + (vs[a] - vb[a]) * (vs[a] - vb[a]);
        CHECK(rel == 0.375 && std::fabs(e - (0.375 * 0.375 - 0.125 * 0.125)) < 1e-15);
    }
    double nh[3];
    fesion::nhat(0x80000000u, 0u, nh);                                         // c = 1 - 2 (2^31 + 0.5) 2^-32 = -2^-32, phi = 0
    CHECK(nh[2] == -0x1p-32 && nh[1] == 0.0 && nh[0] == std::sqrt(1.0 - 0x1p-64));
}

static void tallies_and_result()
{
    using fesion::Fix;
    Fix sum[4] = { 0, 0, 0, 0 };
    unsigned long long out = 0;
    const double w[3] = { 0.5, -0.25, 1.0 };
    fesion::gain(w, sum, out, 4);
    CHECK(out == 0 && sum[0] == fesforce::floor_fix(1.3125) && sum[1] == (Fix(1) << 79) && sum[2] == ~(Fix(1) << 78) + 1 && sum[3] == (Fix(1) << 80));
    const double big[3] = { 200.0, 0.0, kNan };
    fesion::gain(big, sum, out, 4);                                            // |v|^2 is NaN: outside; vx, vy inside; vz outside
    CHECK(out == ((1ull << 4) | (1ull << 7)));
    uint64_t words[fesion::kWords] = {};
    words[0] = 11; words[1] = 4; words[2] = 3; words[3] = 2;
    words[4] = 0; words[5] = 1;                                                // primary energy 2^64 2^-80
    words[4 + 8 + 2] = ~uint64_t(0); words[4 + 8 + 3] = ~uint64_t(0);          // electron momentum x = -1
    words[4 + 16 + 6] = uint64_t(1) << 40;                                     // ion momentum z
    words[fesion::kOutAt] = 1ull << (8 + 2);                                   // ion momentum y outside
    fpic_ionize_result res;
    std::memset(&res, 0, sizeof res);
    const double mass[3] = { 2.0, 2.0, 8.0 }, charge[3] = { -1.0, -1.0, 1.0 };
    fesion::result_of(words, mass, charge, 3.0, &res);
    const double ke = 0.5 * 2.0 * 3.0 * fesforce::kC * fesforce::kC, pm = 2.0 * 3.0 * fesforce::kC, pmi = 8.0 * 3.0 * fesforce::kC;
    CHECK(res.candidates == 11 && res.below == 4 && res.above == 3 && res.ionised == 2 && res.applications == 0);
    CHECK(res.primary.energy == ke * 0x1p-16 && res.primary.energy_fixed[1] == 1 && res.primary.charge == 0.0);
    CHECK(res.electron.momentum[0] == pm * -0x1p-80 && res.electron.charge == (2.0 * -1.0) * 3.0 && res.electron.energy == 0.0);
    CHECK(res.ion.momentum[2] == pmi * 0x1p-40 && std::isnan(res.ion.momentum[1]) && res.ion.momentum[0] == 0.0 && res.ion.charge == 6.0);
}

static void fit()
{
    // the capacity, on both sides: n + M <= capacity
    CHECK(fesion::fit(5, 10, 15, 10, 10, 15, 10) == nullptr);
    CHECK(says(fesion::fit(6, 10, 15, 10, 10, 16, 10), "electron"));
    CHECK(says(fesion::fit(6, 10, 16, 10, 10, 15, 10), "ion"));
    CHECK(fesion::fit(0, 10, 10, 10, 10, 10, 10) == nullptr && says(fesion::fit(1, 10, 10, 10, 10, 11, 10), "electron"));
    // the id bound, on both sides: id span + M <= 2^32 - 1
    const uint64_t end = 0xFFFFFFFFull, cap = 1ull << 40;
    CHECK(fesion::fit(5, 10, cap, end - 5, 10, cap, 10) == nullptr && says(fesion::fit(5, 10, cap, end - 4, 10, cap, 10), "electron"));
    CHECK(fesion::fit(5, 10, cap, 10, 10, cap, end - 5) == nullptr && says(fesion::fit(5, 10, cap, 10, 10, cap, end - 4), "ion"));
}

static void refusals()
{
    CHECK(says(fesion::check(nullptr, 2, kL), ".spec <- Non-optional property is undefined!"));
    fpic_ionize_spec s = good();
    CHECK(fesion::check(&s, 2, kL) == nullptr);
    // the reserved words
    s = good(); s.reserved_i = 1; CHECK(says(fesion::check(&s, 2, kL), ".reserved <- must be zero"));
    s = good(); s.reserved_n = 1; CHECK(says(fesion::check(&s, 2, kL), ".reserved <- must be zero"));
    s = good(); s.reserved_u = 1; CHECK(says(fesion::check(&s, 2, kL), ".reserved <- must be zero"));
    s = good(); s.reserved[3] = 1e-300; CHECK(says(fesion::check(&s, 2, kL), ".reserved <- must be zero"));
    s = good(); s.reserved[0] = kNan; CHECK(says(fesion::check(&s, 2, kL), ".reserved <- must be zero"));
    // the shared fields: the gas operator's checks, by its messages
    for (int k : { 2, -1 }) { s = good(); s.species = k; CHECK(says(fesion::check(&s, 2, kL), ".species <- no such species")); }
    for (double bad : { -1e-300, kInf, kNan }) { s = good(); s.density = bad; CHECK(says(fesion::check(&s, 2, kL), ".density <- must be finite and not negative")); }
    for (double bad : { 0.0, -1.0, kInf, kNan }) { s = good(); s.tau = bad; CHECK(says(fesion::check(&s, 2, kL), ".tau <- must be positive and finite")); }
    std::vector<double> table(FPIC_GAS_TABLE_MAX + 1, 1e-19);
    for (int n : { 1, 0, -3, FPIC_GAS_TABLE_MAX + 1 }) { s = good(); s.sigma = table.data(); s.n = n; CHECK(says(fesion::check(&s, 2, kL), ".n <- must be 2 .. FPIC_GAS_TABLE_MAX (4096)")); }
    s = good(); s.sigma = nullptr; CHECK(says(fesion::check(&s, 2, kL), ".sigma <- Non-optional property is undefined!"));
    for (double bad : { -0.1, kInf, kNan }) { s = good(); s.g_lo = bad; CHECK(says(fesion::check(&s, 2, kL), ".g_lo <- must be finite and not negative")); }
    for (double bad : { 0.125, 0.0, kInf, kNan }) { s = good(); s.g_hi = bad; CHECK(says(fesion::check(&s, 2, kL), ".g_hi <- must be finite and above g_lo")); }
    const double neg[2] = { 1e-19, -1e-30 };
    s = good(); s.sigma = neg; s.n = 2; CHECK(says(fesion::check(&s, 2, kL), ".sigma <- every entry must be finite and not negative"));
    for (double bad : { kInf, kNan }) {
        s = good(); s.drift[1] = bad; CHECK(says(fesion::check(&s, 2, kL), ".drift <- must be finite"));
        s = good(); s.vth[2] = bad; CHECK(says(fesion::check(&s, 2, kL), ".vth <- must be finite and not negative"));
        s = good(); s.lo[1] = bad; CHECK(says(fesion::check(&s, 2, kL), ".lo, .hi <- must be finite"));
    }
    s = good(); s.vth[0] = -1e-9; CHECK(says(fesion::check(&s, 2, kL), ".vth <- must be finite and not negative"));
    const char* window = ".lo, .hi <- the window must lie within 0 <= lo < hi <= L";
    s = good(); s.lo[0] = -1e-300; CHECK(says(fesion::check(&s, 2, kL), window));
    s = good(); s.hi[2] = kL[2] * 1.0000001; CHECK(says(fesion::check(&s, 2, kL), window));
    s = good(); s.lo[1] = s.hi[1] = kL[1] / 2; CHECK(says(fesion::check(&s, 2, kL), window));
    std::vector<double> tab(FPIC_GAS_TAPER_MAX + 1, 1.0);
    for (uint32_t n : { 1u, static_cast<uint32_t>(FPIC_GAS_TAPER_MAX + 1) }) {
        s = good(); s.taper_n[1] = n; s.taper[1] = tab.data(); CHECK(says(fesion::check(&s, 2, kL), ".taper_n <- a table has 2 .. FPIC_GAS_TAPER_MAX nodes (0: none)"));
    }
    s = good(); s.taper_n[2] = 2; CHECK(says(fesion::check(&s, 2, kL), ".taper <- a table is null but its node count is not zero"));
    tab[1] = 1.0000001;
    s = good(); s.taper_n[0] = 2; s.taper[0] = tab.data(); CHECK(says(fesion::check(&s, 2, kL), ".taper <- the nodes must lie in [0, 1] (the density as a fraction of its peak)"));
    const double huge[2] = { 1e300, 1e300 };
    s = good(); s.density = 1e300; s.sigma = huge; s.n = 2; CHECK(says(fesion::check(&s, 2, kL), ".sigma <- the candidate bound density c tau max(sigma g) is not a finite number"));
    // the species rules
    for (int k : { 2, -1 }) { s = good(); s.electron = k; CHECK(says(fesion::check(&s, 2, kL), ".electron <- no such species")); }
    for (int k : { 2, -1 }) { s = good(); s.ion = k; CHECK(says(fesion::check(&s, 2, kL), ".ion <- no such species")); }
    s = good(); s.ion = 0; CHECK(says(fesion::check(&s, 2, kL), ".ion <- must differ from species and from electron"));
    s = good(); s.electron = 1; s.ion = 1; CHECK(says(fesion::check(&s, 2, kL), ".ion <- must differ from species and from electron"));
    s = good(); s.electron = 1; s.ion = 2; CHECK(fesion::check(&s, 3, kL) == nullptr);          // three different species
    s = good(); s.electron = 2; s.ion = 1; CHECK(fesion::check(&s, 3, kL) == nullptr);
    s = good(); s.species = 1; s.electron = 1; s.ion = 0; CHECK(fesion::check(&s, 2, kL) == nullptr);
    // the threshold, on both sides of its bounds
    for (double bad : { -1e-300, kInf, -kInf, kNan }) { s = good(); s.g_threshold = bad; CHECK(says(fesion::check(&s, 2, kL), ".g_threshold <- must be finite and not negative")); }
    s = good(); s.g_threshold = 0.0; CHECK(fesion::check(&s, 2, kL) == nullptr);
    s = good(); s.g_threshold = 0.125; CHECK(fesion::check(&s, 2, kL) == nullptr);                // g_lo == g_threshold
    s = good(); s.g_threshold = std::nextafter(0.125, 1.0); CHECK(says(fesion::check(&s, 2, kL), ".g_lo <- the table must start at or above g_threshold"));
    s = good(); s.g_threshold = std::nextafter(0.125, 0.0); CHECK(fesion::check(&s, 2, kL) == nullptr);
}

// ---- cases from a file.  Per case, little endian: int32 n (table), precision (0: float, 1: double); uint64 seed; uint32 stream,
// epoch; double density, tau, g_lo, g_hi, g_threshold, drift[3], L[3], lo[3], hi[3]; uint32 taper_n[3], 0; the n
// cross-sections; the tapers' doubles; uint64 n_e, span_e, n_i, span_i, id span of the projectiles; uint32 count; count ids;
// count x 6 doubles (p, v).  Out per case, as 64-bit words: the doubles column, x_max, then K; per projectile candidate (0 / 1),
// what, rank + 1 (0: no event); candidates, below, above, ionised; per event in rank order the electron's slot and id, the
// ion's slot and id, the copied position[3] and the ion's stored velocity[3] as doubles.
template <typename V>
static bool get(std::FILE* f, V* v, size_t n = 1) { return std::fread(v, sizeof(V), n, f) == n; }
static void put(std::FILE* f, double d) { std::fwrite(&d, sizeof d, 1, f); }
static void put(std::FILE* f, uint64_t u) { std::fwrite(&u, sizeof u, 1, f); }

static int run_cases(const char* in_path, const char* out_path)
{
    std::FILE* in = std::fopen(in_path, "rb");
    std::FILE* out = std::fopen(out_path, "wb");
    if (!in || !out) { std::printf("FAILED: cannot open the case files\n"); return 1; }
    uint32_t ncases = 0;
    if (!get(in, &ncases)) return 1;
    for (uint32_t c = 0; c < ncases; ++c) {
        fpic_ionize_spec s;
        std::memset(&s, 0, sizeof s);
        s.ion = 1;
        int32_t precision = 0;
        uint32_t pad = 0;
        double L[3];
        bool ok = get(in, &s.n) && get(in, &precision) && get(in, &s.seed) && get(in, &s.stream) && get(in, &s.epoch) && get(in, &s.density) && get(in, &s.tau) &&
                  get(in, &s.g_lo) && get(in, &s.g_hi) && get(in, &s.g_threshold) && get(in, s.drift, 3) && get(in, L, 3) && get(in, s.lo, 3) && get(in, s.hi, 3) &&
                  get(in, s.taper_n, 3) && get(in, &pad);
        if (!ok || s.n < 0 || s.n > FPIC_GAS_TABLE_MAX) { std::printf("FAILED: case %u is cut short\n", c); return 1; }
        std::vector<double> sigma(s.n), tabs[3];
        ok = s.n == 0 || get(in, sigma.data(), sigma.size());
        s.sigma = sigma.data();
        for (int a = 0; a < 3 && ok; ++a) {
            if (s.taper_n[a] > FPIC_GAS_TAPER_MAX) { ok = false; break; }
            tabs[a].resize(s.taper_n[a]);
            ok = s.taper_n[a] == 0 || get(in, tabs[a].data(), tabs[a].size());
            s.taper[a] = s.taper_n[a] ? tabs[a].data() : nullptr;
        }
        uint64_t pop[5] = {};
        uint32_t n = 0;
        ok = ok && get(in, pop, 5) && get(in, &n);
        if (!ok) { std::printf("FAILED: case %u is cut short\n", c); return 1; }
        std::vector<uint32_t> ids(n);
        std::vector<double> state(static_cast<size_t>(n) * 6);
        if (n && (!get(in, ids.data(), n) || !get(in, state.data(), state.size()))) { std::printf("FAILED: case %u is cut short\n", c); return 1; }
        const double Lb[3] = { L[0], L[1], L[2] };
        if (const char* why = fesion::check(&s, 2, Lb)) { std::printf("FAILED: case %u is refused: %s\n", c, why); return 1; }
        const fesion::Rule r = fesion::rule_of(s, Lb, s.epoch, s.sigma, s.sigma, s.taper);
        put(out, r.g.column);
        put(out, r.g.x_max);
        put(out, static_cast<uint64_t>(r.g.K));
        // the deciding pass: the counts, the events, the bitmap of their primaries' ids
        const double* const tab[3] = { r.g.win.tab[0], r.g.win.tab[1], r.g.win.tab[2] };
        std::vector<uint32_t> bitmap(static_cast<size_t>((pop[4] + 31) / 32), 0u);
        std::vector<int> what(n, 0);
        std::vector<uint8_t> cand(n, 0);
        uint64_t count[4] = { 0, 0, 0, 0 };
        for (uint32_t k = 0; k < n; ++k) {
            const double p[3] = { state[6 * k], state[6 * k + 1], state[6 * k + 2] };
            const double v[3] = { state[6 * k + 3], state[6 * k + 4], state[6 * k + 5] };
            cand[k] = fesforce::inside(r.g.win, p) && fesion::drawn(r, ids[k]);
            if (!cand[k]) continue;
            double vb[3], g;
            what[k] = fesion::decide(r, r.g.sigma, tab, ids[k], p, v, vb, &g);
            count[0] += 1;
            count[1] += what[k] & fesion::kBelow ? 1 : 0;
            count[2] += what[k] & fesion::kAbove ? 1 : 0;
            if (what[k] & fesion::kEvent) {
                if (ids[k] >= pop[4]) { std::printf("FAILED: case %u has an id beyond its span\n", c); return 1; }
                bitmap[ids[k] >> 5] |= 1u << (ids[k] & 31u);
                count[3] += 1;
            }
        }
        const char* who = fesion::fit(count[3], pop[0], ~0ull, pop[1], pop[2], ~0ull, pop[3]);
        if (who) { std::printf("FAILED: case %u does not fit its %s ids\n", c, who); return 1; }
        std::vector<uint64_t> below(bitmap.size() + 1, 0);
        for (size_t w = 0; w < bitmap.size(); ++w) below[w + 1] = below[w] + static_cast<uint64_t>(__builtin_popcount(bitmap[w]));
        std::vector<uint32_t> by_rank(count[3], 0);
        for (uint32_t k = 0; k < n; ++k) {
            uint64_t rank1 = 0;
            if (what[k] & fesion::kEvent) {
                const uint32_t i = ids[k];
                const uint64_t rank = below[i >> 5] + static_cast<uint64_t>(__builtin_popcount(bitmap[i >> 5] & ((1u << (i & 31u)) - 1u)));
                by_rank[rank] = k;
                rank1 = rank + 1;
            }
            put(out, static_cast<uint64_t>(cand[k]));
            put(out, static_cast<uint64_t>(what[k]));
            put(out, rank1);
        }
        for (int k = 0; k < 4; ++k) put(out, count[k]);
        // the generation pass: the new rows by rank
        for (uint64_t l = 0; l < count[3]; ++l) {
            const uint32_t k = by_rank[l];
            const double v[3] = { state[6 * k + 3], state[6 * k + 4], state[6 * k + 5] };
            double vb[3];
            (void)fesion::partner(r, ids[k], v, vb);
            put(out, pop[0] + l);
            put(out, pop[1] + l);
            put(out, pop[2] + l);
            put(out, pop[3] + l);
            for (int a = 0; a < 3; ++a) put(out, state[6 * k + a]);
            for (int a = 0; a < 3; ++a) put(out, precision ? vb[a] : static_cast<double>(static_cast<float>(vb[a])));
        }
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}

int main(int argc, char** argv)
{
    numbers();
    rule();
    tallies_and_result();
    fit();
    refusals();
    if (argc == 3 && run_cases(argv[1], argv[2])) return 1;
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
