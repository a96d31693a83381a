// Host test of fusion-sim_amd/csrc/fes_gas_core.hpp (the rule of the windowed background collisions and the checks of a
// request): the host-side numbers (the column, the interval-wise bound, K), the window and the candidate set, the table's
// ends, the exact fixed-point terms, the words' layout and their exact sum over ranks, and every refusal by its message.
// With two arguments it also reads cases from a file (tests/test_gas_host.py writes them: a request, a precision,
// particles) and writes what the rule gives, which the numpy reference must give bit for bit: the cases have vth = 0 and
// EXCHANGE, so that no rounded function of the host's libm enters a decision, a stored velocity or a tally.
// Built with g++ -ffp-contract=off by tests/test_gas_host.py (also with -fsanitize=address,undefined, as a program of its
// own); prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../fusion-sim_amd/csrc/fes_collide_core.hpp"
#include "../../fusion-sim_amd/csrc/fes_gas_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static const double kL[3] = { 0.015625, 0.015625, 0.03125 };
static const double kFlat[4] = { 2e-19, 2e-19, 2e-19, 2e-19 };

static fpic_gas_spec good()
{
    fpic_gas_spec s;
    std::memset(&s, 0, sizeof s);
    s.kind = FPIC_GAS_EXCHANGE;
    s.seed = 0x1234567890ull;
    s.density = 1e21;
    s.tau = 1e-9;
    s.g_lo = 0.0;
    s.g_hi = 0.5;
    s.n = 4;
    s.sigma = kFlat;
    for (int a = 0; a < 3; ++a) { s.lo[a] = 0; s.hi[a] = kL[a]; }
    return s;
}
static bool says(const char* msg, const char* text) { return msg && std::strcmp(msg, text) == 0; }
static const double* const kNoTaper[3] = { nullptr, nullptr, nullptr };

static void numbers()
{
    fpic_gas_spec s = good();
    const double column = (1e21 * fesgas::kC) * 1e-9;
    CHECK(fesgas::column_of(s) == column);
    // a flat table pays g_hi; the last interval is taken with g_hi itself
    CHECK(fesgas::bound_of(kFlat, 4, 0.0, 0.5) == 2e-19 * 0.5);
    // the interval-wise bound: a peak at low speed is not multiplied by g_hi
    const double peak[5] = { 0.0, 8.0, 0.0, 0.0, 1.0 };
    CHECK(fesgas::bound_of(peak, 5, 0.0, 4.0) == 8.0 * 2.0);                 // intervals 0 and 1 hold the peak: max(8 1, 8 2, 0, 1 4)
    const double late[3] = { 5.0, 0.0, 1.0 };
    CHECK(fesgas::bound_of(late, 3, 1.0, 3.0) == 5.0 * 2.0);                 // max(5 (1 + 1), 1 3)
    const double zeros[3] = { 0, 0, 0 };
    CHECK(fesgas::bound_of(zeros, 3, 0.0, 1.0) == 0.0);
    fesgas::Rule r = fesgas::rule_of(s, kL, 7, kFlat, kFlat, kNoTaper);
    const double x_max = column * (2e-19 * 0.5);
    CHECK(r.column == column && r.x_max == x_max && r.K == static_cast<uint64_t>(std::ldexp(-std::expm1(-x_max), 32)) && r.K > 0 && r.K < (uint64_t(1) << 32));
    CHECK(r.epoch == 7 && r.seed_lo == 0x34567890u && r.seed_hi == 0x12u && r.kind == FPIC_GAS_EXCHANGE && r.M == 0.0);
    CHECK(r.xs.n == 4 && r.xs.g_lo == 0.0 && r.xs.g_hi == 0.5 && r.xs.inv_dg == 3.0 / 0.5 && r.xs.s_max == 2e-19);
    CHECK(r.win.whole == 1 && r.win.tapered == 0 && r.win.lo_f[2] == 0 && r.win.hi_f[2] == 1 && r.win.w[0] == 1);
    s.density = 0;
    CHECK(fesgas::rule_of(s, kL, 0, kFlat, kFlat, kNoTaper).K == 0);
    s = good(); s.sigma = zeros; s.n = 3;
    CHECK(fesgas::rule_of(s, kL, 0, zeros, zeros, kNoTaper).K == 0);
    s = good(); s.density = 1e30;
    CHECK(fesgas::rule_of(s, kL, 0, kFlat, kFlat, kNoTaper).K == uint64_t(1) << 32);   // P_max = 1: everybody inside
    s = good(); s.kind = FPIC_GAS_ELASTIC; s.mass_ratio = 3.0;
    CHECK(fesgas::rule_of(s, kL, 0, kFlat, kFlat, kNoTaper).M == 0.75);
    s.mass_ratio = kInf;
    CHECK(fesgas::rule_of(s, kL, 0, kFlat, kFlat, kNoTaper).M == 1.0);
    s = good(); s.lo[0] = kL[0] / 8; s.hi[0] = 7 * kL[0] / 8;
    const double two[2] = { 0.5, 1.0 };
    s.taper_n[2] = 2; s.taper[2] = two;
    const double* const tabs[3] = { nullptr, nullptr, two };
    r = fesgas::rule_of(s, kL, 0, kFlat, kFlat, tabs);
    CHECK(r.win.whole == 0 && r.win.tapered == 1 && r.win.lo_f[0] == 0.125 && r.win.hi_f[0] == 0.875 && r.win.w[0] == 0.75 && r.win.tk[2] == 1 && r.win.tab[2] == two);
    // the tag is this operator's own
    uint32_t a[4], b[4];
    fesgas::words(r, 5, 0, a);
    fesload::philox(5, r.epoch, r.stream, 0x6A500u, r.seed_lo, r.seed_hi, b);
    CHECK(std::memcmp(a, b, sizeof a) == 0 && fesgas::kTag != fescoll::kTag && fesgas::kTag + 1 != fescoll::kTag && fesgas::kTag != fesfusion::kTag);
}

static void rule()
{
    // P_max = 1, a cold background at rest: every particle inside is a candidate, g = |v|
    fpic_gas_spec s = good();
    s.density = 1e30;
    s.g_lo = 0.25;
    s.lo[1] = kL[1] / 4; s.hi[1] = 3 * kL[1] / 4;
    fesgas::Rule r = fesgas::rule_of(s, kL, 0, kFlat, kFlat, kNoTaper);
    bool cand = false;
    const double on_lo[3] = { 0.5, 0.25, 0.5 }, on_hi[3] = { 0.5, 0.75, 0.5 }, nan_p[3] = { 0.5, kNan, 0.5 };
    double v[3] = { 0.0, 0.0, 0.5 };                                         // g = 0.5 = g_hi: above
    CHECK(fesgas::apply(r, 1, on_lo, v, &cand) == fesgas::kAbove && cand && v[2] == 0.5);
    double slow[3] = { 0.125, 0.0, 0.0 };                                    // g < g_lo: below
    CHECK(fesgas::apply(r, 2, on_lo, slow, &cand) == fesgas::kBelow && cand && slow[0] == 0.125);
    double at_lo[3] = { 0.0, 0.25, 0.0 };                                    // g = g_lo: inside the table; x = x_max: collides
    CHECK(fesgas::apply(r, 3, on_lo, at_lo, &cand) == fesgas::kCollided && cand && at_lo[0] == 0 && at_lo[1] == 0 && at_lo[2] == 0);
    double out_v[3] = { 0.0, 0.3, 0.0 };
    CHECK(fesgas::apply(r, 4, on_hi, out_v, &cand) == 0 && !cand && out_v[1] == 0.3);
    CHECK(fesgas::apply(r, 4, nan_p, out_v, &cand) == 0 && !cand);
    double nan_v[3] = { kNan, 0.0, 0.0 };
    CHECK(fesgas::apply(r, 5, on_lo, nan_v, &cand) == fesgas::kAbove && cand);
    // K = 0: nobody
    s.density = 0;
    r = fesgas::rule_of(s, kL, 0, kFlat, kFlat, kNoTaper);
    double w[3] = { 0.0, 0.3, 0.0 };
    CHECK(fesgas::apply(r, 3, on_lo, w, &cand) == 0 && !cand);
}

static void tallies()
{
    using fesgas::Fix;
    CHECK(fesgas::floor_fix(0.0) == 0 && fesgas::floor_fix(1.0) == (Fix(1) << 80) && fesgas::floor_fix(-1.0) == ~(Fix(1) << 80) + 1);
    CHECK(fesgas::floor_fix(0x1p-80) == 1 && fesgas::floor_fix(-0x1p-80) == ~Fix(0) && fesgas::floor_fix(0x1p-81) == 0 && fesgas::floor_fix(-0x1p-81) == ~Fix(0));
    CHECK(fesgas::floor_fix(0x1p14 + 0x1p-38) == (Fix(1) << 94) + (Fix(1) << 42));
    Fix sum[4] = { 0, 0, 0, 0 };
    unsigned long long out = 0;
    const double u0[3] = { 0.5, -0.25, 0.0 }, w[3] = { 0.0, 0.25, 1.0 };
    fesgas::tally(u0, w, sum, out);
    CHECK(out == 0 && sum[0] == fesgas::floor_fix(1.0625) - fesgas::floor_fix(0.3125) && sum[1] == ~(Fix(1) << 79) + 1 && sum[2] == (Fix(1) << 79) && sum[3] == (Fix(1) << 80));
    const double big[3] = { 200.0, 0.0, 0.0 }, far[3] = { 0.0, -40000.0, kNan };
    fesgas::tally(big, w, sum, out);                                         // |v|^2 = 40000 >= 2^15: energy outside, vx inside
    CHECK(out == 0x1);
    out = 0;
    fesgas::tally(u0, far, sum, out);
    CHECK(out == (0x1 | 0x4 | 0x8));
    // the words: candidates, below, above | the forces' ten
    uint64_t a[fesgas::kWords] = { 9, 2, 1, 7, ~uint64_t(0), 0, 5, ~uint64_t(0), 1, 2, 3, 4, 0x5 };
    uint64_t b[fesgas::kWords] = { 1, 1, 1, 1, 1, 0, ~uint64_t(0), 0, 9, 9, 9, 9, 0x4 };
    uint64_t s1[fesgas::kSumWords], s2[fesgas::kSumWords], back[fesgas::kWords];
    fesgas::split_words(a, s1);
    fesgas::split_words(b, s2);
    for (int k = 0; k < fesgas::kSumWords; ++k) s1[k] += s2[k];
    fesgas::join_words(s1, back);
    CHECK(back[0] == 10 && back[1] == 3 && back[2] == 2 && back[3] == 8 && back[4] == 0 && back[5] == 1);   // the carry reaches the high word
    CHECK(back[6] == 4 && back[7] == 0 && back[8] == 10 && back[9] == 11 && back[10] == 12 && back[11] == 13 && back[12] == 0x5);
    fpic_gas_result res;
    std::memset(&res, 0, sizeof res);
    const uint64_t words[fesgas::kWords] = { 11, 4, 3, 2, 0, 1, ~uint64_t(0), ~uint64_t(0), 0, 0, uint64_t(1) << 40, 0, 0x4 };
    fesgas::result_of(words, 2.0, 3.0, &res);
    const double ke = 0.5 * 2.0 * 3.0 * fesgas::kC * fesgas::kC, pm = 2.0 * 3.0 * fesgas::kC;
    CHECK(res.candidates == 11 && res.below == 4 && res.above == 3 && res.collided == 2 && res.applications == 0);
    CHECK(res.energy == ke * 0x1p-16 && res.momentum[0] == pm * -0x1p-80 && std::isnan(res.momentum[1]) && res.momentum[2] == pm * 0x1p-40);
    CHECK(res.energy_fixed[1] == 1 && res.momentum_fixed[0][0] == ~uint64_t(0) && res.momentum_fixed[2][0] == uint64_t(1) << 40);
}

static void refusals()
{
    CHECK(says(fesgas::check(nullptr, 1, kL), ".spec <- Non-optional property is undefined!"));
    fpic_gas_spec s = good();
    CHECK(fesgas::check(&s, 1, kL) == nullptr);
    for (int k : { 2, -1 }) { s = good(); s.kind = k; CHECK(says(fesgas::check(&s, 1, kL), ".kind <- must be 0 (exchange) or 1 (elastic)")); }
    s = good(); s.species = 1; CHECK(says(fesgas::check(&s, 1, kL), ".species <- no such species")); CHECK(fesgas::check(&s, 2, kL) == nullptr);
    s = good(); s.species = -1; CHECK(says(fesgas::check(&s, 1, kL), ".species <- no such species"));
    s = good(); s.reserved_i = 1; CHECK(says(fesgas::check(&s, 1, kL), ".reserved <- must be zero"));
    s = good(); s.reserved_u = 1; CHECK(says(fesgas::check(&s, 1, kL), ".reserved <- must be zero"));
    s = good(); s.reserved[3] = 1e-300; CHECK(says(fesgas::check(&s, 1, kL), ".reserved <- must be zero"));
    s = good(); s.reserved[0] = kNan; CHECK(says(fesgas::check(&s, 1, kL), ".reserved <- must be zero"));
    for (double bad : { -1e-300, kInf, -kInf, kNan }) { s = good(); s.density = bad; CHECK(says(fesgas::check(&s, 1, kL), ".density <- must be finite and not negative")); }
    s = good(); s.density = 0; CHECK(fesgas::check(&s, 1, kL) == nullptr);
    for (double bad : { 0.0, -1.0, kInf, kNan }) { s = good(); s.tau = bad; CHECK(says(fesgas::check(&s, 1, kL), ".tau <- must be positive and finite")); }
    std::vector<double> table(FPIC_GAS_TABLE_MAX + 1, 1e-19);
    for (int n : { 1, 0, -3, FPIC_GAS_TABLE_MAX + 1 }) { s = good(); s.sigma = table.data(); s.n = n; CHECK(says(fesgas::check(&s, 1, kL), ".n <- must be 2 .. FPIC_GAS_TABLE_MAX (4096)")); }
    s = good(); s.sigma = table.data(); s.n = FPIC_GAS_TABLE_MAX; CHECK(fesgas::check(&s, 1, kL) == nullptr);
    s = good(); s.sigma = nullptr; CHECK(says(fesgas::check(&s, 1, kL), ".sigma <- Non-optional property is undefined!"));
    for (double bad : { -0.1, kInf, kNan }) { s = good(); s.g_lo = bad; CHECK(says(fesgas::check(&s, 1, kL), ".g_lo <- must be finite and not negative")); }
    for (double bad : { 0.0, -1.0, kInf, kNan }) { s = good(); s.g_hi = bad; CHECK(says(fesgas::check(&s, 1, kL), ".g_hi <- must be finite and above g_lo")); }
    for (double bad : { -1e-30, kInf, kNan }) {
        table[4095] = bad;
        s = good(); s.sigma = table.data(); s.n = FPIC_GAS_TABLE_MAX; CHECK(says(fesgas::check(&s, 1, kL), ".sigma <- every entry must be finite and not negative"));
        s.n = 4095; CHECK(fesgas::check(&s, 1, kL) == nullptr);
        table[4095] = 1e-19;
    }
    for (double bad : { kInf, -kInf, kNan }) {
        s = good(); s.drift[1] = bad; CHECK(says(fesgas::check(&s, 1, kL), ".drift <- must be finite"));
        s = good(); s.vth[2] = bad; CHECK(says(fesgas::check(&s, 1, kL), ".vth <- must be finite and not negative"));
        s = good(); s.lo[1] = bad; CHECK(says(fesgas::check(&s, 1, kL), ".lo, .hi <- must be finite"));
        s = good(); s.hi[2] = bad; CHECK(says(fesgas::check(&s, 1, kL), ".lo, .hi <- must be finite"));
    }
    s = good(); s.vth[0] = -1e-9; CHECK(says(fesgas::check(&s, 1, kL), ".vth <- must be finite and not negative"));
    const char* elastic = ".mass_ratio <- must be positive (+inf: a fixed target) for FPIC_GAS_ELASTIC";
    for (double bad : { 0.0, -1.0, kNan }) { s = good(); s.kind = FPIC_GAS_ELASTIC; s.mass_ratio = bad; CHECK(says(fesgas::check(&s, 1, kL), elastic)); }
    s = good(); s.kind = FPIC_GAS_ELASTIC; s.mass_ratio = kInf; CHECK(fesgas::check(&s, 1, kL) == nullptr);
    for (double bad : { 1.0, kInf, kNan }) { s = good(); s.mass_ratio = bad; CHECK(says(fesgas::check(&s, 1, kL), ".mass_ratio <- must be 0 for FPIC_GAS_EXCHANGE")); }
    const char* window = ".lo, .hi <- the window must lie within 0 <= lo < hi <= L";
    s = good(); s.lo[0] = -1e-300; CHECK(says(fesgas::check(&s, 1, kL), window));
    s = good(); s.hi[2] = kL[2] * 1.0000001; CHECK(says(fesgas::check(&s, 1, kL), window));
    s = good(); s.lo[1] = s.hi[1] = kL[1] / 2; CHECK(says(fesgas::check(&s, 1, kL), window));
    s = good(); s.lo[1] = kL[1]; s.hi[1] = kL[1] / 2; CHECK(says(fesgas::check(&s, 1, kL), window));
    std::vector<double> tab(FPIC_GAS_TAPER_MAX + 1, 1.0);
    for (uint32_t n : { 1u, static_cast<uint32_t>(FPIC_GAS_TAPER_MAX + 1), ~0u }) {
        s = good(); s.taper_n[1] = n; s.taper[1] = tab.data(); CHECK(says(fesgas::check(&s, 1, kL), ".taper_n <- a table has 2 .. FPIC_GAS_TAPER_MAX nodes (0: none)"));
    }
    s = good(); s.taper_n[2] = 2; CHECK(says(fesgas::check(&s, 1, kL), ".taper <- a table is null but its node count is not zero"));
    s = good(); s.taper_n[0] = FPIC_GAS_TAPER_MAX; s.taper[0] = tab.data(); CHECK(fesgas::check(&s, 1, kL) == nullptr);
    for (double bad : { 1.0000001, -1e-300, kInf, kNan }) {
        tab[1024] = bad;
        s = good(); s.taper_n[0] = FPIC_GAS_TAPER_MAX; s.taper[0] = tab.data();
        CHECK(says(fesgas::check(&s, 1, kL), ".taper <- the nodes must lie in [0, 1] (the density as a fraction of its peak)"));
        s.taper_n[0] = 1024; CHECK(fesgas::check(&s, 1, kL) == nullptr);
        tab[1024] = 1.0;
    }
    tab[0] = 0.0;
    s = good(); s.taper_n[0] = 2; s.taper[0] = tab.data(); CHECK(fesgas::check(&s, 1, kL) == nullptr);      // 0 and 1 themselves are allowed
    const double huge[2] = { 1e300, 1e300 };
    s = good(); s.density = 1e300; s.sigma = huge; s.n = 2; CHECK(says(fesgas::check(&s, 1, kL), ".sigma <- the candidate bound density c tau max(sigma g) is not a finite number"));
}

// ---- cases from a file.  Per case, little endian: int32 kind, n, precision (0: float, 1: double), 0; uint64 seed; uint32 stream,
// epoch; double density, tau, g_lo, g_hi, drift[3], vth[3], mass_ratio, L[3], lo[3], hi[3]; uint32 taper_n[3], 0; the n
// cross-sections; the tapers' doubles; uint32 count, first id; count x 6 doubles (p, v).  Out per case, as 64-bit words: the
// doubles column, x_max, then K; per particle candidate (0 / 1), what, and the stored v'[3] as doubles; then the thirteen
// words of the tallies.
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
        fpic_gas_spec s;
        std::memset(&s, 0, sizeof s);
        int32_t precision = 0, pad = 0;
        double L[3];
        bool ok = get(in, &s.kind) && get(in, &s.n) && get(in, &precision) && get(in, &pad) && get(in, &s.seed) && get(in, &s.stream) && get(in, &s.epoch) &&
                  get(in, &s.density) && get(in, &s.tau) && get(in, &s.g_lo) && get(in, &s.g_hi) && get(in, s.drift, 3) && get(in, s.vth, 3) && get(in, &s.mass_ratio) &&
                  get(in, L, 3) && get(in, s.lo, 3) && get(in, s.hi, 3) && get(in, s.taper_n, 3) && get(in, &s.reserved_u);
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
        uint32_t n = 0, first = 0;
        ok = ok && get(in, &n) && get(in, &first);
        if (!ok) { std::printf("FAILED: case %u is cut short\n", c); return 1; }
        std::vector<double> state(static_cast<size_t>(n) * 6);
        if (n && !get(in, state.data(), state.size())) { std::printf("FAILED: case %u is cut short\n", c); return 1; }
        const double Lb[3] = { L[0], L[1], L[2] };
        if (const char* why = fesgas::check(&s, 1, Lb)) { std::printf("FAILED: case %u is refused: %s\n", c, why); return 1; }
        const fesgas::Rule r = fesgas::rule_of(s, Lb, s.epoch, s.sigma, s.sigma, s.taper);
        put(out, r.column);
        put(out, r.x_max);
        put(out, static_cast<uint64_t>(r.K));
        uint64_t count[4] = { 0, 0, 0, 0 };
        unsigned long long bits = 0;
        fesgas::Fix sum[4] = { 0, 0, 0, 0 };
        for (uint32_t i = 0; i < n; ++i) {
            const double p[3] = { state[6 * i], state[6 * i + 1], state[6 * i + 2] };
            const double u0[3] = { state[6 * i + 3], state[6 * i + 4], state[6 * i + 5] };
            double v[3] = { u0[0], u0[1], u0[2] };
            bool cand = false;
            const int what = fesgas::apply(r, first + i, p, v, &cand);
            double w[3] = { u0[0], u0[1], u0[2] };
            if (what & fesgas::kCollided) {
                for (int a = 0; a < 3; ++a) w[a] = precision ? v[a] : static_cast<double>(static_cast<float>(v[a]));
                fesgas::tally(u0, w, sum, bits);
            }
            count[0] += cand ? 1 : 0;
            count[1] += what & fesgas::kBelow ? 1 : 0;
            count[2] += what & fesgas::kAbove ? 1 : 0;
            count[3] += what & fesgas::kCollided ? 1 : 0;
            put(out, static_cast<uint64_t>(cand ? 1 : 0));
            put(out, static_cast<uint64_t>(what));
            for (int a = 0; a < 3; ++a) put(out, w[a]);
        }
        for (int k = 0; k < 4; ++k) put(out, count[k]);
        for (int k = 0; k < 4; ++k) {
            put(out, static_cast<uint64_t>(sum[k]));
            put(out, static_cast<uint64_t>(sum[k] >> 64));
        }
        put(out, static_cast<uint64_t>(bits));
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}

int main(int argc, char** argv)
{
    numbers();
    rule();
    tallies();
    refusals();
    if (argc == 3 && run_cases(argv[1], argv[2])) return 1;
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
