// Host test of fusion-sim_amd/csrc/fes_fusion_core.hpp (the rule of the fusion yield tally and the checks of a request).
// Without an argument: the key's words against the loader's generator with the tally's own tag, who owns which pair in a cell
// (by hand for like N = 0 .. 7, the weights' sums for like and unlike cells), the interpolation at the table's edges, the
// fixed point (the exponent of hand cases, q < 2^40 at the bound, the join of the two total words), and every refusal by its
// message; prints "ok" and exits 0, or names the first failed check and exits 1.
// With a file name: reads a request and pairs written by tests/test_fusion_host.py (hexadecimal doubles: "n g_lo g_hi tau W
// dV", n table entries, "m", then m lines "N_L vo[3] vp[3]") and prints "e <exponent>" and per pair "<what> <q>" — the test
// compares them with the integers of tests/fusion_reference.py, bit for bit.
// Built with g++ -ffp-contract=off by tests/test_fusion_host.py (also with -fsanitize=address,undefined, as a program of its
// own).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../include/fusionpic.h"
#include "../../fusion-sim_amd/csrc/fes_fusion_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static double table4[4] = { 1e-28, 2e-28, 4e-28, 3e-28 };

static fpic_fusion_spec good()
{
    fpic_fusion_spec s;
    std::memset(&s, 0, sizeof s);
    s.species_a = 0; s.species_b = 1;
    s.seed = 0x0123456789abcdefull; s.stream = 5; s.epoch = 3;
    s.tau = 1e-9; s.g_lo = 0.0078125; s.g_hi = 0.03125;
    s.n = 4; s.sigma = table4;
    return s;
}
static bool says(const char* msg, const char* text) { return msg && std::strcmp(msg, text) == 0; }

static void key()
{
    const fesfusion::Rule r = fesfusion::rule_of(good(), 77u, 1e10, 1.0);
    CHECK(r.epoch == 77u && r.stream == 5u && r.seed_lo == 0x89abcdefu && r.seed_hi == 0x01234567u && r.like == 0 && r.n == 4);
    for (uint32_t id : { 0u, 1u, 0xFFFFFFFFu }) {
        uint32_t direct[4], pair_tag[4];
        fesload::philox(id, 77u, 5u, 0xF0510u, 0x89abcdefu, 0x01234567u, direct);
        fesload::philox(id, 77u, 5u, 0xC0120u, 0x89abcdefu, 0x01234567u, pair_tag);
        CHECK(fesfusion::key_of(r, id) == direct[0] && direct[0] != pair_tag[0]);
    }
    fpic_fusion_spec s = good();
    s.species_b = 0;
    CHECK(fesfusion::rule_of(s, 0u, 1.0, 1.0).like == 1);
}

static void pairing()
{
    CHECK(fesfusion::many_is_a(4u, 4u) && fesfusion::many_is_a(5u, 2u) && !fesfusion::many_is_a(3u, 4u) && fesfusion::many_is_a(1u, 0u) && !fesfusion::many_is_a(0u, 2u));
    // like species, N = 0 .. 7: the partner of every place (-1: the place owns no pair) and twice its N_L
    static const int partner[8][7] = { { -1 }, { -1 }, { 1, -1 }, { 1, 2, 0 }, { 1, -1, 3, -1 }, { 1, 2, 0, 4, -1 }, { 1, -1, 3, -1, 5, -1 }, { 1, 2, 0, 4, -1, 6, -1 } };
    static const int twice_nl[8][7] = { { 0 }, { 0 }, { 4, 0 }, { 3, 3, 3 }, { 8, 0, 8, 0 }, { 5, 5, 5, 10, 0 }, { 12, 0, 12, 0, 12, 0 }, { 7, 7, 7, 14, 0, 14, 0 } };
    for (uint32_t n = 0; n < 8; ++n)
        for (uint32_t q = 0; q < n; ++q) {
            uint32_t p = 99;
            double nl = -1;
            const bool has = fesfusion::like_pair(n, q, p, nl);
            CHECK(has == (partner[n][q] >= 0));
            if (has) CHECK(static_cast<int>(p) == partner[n][q] && 2 * nl == twice_nl[n][q]);
        }
    // the like weights add to N N / 2 exactly, every particle is in one pair or in two of the triple, a partner is in the cell
    for (uint32_t n = 0; n < 2050; ++n) {
        double sum = 0;
        std::vector<int> seen(n, 0);
        for (uint32_t q = 0; q < n; ++q) {
            uint32_t p;
            double nl;
            if (!fesfusion::like_pair(n, q, p, nl)) continue;
            CHECK(p < n && p != q);
            if (p >= n) return;
            seen[q]++; seen[p]++;
            sum += nl;
        }
        CHECK(sum == 0.5 * n * n || n < 2);
        if (n < 2) CHECK(sum == 0);
        for (uint32_t q = 0; q < n && n >= 2; ++q) CHECK(seen[q] == ((n & 1u) && q < 3 ? 2 : 1));
    }
    // unlike: Nm pairs of N_L = Nf add to Na Nb; many[j] meets few[j mod Nf]
    for (auto c : { std::initializer_list<uint32_t>{ 1, 1 }, { 3, 2 }, { 2, 5 }, { 130, 7 }, { 2048, 2048 } }) {
        const uint32_t na = c.begin()[0], nb = c.begin()[1];
        const bool a_many = fesfusion::many_is_a(na, nb);
        const uint32_t nm = a_many ? na : nb, nf = a_many ? nb : na;
        double sum = 0;
        for (uint32_t j = 0; j < nm; ++j) sum += static_cast<double>(nf);
        CHECK(sum == static_cast<double>(na) * nb && nm >= nf);
    }
}

static int one(const fesfusion::Rule& r, const double* S, double nl, double gx, int64_t& q)
{
    const double vo[3] = { gx, 0.0, 0.0 }, vp[3] = { 0.0, 0.0, 0.0 };
    return fesfusion::tally(r, S, nl, vo, vp, q);
}

static void edges()
{
    // nodes at 1/128, 2/128, 3/128, 4/128: inv_dg = 128 exactly
    const fesfusion::Rule r = fesfusion::rule_of(good(), 0u, 1e10, 1.0);
    CHECK(r.inv_dg == 128.0 && r.s_max == 4e-28);
    CHECK(fesfusion::sigma_at(r, table4, 0.0078125) == 1e-28);                  // g == g_lo reads the first node
    CHECK(fesfusion::sigma_at(r, table4, 0.015625) == 2e-28 && fesfusion::sigma_at(r, table4, 0.0234375) == 4e-28);   // on a node: the node
    CHECK(fesfusion::sigma_at(r, table4, 0.01171875) == 1e-28 + 0.5 * (2e-28 - 1e-28));
    const double last = std::nextafter(0.03125, 0.0);
    const double s_last = fesfusion::sigma_at(r, table4, last);                  // the last interval, just below its end
    CHECK(s_last > 3e-28 && s_last < 3e-28 * (1 + 1e-12));
    int64_t q = -1;
    CHECK(one(r, table4, 7.0, 0.0078125, q) == fesfusion::kInside && q > 0);
    CHECK(one(r, table4, 7.0, std::nextafter(0.0078125, 0.0), q) == fesfusion::kBelow && q == 0);
    CHECK(one(r, table4, 7.0, 0.03125, q) == fesfusion::kAbove && q == 0);       // g == g_hi is above
    CHECK(one(r, table4, 7.0, last, q) == fesfusion::kInside && q > 0);
    CHECK(one(r, table4, 7.0, 0.0, q) == fesfusion::kBelow && one(r, table4, 7.0, kNan, q) == fesfusion::kAbove && one(r, table4, 7.0, 1.0, q) == fesfusion::kAbove);
    // g_lo = 0: g = 0 is inside and yields 0
    fpic_fusion_spec s = good();
    s.g_lo = 0.0;
    const fesfusion::Rule z = fesfusion::rule_of(s, 0u, 1e10, 1.0);
    q = -1;
    CHECK(one(z, table4, 2048.0, 0.0, q) == fesfusion::kInside && q == 0);
    // the hand value of one pair: every operation in the stated order
    const double g = 0.015625;
    const double y = ((((1e10 * 1e10) * 7.0) * 1e-9) / 1.0) * (2e-28 * (g * 2.998e8));
    CHECK(one(r, table4, 7.0, g, q) == fesfusion::kInside && q == static_cast<int64_t>(std::floor(std::ldexp(y, -r.e))));
    // a two-entry table: one interval
    double two[2] = { 0.0, 8.0 };
    s = good(); s.n = 2; s.sigma = two; s.g_lo = 0.0; s.g_hi = 0.5;
    const fesfusion::Rule t = fesfusion::rule_of(s, 0u, 1.0, 1.0);
    CHECK(fesfusion::sigma_at(t, two, 0.25) == 4.0 && fesfusion::sigma_at(t, two, 0.0) == 0.0 && fesfusion::sigma_at(t, two, 0.375) == 6.0);
}

static void fixed_point()
{
    CHECK(fesfusion::exponent_of(0.0) == 0 && fesfusion::exponent_of(1.0) == -39 && fesfusion::exponent_of(0.75) == -40 && fesfusion::exponent_of(0x1p40) == 1);
    CHECK(fesfusion::exponent_of(std::nextafter(1.0, 0.0)) == -40 && fesfusion::exponent_of(1e-7) == -63 && fesfusion::exponent_of(5e-324) == fesfusion::kExponentMin);
    CHECK(fesfusion::exponent_of(std::numeric_limits<double>::max()) == 1024 - 40);
    CHECK(fesfusion::y_bound_of(1e10, 1e-9, 1.0, 4e-28, 0.03125) == ((((1e10 * 1e10) * 2048.0) * 1e-9) / 1.0) * (4e-28 * (0.03125 * 2.998e8)));
    // q < 2^40 at the bound: N_L = 2048 at the largest cross-section just below g_hi, for tables whose bound sits just under
    // and just over a power of two
    for (double W : { 1e10, 1.1e10, 1.4142e10, 3.3e7, 1e-3 })
        for (double top : { 4e-28, 3.999e-28, 5.1e-28 }) {
            double S[4] = { 1e-28, 2e-28, 3e-28, top };
            fpic_fusion_spec s = good();
            s.sigma = S;
            const fesfusion::Rule r = fesfusion::rule_of(s, 0u, W, 1.0);
            const double b = fesfusion::y_bound_of(W, s.tau, 1.0, r.s_max, s.g_hi);
            CHECK(b < std::ldexp(1.0, r.e + 40) && b >= std::ldexp(1.0, r.e + 39) && r.unit == std::ldexp(1.0, -r.e));
            int64_t q = 0;
            CHECK(one(r, S, 2048.0, std::nextafter(0.03125, 0.0), q) == fesfusion::kInside && q < (int64_t(1) << 40) && q >= (int64_t(1) << 38));
        }
    uint64_t hi, lo;
    fesfusion::join(5u, 0xFFFFFFFFull, hi, lo);
    CHECK(hi == 5u && lo == 0xFFFFFFFFull);
    fesfusion::join(5u, (7ull << 32) | 9ull, hi, lo);
    CHECK(hi == 12u && lo == 9u);
    fesfusion::join(0u, ~0ull, hi, lo);
    CHECK(hi == 0xFFFFFFFFull && lo == 0xFFFFFFFFull);
}

static void refusals()
{
    CHECK(says(fesfusion::check(nullptr, 2), ".spec <- Non-optional property is undefined!"));
    fpic_fusion_spec s = good();
    CHECK(fesfusion::check(&s, 2) == nullptr);
    CHECK(says(fesfusion::check(&s, 1), ".species_b <- no such species"));
    s.species_b = 0; CHECK(fesfusion::check(&s, 1) == nullptr);
    s = good(); s.species_a = 2; CHECK(says(fesfusion::check(&s, 2), ".species_a <- no such species"));
    s = good(); s.species_a = -1; CHECK(says(fesfusion::check(&s, 2), ".species_a <- no such species"));
    s = good(); s.species_b = -1; CHECK(says(fesfusion::check(&s, 2), ".species_b <- no such species"));
    s = good(); s.reserved_i = 1; CHECK(says(fesfusion::check(&s, 2), ".reserved <- must be zero"));
    for (int k = 0; k < 4; ++k) {
        s = good(); s.reserved[k] = 1e-300; CHECK(says(fesfusion::check(&s, 2), ".reserved <- must be zero"));
        s = good(); s.reserved[k] = kNan; CHECK(says(fesfusion::check(&s, 2), ".reserved <- must be zero"));
    }
    s = good(); s.tau = kNan; CHECK(says(fesfusion::check(&s, 2), ".tau <- must not be NaN"));
    for (double bad : { 0.0, -1.0, kInf, -kInf }) {
        s = good(); s.tau = bad; CHECK(says(fesfusion::check(&s, 2), ".tau <- must be positive and finite"));
    }
    for (int bad : { 1, 0, -1, 4097 }) {
        s = good(); s.n = bad; CHECK(says(fesfusion::check(&s, 2), ".n <- must be 2 .. FPIC_FUSION_TABLE_MAX (4096)"));
    }
    s = good(); s.sigma = nullptr; CHECK(says(fesfusion::check(&s, 2), ".sigma <- Non-optional property is undefined!"));
    for (double bad : { -1e-300, -1.0, kInf, -kInf, kNan }) {
        s = good(); s.g_lo = bad; CHECK(says(fesfusion::check(&s, 2), ".g_lo <- must be finite and not negative"));
    }
    for (double bad : { 0.0078125, 0.001, 0.0, -1.0, kInf, kNan }) {
        s = good(); s.g_hi = bad; CHECK(says(fesfusion::check(&s, 2), ".g_hi <- must be finite and above g_lo"));
    }
    for (double bad : { -1e-300, -1.0, kInf, -kInf, kNan })
        for (int k = 0; k < 4; ++k) {
            double S[4] = { 1e-28, 2e-28, 4e-28, 3e-28 };
            S[k] = bad;
            s = good(); s.sigma = S; CHECK(says(fesfusion::check(&s, 2), ".sigma <- every entry must be finite and not negative"));
        }
    std::vector<double> full(4096, 1e-28);
    s = good(); s.n = 4096; s.sigma = full.data(); CHECK(fesfusion::check(&s, 2) == nullptr);
    double zeros[2] = { 0.0, 0.0 };
    s = good(); s.n = 2; s.sigma = zeros; CHECK(fesfusion::check(&s, 2) == nullptr && fesfusion::check_bound(s, 1e10, 1.0) == nullptr);
    CHECK(fesfusion::rule_of(s, 0u, 1e10, 1.0).e == 0 && fesfusion::rule_of(s, 0u, 1e10, 1.0).s_max == 0.0);
    s = good(); CHECK(fesfusion::check_bound(s, 1e10, 1.0) == nullptr);
    CHECK(says(fesfusion::check_bound(s, 1e200, 1.0), ".sigma <- the yield bound W W 2048 tau max(sigma) g_hi c / dV is not a finite number"));
}

// the file's pairs through tally(): see the head of this file
static int from_file(const char* path)
{
    std::FILE* f = std::fopen(path, "r");
    if (!f) { std::printf("cannot open %s\n", path); return 2; }
    char word[64];
    bool bad = false;
    auto num = [&]() {
        if (std::fscanf(f, "%63s", word) != 1) { bad = true; return 0.0; }
        return std::strtod(word, nullptr);
    };
    const int n = static_cast<int>(num());
    const double g_lo = num(), g_hi = num(), tau = num(), W = num(), dV = num();
    if (bad || n < 2 || n > FPIC_FUSION_TABLE_MAX) { std::fclose(f); std::printf("bad head\n"); return 2; }
    std::vector<double> S(static_cast<size_t>(n));
    for (double& x : S) x = num();
    fpic_fusion_spec s = good();
    s.n = n; s.sigma = S.data(); s.g_lo = g_lo; s.g_hi = g_hi; s.tau = tau;
    if (bad || fesfusion::check(&s, 2) || fesfusion::check_bound(s, W, dV)) { std::fclose(f); std::printf("bad request\n"); return 2; }
    const fesfusion::Rule r = fesfusion::rule_of(s, 0u, W, dV);
    std::printf("e %d\n", r.e);
    const long m = static_cast<long>(num());
    for (long k = 0; k < m && !bad; ++k) {
        const double nl = num();
        double vo[3], vp[3];
        for (double& x : vo) x = num();
        for (double& x : vp) x = num();
        if (bad) break;
        int64_t q;
        const int what = fesfusion::tally(r, S.data(), nl, vo, vp, q);
        std::printf("%d %lld\n", what, static_cast<long long>(q));
    }
    std::fclose(f);
    return bad ? 2 : 0;
}

int main(int argc, char** argv)
{
    if (argc > 1) return from_file(argv[1]);
    key();
    pairing();
    edges();
    fixed_point();
    refusals();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
