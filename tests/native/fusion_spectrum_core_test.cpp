// Host test of fusion-sim_amd/csrc/fes_fusion_spectrum_core.hpp (the rule of the fusion product spectrum and the checks of a
// request).  Without an argument: the host numbers of a request by hand, one try of the isotropic direction (a hit, a miss, the
// unit norm), the direction's blocks against the loader's generator with the tags of both sides, the sixteen-rejection
// fallback through try_direction, the kinematics by hand (a pair at rest, Et <= 0), values on lo, on an inner edge and on hi,
// and every refusal by its message; prints "ok" and exits 0, or names the first failed check and exits 1.
// With a file name: reads a request and pairs written by tests/test_fusion_spectrum_host.py (hexadecimal doubles: "n g_lo g_hi
// tau W dV", n table entries, "axis bins like seed stream epoch", "lo hi q_value m3 m4 lx ly lz m_a m_b", "m", then m lines
// "N_L id side_b vo[3] vp[3]", side_b ignored for like species) and prints "e <exponent>" and per pair "<what> <q> <entry> <x> <try>" (entry, x and try only
// mean something inside the table) — the test compares them with tests/fusion_spectrum_reference.py, bit for bit.
// Built with g++ -ffp-contract=off by tests/test_fusion_spectrum_host.py (also with -fsanitize=address,undefined, as a
// program of its own).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../include/fusionpic.h"
#include "../../fusion-sim_amd/csrc/fes_fusion_spectrum_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static const double kEps = std::numeric_limits<double>::epsilon();
static double table4[4] = { 1e-28, 2e-28, 4e-28, 3e-28 };
static const double MD = 3.3435837724e-27, MT = 5.0073567446e-27, MN = 1.67492749804e-27, MA = 6.6446573357e-27;
static const double MEV = 1.602176634e-13;

static fpic_fusion_spectrum_spec good()
{
    fpic_fusion_spectrum_spec s;
    std::memset(&s, 0, sizeof s);
    s.tally.species_a = 0; s.tally.species_b = 1;
    s.tally.seed = 0x0123456789abcdefull; s.tally.stream = 5; s.tally.epoch = 3;
    s.tally.tau = 1e-9; s.tally.g_lo = 0.0078125; s.tally.g_hi = 0.03125;
    s.tally.n = 4; s.tally.sigma = table4;
    s.axis = FPIC_FSPEC_PRODUCT; s.bins = 8;
    s.lo = 13.0 * MEV; s.hi = 15.0 * MEV;
    s.q_value = 17.59 * MEV; s.product_mass = MN; s.other_mass = MA;
    return s;
}
static bool says(const char* msg, const char* text) { return msg && std::strcmp(msg, text) == 0; }

static void numbers()
{
    fpic_fusion_spectrum_spec s = good();
    s.los[0] = 3.0; s.los[1] = 0.0; s.los[2] = -4.0;
    const fesfspec::Rule r = fesfspec::rule_of(s, MD, MT);
    const double M = MD + MT, cc = 2.998e8 * 2.998e8;
    CHECK(r.axis == FPIC_FSPEC_PRODUCT && r.bins == 8 && r.sight == 1 && r.lo == s.lo && r.hi == s.hi && r.q_value == s.q_value);
    CHECK(r.f_a == MD / M && r.f_b == MT / M && r.hk == (0.5 * ((MD * MT) / M)) * cc);
    CHECK(r.kf == ((2.0 * MA) / (MN * (MN + MA))) / cc && r.h3 == (0.5 * MN) * cc && r.inv_w == 8.0 / (s.hi - s.lo));
    CHECK(r.n[0] == 3.0 / 5.0 && r.n[1] == 0.0 && r.n[2] == -4.0 / 5.0);
    s = good();
    CHECK(fesfspec::rule_of(s, MD, MT).sight == 0);
    CHECK(fesfspec::rule_of(s, MD, MD).f_a == 0.5 && fesfspec::rule_of(s, MD, MD).f_b == 0.5);      // like species: equal fractions
    s.axis = FPIC_FSPEC_CM;
    CHECK(fesfspec::rule_of(s, MD, MT).hk == r.hk);
}

static void direction()
{
    double n[3] = { 9, 9, 9 };
    // the centre of the square: x1 = x2 = 2^-32, s tiny, n = (tiny, tiny, 1 - 2 s)
    CHECK(fesfspec::unit_of(0x80000000u) == 0x1p-32 && fesfspec::unit_of(0u) == 0x1p-32 - 1.0 && fesfspec::unit_of(0xFFFFFFFFu) == 1.0 - 0x1p-32);
    CHECK(fesfspec::try_direction(0x80000000u, 0x80000000u, n) && n[2] == 1.0 - 2.0 * (0x1p-64 + 0x1p-64) && n[0] == (2.0 * 0x1p-32) * std::sqrt(1.0 - 0x1p-63));
    // a corner is outside the disc and leaves n alone
    double keep[3] = { 7, 7, 7 };
    CHECK(!fesfspec::try_direction(0u, 0u, keep) && !fesfspec::try_direction(0xFFFFFFFFu, 0u, keep) && keep[0] == 7 && keep[2] == 7);
    // x1 = -0.5, x2 = 0.5 - 2^-32... a hand value: w = 2^30 gives x1 = (2^30 + 0.5) 2^-31 - 1 = -0.5 + 2^-32
    const double x = -0.5 + 0x1p-32, sx = x * x + x * x, rx = std::sqrt(1.0 - sx);
    CHECK(fesfspec::try_direction(0x40000000u, 0x40000000u, n) && n[0] == (2.0 * x) * rx && n[1] == n[0] && n[2] == 1.0 - 2.0 * sx);
    // the unit norm of every accepted try of a lattice of words and of random blocks
    uint32_t word = 12345u;
    int hits = 0;
    for (int k = 0; k < 20000; ++k) {
        uint32_t w[4];
        fesload::philox(static_cast<uint32_t>(k), 1u, 2u, 3u, 4u, 5u, w);
        word = word * 1664525u + 1013904223u;
        for (int t = 0; t < 2; ++t)
            if (fesfspec::try_direction(w[2 * t], t ? word : w[2 * t + 1], n)) {
                ++hits;
                CHECK(std::fabs(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) - 1.0) <= 4 * kEps);
            }
    }
    CHECK(hits > 30000 && hits < 33000);      // pi / 4 of 40000
    // direction_of: the first accepted try of the blocks with the tags 0xF0520 + a (+ 16 on species_b's side)
    const fesfusion::Rule r = fesfusion::rule_of(good().tally, 77u, 1e10, 1.0);
    int late = 0;
    for (uint32_t id = 0; id < 4000; ++id)
        for (int side = 0; side < 2; ++side) {
            double want[3] = { 0, 0, 1 };
            int at = fesfspec::kTries;
            for (int a = 0; a < fesfspec::kBlocks && at == fesfspec::kTries; ++a) {
                uint32_t w[4];
                fesload::philox(id, 77u, 5u, 0xF0520u + (side ? 16u : 0u) + static_cast<uint32_t>(a), 0x89abcdefu, 0x01234567u, w);
                if (fesfspec::try_direction(w[0], w[1], want)) at = 2 * a;
                else if (fesfspec::try_direction(w[2], w[3], want)) at = 2 * a + 1;
            }
            const int got = fesfspec::direction_of(r, id, side != 0, n);
            CHECK(got == at && n[0] == want[0] && n[1] == want[1] && n[2] == want[2] && got < fesfspec::kTries);
            late += got > 0;
        }
    CHECK(late > 1000 && late < 2500);        // 1 - pi / 4 of 8000
    // the fallback: sixteen rejections through the try helper, as direction_of runs them
    double fb[3] = { 0.0, 0.0, 1.0 };
    int tries = 0;
    while (tries < fesfspec::kTries && !fesfspec::try_direction(0xFFFFFFFFu, 0xFFFFFF00u, fb)) ++tries;
    CHECK(tries == fesfspec::kTries && fb[0] == 0.0 && fb[1] == 0.0 && fb[2] == 1.0);
    CHECK(fesfspec::kTries == 16 && fesfspec::kDirTag == 0xF0520u && fesfspec::kDirSide == 16u);
}

static void kinematics()
{
    fpic_fusion_spectrum_spec s = good();
    s.los[2] = 2.0;
    const fesfspec::Rule r = fesfspec::rule_of(s, MD, MT);
    const double n[3] = { r.n[0], r.n[1], r.n[2] };
    CHECK(n[0] == 0.0 && n[1] == 0.0 && n[2] == 1.0);
    // a pair at rest in the laboratory: K = 0, the product has its share of q_value exactly as the rule orders it
    const double zero[3] = { 0.0, 0.0, 0.0 };
    CHECK(fesfspec::speed_of(zero, zero) == 0.0 && fesfspec::cm_energy(r, 0.0) == 0.0);
    const double u3 = std::sqrt(s.q_value * r.kf);
    const double e0 = fesfspec::product_energy(r, 0.0, r.f_a, r.f_b, zero, zero, n);
    CHECK(e0 == r.h3 * ((0.0 + 0.0) + u3 * u3) && std::fabs(e0 / (MA / (MN + MA) * s.q_value) - 1.0) < 1e-14);
    // a moving pair by hand, every operation in the stated order
    const double vo[3] = { 0.01, -0.002, 0.003 }, vp[3] = { -0.004, 0.001, 0.0005 };
    const double g = fesfspec::speed_of(vo, vp);
    const double ux = vo[0] - vp[0], uy = vo[1] - vp[1], uz = vo[2] - vp[2];
    CHECK(g == std::sqrt((ux * ux + uy * uy) + uz * uz));
    const double K = fesfspec::cm_energy(r, g);
    CHECK(K == r.hk * (g * g));
    const double et = s.q_value + K, u = std::sqrt(et * r.kf);
    double w[3];
    for (int i = 0; i < 3; ++i) w[i] = (r.f_a * vo[i] + r.f_b * vp[i]) + u * n[i];
    CHECK(fesfspec::product_energy(r, K, r.f_a, r.f_b, vo, vp, n) == r.h3 * ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]));
    // Et <= 0: an endothermic reaction below its threshold emits the product with the centre of mass
    s.q_value = -1.0 * MEV;
    const fesfspec::Rule neg = fesfspec::rule_of(s, MD, MT);
    for (int i = 0; i < 3; ++i) w[i] = neg.f_a * vo[i] + neg.f_b * vp[i];
    CHECK(s.q_value + K < 0 && fesfspec::product_energy(neg, K, neg.f_a, neg.f_b, vo, vp, n) == neg.h3 * ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]));
    s.q_value = -K;                    // Et == 0 exactly
    const fesfspec::Rule nul = fesfspec::rule_of(s, MD, MT);
    CHECK(fesfspec::product_energy(nul, K, nul.f_a, nul.f_b, vo, vp, n) == neg.h3 * ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]));
    CHECK(fesfspec::entry_of(nul, fesfspec::product_energy(nul, kNan, nul.f_a, nul.f_b, vo, vp, n)) >= 0);   // (a NaN is held to 0 too)
}

static void binning()
{
    fpic_fusion_spectrum_spec s = good();
    s.lo = 1.0; s.hi = 3.0; s.bins = 8;       // edges at quarters: inv_w = 4 exactly
    const fesfspec::Rule r = fesfspec::rule_of(s, MD, MT);
    CHECK(r.inv_w == 4.0);
    CHECK(fesfspec::entry_of(r, 1.0) == 0 && fesfspec::entry_of(r, std::nextafter(1.0, 0.0)) == 8 && fesfspec::entry_of(r, -kInf) == 8);      // lo is inside
    CHECK(fesfspec::entry_of(r, 1.25) == 1 && fesfspec::entry_of(r, std::nextafter(1.25, 0.0)) == 0 && fesfspec::entry_of(r, 2.0) == 4);    // an inner edge opens its bin
    CHECK(fesfspec::entry_of(r, 3.0) == 9 && fesfspec::entry_of(r, std::nextafter(3.0, 0.0)) == 7 && fesfspec::entry_of(r, kInf) == 9);      // hi is over
    CHECK(fesfspec::entry_of(r, kNan) == 9);
    s.bins = 1;
    const fesfspec::Rule one = fesfspec::rule_of(s, MD, MT);
    CHECK(fesfspec::entry_of(one, 1.0) == 0 && fesfspec::entry_of(one, 2.999) == 0 && fesfspec::entry_of(one, 0.5) == 1 && fesfspec::entry_of(one, 3.0) == 2);
    // a range whose last rounding would reach `bins`: the clamp
    s.bins = 7; s.lo = 0.0; s.hi = 0.7;
    const fesfspec::Rule odd = fesfspec::rule_of(s, MD, MT);
    CHECK(fesfspec::entry_of(odd, std::nextafter(0.7, 0.0)) == 6);
}

static void refusals()
{
    CHECK(says(fesfspec::check(nullptr, 2), ".spec <- Non-optional property is undefined!"));
    fpic_fusion_spectrum_spec s = good();
    CHECK(fesfspec::check(&s, 2) == nullptr);
    // the tally's refusals pass through
    CHECK(says(fesfspec::check(&s, 1), ".species_b <- no such species"));
    s.tally.tau = 0.0; CHECK(says(fesfspec::check(&s, 2), ".tau <- must be positive and finite"));
    s = good(); s.tally.reserved[1] = 1.0; CHECK(says(fesfspec::check(&s, 2), ".reserved <- must be zero"));
    s = good(); s.tally.sigma = nullptr; CHECK(says(fesfspec::check(&s, 2), ".sigma <- Non-optional property is undefined!"));
    for (int k = 0; k < 4; ++k) {
        s = good(); s.reserved[k] = 1e-300; CHECK(says(fesfspec::check(&s, 2), ".reserved <- must be zero"));
        s = good(); s.reserved[k] = kNan; CHECK(says(fesfspec::check(&s, 2), ".reserved <- must be zero"));
    }
    for (int bad : { -1, 2, 7 }) {
        s = good(); s.axis = bad; CHECK(says(fesfspec::check(&s, 2), ".axis <- must be FPIC_FSPEC_CM (0) or FPIC_FSPEC_PRODUCT (1)"));
    }
    for (int bad : { 0, -1, 257 }) {
        s = good(); s.bins = bad; CHECK(says(fesfspec::check(&s, 2), ".bins <- must be 1 .. FPIC_FUSION_SPECTRUM_BINS_MAX (256)"));
    }
    s = good(); s.bins = 1; CHECK(fesfspec::check(&s, 2) == nullptr);
    s = good(); s.bins = 256; CHECK(fesfspec::check(&s, 2) == nullptr);
    for (double bad : { kInf, -kInf, kNan }) {
        s = good(); s.lo = bad; CHECK(says(fesfspec::check(&s, 2), ".lo <- must be finite"));
    }
    for (double bad : { 13.0 * MEV, 0.0, -1.0, kInf, kNan }) {
        s = good(); s.hi = bad; CHECK(says(fesfspec::check(&s, 2), ".hi <- must be finite and above lo"));
    }
    s = good(); s.lo = -2.0; s.hi = -1.0; CHECK(fesfspec::check(&s, 2) == nullptr);
    for (double bad : { kInf, -kInf, kNan }) {
        s = good(); s.q_value = bad; CHECK(says(fesfspec::check(&s, 2), ".q_value <- must be finite"));
    }
    s = good(); s.q_value = -1.0; CHECK(fesfspec::check(&s, 2) == nullptr);
    for (double bad : { 0.0, -1.0, kInf, kNan }) {
        s = good(); s.product_mass = bad; CHECK(says(fesfspec::check(&s, 2), ".product_mass <- must be positive and finite"));
        s = good(); s.other_mass = bad; CHECK(says(fesfspec::check(&s, 2), ".other_mass <- must be positive and finite"));
        s = good(); s.axis = FPIC_FSPEC_CM; s.product_mass = bad; s.other_mass = bad; CHECK(fesfspec::check(&s, 2) == nullptr);    // ignored for CM
    }
    for (int k = 0; k < 3; ++k)
        for (double bad : { kInf, -kInf, kNan }) {
            s = good(); s.los[k] = bad; CHECK(says(fesfspec::check(&s, 2), ".los <- must be finite"));
        }
    s = good(); s.los[0] = 1e-200; CHECK(says(fesfspec::check(&s, 2), ".los <- must be all zero (isotropic) or have a non-zero, finite norm"));
    s = good(); s.los[1] = 1e200; CHECK(says(fesfspec::check(&s, 2), ".los <- must be all zero (isotropic) or have a non-zero, finite norm"));
    s = good(); s.los[2] = -1.0; CHECK(fesfspec::check(&s, 2) == nullptr);
}

// the file's pairs through the rule: see the head of this file
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
    auto whole = [&]() {
        if (std::fscanf(f, "%63s", word) != 1) { bad = true; return 0ull; }
        return std::strtoull(word, nullptr, 0);
    };
    fpic_fusion_spectrum_spec s = good();
    const int n = static_cast<int>(num());
    s.tally.g_lo = num(); s.tally.g_hi = num(); s.tally.tau = num();
    const double W = num(), dV = num();
    if (bad || n < 2 || n > FPIC_FUSION_TABLE_MAX) { std::fclose(f); std::printf("bad head\n"); return 2; }
    std::vector<double> S(static_cast<size_t>(n));
    for (double& x : S) x = num();
    s.tally.n = n; s.tally.sigma = S.data();
    s.axis = static_cast<int>(whole()); s.bins = static_cast<int>(whole());
    const bool like = whole() != 0;
    s.tally.species_b = like ? 0 : 1;
    s.tally.seed = whole(); s.tally.stream = static_cast<uint32_t>(whole()); s.tally.epoch = static_cast<uint32_t>(whole());
    s.lo = num(); s.hi = num(); s.q_value = num(); s.product_mass = num(); s.other_mass = num();
    for (double& x : s.los) x = num();
    const double m_a = num(), m_b = num();
    if (bad || fesfspec::check(&s, 2) || fesfusion::check_bound(s.tally, W, dV)) { std::fclose(f); std::printf("bad request\n"); return 2; }
    const fesfusion::Rule r = fesfusion::rule_of(s.tally, s.tally.epoch, W, dV);
    const fesfspec::Rule a = fesfspec::rule_of(s, m_a, m_b);
    std::printf("e %d\n", r.e);
    const long m = static_cast<long>(whole());
    for (long k = 0; k < m && !bad; ++k) {
        const double nl = num();
        const uint32_t id = static_cast<uint32_t>(whole());
        const bool side_b = whole() != 0 && !like;      // (like species have one side)
        double vo[3], vp[3];
        for (double& x : vo) x = num();
        for (double& x : vp) x = num();
        if (bad) break;
        int64_t q;
        const int what = fesfusion::tally(r, S.data(), nl, vo, vp, q);
        const double K = fesfspec::cm_energy(a, fesfspec::speed_of(vo, vp));
        double x = K;
        int tries = 0;
        if (a.axis == FPIC_FSPEC_PRODUCT) {
            double dir[3] = { a.n[0], a.n[1], a.n[2] };
            if (!a.sight) tries = fesfspec::direction_of(r, id, side_b, dir);
            x = fesfspec::product_energy(a, K, side_b ? a.f_b : a.f_a, like || side_b ? a.f_a : a.f_b, vo, vp, dir);
        }
        std::printf("%d %lld %d %a %d\n", what, static_cast<long long>(q), fesfspec::entry_of(a, x), x, tries);
    }
    std::fclose(f);
    return bad ? 2 : 0;
}

int main(int argc, char** argv)
{
    if (argc > 1) return from_file(argv[1]);
    numbers();
    direction();
    kinematics();
    binning();
    refusals();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
