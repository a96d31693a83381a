// Host test of fusion-sim_amd/csrc/fes_pair_core.hpp (the rule of the binary Coulomb collision operator and the checks of a
// request): the host-side numbers against values of the numpy reference (tests/pair_reference.py), the block-0 words of three
// ids against that reference's (tests/test_pair_reference.py, WORDS_OF_THREE_IDS), the order, who leads what in a cell, five
// pairs (a weak one, two strong ones, an axial one, a resting one) against the reference's results, the conservation of a
// pair's momentum, the cast after a pair, and every refusal by its message.  Built with g++ -ffp-contract=off by
// tests/test_pair_host.py (also with -fsanitize=address,undefined, as a program of its own); prints "ok" and exits 0, or
// names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../fusion-sim_amd/csrc/fes_pair_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static const double kMe = 9.1093837015e-31, kQe = -1.602176634e-19, kMp = 1.67262192369e-27;

static fpic_pair_spec good()
{
    fpic_pair_spec s;
    std::memset(&s, 0, sizeof s);
    s.species_a = 0; s.species_b = 1;
    s.seed = 0x0123456789abcdefull; s.stream = 5; s.epoch = 3;
    s.log_lambda = 10.0; s.tau = 1e-9;
    return s;
}
static bool says(const char* msg, const char* text) { return msg && std::strcmp(msg, text) == 0; }

static void numbers()
{
    // request(10, 1e-9, ME, QE, MP, -QE, W = 3e21, dV = 0.5) of the reference: every operation of rule_of is one rounding
    const fespair::Rule r = fespair::rule_of(good(), 77u, kMe, kQe, kMp, -kQe, 3.0e21, 0.5);
    CHECK(r.epoch == 77u && r.stream == 5u && r.seed_lo == 0x89abcdefu && r.seed_hi == 0x01234567u && r.like == 0);
    CHECK(r.kappa == 0x1.e24f1ec35132ep-21 && r.fa == 0x1.ffb8a7a1dc95ap-1 && r.fb == 0x1.1d61788da9877p-11);
    fpic_pair_spec s = good();
    s.species_b = 0;
    const fespair::Rule l = fespair::rule_of(s, 0u, kMe, kQe, kMe, kQe, 1.0, 1.0);
    CHECK(l.like == 1 && l.fa == 0.5 && l.fb == 0.5);
}

static void words_and_order()
{
    static const uint32_t want[3][4] = { { 0xdb3527ceu, 0xeab17efbu, 0x45a4aec9u, 0x3dc11ec5u },
                                         { 0xaf769be6u, 0x05f58b6au, 0xf8cee517u, 0xec47426du },
                                         { 0xa05ed635u, 0xcfa18e33u, 0x4e01cffcu, 0x096542b2u } };
    static const uint32_t ids[3] = { 0u, 1u, 0xFFFFFFFFu };
    const fespair::Rule r = fespair::rule_of(good(), 77u, kMe, kQe, kMp, -kQe, 1.0, 1.0);
    for (int k = 0; k < 3; ++k) {
        uint32_t w[4], direct[4];
        fespair::words(r, ids[k], 0u, w);
        CHECK(w[0] == want[k][0] && w[1] == want[k][1] && w[2] == want[k][2] && w[3] == want[k][3]);
        CHECK(fespair::key_of(r, ids[k]) == want[k][0]);
        fespair::words(r, ids[k], 1u, w);
        fesload::philox(ids[k], 77u, 5u, 0xC0121u, 0x89abcdefu, 0x01234567u, direct);
        CHECK(std::memcmp(w, direct, sizeof w) == 0);
    }
    CHECK(fespair::before(1u, 9u, 2u, 0u) && !fespair::before(2u, 0u, 1u, 9u));
    CHECK(fespair::before(5u, 3u, 5u, 4u) && !fespair::before(5u, 4u, 5u, 3u) && !fespair::before(5u, 4u, 5u, 4u));
    CHECK(fespair::before(0u, 0u, 0xFFFFFFFFu, 0u) && !fespair::before(0xFFFFFFFFu, 0u, 0u, 0xFFFFFFFFu));
}

static void pairing()
{
    CHECK(fespair::many_is_a(4u, 4u) && fespair::many_is_a(5u, 2u) && !fespair::many_is_a(3u, 4u) && fespair::many_is_a(1u, 0u) && !fespair::many_is_a(0u, 2u));
    // like species, N = 0 .. 7: what starts at every place (tests/test_pair_reference.py has the same tables by hand)
    static const int want[8][7] = { { 0 }, { 0 }, { 1, 0 }, { 3, 0, 0 }, { 1, 0, 1, 0 }, { 3, 0, 0, 1, 0 }, { 1, 0, 1, 0, 1, 0 }, { 3, 0, 0, 1, 0, 1, 0 } };
    for (uint32_t n = 0; n < 8; ++n)
        for (uint32_t q = 0; q < n; ++q) CHECK(fespair::like_lead(n, q) == want[n][q]);
    CHECK(fespair::like_nl(5u, fespair::kTripleLead) == 2.5 && fespair::like_nl(5u, fespair::kPairLead) == 5.0 && fespair::like_nl(3u, fespair::kTripleLead) == 1.5);
    CHECK(fespair::like_nl(1024u, fespair::kPairLead) == 1024.0 && fespair::like_lead(1025u, 1024u) == 0 && fespair::like_lead(1025u, 1023u) == 1);
    // every particle of a cell is in exactly one pair, or in two of the triple
    for (uint32_t n = 2; n < 70; ++n) {
        int seen[70] = {};
        for (uint32_t q = 0; q < n; ++q) {
            const int lead = fespair::like_lead(n, q);
            if (lead == fespair::kPairLead) { seen[q]++; seen[q + 1]++; CHECK(q + 1 < n); }
            if (lead == fespair::kTripleLead) { seen[0] += 2; seen[1] += 2; seen[2] += 2; }
        }
        for (uint32_t q = 0; q < n; ++q) CHECK(seen[q] == ((n & 1u) && q < 3 ? 2 : 1));
    }
}

struct Case {
    uint32_t owner;
    double n_l, vo[3], vp[3], wo[3], wp[3];
    int what;
};

static void pairs()
{
    // ref.collide(request(10, 1e-9, ME, QE, MP, -QE, 3e21, 0.5, seed 0x0123456789abcdef, stream 5, epoch 77), ...): var =
    // 0.286, 1.04, 11.9 (the relative velocity along z), inf (at rest), 60.6
    static const Case cases[5] = {
    { 0u, 1.0, { -0x1.06c6e239b9c95p-7, -0x1.b1f748df36e64p-7, -0x1.458854e3bd9dep-9 }, { -0x1.c6119a008d978p-10, -0x1.5f0c1a4cfc58bp-14, -0x1.30eec60e225cfp-10 },
      { -0x1.2f7831a8658d5p-7, -0x1.868b1aa00ba08p-7, -0x1.5ff6479c1bdaap-8 }, { -0x1.c5e436c9af25ep-10, -0x1.621305c72c203p-14, -0x1.308542f0772efp-10 }, 1 },
    { 1u, 2.5, { 0x1.138b0178f5fd2p-8, 0x1.74427d84d5b7fp-7, 0x1.1f96b7e3d4a2bp-10 }, { -0x1.49ed9e4522274p-11, -0x1.ffb610d1d8499p-12, -0x1.75fb4cd2dcaebp-11 },
      { -0x1.172cf4d9d30c8p-9, 0x1.a18b1f8c19780p-11, -0x1.b9a2e410e4b0ap-7 }, { -0x1.481e9769a8217p-11, -0x1.f9ada84afac81p-12, -0x1.71d1ed4e7d116p-11 }, 3 },
    { 4294967295u, 7.0, { -0x1.6a2ed5ade36ccp-8, -0x1.012825cdc18e3p-7, 0x1.eab2b1fbb5365p-8 }, { -0x1.6a2ed5ade36ccp-8, -0x1.012825cdc18e3p-7, -0x1.35081fcfda14bp-11 },
      { -0x1.ae8f79530a7b8p-9, -0x1.b72090acdf9bbp-7, 0x1.3c6934690ffc2p-8 }, { -0x1.6a4350ef36eddp-8, -0x1.010ec6e9be757p-7, -0x1.3445ba8c8a5e4p-11 }, 3 },
    { 7u, 3.0, { 0x1.0bd7c5438f5a3p-6, 0x1.6586036eb5be8p-9, -0x1.94231b62db3adp-7 }, { 0x1.0bd7c5438f5a3p-6, 0x1.6586036eb5be8p-9, -0x1.94231b62db3adp-7 },
      { 0x1.0bd7c5438f5a3p-6, 0x1.6586036eb5be8p-9, -0x1.94231b62db3adp-7 }, { 0x1.0bd7c5438f5a3p-6, 0x1.6586036eb5be8p-9, -0x1.94231b62db3adp-7 }, 0 },
    { 123456789u, 500.0, { -0x1.3a011c9759c68p-7, 0x1.0625aa268b933p-6, 0x1.09ec0cf0373b6p-9 }, { -0x1.0d3377f23a6b5p-12, -0x1.0118d747861a8p-10, -0x1.6b2200e4abcddp-13 },
      { -0x1.3f8f3f1142a5ep-7, 0x1.533766d655c7cp-7, 0x1.9ac023e4378cep-7 }, { -0x1.0d1aaf16aef6ep-12, -0x1.004a68dc83639p-10, -0x1.7721ed41801a8p-13 }, 3 },
    };
    const fespair::Rule r = fespair::rule_of(good(), 77u, kMe, kQe, kMp, -kQe, 3.0e21, 0.5);
    for (const Case& c : cases) {
        double vo[3] = { c.vo[0], c.vo[1], c.vo[2] }, vp[3] = { c.vp[0], c.vp[1], c.vp[2] };
        const int what = fespair::collide(r, c.owner, c.n_l, r.fa, r.fb, vo, vp);
        CHECK(what == c.what);
        double speed = 0;
        for (int a = 0; a < 3; ++a) speed = std::fmax(speed, std::fabs(c.vo[a] - c.vp[a]));
        for (int a = 0; a < 3; ++a) {
            // the host's sine, cosine and logarithm are libm's and the reference's are numpy's: a few ulps of each rounded
            // function, the bound of tests/test_pair_reference.py (3 x 4 + 11 half-ulp pairs of the terms, all below 3 |u|)
            CHECK(std::fabs(vo[a] - c.wo[a]) <= 64 * 0x1p-53 * 3 * speed && std::fabs(vp[a] - c.wp[a]) <= 64 * 0x1p-53 * 3 * speed);
            if (!what) CHECK(vo[a] == c.vo[a] && vp[a] == c.vp[a]);                     // at rest: the bits are kept
            // momentum: m_a f_a = m_ab = m_b f_b
            const double before = kMe * c.vo[a] + kMp * c.vp[a], after = kMe * vo[a] + kMp * vp[a];
            CHECK(std::fabs(after - before) <= 16 * 0x1p-53 * (kMe * std::fabs(c.vo[a]) + kMp * std::fabs(c.vp[a]) + kMe * speed));
        }
        if (what) CHECK(vo[0] != c.vo[0] && vp[2] != c.vp[2] && std::isfinite(vo[0] + vo[1] + vo[2] + vp[0] + vp[1] + vp[2]));
    }
    // the cast after a pair: a float handle's next pair starts from float values
    double v[3] = { 0.1, -0x1.123456789abcdp-5, 3.0 };
    fespair::settle<float>(v);
    CHECK(v[0] == static_cast<double>(0.1f) && v[1] == static_cast<double>(static_cast<float>(-0x1.123456789abcdp-5)) && v[2] == 3.0);
    double w[3] = { 0.1, 0.2, 0.3 };
    fespair::settle<double>(w);
    CHECK(w[0] == 0.1 && w[1] == 0.2 && w[2] == 0.3);
}

static void refusals()
{
    CHECK(says(fespair::check(nullptr, 2), ".spec <- Non-optional property is undefined!"));
    fpic_pair_spec s = good();
    CHECK(fespair::check(&s, 2) == nullptr);
    CHECK(says(fespair::check(&s, 1), ".species_b <- no such species"));
    s.species_b = 0; CHECK(fespair::check(&s, 1) == nullptr);
    s = good(); s.species_a = 2; CHECK(says(fespair::check(&s, 2), ".species_a <- no such species"));
    s = good(); s.species_a = -1; CHECK(says(fespair::check(&s, 2), ".species_a <- no such species"));
    s = good(); s.species_b = -1; CHECK(says(fespair::check(&s, 2), ".species_b <- no such species"));
    for (int k = 0; k < 4; ++k) {
        s = good(); s.reserved[k] = 1e-300; CHECK(says(fespair::check(&s, 2), ".reserved <- must be zero"));
        s = good(); s.reserved[k] = kNan; CHECK(says(fespair::check(&s, 2), ".reserved <- must be zero"));
    }
    s = good(); s.log_lambda = kNan; CHECK(says(fespair::check(&s, 2), ".log_lambda <- must not be NaN"));
    s = good(); s.tau = kNan; CHECK(says(fespair::check(&s, 2), ".tau <- must not be NaN"));
    for (double bad : { 0.0, -1.0, kInf, -kInf }) {
        s = good(); s.log_lambda = bad; CHECK(says(fespair::check(&s, 2), ".log_lambda <- must be positive and finite"));
        s = good(); s.tau = bad; CHECK(says(fespair::check(&s, 2), ".tau <- must be positive and finite"));
    }
}

int main()
{
    numbers();
    words_and_order();
    pairing();
    pairs();
    refusals();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
