// Host test of fusion-sim_amd/csrc/fes_collide_core.hpp (the rule of the collision operator and the checks of a request):
// the host-side numbers and their edge values, the block-0 words of three ids against constants taken from the numpy
// reference (tests/test_collide_reference.py), the exact parts of the three updates, and every refusal by its message.
// Built with g++ -ffp-contract=off by tests/test_collide_host.py (also with -fsanitize=address,undefined, as a program of
// its own); prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../fusion-sim_amd/csrc/fes_collide_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();

static fpic_collide_spec good(int kind)
{
    fpic_collide_spec s;
    std::memset(&s, 0, sizeof s);
    s.species = 0; s.kind = kind;
    s.seed = 0x0123456789abcdefull; s.stream = 5; s.epoch = 77;
    s.nu_tau = 1.0;
    for (int a = 0; a < 3; ++a) { s.drift[a] = 0.001 * a; s.vth[a] = 0.01; }
    if (kind == FPIC_COLLIDE_ELASTIC) s.mass_ratio = 3.0;
    return s;
}
static bool says(const char* msg, const char* text) { return msg && std::strcmp(msg, text) == 0; }

static void numbers()
{
    fpic_collide_spec s = good(FPIC_COLLIDE_ELASTIC);
    s.nu_tau = 0.25; s.sigma_tau = 2.0; s.g_max = 0.5;
    fescoll::Rule r = fescoll::rule_of(s, 9);
    CHECK(r.kind == FPIC_COLLIDE_ELASTIC && r.nullc == 1 && r.epoch == 9 && r.stream == 5 && r.seed_lo == 0x89abcdefu && r.seed_hi == 0x01234567u);
    CHECK(r.x_max == 1.25 && r.M == 0.75 && r.g_max == 0.5 && r.nu_tau == 0.25 && r.sigma_tau == 2.0);
    CHECK(r.K == static_cast<uint64_t>(std::ldexp(-std::expm1(-1.25), 32)) && r.K > 0 && r.K < (uint64_t(1) << 32));
    CHECK(r.drift[2] == 0.002 && r.vth[1] == 0.01);
    // the edges: K = 0, K = 2^32 (x_max = +inf, and a P_max that rounds to 1), M = 1
    s = good(FPIC_COLLIDE_EXCHANGE); s.nu_tau = 0;
    r = fescoll::rule_of(s, 0);
    CHECK(r.K == 0 && r.nullc == 0 && r.x_max == 0);
    s.nu_tau = kInf;
    CHECK(fescoll::rule_of(s, 0).K == uint64_t(1) << 32);
    s.nu_tau = 50.0;
    CHECK(fescoll::rule_of(s, 0).K == uint64_t(1) << 32);
    s.nu_tau = 1e-12;
    CHECK(fescoll::rule_of(s, 0).K == 0);                                  // P_max 2^32 < 1
    s = good(FPIC_COLLIDE_ELASTIC); s.mass_ratio = kInf;
    CHECK(fescoll::rule_of(s, 0).M == 1.0);
    s.mass_ratio = 1.0;
    CHECK(fescoll::rule_of(s, 0).M == 0.5);
    s = good(FPIC_COLLIDE_RELAX); s.nu_tau = 0.5; s.vth[1] = 2.0; s.vth[2] = 0;
    r = fescoll::rule_of(s, 0);
    CHECK(r.decay == std::exp(-0.5) && r.sv[0] == std::sqrt(-std::expm1(-1.0)) * 0.01 && r.sv[1] == std::sqrt(-std::expm1(-1.0)) * 2.0 && r.sv[2] == 0);
}

static void words_and_candidates()
{
    // (seed 0x0123456789abcdef, stream 5, epoch 77, block 0) of ids 0, 1, 2^32 - 1: the numpy reference's words
    static const uint32_t want[3][4] = { { 0x373469d3u, 0xfeeda24bu, 0x6bb82344u, 0x614548a1u },
                                         { 0xe8427845u, 0x0b69b034u, 0x0cc70f85u, 0x709c2f32u },
                                         { 0x12b30ae2u, 0xd221c64bu, 0xb8af0f74u, 0x80a771b8u } };
    static const uint32_t ids[3] = { 0u, 1u, 0xFFFFFFFFu };
    fescoll::Rule r = fescoll::rule_of(good(FPIC_COLLIDE_EXCHANGE), 77);
    for (int k = 0; k < 3; ++k) {
        uint32_t w[4];
        fescoll::words(r, ids[k], 0u, w);
        CHECK(w[0] == want[k][0] && w[1] == want[k][1] && w[2] == want[k][2] && w[3] == want[k][3]);
        uint32_t direct[4];
        fesload::philox(ids[k], 77u, 5u, 0xC0110u, 0x89abcdefu, 0x01234567u, direct);
        CHECK(std::memcmp(w, direct, sizeof w) == 0);
        fescoll::words(r, ids[k], 1u, w);
        fesload::philox(ids[k], 77u, 5u, 0xC0111u, 0x89abcdefu, 0x01234567u, direct);
        CHECK(std::memcmp(w, direct, sizeof w) == 0);
    }
    // candidacy is w0 < K
    r.K = 0x373469d3ull;     CHECK(!fescoll::candidate(r, 0u));
    r.K = 0x373469d4ull;     CHECK(fescoll::candidate(r, 0u));
    r.K = 0;                 CHECK(!fescoll::candidate(r, 1u));
    r.K = uint64_t(1) << 32; CHECK(fescoll::candidate(r, 0u) && fescoll::candidate(r, 1u) && fescoll::candidate(r, 0xFFFFFFFFu));
}

static void updates()
{
    // EXCHANGE: the partner's velocity, drift + vth n with the loader's normals of block 1
    fpic_collide_spec s = good(FPIC_COLLIDE_EXCHANGE); s.nu_tau = kInf;
    fescoll::Rule r = fescoll::rule_of(s, 77);
    uint32_t w[4];
    double n[3], v[3] = { 0.5, -0.25, 0.125 };
    fescoll::words(r, 7u, 1u, w);
    fesload::normals_from(w, n);
    bool cand = false;
    CHECK(fescoll::apply(r, 7u, v, &cand) == fescoll::kCollided && cand);
    for (int a = 0; a < 3; ++a) {
        const double t = 0.01 * n[a];
        CHECK(v[a] == 0.001 * a + t && std::fabs(n[a]) < 6.77);
    }
    // nobody is a candidate at K = 0: the velocity keeps its bits
    s.nu_tau = 0;
    r = fescoll::rule_of(s, 77);
    double u[3] = { 0.5, -0.25, 0.125 };
    CHECK(fescoll::apply(r, 7u, u, &cand) == 0 && !cand && u[0] == 0.5 && u[1] == -0.25 && u[2] == 0.125);
    // ELASTIC on a cold fixed target at rest: v' = g nhat up to the roundings, the speed is kept; an equal mass halves r
    s = good(FPIC_COLLIDE_ELASTIC); s.nu_tau = kInf; s.mass_ratio = kInf;
    for (int a = 0; a < 3; ++a) s.drift[a] = s.vth[a] = 0;
    r = fescoll::rule_of(s, 3);
    double e[3] = { 0.3, 0.0, -0.4 };
    CHECK(fescoll::apply(r, 11u, e, &cand) == fescoll::kCollided);
    CHECK(std::fabs(std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) - 0.5) < 1e-15 && !(e[0] == 0.3 && e[2] == -0.4));
    // the null-collision test: a cold beam slower than g_max collides iff u x_max < x; faster, it is clipped and accepted
    s = good(FPIC_COLLIDE_EXCHANGE); s.nu_tau = 0.1; s.sigma_tau = 20.0; s.g_max = 0.0625;
    for (int a = 0; a < 3; ++a) s.drift[a] = s.vth[a] = 0;
    r = fescoll::rule_of(s, 9);
    r.K = uint64_t(1) << 32;
    int hits = 0;
    for (uint32_t i = 0; i < 2000; ++i) {
        double b[3] = { 0.03125, 0, 0 };
        fescoll::words(r, i, 0u, w);
        const double ux = (static_cast<double>(w[1]) + 0.5) * std::ldexp(1.0, -32) * r.x_max;
        const int what = fescoll::apply(r, i, b, &cand);
        CHECK(what == (ux < 0.1 + 20.0 * 0.03125 ? fescoll::kCollided : 0));
        CHECK(what ? b[0] == 0 : b[0] == 0.03125);
        hits += what ? 1 : 0;
        double f[3] = { 0.125, 0, 0 };
        CHECK(fescoll::apply(r, i, f, &cand) == (fescoll::kCollided | fescoll::kClipped) && f[0] == 0);
    }
    CHECK(hits > 900 && hits < 1250);                                      // x / x_max = 0.725 / 1.35
    // RELAX: drift + (decay (v - drift) + sv n)
    s = good(FPIC_COLLIDE_RELAX); s.nu_tau = 0.5;
    r = fescoll::rule_of(s, 77);
    double q[3] = { 0.5, -0.25, 0.125 };
    CHECK(fescoll::apply(r, 7u, q, &cand) == fescoll::kCollided && !cand);
    const double v0[3] = { 0.5, -0.25, 0.125 };
    for (int a = 0; a < 3; ++a) {
        const double rr = v0[a] - r.drift[a], p = r.decay * rr, k = r.sv[a] * n[a], sum = p + k;
        CHECK(q[a] == r.drift[a] + sum);
    }
}

static void refusals()
{
    CHECK(says(fescoll::check(nullptr, 1), ".spec <- Non-optional property is undefined!"));
    for (int kind : { FPIC_COLLIDE_EXCHANGE, FPIC_COLLIDE_ELASTIC, FPIC_COLLIDE_RELAX }) {
        fpic_collide_spec s = good(kind);
        CHECK(fescoll::check(&s, 1) == nullptr);
        s.species = 1; CHECK(says(fescoll::check(&s, 1), ".species <- no such species")); CHECK(fescoll::check(&s, 2) == nullptr);
        s = good(kind); s.species = -1; CHECK(says(fescoll::check(&s, 1), ".species <- no such species"));
        for (int k = 0; k < 4; ++k) {
            s = good(kind); s.reserved[k] = 1e-300; CHECK(says(fescoll::check(&s, 1), ".reserved <- must be zero"));
            s = good(kind); s.reserved[k] = kNan; CHECK(says(fescoll::check(&s, 1), ".reserved <- must be zero"));
        }
        s = good(kind); s.nu_tau = kNan; CHECK(says(fescoll::check(&s, 1), ".nu_tau <- must not be NaN"));
        s = good(kind); s.sigma_tau = kNan; CHECK(says(fescoll::check(&s, 1), ".sigma_tau <- must not be NaN"));
        s = good(kind); s.g_max = kNan; CHECK(says(fescoll::check(&s, 1), ".g_max <- must not be NaN"));
        s = good(kind); s.mass_ratio = kNan; CHECK(says(fescoll::check(&s, 1), ".mass_ratio <- must not be NaN"));
        s = good(kind); s.nu_tau = -1e-300; CHECK(says(fescoll::check(&s, 1), ".nu_tau <- must not be negative"));
        s = good(kind); s.sigma_tau = -1.0; CHECK(says(fescoll::check(&s, 1), ".sigma_tau <- must be finite and not negative"));
        s = good(kind); s.sigma_tau = kInf; CHECK(says(fescoll::check(&s, 1), ".sigma_tau <- must be finite and not negative"));
        for (double bad : { kInf, -kInf, kNan }) {
            s = good(kind); s.drift[1] = bad; CHECK(says(fescoll::check(&s, 1), ".drift <- must be finite"));
            s = good(kind); s.vth[2] = bad; CHECK(says(fescoll::check(&s, 1), ".vth <- must be finite and not negative"));
        }
        s = good(kind); s.vth[0] = -1e-300; CHECK(says(fescoll::check(&s, 1), ".vth <- must be finite and not negative"));
        s = good(kind); s.vth[0] = 0; CHECK(fescoll::check(&s, 1) == nullptr);
        s = good(kind); s.g_max = 0.5; CHECK(says(fescoll::check(&s, 1), ".g_max <- must be 0 when sigma_tau == 0"));
        s = good(kind); s.g_max = -0.5; CHECK(says(fescoll::check(&s, 1), ".g_max <- must be 0 when sigma_tau == 0"));
    }
    fpic_collide_spec s = good(FPIC_COLLIDE_EXCHANGE);
    s.kind = 3; CHECK(says(fescoll::check(&s, 1), ".kind <- must be 0 (exchange), 1 (elastic) or 2 (relax)"));
    s.kind = -1; CHECK(says(fescoll::check(&s, 1), ".kind <- must be 0 (exchange), 1 (elastic) or 2 (relax)"));
    for (int kind : { FPIC_COLLIDE_EXCHANGE, FPIC_COLLIDE_ELASTIC }) {
        s = good(kind); s.sigma_tau = 2.0; s.g_max = 0.5; CHECK(fescoll::check(&s, 1) == nullptr);
        for (double bad : { 0.0, -1.0, kInf }) {
            s = good(kind); s.sigma_tau = 2.0; s.g_max = bad;
            CHECK(says(fescoll::check(&s, 1), ".g_max <- must be positive and finite when sigma_tau > 0"));
        }
        s = good(kind); s.sigma_tau = 2.0; s.g_max = 0.5; s.nu_tau = kInf;
        CHECK(says(fescoll::check(&s, 1), ".nu_tau <- +inf needs sigma_tau == 0 (the acceptance x / x_max would be inf / inf)"));
        s = good(kind); s.nu_tau = kInf; CHECK(fescoll::check(&s, 1) == nullptr);
        s = good(kind); s.nu_tau = 0; CHECK(fescoll::check(&s, 1) == nullptr);
    }
    s = good(FPIC_COLLIDE_ELASTIC); s.mass_ratio = kInf; CHECK(fescoll::check(&s, 1) == nullptr);
    for (double bad : { 0.0, -1.0, -kInf }) {
        s = good(FPIC_COLLIDE_ELASTIC); s.mass_ratio = bad;
        CHECK(says(fescoll::check(&s, 1), ".mass_ratio <- must be positive (+inf: a fixed target) for FPIC_COLLIDE_ELASTIC"));
    }
    for (int kind : { FPIC_COLLIDE_EXCHANGE, FPIC_COLLIDE_RELAX }) {
        s = good(kind); s.mass_ratio = 1.0; CHECK(says(fescoll::check(&s, 1), ".mass_ratio <- must be 0 for a kind other than FPIC_COLLIDE_ELASTIC"));
    }
    s = good(FPIC_COLLIDE_RELAX); s.sigma_tau = 1.0; s.g_max = 1.0; CHECK(says(fescoll::check(&s, 1), ".sigma_tau <- must be 0 for FPIC_COLLIDE_RELAX"));
    s = good(FPIC_COLLIDE_RELAX); s.nu_tau = 0; CHECK(says(fescoll::check(&s, 1), ".nu_tau <- must be positive and finite for FPIC_COLLIDE_RELAX"));
    s = good(FPIC_COLLIDE_RELAX); s.nu_tau = kInf; CHECK(says(fescoll::check(&s, 1), ".nu_tau <- must be positive and finite for FPIC_COLLIDE_RELAX"));
}

int main()
{
    numbers();
    words_and_candidates();
    updates();
    refusals();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
