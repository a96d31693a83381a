// Host test of fusion-sim_amd/csrc/fes_load_core.hpp (the rule of the particle loader and the checks of a request): the
// Random123 known-answer vectors of Philox4x32-10, the lattice words, the fraction mapping, the exact parts of a position,
// the pairing, and every refusal by its message.  Built with g++ -ffp-contract=off by tests/test_load_host.py (also with
// -fsanitize=address,undefined, as a program of its own); prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../fusion-sim_amd/csrc/fes_load_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static bool block_is(const uint32_t (&w)[4], uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return w[0] == a && w[1] == b && w[2] == c && w[3] == d; }

static void known_answers()
{
    uint32_t w[4];
    fesload::philox(0, 0, 0, 0, 0, 0, w);
    CHECK(block_is(w, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u));
    fesload::philox(~0u, ~0u, ~0u, ~0u, ~0u, ~0u, w);
    CHECK(block_is(w, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu));
    fesload::philox(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, w);
    CHECK(block_is(w, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u));
}

static void lattice_and_fractions()
{
    CHECK(fesload::lattice_word(0, fesload::kMult0, 17u) == 17u);
    CHECK(fesload::lattice_word(1, fesload::kMult0, 0u) == 3518319155u);
    CHECK(fesload::lattice_word(2, fesload::kMult0, 0u) == static_cast<uint32_t>(2ull * 3518319155ull));          // wraps
    CHECK(fesload::lattice_word(3, fesload::kMult1, 0xFFFFFFFFu) == static_cast<uint32_t>(3ull * 2882110345ull + 0xFFFFFFFFull));
    CHECK(fesload::lattice_word(0xFFFFFFFFu, fesload::kMult2, 5u) == static_cast<uint32_t>(0xFFFFFFFFull * 2360945575ull + 5ull));
    CHECK(fesload::fraction_of(0u) == 0.0);
    CHECK(fesload::fraction_of(0x80000000u) == 0.5);
    CHECK(fesload::fraction_of(1u) == std::ldexp(1.0, -32));
    CHECK(fesload::fraction_of(0xFFFFFFFFu) == 1.0 - std::ldexp(1.0, -32) && fesload::fraction_of(0xFFFFFFFFu) < 1.0);
}

static fpic_load_spec good()
{
    fpic_load_spec s;
    std::memset(&s, 0, sizeof s);
    s.species = 0; s.flags = FPIC_LOAD_POS | FPIC_LOAD_VEL;
    s.first = 3; s.count = 90; s.seed = 0x0123456789abcdefull; s.stream = 4;
    for (int a = 0; a < 3; ++a) { s.lo[a] = 0.25 * a; s.hi[a] = 1.0 + a; s.vth[a] = 0.01; s.drift[a] = 0.001 * a; }
    s.mode[0] = 2; s.mode[2] = -32768;
    s.xamp[0] = 1e-3; s.vamp[2] = 1e-4; s.xphase = 0.25; s.vphase = -0.5;
    return s;
}
static const double kBox[3] = { 1.0, 2.0, 3.0 };
static bool names(const char* msg, const char* property) { return msg && std::strncmp(msg, property, std::strlen(property)) == 0; }

static void rule()
{
    fpic_load_spec s = good();
    const fesload::Rule r = fesload::rule_of(s, 100, kBox);
    CHECK(r.first == 3 && r.count == 90 && r.seed_lo == 0x89abcdefu && r.seed_hi == 0x01234567u && r.stream == 4);
    CHECK(r.lo_f[1] == 0.25 / 2.0 && r.w_f[2] == (3.0 - 0.5) / 3.0 && r.xamp_f[0] == 1e-3 && r.m[2] == -32768.0 && r.displaced && r.waved);
    uint32_t w[4];
    fesload::philox(0, 4, 2, 0x10AD, r.seed_lo, r.seed_hi, w);
    CHECK(r.shift[0] == w[0] && r.shift[1] == w[1] && r.shift[2] == w[2]);
    CHECK(r.mult[0] == 3518319155u && r.mult[1] == 2882110345u && r.mult[2] == 2360945575u);
    s.count = ~0ull;
    CHECK(fesload::rule_of(s, 100, kBox).count == 97);
    // the exact parts: p = lo_f + f w_f with the words of block 0; the lattice words with LATTICE
    double p[3], theta;
    fesload::base_of(r, 7, p, theta);
    fesload::philox(7, 4, 0, 0x10AD, r.seed_lo, r.seed_hi, w);
    for (int a = 0; a < 3; ++a) {
        const double t = std::ldexp(static_cast<double>(w[a]), -32) * r.w_f[a];
        CHECK(p[a] == r.lo_f[a] + t);
    }
    const double t01 = 2.0 * p[0] + 0.0 * p[1];
    CHECK(theta == t01 + -32768.0 * p[2]);
    s.flags |= FPIC_LOAD_LATTICE;
    const fesload::Rule rl = fesload::rule_of(s, 100, kBox);
    fesload::base_of(rl, 7, p, theta);
    for (int a = 0; a < 3; ++a) {
        const double t = std::ldexp(static_cast<double>(static_cast<uint32_t>(7u * rl.mult[a] + rl.shift[a])), -32) * rl.w_f[a];
        CHECK(p[a] == rl.lo_f[a] + t);
    }
    // the pair: the same block, the thermal term negated
    s = good();
    s.flags |= FPIC_LOAD_PAIRED;
    for (int a = 0; a < 3; ++a) s.drift[a] = s.vamp[a] = 0;
    const fesload::Rule rp = fesload::rule_of(s, 100, kBox);
    double v0[3], v1[3], n[3];
    fesload::velocity_of(rp, 10, 0.0, v0);
    fesload::velocity_of(rp, 11, 0.0, v1);
    fesload::normals_of(rp, 11, n);
    for (int a = 0; a < 3; ++a) CHECK(v0[a] + v1[a] == 0.0 && v0[a] != 0.0 && std::fabs(n[a]) < 6.77 && v0[a] == 0.01 * n[a]);
    // the host's circular functions at their exact points
    CHECK(fesload::sinpi_(0.0) == 0.0 && fesload::sinpi_(0.5) == 1.0 && fesload::sinpi_(1.0) == 0.0 && fesload::sinpi_(1.5) == -1.0 && fesload::sinpi_(-0.5) == -1.0);
    CHECK(fesload::cospi_(0.0) == 1.0 && fesload::cospi_(0.5) == 0.0 && fesload::cospi_(1.0) == -1.0 && fesload::cospi_(1.5) == 0.0 && fesload::cospi_(-1.0) == -1.0);
}

static void refusals()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    fpic_load_spec s = good();
    CHECK(fesload::check(s, 1, 100, kBox, false) == nullptr);
    CHECK(fesload::check(s, 1, 93, kBox, false) == nullptr);                                  // [3, 93) of 93
    CHECK(names(fesload::check(s, 1, 92, kBox, false), ".count <- "));
    s = good(); s.count = ~0ull; CHECK(fesload::check(s, 1, 3, kBox, false) == nullptr);       // an empty tail
    s = good(); s.count = ~0ull; s.first = 4; CHECK(names(fesload::check(s, 1, 3, kBox, false), ".first <- "));
    s = good(); s.species = 1; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".species <- ")); CHECK(fesload::check(s, 2, 100, kBox, false) == nullptr);
    s = good(); s.species = -1; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".species <- "));
    s = good(); s.flags = 0; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".flags <- at least one"));
    s = good(); s.flags = FPIC_LOAD_LATTICE | FPIC_LOAD_PAIRED; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".flags <- at least one"));
    s = good(); s.flags |= 32u; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".flags <- unknown bits"));
    s = good(); s.flags |= 0x80000000u; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".flags <- unknown bits"));
    s = good(); s.flags = FPIC_LOAD_POS; CHECK(fesload::check(s, 1, 100, kBox, false) == nullptr);
    s = good(); s.flags = FPIC_LOAD_VEL | FPIC_LOAD_PAIRED | FPIC_LOAD_LATTICE; CHECK(fesload::check(s, 1, 100, kBox, false) == nullptr);
    s = good(); s.flags |= FPIC_LOAD_APPEND; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".flags <- FPIC_LOAD_APPEND"));
    s = good(); s.reserved = 1; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".reserved <- "));
    s = good(); s.reserved2 = -1; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".reserved <- "));
    for (double bad : { inf, -inf, nan }) {
        s = good(); s.lo[1] = bad; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".lo <- "));
        s = good(); s.hi[2] = bad; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".lo <- "));
        s = good(); s.drift[0] = bad; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".drift <- "));
        s = good(); s.vth[1] = bad; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".vth <- "));
        s = good(); s.xamp[2] = bad; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".xamp <- "));
        s = good(); s.vamp[0] = bad; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".vamp <- "));
        s = good(); s.xphase = bad; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".xphase <- "));
        s = good(); s.vphase = bad; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".vphase <- "));
    }
    s = good(); s.vth[2] = -1e-300; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".vth <- "));
    s = good(); s.vth[2] = 0; CHECK(fesload::check(s, 1, 100, kBox, false) == nullptr);
    s = good(); s.lo[0] = -1e-9; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".lo <- "));
    s = good(); s.lo[0] = 1.0; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".lo <- "));             // lo == hi
    s = good(); s.lo[1] = 1.5; s.hi[1] = 1.25; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".lo <- "));
    s = good(); s.hi[1] = std::nextafter(2.0, 3.0); CHECK(names(fesload::check(s, 1, 100, kBox, false), ".lo <- "));
    s = good(); s.hi[1] = 2.0; s.lo[1] = 0; CHECK(fesload::check(s, 1, 100, kBox, false) == nullptr);       // the whole box
    s = good(); s.mode[1] = 32769; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".mode <- "));
    s = good(); s.mode[1] = -32769; CHECK(names(fesload::check(s, 1, 100, kBox, false), ".mode <- "));
    s = good(); s.mode[1] = 32768; CHECK(fesload::check(s, 1, 100, kBox, false) == nullptr);
    // a rank of a decomposition: both arrays, a count, 32-bit ids; APPEND is allowed
    s = good(); CHECK(fesload::check(s, 1, ~0ull, kBox, true) == nullptr);
    s = good(); s.flags |= FPIC_LOAD_APPEND; CHECK(fesload::check(s, 1, ~0ull, kBox, true) == nullptr);
    s = good(); s.flags = FPIC_LOAD_POS; CHECK(names(fesload::check(s, 1, ~0ull, kBox, true), ".flags <- a rank"));
    s = good(); s.flags = FPIC_LOAD_VEL; CHECK(names(fesload::check(s, 1, ~0ull, kBox, true), ".flags <- a rank"));
    s = good(); s.count = ~0ull; CHECK(names(fesload::check(s, 1, ~0ull, kBox, true), ".count <- "));
    s = good(); s.first = 1ull << 32; CHECK(names(fesload::check(s, 1, ~0ull, kBox, true), ".first <- "));
    s = good(); s.first = 0xFFFFFFF0ull; s.count = 16; CHECK(names(fesload::check(s, 1, ~0ull, kBox, true), ".first <- "));
    s = good(); s.first = 0xFFFFFFF0ull; s.count = 15; CHECK(fesload::check(s, 1, ~0ull, kBox, true) == nullptr);
}

int main()
{
    known_answers();
    lattice_and_fractions();
    rule();
    refusals();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
