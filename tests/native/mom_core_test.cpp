// Host test of the rule of the fluid moment grids (fusion-sim_amd/csrc/fes_mom_core.hpp), built with g++ -ffp-contract=off:
// the split against a 128-bit restatement over random (w1, t) with the extremes w1 in {0, 16384} and |t| near 2^46, the
// exact-sum identity of mom_terms, n_terms, the fixed-point conversion (one floor, also below zero), the rejection test,
// and every refusal of the request check.  Prints "ok".
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "../../fusion-sim_amd/csrc/fes_mom_core.hpp"

static int fails = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } \
    } while (0)

// floor((w1 t + 8192) / 2^14) in 128-bit arithmetic with an explicit floor (no shift of a negative number)
static int64_t upper128(int64_t t, int w1)
{
    const __int128 p = static_cast<__int128>(w1) * t + 8192;
    __int128 q = p / 16384;
    if (p % 16384 != 0 && p < 0) --q;
    return static_cast<int64_t>(q);
}

static void terms128(int64_t t, int wx1, int wy1, int wz1, int64_t (&out)[8])
{
    const int64_t z1 = upper128(t, wz1), tz[2] = { t - z1, z1 };
    for (int c = 0; c < 2; ++c) {
        const int64_t y1 = upper128(tz[c], wy1), ty[2] = { tz[c] - y1, y1 };
        for (int b = 0; b < 2; ++b) {
            const int64_t x1 = upper128(ty[b], wx1);
            out[2 * b + 4 * c] = ty[b] - x1;
            out[1 + 2 * b + 4 * c] = x1;
        }
    }
}

static void one(int64_t t, int wx1, int wy1, int wz1)
{
    int64_t got[8], want[8];
    fesmom::mom_terms(t, wx1, wy1, wz1, got);
    terms128(t, wx1, wy1, wz1, want);
    int64_t sum = 0;
    for (int e = 0; e < 8; ++e) { CHECK(got[e] == want[e]); sum += got[e]; }
    CHECK(sum == t);
}

int main()
{
    std::mt19937_64 rng(12345);
    const int64_t big = (int64_t(1) << 46) - 1;
    const int64_t ts[] = { 0, 1, -1, 2, -2, 8191, 8192, 8193, -8191, -8192, -8193, 16383, 16384, -16384, big, -big, big - 1, -(big - 1), -(int64_t(1) << 46), int64_t(1) << 32, -(int64_t(1) << 32) };
    const int ws[] = { 0, 1, 2, 8191, 8192, 8193, 16382, 16383, 16384 };
    for (int64_t t : ts)
        for (int wx : ws)
            for (int wy : ws)
                for (int wz : ws) one(t, wx, wy, wz);
    for (int n = 0; n < 400000; ++n) {
        int64_t t = static_cast<int64_t>(rng() >> 17) - (int64_t(1) << 46);          // [-2^46, 2^46)
        if (n % 3 == 0) t = (n & 1 ? 1 : -1) * (big - static_cast<int64_t>(rng() % 1000)); // near the extremes
        if (n % 7 == 0) t = static_cast<int64_t>(rng() % 65536) - 32768;              // around the rounding constant
        int w[3];
        for (int& x : w) {
            x = static_cast<int>(rng() % 16385);
            if (rng() % 8 == 0) x = rng() & 1 ? 0 : 16384;
        }
        one(t, w[0], w[1], w[2]);
        // one split: upper + lower = t, upper as the 128-bit restatement, the extremes exact
        int64_t lo, hi;
        fesmom::split(t, w[0], lo, hi);
        CHECK(hi == upper128(t, w[0]) && lo + hi == t);
        fesmom::split(t, 0, lo, hi);
        CHECK(hi == 0 && lo == t);
        fesmom::split(t, 16384, lo, hi);
        CHECK(hi == t && lo == 0);
    }
    // N: the product of the weights, 2^42 in all
    for (int wx : ws)
        for (int wy : ws)
            for (int wz : ws) {
                int64_t t[8], sum = 0;
                fesmom::n_terms(wx, wy, wz, t);
                for (int e = 0; e < 8; ++e) {
                    const int64_t a = e & 1 ? wx : 16384 - wx, b = e & 2 ? wy : 16384 - wy, c = e & 4 ? wz : 16384 - wz;
                    CHECK(t[e] == a * b * c);
                    sum += t[e];
                }
                CHECK(sum == int64_t(1) << 42);
            }
    // the fixed-point conversion: exact scaling, one floor, also for negative values
    CHECK(fesmom::fixed(0.0) == 0 && fesmom::fixed(1.0) == int64_t(1) << 32 && fesmom::fixed(-1.0) == -(int64_t(1) << 32));
    CHECK(fesmom::fixed(0x1p-33) == 0 && fesmom::fixed(-0x1p-33) == -1 && fesmom::fixed(-0x1p-60) == -1 && fesmom::fixed(0x1p-32) == 1);
    CHECK(fesmom::fixed(1.5 * 0x1p-32) == 1 && fesmom::fixed(-1.5 * 0x1p-32) == -2);
    const double top = std::nextafter(128.0, 0.0);
    CHECK(fesmom::fixed(top * top) < int64_t(1) << 46 && fesmom::fixed(-(top * top)) > -(int64_t(1) << 46) - 1);
    // values: one multiplication
    CHECK(fesmom::value(1, 2, 3, 5) == 2 && fesmom::value(2, 2, 3, 5) == 3 && fesmom::value(3, 2, 3, 5) == 5);
    CHECK(fesmom::value(4, 2, 3, 5) == 4 && fesmom::value(5, 2, 3, 5) == 9 && fesmom::value(6, 2, 3, 5) == 25);
    CHECK(fesmom::value(7, 2, 3, 5) == 6 && fesmom::value(8, 2, 3, 5) == 10 && fesmom::value(9, 2, 3, 5) == 15);
    // rejection
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(!fesmom::rejected(0, 0, 0) && !fesmom::rejected(top, -top, top) && !fesmom::rejected(-0.0, 1e-300, -127.9));
    CHECK(fesmom::rejected(128, 0, 0) && fesmom::rejected(0, -128, 0) && fesmom::rejected(0, 0, 128.5));
    CHECK(fesmom::rejected(nan, 0, 0) && fesmom::rejected(0, nan, 0) && fesmom::rejected(0, 0, nan));
    CHECK(fesmom::rejected(inf, 0, 0) && fesmom::rejected(0, -inf, 0) && fesmom::rejected(0, 0, inf));
    // the request check
    fpic_moments_spec s;
    std::memset(&s, 0, sizeof s);
    s.mask = FPIC_MOM_ORDER2;
    CHECK(fesmom::check(s, 1) == nullptr && fesmom::popcount(s.mask) == 10);
    s.mask = FPIC_MOM_N; CHECK(fesmom::check(s, 1) == nullptr && fesmom::popcount(s.mask) == 1);
    s.mask = FPIC_MOM_SYZ | FPIC_MOM_FX; CHECK(fesmom::check(s, 2) == nullptr && fesmom::popcount(s.mask) == 2);
    auto refused = [&](const fpic_moments_spec& r, int nsp, const char* prop) {
        const char* why = fesmom::check(r, nsp);
        return why && std::strncmp(why, prop, std::strlen(prop)) == 0 && std::strstr(why, " <- ");
    };
    fpic_moments_spec r = s;
    r.species = 2; CHECK(refused(r, 2, ".species"));
    r.species = -1; CHECK(refused(r, 2, ".species"));
    r = s; r.mask = 0; CHECK(refused(r, 1, ".mask"));
    r.mask = 1u << 10; CHECK(refused(r, 1, ".mask"));
    r.mask = FPIC_MOM_ORDER2 | (1u << 31); CHECK(refused(r, 1, ".mask"));
    for (int k = 0; k < 4; ++k) {
        r = s; r.reserved[k] = 1e-300; CHECK(refused(r, 1, ".reserved"));
        r.reserved[k] = nan; CHECK(refused(r, 1, ".reserved"));
    }
    CHECK(FPIC_MOM_ORDER0 == FPIC_MOM_N && FPIC_MOM_ORDER1 == (FPIC_MOM_N | FPIC_MOM_FX | FPIC_MOM_FY | FPIC_MOM_FZ) && FPIC_MOM_ORDER2 == 0x3FFu);
    CHECK(FPIC_MOM_SYZ == 1u << 9 && FPIC_MOM_SXX == 1u << 4 && FPIC_MOM_SXY == 1u << 7);
    if (!fails) std::printf("ok\n");
    return fails ? 1 : 0;
}
