// Host test of fusion-sim_amd/csrc/fes_modes_core.hpp (the host rules of the modes diagnostic): every refusal of a request
// with its message, the reduction of a wave number (negative ones too) and the incremental index the kernel keeps, the two
// guaranteed properties of the twiddle tables (exact quadrant entries, bit-for-bit mirror conjugates) and their accuracy for
// n odd, n = 2 and n no multiple of 4, the places of the quantities, the launch shape, and the ranks' sum.  Built with g++
// -ffp-contract=off by tests/test_modes_host.py; prints "ok" and exits 0, or names the first failed check and exits 1.
// With an argument n it prints the table of n as hexadecimal doubles instead (the Python restatement is compared with it).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../fusion-sim_amd/csrc/fes_modes_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static bool refused(const fpic_modes_spec& s, int nx, int ny, int nz, const char* with)
{
    const char* why = fesmod::check(s, nx, ny, nz);
    return why && std::strncmp(why, with, std::strlen(with)) == 0;
}

static void checks()
{
    const int32_t m[9] = { 0, 0, 0, 4, -5, 3, -4, 5, -3 };
    fpic_modes_spec s{};
    s.mask = FPIC_MODE_EX;
    s.modes = m;
    CHECK(refused(s, 8, 10, 7, ".nmodes <- must lie in [1, FPIC_MODES_MAX (256)]"));
    s.nmodes = FPIC_MODES_MAX + 1;
    CHECK(refused(s, 8, 10, 7, ".nmodes <- must lie in"));
    s.nmodes = 3;
    CHECK(fesmod::check(s, 8, 10, 7) == nullptr);              // 4 = 8/2, -5 = -10/2, 3 = floor(7/2): the ends are inside
    s.modes = nullptr;
    CHECK(refused(s, 8, 10, 7, ".modes <- Non-optional property is undefined!"));
    s.modes = m;
    s.mask = 0;
    CHECK(refused(s, 8, 10, 7, ".mask <- no quantity is selected"));
    s.mask = 0x100u;
    CHECK(refused(s, 8, 10, 7, ".mask <- unknown bits"));
    s.mask = FPIC_MODE_ALL | 0x80000000u;
    CHECK(refused(s, 8, 10, 7, ".mask <- unknown bits"));
    s.mask = FPIC_MODE_ALL;
    CHECK(fesmod::check(s, 8, 10, 7) == nullptr);
    CHECK(refused(s, 7, 10, 7, ".modes <- a component lies outside [-n/2, n/2]"));    // 4 on an axis of 7
    CHECK(refused(s, 8, 9, 7, ".modes <- a component lies outside"));                 // -5 on an axis of 9
    CHECK(refused(s, 8, 10, 6, ".modes <- a component lies outside") == false);       // 3 = 6/2 is inside
    CHECK(refused(s, 8, 10, 5, ".modes <- a component lies outside"));
    const int32_t big[3] = { INT32_MIN, 0, 0 };
    fpic_modes_spec b = s;
    b.nmodes = 1; b.modes = big;
    CHECK(refused(b, 8, 10, 7, ".modes <- a component lies outside"));
    const int32_t dup[9] = { 1, 2, 3, 0, 0, 0, 1, 2, 3 };
    s.modes = dup;
    CHECK(refused(s, 8, 10, 7, ".modes <- the same wave vector twice"));
    const int32_t alias[6] = { 4, 0, 0, -4, 0, 0 };             // the same bin of an axis of 8, but two triples
    s.modes = alias; s.nmodes = 2;
    CHECK(fesmod::check(s, 8, 10, 7) == nullptr);
    s.reserved[3] = 1.0;
    CHECK(refused(s, 8, 10, 7, ".reserved <- must be zero"));
}

static void indices()
{
    CHECK(fesmod::reduce(0, 7) == 0 && fesmod::reduce(-1, 7) == 6 && fesmod::reduce(-7, 7) == 0 && fesmod::reduce(-3, 6) == 3 && fesmod::reduce(3, 6) == 3);
    CHECK(fesmod::reduce(-4, 8) == 4 && fesmod::reduce(INT32_MIN, 3) == 1 && fesmod::reduce(INT32_MAX, 2) == 1);
    // the kernel's walk: t += step, one conditional subtraction — against the product, for every m, slot count and n
    for (int n : { 2, 3, 5, 8, 33, 256, 300, 2050 })
        for (int m = -n / 2; m <= n / 2; m += (n > 64 ? 37 : 1))
            for (int slots : { 1, 4, 16, 256 }) {
                const int mr = fesmod::reduce(m, n), step = fesmod::index_of(mr, slots, n);
                for (int slot = 0; slot < slots; slot += (slots > 4 ? 5 : 1)) {
                    int t = fesmod::index_of(mr, slot, n);
                    for (int i = slot; i < n; i += slots) {
                        const long long want = ((static_cast<long long>(m) * i) % n + n) % n;
                        CHECK(t == want);
                        t += step;
                        if (t >= n) t -= n;
                    }
                }
            }
    CHECK(fesmod::index_of(2147483646, 2147483646, 2147483647) == 1);   // (n - 1)^2 mod n: no 32-bit overflow
}

static void tables()
{
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int n : { 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 17, 18, 33, 100, 255, 256, 300, 1001 }) {
        const std::vector<double> w = fesmod::table(n);
        CHECK(w.size() == 2 * static_cast<size_t>(n));
        CHECK(w[0] == 1.0 && w[1] == 0.0 && !std::signbit(w[1]));
        for (int t = 0; t < n; ++t) {
            const double re = w[2 * t], im = w[2 * t + 1];
            if ((4 * t) % n == 0) {      // the quadrant entries are exact
                const int quarter = 4 * t / n;
                CHECK(re == (quarter == 0 ? 1.0 : quarter == 2 ? -1.0 : 0.0) && im == (quarter == 1 ? -1.0 : quarter == 3 ? 1.0 : 0.0));
            }
            if (t > 0 && 2 * t != n) {   // the mirror is the conjugate, bit for bit
                const double mre = w[2 * (n - t)], mim = w[2 * (n - t) + 1], neg = -im;
                CHECK(std::memcmp(&mre, &re, 8) == 0 && std::memcmp(&mim, &neg, 8) == 0);
            }
            // every entry is the correctly rounded value, give or take the last bit
            const long double a = two_pi * t / n;
            CHECK(std::fabs(static_cast<double>(re - std::cos(a))) <= 0x1p-53 && std::fabs(static_cast<double>(im + std::sin(a))) <= 0x1p-53);
        }
    }
    const std::vector<double> two = fesmod::table(2);
    CHECK(two[0] == 1.0 && two[1] == 0.0 && two[2] == -1.0 && two[3] == 0.0);
    const std::vector<double> six = fesmod::table(6);      // no multiple of 4: only t = 0 and t = 3 are exact
    CHECK(six[6] == -1.0 && six[7] == 0.0 && six[2] == six[10] && six[3] == -six[11] && six[3] < 0);
}

static void places_and_shape()
{
    int place[fesmod::kQuantities];
    CHECK(fesmod::places(FPIC_MODE_ALL, place) == 8);
    for (int b = 0; b < 8; ++b) CHECK(place[b] == b);
    CHECK(fesmod::places(FPIC_MODE_EY | FPIC_MODE_BZ | FPIC_MODE_RHO, place) == 3);
    CHECK(place[0] == -1 && place[1] == 0 && place[6] == 1 && place[7] == 2 && place[3] == -1);
    for (uint32_t nm : { 1u, 2u, 3u, 16u, 17u, 32u, 200u, 256u })
        for (uint64_t rows : { 1ull, 4ull, 90ull, 1023ull, 1024ull, 1025ull, 65536ull, 100000ull }) {
            const fesmod::Shape s = fesmod::shape(nm, rows);
            CHECK((1u << s.log2p) >= nm && (s.log2p == 0 || (1u << (s.log2p - 1)) < nm));
            CHECK(s.slots * (1 << s.log2p) == fesmod::kThreads);
            CHECK(s.blocks >= 1 && s.blocks <= fesmod::kBlocks && s.blocks <= rows);
            CHECK(static_cast<uint64_t>(s.blocks) * s.rows_per_block >= rows && static_cast<uint64_t>(s.blocks - 1) * s.rows_per_block < rows);
        }
}

static void sums()
{
    // three parts of four numbers, added left to right from part 0 on
    const double parts[12] = { 1e16, -0.0, 1.0, 3.0, 1.0, -0.0, 1e16, -3.0, -1e16, 0.0, -1e16, 0.5 };
    double out[4];
    fesmod::add_parts(parts, 4, 3, 4, out);
    CHECK(out[0] == (1e16 + 1.0) - 1e16 && out[1] == 0.0 && out[2] == (1.0 + 1e16) - 1e16 && out[3] == 0.5);
    fesmod::add_parts(parts, 4, 1, 4, out);
    CHECK(out[0] == 1e16 && std::signbit(out[1]) && out[3] == 3.0);
}

int main(int argc, char** argv)
{
    if (argc > 1) {
        const std::vector<double> w = fesmod::table(std::atoi(argv[1]));
        for (double v : w) std::printf("%a\n", v);
        return 0;
    }
    checks();
    indices();
    tables();
    places_and_shape();
    sums();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
