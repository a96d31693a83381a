// Host test of fusion-sim_amd/csrc/fes_hist_core.hpp (the bin rule of the phase-space histograms and the checks of a
// request): the edge cases of the inside test and of the index, the product that rounds up to `bins`, |v|^2 added left to
// right, and every refusal.  Built with g++ -ffp-contract=off by tests/test_histogram_host.py; prints "ok" and exits 0, or
// names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../fusion-sim_amd/csrc/fes_hist_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static feshist::Axis axis(double lo, double hi, int64_t bins) { return feshist::Axis{ lo, hi, feshist::scale_of(bins, lo, hi), bins }; }

static void edges()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const feshist::Axis a = axis(-1.0, 3.0, 8);   // dyadic: bins of width 0.5
    CHECK(a.scale == 2.0);
    CHECK(feshist::inside(-1.0, a) && feshist::index_of(-1.0, a) == 0);                  // q == lo: inside, bin 0
    CHECK(!feshist::inside(3.0, a));                                                      // q == hi: outside
    const double below = std::nextafter(3.0, 0.0);
    CHECK(feshist::inside(below, a) && feshist::index_of(below, a) == 7);                // the largest double below hi
    CHECK(!feshist::inside(std::nextafter(-1.0, -2.0), a));
    CHECK(!feshist::inside(nan, a) && !feshist::inside(inf, a) && !feshist::inside(-inf, a));
    const feshist::Axis z = axis(0.0, 4.0, 8);    // lo = 0: q - lo and the product by 2 are exact, so each bin's own edges are sharp
    for (int k = 0; k < 8; ++k) {
        CHECK(feshist::index_of(0.5 * k, z) == k);
        CHECK(feshist::index_of(std::nextafter(0.5 * (k + 1), 0.0), z) == k);
    }
    // (with lo = -1 the subtraction rounds: the double below the edge 1.0 gives q - lo = 2.0 exactly and falls in the next bin)
    CHECK(feshist::index_of(std::nextafter(1.0, 0.0), a) == 4);
    const feshist::Axis one = axis(0.0, 1.0, 1);
    CHECK(feshist::inside(0.0, one) && feshist::index_of(0.999, one) == 0 && !feshist::inside(1.0, one));
}

// (q - lo) * scale of the largest q below hi rounds up to `bins` for this triple (found by search in numpy; the python
// test searches its own): the min is what keeps the index inside
static void rounds_up()
{
    const double lo = -0.7322673547034516, hi = -0.18700837184614172;
    const int64_t bins = 111;
    const feshist::Axis a = axis(lo, hi, bins);
    const double q = std::nextafter(hi, lo);
    CHECK(feshist::inside(q, a));
    const double d = q - lo, t = d * a.scale;
    CHECK(std::floor(t) == static_cast<double>(bins));       // without the min: one past the last bin
    CHECK(feshist::index_of(q, a) == bins - 1);
    // a search of this test's own, so that the property does not rest on one constant
    int found = 0;
    unsigned long long s = 12345;
    for (int i = 0; i < 2000; ++i) {
        auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<double>(s >> 11) * 0x1p-53; };
        const double l = next() * 2 - 1, h = l + next() + 1e-3;
        const int64_t b = 1 + static_cast<int64_t>(next() * 1000);
        const feshist::Axis x = axis(l, h, b);
        const double top = std::nextafter(h, l);
        if (std::floor((top - l) * x.scale) >= static_cast<double>(b)) {
            ++found;
            CHECK(feshist::index_of(top, x) == b - 1);
        }
        CHECK(feshist::index_of(l, x) == 0);
    }
    CHECK(found > 0);
}

static void v2()
{
    // left to right, each operation rounded once: (x*x + y*y) + z*z.  y*y = z*z = 1.5625 * 2^-54: each alone is less than
    // half an ulp of 1 and is lost against it, their sum is more than half an ulp and is not
    const double y = 1.25 * 0x1p-27;
    CHECK(feshist::v2_of(1.0, y, y) == 1.0);
    CHECK(feshist::v2_of(y, y, 1.0) == 1.0 + 0x1p-52);
    CHECK(feshist::v2_of(3.0, 4.0, 12.0) == 169.0);
}

static fpic_hist_spec good()
{
    fpic_hist_spec s;
    std::memset(&s, 0, sizeof s);
    s.species = 0; s.naxes = 2;
    s.axis[0] = FPIC_AXIS_X; s.axis[1] = FPIC_AXIS_VX;
    s.bins[0] = 2048; s.bins[1] = 2048;
    s.lo[0] = 0; s.hi[0] = 1; s.lo[1] = -0.1; s.hi[1] = 0.1;
    return s;
}
static bool names(const char* msg, const char* property) { return msg && std::strncmp(msg, property, std::strlen(property)) == 0; }

static void refusals()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    fpic_hist_spec s = good();
    CHECK(feshist::check(s, 1) == nullptr);                    // 2^22 bins exactly
    s.bins[1] = 2049; CHECK(names(feshist::check(s, 1), ".bins <- "));
    s = good(); s.bins[0] = 0; CHECK(names(feshist::check(s, 1), ".bins <- "));
    s = good(); s.bins[1] = -3; CHECK(names(feshist::check(s, 1), ".bins <- "));
    s = good(); s.bins[0] = s.bins[1] = 0x7fffffff; CHECK(names(feshist::check(s, 1), ".bins <- "));
    s = good(); s.naxes = 0; CHECK(names(feshist::check(s, 1), ".naxes <- "));
    s = good(); s.naxes = 3; CHECK(names(feshist::check(s, 1), ".naxes <- "));
    s = good(); s.axis[0] = 7; CHECK(names(feshist::check(s, 1), ".axis <- "));
    s = good(); s.axis[1] = -1; CHECK(names(feshist::check(s, 1), ".axis <- "));
    s = good(); s.axis[1] = FPIC_AXIS_X; CHECK(names(feshist::check(s, 1), ".axis <- "));
    s = good(); s.species = 1; CHECK(names(feshist::check(s, 1), ".species <- ")); CHECK(feshist::check(s, 2) == nullptr);
    s = good(); s.species = -1; CHECK(names(feshist::check(s, 1), ".species <- "));
    s = good(); s.lo[0] = nan; CHECK(names(feshist::check(s, 1), ".range <- "));
    s = good(); s.hi[1] = inf; CHECK(names(feshist::check(s, 1), ".range <- "));
    s = good(); s.lo[1] = -inf; CHECK(names(feshist::check(s, 1), ".range <- "));
    s = good(); s.lo[0] = 1; s.hi[0] = 1; CHECK(names(feshist::check(s, 1), ".range <- "));
    s = good(); s.lo[0] = 2; s.hi[0] = 1; CHECK(names(feshist::check(s, 1), ".range <- "));
    s = good(); s.lo[1] = -1.7e308; s.hi[1] = 1.7e308; CHECK(names(feshist::check(s, 1), ".range <- "));   // hi - lo overflows
    s = good(); s.lo[1] = 0; s.hi[1] = 5e-324; CHECK(names(feshist::check(s, 1), ".range <- "));            // bins / (hi - lo) overflows
    s = good(); s.reserved[2] = 1; CHECK(names(feshist::check(s, 1), ".reserved <- "));
    // the second axis of a one-axis request is not looked at
    s = good(); s.naxes = 1; s.axis[1] = 99; s.bins[1] = -1; s.lo[1] = nan; CHECK(feshist::check(s, 1) == nullptr);
    const feshist::Axis a = feshist::axis_of(good(), 1);
    CHECK(a.lo == -0.1 && a.hi == 0.1 && a.bins == 2048 && a.scale == 2048.0 / (0.1 - -0.1));
}

int main()
{
    edges();
    rounds_up();
    v2();
    refusals();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
