// Host test of fusion-sim_amd/csrc/fes_select_core.hpp (the rule of the particle selection and the checks of a request):
// the inside test at its edges and with infinite bounds, the id rule, the arrays a request reads, and every refusal by its
// message.  Built with g++ -ffp-contract=off by tests/test_select_host.py; prints "ok" and exits 0, or names the first failed
// check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../fusion-sim_amd/csrc/fes_select_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static void edges()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(fessel::inside(-1.0, -1.0, 3.0));                                  // q == lo: inside
    CHECK(!fessel::inside(3.0, -1.0, 3.0));                                  // q == hi: outside
    CHECK(fessel::inside(std::nextafter(3.0, 0.0), -1.0, 3.0));
    CHECK(!fessel::inside(std::nextafter(-1.0, -2.0), -1.0, 3.0));
    CHECK(!fessel::inside(nan, -1.0, 3.0) && !fessel::inside(inf, -1.0, 3.0) && !fessel::inside(-inf, -1.0, 3.0));
    // infinite bounds: -inf is inside [-inf, hi), +inf is in no interval (q < hi fails even for hi = +inf), a NaN in none
    CHECK(fessel::inside(-inf, -inf, 0.0) && fessel::inside(-1e308, -inf, 0.0) && !fessel::inside(0.0, -inf, 0.0));
    CHECK(fessel::inside(1e308, 0.0, inf) && fessel::inside(0.0, 0.0, inf) && !fessel::inside(inf, 0.0, inf));
    CHECK(fessel::inside(0.0, -inf, inf) && !fessel::inside(inf, -inf, inf) && fessel::inside(-inf, -inf, inf) && !fessel::inside(nan, -inf, inf));
    // a float converts exactly: the float below 0.1f is below the double 0.1f converts to
    const float f = 0.1f;
    CHECK(fessel::inside(static_cast<double>(f), static_cast<double>(f), 1.0) && !fessel::inside(static_cast<double>(std::nextafter(f, 0.0f)), static_cast<double>(f), 1.0));
}

static void ids()
{
    CHECK(fessel::id_passes(5, 0, 0) && fessel::id_passes(5, 1, 0) && fessel::id_passes(0xffffffffu, 0, 7));
    CHECK(fessel::id_passes(10, 7, 3) && !fessel::id_passes(11, 7, 3) && fessel::id_passes(3, 7, 3) && !fessel::id_passes(0, 7, 3));
    CHECK(fessel::id_passes(0xffffffffu, 0xffffffffu, 0) && fessel::id_passes(0xfffffffeu, 0xffffffffu, 0xfffffffeu));
}

static fpic_select_spec good()
{
    fpic_select_spec s;
    std::memset(&s, 0, sizeof s);
    s.species = 0; s.nterms = 3;
    s.axis[0] = FPIC_AXIS_X; s.axis[1] = FPIC_AXIS_VX; s.axis[2] = FPIC_AXIS_V2;
    s.lo[0] = 0.25; s.hi[0] = 0.5;
    s.lo[1] = -std::numeric_limits<double>::infinity(); s.hi[1] = 0.1;
    s.lo[2] = 1e-4; s.hi[2] = std::numeric_limits<double>::infinity();
    s.id_mod = 7; s.id_rem = 3;
    return s;
}
static bool names(const char* msg, const char* property) { return msg && std::strncmp(msg, property, std::strlen(property)) == 0; }

static void arrays()
{
    fpic_select_spec s = good();
    CHECK(fessel::arrays_of(s) == (1u | 1u << 3 | 0x38u));
    s.nterms = 1; CHECK(fessel::arrays_of(s) == 1u);
    s.nterms = 0; CHECK(fessel::arrays_of(s) == 0u);
    std::memset(&s, 0, sizeof s);
    s.nterms = 1; s.axis[0] = FPIC_AXIS_V2; CHECK(fessel::arrays_of(s) == 0x38u);
    s.axis[0] = FPIC_AXIS_VZ; CHECK(fessel::arrays_of(s) == 1u << 5);
}

static void refusals()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const uint64_t most = FPIC_SELECT_MAX_ROWS;
    fpic_select_spec s = good();
    CHECK(fessel::check(s, 1, 16, true, FPIC_F32) == nullptr);
    CHECK(fessel::check(s, 1, most, true, FPIC_F64) == nullptr);
    CHECK(fessel::check(s, 1, 0, false, FPIC_F32) == nullptr);               // the count query
    CHECK(fessel::check(s, 1, 0, true, FPIC_F32) == nullptr);
    CHECK(names(fessel::check(s, 1, most + 1, true, FPIC_F32), ".capacity <- "));
    CHECK(names(fessel::check(s, 1, 1, false, FPIC_F32), ".capacity <- "));
    CHECK(names(fessel::check(s, 1, 1, true, 2), ".dtype <- "));
    CHECK(names(fessel::check(s, 1, 1, true, -1), ".dtype <- "));
    s = good(); s.nterms = -1; CHECK(names(fessel::check(s, 1, 1, true, 0), ".nterms <- "));
    s = good(); s.nterms = 8; CHECK(names(fessel::check(s, 1, 1, true, 0), ".nterms <- "));
    s = good(); s.species = 1; CHECK(names(fessel::check(s, 1, 1, true, 0), ".species <- ")); CHECK(fessel::check(s, 2, 1, true, 0) == nullptr);
    s = good(); s.species = -1; CHECK(names(fessel::check(s, 1, 1, true, 0), ".species <- "));
    s = good(); s.axis[0] = 7; CHECK(names(fessel::check(s, 1, 1, true, 0), ".axis <- "));
    s = good(); s.axis[1] = -1; CHECK(names(fessel::check(s, 1, 1, true, 0), ".axis <- "));
    s = good(); s.axis[2] = FPIC_AXIS_X; CHECK(names(fessel::check(s, 1, 1, true, 0), ".axis <- the same axis twice"));
    s = good(); s.lo[0] = nan; CHECK(names(fessel::check(s, 1, 1, true, 0), ".range <- "));
    s = good(); s.hi[2] = nan; CHECK(names(fessel::check(s, 1, 1, true, 0), ".range <- "));
    s = good(); s.lo[0] = 0.5; CHECK(names(fessel::check(s, 1, 1, true, 0), ".range <- "));            // lo == hi
    s = good(); s.lo[0] = 2; s.hi[0] = 1; CHECK(names(fessel::check(s, 1, 1, true, 0), ".range <- "));
    s = good(); s.lo[0] = inf; s.hi[0] = inf; CHECK(names(fessel::check(s, 1, 1, true, 0), ".range <- "));
    s = good(); s.lo[0] = -inf; s.hi[0] = -inf; CHECK(names(fessel::check(s, 1, 1, true, 0), ".range <- "));
    s = good(); s.lo[0] = -inf; s.hi[0] = inf; CHECK(fessel::check(s, 1, 1, true, 0) == nullptr);
    s = good(); s.lo[1] = -1.7e308; s.hi[1] = 1.7e308; CHECK(fessel::check(s, 1, 1, true, 0) == nullptr);   // (no width is formed)
    s = good(); s.id_rem = 7; CHECK(names(fessel::check(s, 1, 1, true, 0), ".id_rem <- "));
    s = good(); s.id_mod = 1; s.id_rem = 9; CHECK(fessel::check(s, 1, 1, true, 0) == nullptr);          // id_mod 0 or 1: id_rem is not looked at
    s = good(); s.id_mod = 0; s.id_rem = 9; CHECK(fessel::check(s, 1, 1, true, 0) == nullptr);
    s = good(); s.reserved[3] = 1; CHECK(names(fessel::check(s, 1, 1, true, 0), ".reserved <- "));
    s = good(); s.axis[3] = 1; CHECK(names(fessel::check(s, 1, 1, true, 0), ".axis <- entries past nterms"));
    s = good(); s.lo[7] = 1; CHECK(names(fessel::check(s, 1, 1, true, 0), ".axis <- entries past nterms"));
    s = good(); s.hi[4] = nan; CHECK(names(fessel::check(s, 1, 1, true, 0), ".axis <- entries past nterms"));
    // seven terms, every axis once; no terms at all
    std::memset(&s, 0, sizeof s);
    s.nterms = 7;
    for (int t = 0; t < 7; ++t) { s.axis[t] = 6 - t; s.lo[t] = -1; s.hi[t] = 1; }
    CHECK(fessel::check(s, 1, 1, true, 0) == nullptr);
    CHECK(fessel::arrays_of(s) == 0x3fu);
    std::memset(&s, 0, sizeof s);
    CHECK(fessel::check(s, 1, 0, false, 0) == nullptr);
}

int main()
{
    edges();
    ids();
    arrays();
    refusals();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
