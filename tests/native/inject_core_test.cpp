// Host test of fusion-sim_amd/csrc/fes_inject_core.hpp (the rule of the particle sources and the checks of a request): the
// sequence numbers of an application and their 2^32 bound, the capacity and id rule, every refusal by its message, the kind
// logic — a VOLUME particle is the loader's, a FLUX particle's exact parts spelled out —, the capacity check (the
// registration and index checks are fes_ops_core.hpp's: ops_core_test.cpp), and the conversion of a row of totals to the result, the NaN rule included.  Built with g++ -ffp-contract=off by
// tests/test_inject_host.py; prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../fusion-sim_amd/csrc/fes_inject_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static const double L[3] = { 2.0, 4.0, 8.0 };

static fpic_inject_spec volume()
{
    fpic_inject_spec s;
    std::memset(&s, 0, sizeof s);
    s.load.flags = FPIC_LOAD_POS | FPIC_LOAD_VEL;
    s.load.first = 100; s.load.count = 10; s.load.seed = 0x1234567890ull; s.load.stream = 3;
    for (int a = 0; a < 3; ++a) { s.load.lo[a] = 0.25 * L[a]; s.load.hi[a] = 0.75 * L[a]; s.load.vth[a] = 0.01 * (a + 1); }
    s.load.drift[0] = 0.02;
    s.kind = FPIC_INJECT_VOLUME;
    return s;
}
static fpic_inject_spec flux()
{
    fpic_inject_spec s = volume();
    s.load.drift[0] = 0; s.load.drift[2] = -0.03;
    s.kind = FPIC_INJECT_FLUX; s.axis = 0; s.side = -1; s.plane = 1.5;
    return s;
}
static bool names(const char* msg, const char* property) { return msg && std::strncmp(msg, property, std::strlen(property)) == 0; }

static void sequences()
{
    fpic_inject_spec s = volume();
    uint64_t f = 0;
    CHECK(fesinj::first_of(s, 0, &f) && f == 100);
    CHECK(fesinj::first_of(s, 7, &f) && f == 170);
    s.epoch = 5; CHECK(fesinj::first_of(s, 7, &f) && f == 220);
    s = volume(); s.load.first = 1; s.load.count = (1ull << 31) - 1;
    CHECK(fesinj::check(&s, 1, L) == nullptr);
    CHECK(fesinj::first_of(s, 1, &f) && f == (1ull << 31));       // first + count = 2^32 - 1: the loader's bound, met exactly
    CHECK(!fesinj::first_of(s, 2, &f));
    s.load.first = 2; CHECK(!fesinj::first_of(s, 1, &f));
    // application 0 and the request's own check draw the same line
    s = volume(); s.load.first = 0xFFFFFFFFull - 10; s.load.count = 10; CHECK(fesinj::check(&s, 1, L) == nullptr && fesinj::first_of(s, 0, &f));
    s.load.count = 11; CHECK(fesinj::check(&s, 1, L) != nullptr && !fesinj::first_of(s, 0, &f));
    s = volume(); s.epoch = ~0ull; CHECK(!fesinj::first_of(s, 3, &f));   // (no 64-bit wrap hides it)
    CHECK(fesinj::fits(5, 8, 5, 3) && !fesinj::fits(5, 8, 5, 4) && fesinj::fits(5, 8, 5, 0) && !fesinj::fits(9, 8, 9, 1));
    CHECK(fesinj::fits(0, 1ull << 40, (1ull << 32) - 4, 3) && !fesinj::fits(0, 1ull << 40, (1ull << 32) - 3, 3));
}

static void refusals()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    fpic_inject_spec s = volume();
    CHECK(fesinj::check(&s, 1, L) == nullptr);
    CHECK(names(fesinj::check(nullptr, 1, L), ".spec <- "));
    // the flag and count rules of a source
    s = volume(); s.load.flags = FPIC_LOAD_POS; CHECK(names(fesinj::check(&s, 1, L), ".flags <- a source needs"));
    s = volume(); s.load.flags = FPIC_LOAD_VEL; CHECK(names(fesinj::check(&s, 1, L), ".flags <- a source needs"));
    s = volume(); s.load.flags |= FPIC_LOAD_APPEND; CHECK(names(fesinj::check(&s, 1, L), ".flags <- FPIC_LOAD_APPEND"));
    s = volume(); s.load.count = ~0ull; CHECK(names(fesinj::check(&s, 1, L), ".count <- "));
    s = volume(); s.load.count = 0; CHECK(fesinj::check(&s, 1, L) == nullptr);
    // what the loader refuses of the embedded request
    s = volume(); s.load.species = 1; CHECK(names(fesinj::check(&s, 1, L), ".species <- ")); CHECK(fesinj::check(&s, 2, L) == nullptr);
    s = volume(); s.load.flags |= 0x100u; CHECK(names(fesinj::check(&s, 1, L), ".flags <- unknown"));
    s = volume(); s.load.reserved = 1; CHECK(names(fesinj::check(&s, 1, L), ".reserved <- "));
    s = volume(); s.load.first = 1ull << 32; CHECK(names(fesinj::check(&s, 1, L), ".first <- "));
    s = volume(); s.load.first = 0xFFFFFFF0ull; s.load.count = 0x20; CHECK(names(fesinj::check(&s, 1, L), ".first <- "));
    s = volume(); s.load.hi[1] = 4.5; CHECK(names(fesinj::check(&s, 1, L), ".lo <- "));
    s = volume(); s.load.vth[2] = -1; CHECK(names(fesinj::check(&s, 1, L), ".vth <- "));
    s = volume(); s.load.drift[1] = nan; CHECK(names(fesinj::check(&s, 1, L), ".drift <- "));
    s = volume(); s.load.mode[0] = 40000; CHECK(names(fesinj::check(&s, 1, L), ".mode <- "));
    s = volume(); s.load.xphase = nan; CHECK(names(fesinj::check(&s, 1, L), ".xphase <- "));
    // its own
    s = volume(); s.kind = 2; CHECK(names(fesinj::check(&s, 1, L), ".kind <- "));
    s = volume(); s.kind = -1; CHECK(names(fesinj::check(&s, 1, L), ".kind <- "));
    s = volume(); s.reserved_i = 1; CHECK(names(fesinj::check(&s, 1, L), ".reserved <- "));
    s = volume(); s.reserved[2] = 1; CHECK(names(fesinj::check(&s, 1, L), ".reserved <- "));
    s = volume(); s.reserved[0] = nan; CHECK(names(fesinj::check(&s, 1, L), ".reserved <- "));
    s = volume(); s.axis = 1; CHECK(names(fesinj::check(&s, 1, L), ".axis <- "));
    s = volume(); s.side = 1; CHECK(names(fesinj::check(&s, 1, L), ".axis <- "));
    s = volume(); s.plane = 0.5; CHECK(names(fesinj::check(&s, 1, L), ".axis <- "));
    s = volume(); s.load.flags |= FPIC_LOAD_PAIRED | FPIC_LOAD_LATTICE; s.load.xamp[0] = 1e-3; s.load.mode[1] = 2; CHECK(fesinj::check(&s, 1, L) == nullptr);
    // the flux kind
    s = flux(); CHECK(fesinj::check(&s, 1, L) == nullptr);
    s = flux(); s.load.flags |= FPIC_LOAD_LATTICE; CHECK(fesinj::check(&s, 1, L) == nullptr);
    s = flux(); s.axis = 3; CHECK(names(fesinj::check(&s, 1, L), ".axis <- "));
    s = flux(); s.axis = -1; CHECK(names(fesinj::check(&s, 1, L), ".axis <- "));
    s = flux(); s.side = 0; CHECK(names(fesinj::check(&s, 1, L), ".side <- "));
    s = flux(); s.side = 2; CHECK(names(fesinj::check(&s, 1, L), ".side <- "));
    s = flux(); s.plane = -0.1; CHECK(names(fesinj::check(&s, 1, L), ".plane <- "));
    s = flux(); s.plane = 2.0; CHECK(fesinj::check(&s, 1, L) == nullptr);       // (the far face is a plane of the box)
    s = flux(); s.plane = 2.1; CHECK(names(fesinj::check(&s, 1, L), ".plane <- "));
    s = flux(); s.plane = nan; CHECK(names(fesinj::check(&s, 1, L), ".plane <- "));
    s = flux(); s.axis = 2; s.plane = 7.9; CHECK(names(fesinj::check(&s, 1, L), ".drift <- "));   // (drift[2] is set)
    s = flux(); s.load.drift[0] = 1e-9; CHECK(names(fesinj::check(&s, 1, L), ".drift <- "));
    s = flux(); s.load.flags |= FPIC_LOAD_PAIRED; CHECK(names(fesinj::check(&s, 1, L), ".flags <- FPIC_LOAD_PAIRED"));
    s = flux(); s.load.xamp[1] = 1e-3; CHECK(names(fesinj::check(&s, 1, L), ".xamp <- "));
    s = flux(); s.load.vamp[2] = 1e-3; CHECK(names(fesinj::check(&s, 1, L), ".vamp <- "));
    s = flux(); s.load.mode[0] = 1; CHECK(names(fesinj::check(&s, 1, L), ".mode <- "));
    CHECK(fesinj::check_capacity(1) == nullptr && fesinj::check_capacity(0xFFFFFFFFull - 4097) == nullptr);
    CHECK(names(fesinj::check_capacity(0xFFFFFFFFull - 4096), ".capacity <- ") && names(fesinj::check_capacity(~0ull), ".capacity <- "));
}

static void kinds()
{
    // VOLUME: the loader's particle, call for call
    fpic_inject_spec s = volume();
    s.load.flags |= FPIC_LOAD_PAIRED; s.load.mode[0] = 2; s.load.xamp[1] = 1e-3; s.load.vamp[2] = 1e-3; s.load.vphase = 0.3;
    const fesinj::Rule q = fesinj::rule_of(s, 170, L, 1e-9);
    fpic_load_spec l = s.load; l.first = 170;
    const fesload::Rule r = fesload::rule_of(l, ~0ull, L);
    CHECK(q.kind == FPIC_INJECT_VOLUME && q.r.first == 170 && q.r.count == 10);
    for (uint32_t j = 170; j < 180; ++j) {
        double p[3], v[3], wp[3], wv[3], theta;
        fesinj::state_of(q, j, p, v);
        fesload::base_of(r, j, wp, theta);
        fesload::velocity_of(r, j, theta, wv);
        fesload::displace(r, theta, wp);
        for (int a = 0; a < 3; ++a) CHECK(p[a] == wp[a] && v[a] == wv[a]);
    }
    // FLUX, axis 0 towards -x from the plane x = 1.5: every operation spelled out
    s = flux();
    const double dt = 1e-9;
    const fesinj::Rule f = fesinj::rule_of(s, 100, L, dt);
    CHECK(f.kind == FPIC_INJECT_FLUX && f.axis == 0 && f.t1 == 1 && f.t2 == 2 && f.side == -1.0 && f.plane_f == 1.5 / 2.0);
    CHECK(f.step_f == (dt * 2.998e8) / 2.0 && f.r.lo_f[0] == 0.0 && f.r.w_f[0] == 1.0 && f.r.lo_f[1] == 0.25 && f.r.w_f[2] == 0.5);
    for (uint32_t j = 100; j < 140; ++j) {
        uint32_t w0[4], w1[4];
        fesload::philox(j, 3u, 0u, fesload::kTag, f.r.seed_lo, f.r.seed_hi, w0);
        fesload::philox(j, 3u, 1u, fesload::kTag, f.r.seed_lo, f.r.seed_hi, w1);
        double n[3];
        fesload::normals_from(w1, n);
        const double sp = std::sqrt(-2.0 * std::log((static_cast<double>(w1[2]) + 0.5) / 4294967296.0));
        const double vx = -(0.01 * sp);
        double p[3], v[3];
        fesinj::state_of(f, j, p, v);
        CHECK(v[0] == vx && vx < 0);
        const double t1 = 0.02 * n[0], t2 = 0.03 * n[1];
        CHECK(v[1] == 0.0 + t1 && v[2] == -0.03 + t2);
        const double ft = static_cast<double>(w0[0]) / 4294967296.0;
        const double d = vx * f.step_f, e = d * ft;
        CHECK(p[0] == 0.75 + e && p[0] <= 0.75 && p[0] >= 0.75 - 0.01 * 6.76 * f.step_f);
        const double y = (static_cast<double>(w0[1]) / 4294967296.0) * 0.5, z = (static_cast<double>(w0[2]) / 4294967296.0) * 0.5;
        CHECK(p[1] == 0.25 + y && p[2] == 0.25 + z);
    }
    // the other axes name their tangential pair in ascending order
    s = flux(); s.axis = 1; s.plane = 0; s.load.drift[2] = 0;
    const fesinj::Rule g = fesinj::rule_of(s, 0, L, dt);
    CHECK(g.t1 == 0 && g.t2 == 2 && g.plane_f == 0.0 && g.step_f == (dt * 2.998e8) / 4.0);
    s.axis = 2; s.side = 1;
    const fesinj::Rule k = fesinj::rule_of(s, 0, L, dt);
    CHECK(k.t1 == 0 && k.t2 == 1 && k.side == 1.0);
    double p[3], v[3];
    fesinj::state_of(k, 5, p, v);
    CHECK(v[2] > 0 && p[2] >= 0 && p[2] <= 0.03 * 6.76 * k.step_f);
}

static void results()
{
    const double mass = 9.109e-31, charge = -1.602e-19, W = 2.5e5, c = 2.998e8;
    uint64_t w[fesinj::kRowWords] = {};
    fpic_inject_result r;
    std::memset(&r, 0xff, sizeof r);
    r.applications = 7;
    fesinj::result_of(w, mass, charge, W, &r);
    CHECK(r.applications == 7);     // (not the row's to set)
    CHECK(r.injected == 0 && r.energy == 0 && r.momentum[0] == 0 && r.momentum[2] == 0 && r.charge == 0 && r.energy_fixed[1] == 0);
    w[0] = 3;
    w[1] = 0; w[2] = 3ull << 14;         // 3 * 2^78 = (3 << 14) * 2^64: |v|^2 sum 0.75
    const unsigned __int128 half = static_cast<unsigned __int128>(1) << 79, neg = ~half + 1;
    w[3] = static_cast<uint64_t>(neg); w[4] = static_cast<uint64_t>(neg >> 64);   // vx sum -0.5
    w[5] = 1; w[6] = 0;
    fesinj::result_of(w, mass, charge, W, &r);
    CHECK(r.injected == 3 && r.energy_fixed[0] == 0 && r.energy_fixed[1] == (3ull << 14) && r.momentum_fixed[0][1] == w[4] && r.momentum_fixed[1][0] == 1);
    CHECK(r.energy == 0.5 * mass * W * c * c * 0.75 && r.momentum[0] == mass * W * c * -0.5 && r.momentum[1] == mass * W * c * 0x1p-80 && r.momentum[2] == 0);
    CHECK(r.charge == 3.0 * charge * W);
    w[10] = 1u | 1u << 2;
    fesinj::result_of(w, mass, charge, W, &r);
    CHECK(std::isnan(r.energy) && std::isnan(r.momentum[1]) && r.momentum[0] == mass * W * c * -0.5 && r.injected == 3 && r.energy_fixed[1] == (3ull << 14));
}

int main()
{
    sequences();
    refusals();
    kinds();
    results();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
