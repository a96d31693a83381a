// Host test of fusion-sim_amd/csrc/fes_force_core.hpp (the rule of the prescribed external forces and the checks of a
// request): the table lookups at f = 0, on a node and in the last interval, tfrac at a large s, the activity window, the
// envelope, the exact parts of the kick, the tallies' conversions, and every refusal by its message.  With two arguments it
// also reads cases from a file (tests/test_force_host.py writes them: a request, a sub-step count, particles) and writes what
// the rule gives, which the numpy reference must give bit for bit.
// Built with g++ -ffp-contract=off by tests/test_force_host.py (also with -fsanitize=address,undefined, as a program of its
// own); prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../fusion-sim_amd/csrc/fes_force_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static const double kL[3] = { 0.0078125, 0.0078125, 0.015625 };

static fpic_force_spec good()
{
    fpic_force_spec s;
    std::memset(&s, 0, sizeof s);
    s.kind = FPIC_FORCE_FIELD;
    s.nwaves = 1;
    s.stop = FPIC_FORCE_FOREVER;
    for (int a = 0; a < 3; ++a) { s.lo[a] = 0; s.hi[a] = kL[a]; }
    s.wave[0].amp[0] = 1e5;
    return s;
}
static bool says(const char* msg, const char* text) { return msg && std::strcmp(msg, text) == 0; }
static const double* const kNoTaper[3] = { nullptr, nullptr, nullptr };

static void numbers()
{
    // tfrac: nu s - floor(nu s), also where s is large and for a negative nu
    CHECK(fesforce::tfrac_of(0.25, 3) == 0.75 && fesforce::tfrac_of(0.0, 123456789) == 0.0 && fesforce::tfrac_of(0.5, (uint64_t(1) << 40) + 1) == 0.5);
    CHECK(fesforce::tfrac_of(-0.25, 1) == 0.75 && fesforce::tfrac_of(0.125, (uint64_t(1) << 52) + 3) == 0.375);
    CHECK(fesforce::tfrac_of(0.1, 1000003) >= 0 && fesforce::tfrac_of(0.1, 1000003) < 1);
    CHECK(fesforce::tfrac_of(1.0, ~uint64_t(0)) == 0.0);                    // (double) s = 2^64: a whole number of turns
    // the activity window
    fpic_force_spec s = good();
    CHECK(fesforce::active(s, 0) && fesforce::active(s, ~uint64_t(0)));
    s.start = 5; s.stop = 9;
    CHECK(!fesforce::active(s, 4) && fesforce::active(s, 5) && fesforce::active(s, 9) && !fesforce::active(s, 10));
    s.start = s.stop = 7;
    CHECK(!fesforce::active(s, 6) && fesforce::active(s, 7) && !fesforce::active(s, 8));
    // the envelope: on the nodes, between them, at stop (the last interval with r = 1)
    const double env[5] = { 0.0, 1.0, 0.5, 2.0, -1.0 };
    s = good(); s.start = 3; s.stop = 11; s.envelope_n = 5; s.envelope = env;
    CHECK(fesforce::envelope_of(s, env, 3) == 0.0 && fesforce::envelope_of(s, env, 5) == 1.0 && fesforce::envelope_of(s, env, 7) == 0.5 && fesforce::envelope_of(s, env, 9) == 2.0);
    CHECK(fesforce::envelope_of(s, env, 11) == -1.0 && fesforce::envelope_of(s, env, 4) == 0.5 && fesforce::envelope_of(s, env, 6) == 0.75 && fesforce::envelope_of(s, env, 10) == 0.5);
    s.envelope_n = 0;
    CHECK(fesforce::envelope_of(s, nullptr, 4) == 1.0);
    // kq
    const double q = -1.602e-19, m = 9.109e-31, dt = 5e-12;
    const double num = q * dt, den = m * fesforce::kC;
    CHECK(fesforce::kq_of(FPIC_FORCE_FIELD, q, m, dt) == num / den && fesforce::kq_of(FPIC_FORCE_ACCEL, q, m, dt) == dt / fesforce::kC);
    // the rule's fractions and flags
    s = good();
    fesforce::Rule r = fesforce::rule_of(s, kL, q, m, dt, 0, nullptr, kNoTaper);
    CHECK(r.whole == 1 && r.tapered == 0 && r.nwaves == 1 && r.scale == num / den && r.lo_f[2] == 0 && r.hi_f[2] == 1 && r.w[0] == 1);
    s.lo[0] = kL[0] / 4; s.hi[0] = 3 * kL[0] / 4;
    r = fesforce::rule_of(s, kL, q, m, dt, 0, nullptr, kNoTaper);
    CHECK(r.whole == 0 && r.lo_f[0] == 0.25 && r.hi_f[0] == 0.75 && r.w[0] == 0.5);
}

static void lookups()
{
    // the loader's rule: at f = 0, on a node, in the last interval and at its end
    const double tab[5] = { 1.0, 3.0, 2.0, 6.0, 4.0 };
    CHECK(fesload::lookup(tab, 4, 0.0) == 1.0 && fesload::lookup(tab, 4, 0.25) == 3.0 && fesload::lookup(tab, 4, 0.5) == 2.0 && fesload::lookup(tab, 4, 0.75) == 6.0);
    CHECK(fesload::lookup(tab, 4, 0.875) == 5.0 && fesload::lookup(tab, 4, 1.0) == 4.0 && fesload::lookup(tab, 4, 0.125) == 2.0);
    const double two[2] = { -2.0, 2.0 };
    CHECK(fesload::lookup(two, 1, 0.0) == -2.0 && fesload::lookup(two, 1, 0.5) == 0.0 && fesload::lookup(two, 1, 1.0) == 2.0);
    std::vector<double> big(FPIC_FORCE_TABLE_MAX);
    for (int k = 0; k < FPIC_FORCE_TABLE_MAX; ++k) big[k] = k * 0.5;
    uint32_t j; double sfrac;
    CHECK(fesload::lookup(big.data(), 1024, 1023.5 / 1024, j, sfrac) == 511.75 && j == 1023 && sfrac == 0.5);
    CHECK(fesload::lookup(big.data(), 1024, 0.0, j, sfrac) == 0.0 && j == 0 && sfrac == 0.0);
    // the taper of a rule: (tx ty) tz over the window's fractions, a missing table no multiply
    fpic_force_spec s = good();
    s.lo[0] = kL[0] / 4; s.hi[0] = 3 * kL[0] / 4;
    s.taper_n[0] = 5; s.taper[0] = tab; s.taper_n[2] = 2; s.taper[2] = two;
    const double* const tabs[3] = { tab, nullptr, two };
    fesforce::Rule r = fesforce::rule_of(s, kL, 1.0, 1.0, 1.0, 0, nullptr, tabs);
    CHECK(r.tapered == 1 && r.tk[0] == 4 && r.tk[1] == 0 && r.tk[2] == 1 && r.tab[0] == tab && r.tab[1] == nullptr);
    const double p[3] = { 0.25 + 0.5 * 0.875, 0.3, 0.75 };
    CHECK(fesforce::taper_of(r, tabs, p) == 5.0 * 1.0);
    const double p0[3] = { 0.25, 0.9, 0.0 };
    CHECK(fesforce::taper_of(r, tabs, p0) == 1.0 * -2.0);
}

static void kicks()
{
    // zero mode, nu and phase: cospi(0) = 1 exactly and v' = v + scale amp
    fpic_force_spec s = good();
    s.wave[0].amp[0] = 3.0; s.wave[0].amp[1] = -5.0; s.wave[0].amp[2] = 0.0;
    fesforce::Rule r = fesforce::rule_of(s, kL, 2.0, 4.0, 0.5, 17, nullptr, kNoTaper);
    const double scale = (2.0 * 0.5) / (4.0 * fesforce::kC);
    double v[3] = { 0.5, -0.25, 0.125 };
    const double p[3] = { 0.1, 0.999, 0.0 };
    CHECK(fesforce::apply(r, p, v));
    CHECK(v[0] == 0.5 + scale * 3.0 && v[1] == -0.25 + scale * -5.0 && v[2] == 0.125);
    // the window: lo counted, hi not, and a particle outside keeps its bits
    s.lo[1] = kL[1] / 4; s.hi[1] = 3 * kL[1] / 4;
    r = fesforce::rule_of(s, kL, 2.0, 4.0, 0.5, 17, nullptr, kNoTaper);
    const double on_lo[3] = { 0.5, 0.25, 0.5 }, on_hi[3] = { 0.5, 0.75, 0.5 }, nan_p[3] = { 0.5, kNan, 0.5 };
    double a[3] = { 1, 2, 3 }, b[3] = { 1, 2, 3 }, c[3] = { 1, 2, 3 };
    CHECK(fesforce::apply(r, on_lo, a) && a[0] == 1 + scale * 3.0);
    CHECK(!fesforce::apply(r, on_hi, b) && b[0] == 1 && b[1] == 2 && b[2] == 3);
    CHECK(!fesforce::apply(r, nan_p, c) && c[0] == 1);
    // a quarter and a half wave (host cospi_ is exact there): mode (1, 0, 2), nu 1/4 at s = 1, phase 1/8
    s = good();
    s.wave[0].mode[0] = 1; s.wave[0].mode[2] = 2; s.wave[0].nu = 0.25; s.wave[0].phase = 0.125; s.wave[0].amp[0] = 1.0;
    r = fesforce::rule_of(s, kL, fesforce::kC, 1.0, 1.0, 1, nullptr, kNoTaper);
    CHECK(r.scale == 1.0 && r.wave[0].tfrac == 0.25);
    const double quarter[3] = { 0.125, 0.7, 0.125 };      // theta = 0.375, arg = (0.375 - 0.25) + 0.125 = 0.25
    const double half[3] = { 0.375, 0.1, 0.125 };         // theta = 0.625, arg = 0.5
    const double whole[3] = { 0.125, 0.1, 0.0 };          // theta = 0.125, arg = 0
    double q0[3] = { 0.5, 0, 0 }, q1[3] = { 0.5, 0, 0 }, q2[3] = { 0.5, 0, 0 };
    CHECK(fesforce::apply(r, quarter, q0) && q0[0] == 0.5);
    CHECK(fesforce::apply(r, half, q1) && q1[0] == -0.5);
    CHECK(fesforce::apply(r, whole, q2) && q2[0] == 1.5);
    // four waves are added in sequence
    s = good(); s.nwaves = 4;
    for (int k = 0; k < 4; ++k) s.wave[k].amp[1] = 1.0 + k;
    r = fesforce::rule_of(s, kL, fesforce::kC, 1.0, 1.0, 0, nullptr, kNoTaper);
    double w[3] = { 0, 0, 0 };
    CHECK(fesforce::apply(r, whole, w) && w[1] == 10.0 && w[0] == 1e5);
}

static void tallies()
{
    CHECK(fesforce::fixed_to_double(0, 0) == 0.0 && fesforce::fixed_to_double(uint64_t(1) << 40, 0) == 0x1p-40);
    CHECK(fesforce::fixed_to_double(0, 1) == 0x1p-16 && fesforce::fixed_to_double(~uint64_t(0), ~uint64_t(0)) == -0x1p-80);
    CHECK(fesforce::fixed_to_double(0, ~uint64_t(0)) == -0x1p-16);
    // one rounding: 2^64 + 2^11 + 1 lies above the tie between 2^64 and 2^64 + 2^12
    CHECK(fesforce::fixed_to_double((uint64_t(1) << 11) + 1, 1) == (0x1p64 + 0x1p12) * 0x1p-80);
    CHECK(fesforce::fixed_to_double(uint64_t(1) << 11, 1) == 0x1p64 * 0x1p-80);                  // the tie goes to even
    uint64_t a[fesforce::kWords] = { 7, ~uint64_t(0), 0, 5, ~uint64_t(0), 1, 2, 3, 4, 0x5 }, s1[fesforce::kSumWords], s2[fesforce::kSumWords], back[fesforce::kWords];
    uint64_t b[fesforce::kWords] = { 1, 1, 0, ~uint64_t(0), 0, 9, 9, 9, 9, 0x4 };
    fesforce::split_words(a, s1);
    fesforce::split_words(b, s2);
    for (int k = 0; k < fesforce::kSumWords; ++k) s1[k] += s2[k];
    fesforce::join_words(s1, back);
    CHECK(back[0] == 8 && back[1] == 0 && back[2] == 1);                   // the carry of the low word reaches the high word
    CHECK(back[3] == 4 && back[4] == 0 && back[5] == 10 && back[6] == 11 && back[7] == 12 && back[8] == 13 && back[9] == 0x5);
    fpic_force_result out;
    std::memset(&out, 0, sizeof out);
    const uint64_t w[fesforce::kWords] = { 3, 0, 1, ~uint64_t(0), ~uint64_t(0), 0, 0, uint64_t(1) << 40, 0, 0x4 };
    fesforce::result_of(w, 2.0, 3.0, &out);
    const double ke = 0.5 * 2.0 * 3.0 * fesforce::kC * fesforce::kC, pm = 2.0 * 3.0 * fesforce::kC;
    CHECK(out.kicked == 3 && out.work == ke * 0x1p-16 && out.impulse[0] == pm * -0x1p-80 && std::isnan(out.impulse[1]) && out.impulse[2] == pm * 0x1p-40);
    CHECK(out.work_fixed[1] == 1 && out.impulse_fixed[0][0] == ~uint64_t(0) && out.impulse_fixed[2][0] == uint64_t(1) << 40);
}

static void refusals()
{
    CHECK(says(fesforce::check(nullptr, 1, kL), ".spec <- Non-optional property is undefined!"));
    fpic_force_spec s = good();
    CHECK(fesforce::check(&s, 1, kL) == nullptr);
    s.kind = 2; CHECK(says(fesforce::check(&s, 1, kL), ".kind <- must be 0 (field) or 1 (accel)"));
    s = good(); s.kind = -1; CHECK(says(fesforce::check(&s, 1, kL), ".kind <- must be 0 (field) or 1 (accel)"));
    s = good(); s.kind = FPIC_FORCE_ACCEL; CHECK(fesforce::check(&s, 1, kL) == nullptr);
    s = good(); s.species = 1; CHECK(says(fesforce::check(&s, 1, kL), ".species <- no such species")); CHECK(fesforce::check(&s, 2, kL) == nullptr);
    s = good(); s.species = -1; CHECK(says(fesforce::check(&s, 1, kL), ".species <- no such species"));
    for (int n : { 0, -1, 5 }) { s = good(); s.nwaves = n; CHECK(says(fesforce::check(&s, 1, kL), ".nwaves <- must be 1 .. FPIC_FORCE_MAX_WAVES (4)")); }
    s = good(); s.nwaves = 4; CHECK(fesforce::check(&s, 1, kL) == nullptr);
    s = good(); s.reserved_i32 = 1; CHECK(says(fesforce::check(&s, 1, kL), ".reserved <- must be zero"));
    s = good(); s.reserved[3] = 1e-300; CHECK(says(fesforce::check(&s, 1, kL), ".reserved <- must be zero"));
    s = good(); s.reserved[0] = kNan; CHECK(says(fesforce::check(&s, 1, kL), ".reserved <- must be zero"));
    s = good(); s.wave[3].reserved = 7; CHECK(says(fesforce::check(&s, 1, kL), ".reserved <- must be zero"));
    for (double bad : { kInf, -kInf, kNan }) {
        s = good(); s.wave[0].amp[2] = bad; CHECK(says(fesforce::check(&s, 1, kL), ".amp <- must be finite"));
        s = good(); s.wave[0].nu = bad; CHECK(says(fesforce::check(&s, 1, kL), ".nu <- must be finite"));
        s = good(); s.wave[0].phase = bad; CHECK(says(fesforce::check(&s, 1, kL), ".phase <- must be finite"));
        s = good(); s.lo[1] = bad; CHECK(says(fesforce::check(&s, 1, kL), ".lo, .hi <- must be finite"));
        s = good(); s.hi[2] = bad; CHECK(says(fesforce::check(&s, 1, kL), ".lo, .hi <- must be finite"));
        s = good(); s.wave[1].amp[0] = bad; CHECK(fesforce::check(&s, 1, kL) == nullptr);          // (a wave beyond nwaves is not read)
    }
    const char* window = ".lo, .hi <- the window must lie within 0 <= lo < hi <= L";
    s = good(); s.lo[0] = -1e-300; CHECK(says(fesforce::check(&s, 1, kL), window));
    s = good(); s.hi[2] = kL[2] * 1.0000001; CHECK(says(fesforce::check(&s, 1, kL), window));
    s = good(); s.lo[1] = s.hi[1] = kL[1] / 2; CHECK(says(fesforce::check(&s, 1, kL), window));
    s = good(); s.lo[1] = kL[1]; s.hi[1] = kL[1] / 2; CHECK(says(fesforce::check(&s, 1, kL), window));
    s = good(); s.hi[0] = 0; CHECK(says(fesforce::check(&s, 1, kL), window));
    for (int bad : { 32769, -32769 }) { s = good(); s.wave[0].mode[1] = bad; CHECK(says(fesforce::check(&s, 1, kL), ".mode <- components must lie within +-2^15")); }
    s = good(); s.wave[0].mode[1] = -32768; s.wave[0].mode[2] = 32768; CHECK(fesforce::check(&s, 1, kL) == nullptr);
    std::vector<double> tab(FPIC_FORCE_TABLE_MAX + 1, 1.0);
    for (uint32_t n : { 1u, static_cast<uint32_t>(FPIC_FORCE_TABLE_MAX + 1), ~0u }) {
        s = good(); s.taper_n[1] = n; s.taper[1] = tab.data(); CHECK(says(fesforce::check(&s, 1, kL), ".taper_n <- a table has 2 .. FPIC_FORCE_TABLE_MAX nodes (0: none)"));
        s = good(); s.envelope_n = n; s.envelope = tab.data(); s.stop = 9; CHECK(says(fesforce::check(&s, 1, kL), ".envelope_n <- a table has 2 .. FPIC_FORCE_TABLE_MAX nodes (0: none)"));
    }
    s = good(); s.taper_n[2] = 2; CHECK(says(fesforce::check(&s, 1, kL), ".taper <- a table is null but its node count is not zero"));
    s = good(); s.envelope_n = 2; s.stop = 9; CHECK(says(fesforce::check(&s, 1, kL), ".envelope <- the table is null but its node count is not zero"));
    s = good(); s.taper_n[0] = FPIC_FORCE_TABLE_MAX; s.taper[0] = tab.data(); s.envelope_n = 2; s.envelope = tab.data(); s.stop = 9; CHECK(fesforce::check(&s, 1, kL) == nullptr);
    s = good(); s.start = 10; s.stop = 9; CHECK(says(fesforce::check(&s, 1, kL), ".start <- must not lie after stop"));
    s = good(); s.start = s.stop = 9; CHECK(fesforce::check(&s, 1, kL) == nullptr);
    const char* span = ".stop <- an envelope table needs start < stop < FPIC_FORCE_FOREVER";
    s = good(); s.envelope_n = 2; s.envelope = tab.data(); CHECK(says(fesforce::check(&s, 1, kL), span));
    s = good(); s.envelope_n = 2; s.envelope = tab.data(); s.start = s.stop = 4; CHECK(says(fesforce::check(&s, 1, kL), span));
    for (double bad : { kInf, kNan }) {
        tab[1024] = bad;
        s = good(); s.taper_n[0] = FPIC_FORCE_TABLE_MAX; s.taper[0] = tab.data(); CHECK(says(fesforce::check(&s, 1, kL), ".taper <- the nodes must be finite"));
        s = good(); s.envelope_n = FPIC_FORCE_TABLE_MAX; s.envelope = tab.data(); s.stop = 5000; CHECK(says(fesforce::check(&s, 1, kL), ".envelope <- the nodes must be finite"));
        s = good(); s.taper_n[0] = 1024; s.taper[0] = tab.data(); CHECK(fesforce::check(&s, 1, kL) == nullptr);
        tab[1024] = 1.0;
    }
}

// ---- cases from a file.  Per case, little endian: int32 kind, nwaves; uint64 epoch, start, stop, count; double L[3], lo[3],
// hi[3], charge, mass, dt; per wave (four of them) double amp[3], int32 mode[3], int32 0, double nu, phase; uint32 taper_n[3],
// envelope_n; the tables' doubles in that order; uint32 n, uint32 0; n x 6 doubles (p, v).  Out per case: doubles active, scale,
// tfrac[4], then per particle inside, v'[3].
template <typename V>
static bool get(std::FILE* f, V* v, size_t n = 1) { return std::fread(v, sizeof(V), n, f) == n; }

static int run_cases(const char* in_path, const char* out_path)
{
    std::FILE* in = std::fopen(in_path, "rb");
    std::FILE* out = std::fopen(out_path, "wb");
    if (!in || !out) { std::printf("FAILED: cannot open the case files\n"); return 1; }
    uint32_t ncases = 0;
    if (!get(in, &ncases)) return 1;
    for (uint32_t c = 0; c < ncases; ++c) {
        fpic_force_spec s;
        std::memset(&s, 0, sizeof s);
        uint64_t count = 0;
        double L[3], charge, mass, dt;
        bool ok = get(in, &s.kind) && get(in, &s.nwaves) && get(in, &s.epoch) && get(in, &s.start) && get(in, &s.stop) && get(in, &count) && get(in, L, 3) && get(in, s.lo, 3) &&
                  get(in, s.hi, 3) && get(in, &charge) && get(in, &mass) && get(in, &dt);
        for (int k = 0; k < FPIC_FORCE_MAX_WAVES && ok; ++k)
            ok = get(in, s.wave[k].amp, 3) && get(in, s.wave[k].mode, 3) && get(in, &s.wave[k].reserved) && get(in, &s.wave[k].nu) && get(in, &s.wave[k].phase);
        ok = ok && get(in, s.taper_n, 3) && get(in, &s.envelope_n);
        std::vector<double> tabs[4];
        for (int a = 0; a < 4 && ok; ++a) {
            const uint32_t n = a < 3 ? s.taper_n[a] : s.envelope_n;
            if (n > FPIC_FORCE_TABLE_MAX) { ok = false; break; }
            tabs[a].resize(n);
            ok = n == 0 || get(in, tabs[a].data(), n);
            if (a < 3) s.taper[a] = n ? tabs[a].data() : nullptr;
            else s.envelope = n ? tabs[a].data() : nullptr;
        }
        uint32_t n = 0, pad = 0;
        ok = ok && get(in, &n) && get(in, &pad);
        if (!ok) { std::printf("FAILED: case %u is cut short\n", c); return 1; }
        std::vector<double> state(static_cast<size_t>(n) * 6);
        if (n && !get(in, state.data(), state.size())) { std::printf("FAILED: case %u is cut short\n", c); return 1; }
        const double Lb[3] = { L[0], L[1], L[2] };
        if (const char* why = fesforce::check(&s, 1, Lb)) { std::printf("FAILED: case %u is refused: %s\n", c, why); return 1; }
        const uint64_t at = count + s.epoch;
        const bool on = fesforce::active(s, at);
        double head[6] = { on ? 1.0 : 0.0, 0, 0, 0, 0, 0 };
        fesforce::Rule r{};
        if (on) {
            r = fesforce::rule_of(s, Lb, charge, mass, dt, at, s.envelope, s.taper);
            head[1] = r.scale;
            for (int k = 0; k < s.nwaves; ++k) head[2 + k] = r.wave[k].tfrac;
        }
        std::fwrite(head, sizeof(double), 6, out);
        for (uint32_t i = 0; i < n; ++i) {
            const double p[3] = { state[6 * i], state[6 * i + 1], state[6 * i + 2] };
            double v[3] = { state[6 * i + 3], state[6 * i + 4], state[6 * i + 5] };
            const bool in_window = on && fesforce::apply(r, p, v);
            const double row[4] = { in_window ? 1.0 : 0.0, v[0], v[1], v[2] };
            std::fwrite(row, sizeof(double), 4, out);
        }
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}

int main(int argc, char** argv)
{
    numbers();
    lookups();
    kicks();
    tallies();
    refusals();
    if (argc == 3 && run_cases(argv[1], argv[2])) return 1;
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
