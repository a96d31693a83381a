// Host test of fusion-sim_amd/csrc/fes_burn_core.hpp (the rule of the fusion burn and the checks of a request): the request
// as fpic_fusion's, the tags, the words' layout, hand-made pairs, the fit rule on both sides of every bound, the result's
// conversion, and every refusal by its message.
// With two arguments it also reads cases from a file (tests/test_burn_host.py writes them: a request and random pairs with
// their chains, then events) and writes what the rule gives — P, the acceptance word, the acceptance, the chain's minimum and
// who reacts, the direction's try and the outcome — which the numpy reference must give bit for bit.
// Built with g++ -ffp-contract=off by tests/test_burn_host.py (also with -fsanitize=address,undefined, as a program of its
// own); prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../fusion-sim_amd/csrc/fes_burn_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
static const double kFlat[4] = { 2e-28, 2e-28, 2e-28, 2e-28 };

static fpic_burn_spec good()
{
    fpic_burn_spec s;
    std::memset(&s, 0, sizeof s);
    s.species_a = 0;
    s.species_b = 1;
    s.product_a = 2;
    s.product_b = 3;
    s.seed = 0x1234567890ull;
    s.tau = 1e-9;
    s.g_lo = 0.0;
    s.g_hi = 0.5;
    s.n = 4;
    s.sigma = kFlat;
    s.q_value = 2.8e-12;
    return s;
}
static bool says(const char* msg, const char* text) { return msg && std::strcmp(msg, text) == 0; }

static void numbers()
{
    const fpic_burn_spec s = good();
    const fpic_fusion_spec q = fesburn::fusion_of(s);
    CHECK(q.species_a == 0 && q.species_b == 1 && q.seed == s.seed && q.tau == s.tau && q.g_lo == 0 && q.g_hi == 0.5 && q.n == 4 && q.sigma == kFlat && q.reserved_i == 0);
    const double ma = 3.0, mb = 5.0, m3 = 6.0, m4 = 2.0;
    const fesburn::Rule r = fesburn::rule_of(s, 7, 1e10, 2.0, ma, mb, m3, m4);
    const fesfusion::Rule f = fesfusion::rule_of(q, 7, 1e10, 2.0);
    CHECK(r.f.epoch == 7 && r.f.ww == f.ww && r.f.inv_dg == f.inv_dg && r.f.s_max == 2e-28 && r.w == 1e10 && r.tracked_b == 1);
    const double cc = fesfusion::kC * fesfusion::kC;
    CHECK(r.f_a == 3.0 / 8.0 && r.f_b == 5.0 / 8.0 && r.hk == (0.5 * (15.0 / 8.0)) * cc && r.kf == ((2.0 * m4) / (m3 * (m3 + m4))) / cc && r.r34 == 3.0 && r.q_value == s.q_value);
    // the tags are this operator's own
    uint32_t b[4];
    fesload::philox(5, 7, r.f.stream, 0xB0510u, r.f.seed_lo, r.f.seed_hi, b);
    CHECK(fesburn::key_of(r, 5) == b[0] && fesburn::kTag != fesfusion::kTag && fesburn::kTag != fesion::kTag && fesburn::kDirTag != fesfspec::kDirTag);
    fesload::philox(5, 7, r.f.stream, 0xB0512u, r.f.seed_lo, r.f.seed_hi, b);
    CHECK(fesburn::accept_word(r, 5, true) == b[0] && fesburn::accept_word(r, 5, false) != b[0]);
    // the words: four tallies one behind the other
    CHECK(fesburn::kWords == 47 && fesburn::kGenAt == 9 && fesburn::kLostAt == 27);
    int counts = 0, lows = 0, highs = 0, bits = 0;
    for (int k = 0; k < fesburn::kWords; ++k) {
        const int kind = fesburn::word_kind(k);
        counts += kind == fesburn::kCount;
        lows += kind == fesburn::kSumLo;
        highs += kind == fesburn::kSumHi;
        bits += kind == fesburn::kBits;
        if (kind == fesburn::kSumLo) CHECK(fesburn::word_kind(k + 1) == fesburn::kSumHi);
    }
    CHECK(counts == 12 && lows == 16 && highs == 16 && bits == 3 && fesburn::word_kind(26) == fesburn::kBits && fesburn::word_kind(27) == fesburn::kCount && fesburn::word_kind(46) == fesburn::kBits);
}

static void rule()
{
    fpic_burn_spec s = good();
    s.g_lo = 0.125;
    const fesburn::Rule r = fesburn::rule_of(s, 0, 1e10, 2.0, 3.0, 5.0, 6.0, 2.0);
    double p = -1;
    const double rest[3] = { 0.25, 0.0, 0.0 }, slow[3] = { 0.25, 0.0625, 0.0 }, fast[3] = { 0.75, 0.0, 0.0 }, nan_v[3] = { kNan, 0.0, 0.0 }, mid[3] = { 0.25, 0.0, 0.25 };
    CHECK(fesburn::probability(r, kFlat, 7.0, rest, rest, &p) == fesburn::kBelow && p == 0);      // a pair at rest: below when g_lo > 0
    CHECK(fesburn::probability(r, kFlat, 7.0, rest, slow, &p) == fesburn::kBelow && p == 0);
    CHECK(fesburn::probability(r, kFlat, 7.0, rest, fast, &p) == fesburn::kAbove && p == 0);
    CHECK(fesburn::probability(r, kFlat, 7.0, rest, nan_v, &p) == fesburn::kAbove);
    CHECK(fesburn::probability(r, kFlat, 7.0, rest, mid, &p) == fesburn::kInside);
    const double y = ((((1e10 * 1e10) * 7.0) * 1e-9) / 2.0) * (2e-28 * (0.25 * fesfusion::kC));
    CHECK(p == y / 1e10 && p > 0);
    // the acceptance: strictly below P; P >= 1 takes every word
    CHECK(fesburn::accepts(0xFFFFFFFFu, 1.0) && !fesburn::accepts(0u, 0.0) && fesburn::accepts(0u, 0x1p-33 + 0x1p-60) && !fesburn::accepts(0u, 0x1p-33));
    CHECK(fesburn::few_of(13, 5) == 3 && fesburn::wins(3, 3) && !fesburn::wins(3, 8) && !fesburn::wins(fesburn::kNoPlace, 0));
    // the outcome conserves momentum and shares q + K; like species: both fractions are one half
    const double n[3] = { 0.6, 0.0, 0.8 }, va[3] = { 0.01, 0.0, 0.0 }, vb[3] = { 0.0, 0.0, -0.01 };
    double w3[3], w4[3];
    fesburn::outcome(r, va, vb, n, w3, w4);
    for (int i = 0; i < 3; ++i) {
        const double V = (3.0 / 8.0) * va[i] + (5.0 / 8.0) * vb[i];
        CHECK(std::fabs((6.0 * w3[i] + 2.0 * w4[i]) - 8.0 * V) < 1e-15);
    }
    const fesburn::Rule like = fesburn::rule_of(s, 0, 1e10, 2.0, 3.0, 3.0, 6.0, 2.0);
    CHECK(like.f_a == 0.5 && like.f_b == 0.5);
    // a negative q_value below the threshold: Et is held to 0, the products move with the centre of mass
    s.q_value = -1e30;                                 // (the masses here are kilograms: K is about 1e13 J)
    const fesburn::Rule cold = fesburn::rule_of(s, 0, 1e10, 2.0, 3.0, 5.0, 6.0, 2.0);
    fesburn::outcome(cold, va, vb, n, w3, w4);
    CHECK(w3[0] == (3.0 / 8.0) * 0.01 && w4[0] == w3[0] && w3[2] == (5.0 / 8.0) * -0.01 && w4[2] == w3[2]);
}

static void fit_and_result()
{
    const uint64_t end = 0xFFFFFFFFull;
    CHECK(fesburn::fit(5, 10, 15, 10, true, 0, 5, 0) == fesburn::kFits);
    CHECK(fesburn::fit(6, 10, 15, 10, true, 0, 6, 0) == fesburn::kNoRoomA && fesburn::fit(6, 10, 16, 10, true, 0, 5, 0) == fesburn::kNoRoomB);
    CHECK(fesburn::fit(6, 10, 16, 10, false, 0, 0, 0) == fesburn::kFits);                           // an untracked product needs no room
    CHECK(fesburn::fit(5, 10, 100, end - 5, true, 0, 5, 0) == fesburn::kFits && fesburn::fit(5, 10, 100, end - 4, true, 0, 5, 0) == fesburn::kNoRoomA);
    CHECK(fesburn::fit(5, 0, 5, 0, true, 10, 100, end - 5) == fesburn::kFits && fesburn::fit(5, 0, 5, 0, true, 10, 100, end - 4) == fesburn::kNoRoomB);
    CHECK(fesburn::fit(0, 7, 7, end, true, 7, 7, end) == fesburn::kFits && fesburn::fit(1, 7, 7, 3, true, 9, 9, 3) == fesburn::kNoRoomA);
    CHECK(says(fesburn::fit_field(fesburn::kNoRoomA), "product_a") && says(fesburn::fit_field(fesburn::kNoRoomB), "product_b"));
    uint64_t w[fesburn::kWords] = {};
    for (int k = 0; k < 9; ++k) w[k] = 10 + k;
    w[fesburn::kGenAt] = 4;
    w[fesburn::kGenAt + 1] = 1ull << 16;              // product_a's energy: 2^16 2^-80
    w[fesburn::kGenAt + 9 + 2] = 3;                   // product_b's momentum x
    w[fesburn::kGenAt + fesburn::kGenWords - 1] = 1u << 5;      // product_b's momentum x is out of range
    w[fesburn::kLostAt] = 4;
    w[fesburn::kLostAt + fesburn::kLostWords] = 4;
    w[fesburn::kLostAt + fesburn::kLostWords + 3] = 7;
    const double mass[4] = { 3.0, 5.0, 6.0, 2.0 }, charge[4] = { 1.0, 1.0, 2.0, 0.0 };
    fpic_burn_result out;
    std::memset(&out, 0, sizeof out);
    fesburn::result_of(w, mass, charge, 10.0, &out);
    CHECK(out.pairs == 10 && out.below == 11 && out.above == 12 && out.cells == 13 && out.overfull_cells == 14 && out.overfull_particles == 15 && out.accepted == 16 &&
          out.blocked == 17 && out.saturated == 18 && out.burnt == 4 && out.applications == 0);
    CHECK(out.product_a.energy_fixed[0] == (1ull << 16) && out.product_a.energy == 0.5 * 6.0 * 10.0 * fesforce::kC * fesforce::kC * std::ldexp(1.0, -64) && out.product_a.charge == 80.0);
    CHECK(out.product_b.momentum_fixed[0][0] == 3 && std::isnan(out.product_b.momentum[0]) && out.product_b.momentum[1] == 0 && out.product_b.charge == 0.0);
    CHECK(out.reactant_a.charge == 40.0 && out.reactant_b.momentum_fixed[0][0] == 7 && out.reactant_b.momentum[0] == 5.0 * 10.0 * fesforce::kC * (7.0 * std::ldexp(1.0, -80)));
}

static void refusals()
{
    const int ns = 4;
    fpic_burn_spec s = good();
    CHECK(fesburn::check(&s, ns) == nullptr && fesburn::check_bound(s, 1e10, 1.0) == nullptr);
    CHECK(says(fesburn::check(nullptr, ns), ".spec <- Non-optional property is undefined!"));
#define REFUSED(change, text)                       \
    do {                                            \
        fpic_burn_spec t = good();                  \
        change;                                     \
        CHECK(says(fesburn::check(&t, ns), text));  \
    } while (0)
    REFUSED(t.reserved_i = 1, ".reserved <- must be zero");
    REFUSED(t.reserved[3] = 1e-300, ".reserved <- must be zero");
    REFUSED(t.reserved[0] = kNan, ".reserved <- must be zero");
    // everything fpic_fusion refuses of the shared fields
    REFUSED(t.species_a = -1, ".species_a <- no such species");
    REFUSED(t.species_a = 4, ".species_a <- no such species");
    REFUSED(t.species_b = 4, ".species_b <- no such species");
    REFUSED(t.tau = kNan, ".tau <- must not be NaN");
    REFUSED(t.tau = 0, ".tau <- must be positive and finite");
    REFUSED(t.tau = kInf, ".tau <- must be positive and finite");
    REFUSED(t.n = 1, ".n <- must be 2 .. FPIC_FUSION_TABLE_MAX (4096)");
    REFUSED(t.n = 4097, ".n <- must be 2 .. FPIC_FUSION_TABLE_MAX (4096)");
    REFUSED(t.sigma = nullptr, ".sigma <- Non-optional property is undefined!");
    REFUSED(t.g_lo = -0.1, ".g_lo <- must be finite and not negative");
    REFUSED(t.g_hi = 0.0, ".g_hi <- must be finite and above g_lo");
    REFUSED(t.g_hi = kInf, ".g_hi <- must be finite and above g_lo");
    static const double bad[4] = { 1e-28, -1e-28, 0, 0 }, inf_s[4] = { 1e-28, kInf, 0, 0 };
    REFUSED(t.sigma = bad, ".sigma <- every entry must be finite and not negative");
    REFUSED(t.sigma = inf_s, ".sigma <- every entry must be finite and not negative");
    // the products
    REFUSED(t.product_a = -1, ".product_a <- no such species");
    REFUSED(t.product_a = 4, ".product_a <- no such species");
    REFUSED(t.product_b = -2, ".product_b <- must be -1 (not tracked) or a species of the handle");
    REFUSED(t.product_b = 4, ".product_b <- must be -1 (not tracked) or a species of the handle");
    REFUSED(t.product_a = 0, ".product_a <- must differ from the reactants");
    REFUSED(t.product_a = 1, ".product_a <- must differ from the reactants");
    REFUSED(t.product_b = 0, ".product_b <- must differ from the reactants");
    REFUSED(t.product_b = 1, ".product_b <- must differ from the reactants");
    REFUSED(t.product_b = 2, ".product_b <- must differ from product_a");
    REFUSED(t.other_mass = 1e-27, ".other_mass <- must be zero when product_b is a species: its mass is the species'");
    REFUSED(t.other_mass = kNan, ".other_mass <- must be zero when product_b is a species: its mass is the species'");
    REFUSED(t.product_b = -1, ".other_mass <- must be positive and finite when product_b is -1");
    REFUSED((t.product_b = -1, t.other_mass = kInf), ".other_mass <- must be positive and finite when product_b is -1");
    REFUSED((t.product_b = -1, t.other_mass = -1.0), ".other_mass <- must be positive and finite when product_b is -1");
    REFUSED(t.q_value = kNan, ".q_value <- must be finite");
    REFUSED(t.q_value = -kInf, ".q_value <- must be finite");
#undef REFUSED
    fpic_burn_spec t = good();
    t.product_b = -1;
    t.other_mass = 1.6e-27;
    t.species_b = 0;                                   // like species, an untracked product, a negative q_value: good
    t.q_value = -1e-13;
    CHECK(fesburn::check(&t, ns) == nullptr);
    t = good();
    t.tau = 1e300;
    CHECK(says(fesburn::check_bound(t, 1e10, 1e-300), ".sigma <- the yield bound W W 2048 tau max(sigma) g_hi c / dV is not a finite number"));
}

// ---- the cases of tests/test_burn_host.py
template <typename T>
static bool take(const std::vector<unsigned char>& in, size_t& at, T* out, size_t count)
{
    if (at + count * sizeof(T) > in.size()) return false;
    std::memcpy(out, in.data() + at, count * sizeof(T));
    at += count * sizeof(T);
    return true;
}
static uint64_t bits_of(double x)
{
    uint64_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}

static int run_cases(const char* in_path, const char* out_path)
{
    std::FILE* f = std::fopen(in_path, "rb");
    if (!f) return 1;
    std::vector<unsigned char> in;
    unsigned char buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
    std::vector<uint64_t> out;
    size_t at = 0;
    uint32_t ncases = 0;
    if (!take(in, at, &ncases, 1)) return 1;
    for (uint32_t c = 0; c < ncases; ++c) {
        uint32_t head[6];                             // n, stream, epoch, npairs, nchains, nevents
        uint64_t seed;
        double real[11];                              // tau, g_lo, g_hi, W, dV, m_a, m_b, m3, m4, q_value, (unused)
        if (!take(in, at, head, 6) || !take(in, at, &seed, 1) || !take(in, at, real, 11)) return 1;
        std::vector<double> S(head[0]);
        if (!take(in, at, S.data(), S.size())) return 1;
        fpic_burn_spec s = good();
        s.seed = seed;
        s.stream = head[1];
        s.tau = real[0];
        s.g_lo = real[1];
        s.g_hi = real[2];
        s.n = static_cast<int32_t>(head[0]);
        s.sigma = S.data();
        s.q_value = real[9];
        if (fesburn::check(&s, 4) || fesburn::check_bound(s, real[3], real[4])) return 1;
        const fesburn::Rule r = fesburn::rule_of(s, head[2], real[3], real[4], real[5], real[6], real[7], real[8]);
        const uint32_t npairs = head[3], nchains = head[4], nevents = head[5];
        std::vector<uint32_t> id(npairs), side(npairs), chain(npairs), place(npairs);
        std::vector<double> nl(npairs), v(static_cast<size_t>(npairs) * 6);
        if (!take(in, at, id.data(), npairs) || !take(in, at, side.data(), npairs) || !take(in, at, chain.data(), npairs) || !take(in, at, place.data(), npairs) ||
            !take(in, at, nl.data(), npairs) || !take(in, at, v.data(), v.size()))
            return 1;
        // the chains' words as the kernel keeps them: kNoPlace, then the least accepted place
        std::vector<uint32_t> least(nchains, fesburn::kNoPlace);
        std::vector<double> P(npairs);
        std::vector<int> what(npairs), accepted(npairs);
        std::vector<uint32_t> u(npairs);
        for (uint32_t k = 0; k < npairs; ++k) {
            const double vo[3] = { v[6 * k], v[6 * k + 1], v[6 * k + 2] }, vp[3] = { v[6 * k + 3], v[6 * k + 4], v[6 * k + 5] };
            if (chain[k] >= nchains) return 1;
            what[k] = fesburn::probability(r, S.data(), nl[k], vo, vp, &P[k]);
            u[k] = fesburn::accept_word(r, id[k], side[k] != 0);
            accepted[k] = what[k] == fesburn::kInside && fesburn::accepts(u[k], P[k]);
            if (accepted[k] && place[k] < least[chain[k]]) least[chain[k]] = place[k];
        }
        for (uint32_t k = 0; k < npairs; ++k) {
            out.push_back(bits_of(P[k]));
            out.push_back(static_cast<uint64_t>(what[k]));
            out.push_back(u[k]);
            out.push_back(static_cast<uint64_t>(accepted[k]));
            out.push_back(accepted[k] && fesburn::wins(least[chain[k]], place[k]) ? 1u : 0u);
        }
        std::vector<uint32_t> ida(nevents);
        std::vector<double> ev(static_cast<size_t>(nevents) * 6);
        if (!take(in, at, ida.data(), nevents) || !take(in, at, ev.data(), ev.size())) return 1;
        for (uint32_t k = 0; k < nevents; ++k) {
            const double va[3] = { ev[6 * k], ev[6 * k + 1], ev[6 * k + 2] }, vb[3] = { ev[6 * k + 3], ev[6 * k + 4], ev[6 * k + 5] };
            double n[3], w3[3], w4[3];
            out.push_back(static_cast<uint64_t>(fesburn::direction_of(r, ida[k], n)));
            fesburn::outcome(r, va, vb, n, w3, w4);
            for (double x : w3) out.push_back(bits_of(x));
            for (double x : w4) out.push_back(bits_of(x));
        }
    }
    if (at != in.size()) return 1;
    f = std::fopen(out_path, "wb");
    if (!f) return 1;
    const bool wrote = std::fwrite(out.data(), sizeof(uint64_t), out.size(), f) == out.size();
    std::fclose(f);
    return wrote ? 0 : 1;
}

int main(int argc, char** argv)
{
    numbers();
    rule();
    fit_and_result();
    refusals();
    if (argc == 3 && run_cases(argv[1], argv[2])) {
        std::printf("FAILED: the cases of %s\n", argv[1]);
        ++failures;
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
