// Host test of fusion-sim_amd/csrc/fes_load_radial_core.hpp (the rule of a radial load and the checks of its request).
// Without arguments: the cumulative masses, the layout of the tables, a few values known in closed form and every refusal
// by its message.  With <cases> <out>: also evaluates the cases tests/test_load_radial_host.py wrote (little-endian) and
// writes the results as doubles, which that test compares bit for bit with tests/load_radial_reference.py:
//     kind 1  a geometry, a density table and m words  -> per word rho, j, s                      (fesload::radius_of)
//     kind 3  a request, its tables, m indices          -> per index rho, the exact coordinate, mu, q, the exact velocity
//                                                          component, the four look-ups at rho
//             (the exact coordinate and component: z for the sphere, the axis for the cylinder; vth = 0)
// Built with g++ -ffp-contract=off (also with -fsanitize=address,undefined, as a program of its own); prints "ok" and exits
// 0, or names the first failed check and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../fusion-sim_amd/csrc/fes_load_radial_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static bool names(const char* msg, const char* property) { return msg && std::strncmp(msg, property, std::strlen(property)) == 0; }

static const double kBox[3] = { 0.016, 0.012, 0.008 };

static void closed_forms()
{
    const double flat[2] = { 3.0, 3.0 }, holes[7] = { 1, 1, 0, 0, 0, 2, 0 };
    double C[7];
    uint32_t j;
    double s;
    fesload::radial_cumulative(true, flat, 2, C);
    CHECK(C[0] == 0.0 && C[1] == 1.0);                                              // 3 s^3 / 3
    CHECK(fesload::radius_of(true, flat, C, 1, 0.125, j, s) == 0.5 && j == 0);       // the cube root
    CHECK(fesload::radius_of(true, flat, C, 1, 0.0, j, s) == 0.0 && s == 0.0);
    fesload::radial_cumulative(false, flat, 2, C);
    CHECK(C[1] == 1.5);
    CHECK(fesload::radius_of(false, flat, C, 1, 0.25, j, s) == 0.5 && j == 0);       // the square root
    CHECK(fesload::radius_of(false, flat, C, 1, fesload::fraction_of(0xFFFFFFFFu), j, s) < 1.0);
    for (int sphere = 0; sphere < 2; ++sphere) {
        fesload::radial_cumulative(sphere, holes, 7, C);
        CHECK(C[1] > 0 && C[2] > C[1] && C[3] == C[2] && C[4] == C[2] && C[5] > C[4] && C[6] > C[5]);
        fesload::radius_of(sphere, holes, C, 6, 0.0, j, s);
        CHECK(j == 0 && s == 0.0);
        const double rho = fesload::radius_of(sphere, holes, C, 6, fesload::fraction_of(0xFFFFFFFFu), j, s);
        CHECK(j == 5 && s < 1.0 && rho < 1.0);
        fesload::radius_of(sphere, holes, C, 6, C[2] / C[6], j, s);                  // on the hole's edge (or a last bit below it)
        CHECK(j == 1 || j == 4);
    }
    double mu, q;
    fesload::polar_of(0.5, mu, q);
    CHECK(mu == 0.0 && q == 1.0);
    fesload::polar_of(0.0, mu, q);
    CHECK(mu == -1.0 && q == 0.0);
    fesload::polar_of(0.8, mu, q);
    CHECK(std::fabs(mu - 0.6) < 1e-15 && std::fabs(q - 0.8) < 1e-15);
}

static double kD[3] = { 0.0, 1.0, 0.5 }, kT[2] = { 1.0, 2.0 }, kR[4] = { -0.1, 0.0, 0.2, 0.1 }, kZ[2] = { 0.0, 0.01 }, kA[3] = { 0.03, 0.0, -0.03 };
static struct fpic_load_radial good(uint32_t geometry)
{
    struct fpic_load_radial p;
    std::memset(&p, 0, sizeof p);
    p.geometry = geometry;
    p.center[0] = 0.008; p.center[1] = 0.006; p.center[2] = 0.004;
    p.r_max = 0.003;
    p.density_n = 3; p.density = kD;
    p.thermal_n = 2; p.thermal = kT;
    p.radial_n = 4; p.radial = kR;
    if (geometry == FPIC_LOAD_CYLINDER) {
        p.axis = 1;
        p.azimuthal_n = 2; p.azimuthal = kZ;
        p.axial_n = 3; p.axial = kA;
    }
    return p;
}

static void layout_of_the_tables()
{
    struct fpic_load_radial p = good(FPIC_LOAD_CYLINDER);
    CHECK(fesload::check_radial(p, kBox) == nullptr);
    const size_t n = fesload::radial_layout(p, kBox, nullptr, nullptr, nullptr);
    CHECK(n == 2 * 3 + 2 + 4 + 2 + 3);
    std::vector<double> block(n);
    fesload::Radial q;
    CHECK(fesload::radial_layout(p, kBox, block.data(), block.data(), &q) == n);
    CHECK(q.dk == 2 && q.tk == 1 && q.rk == 3 && q.zk == 1 && q.ak == 2 && q.lds_doubles == n && q.needs_pos == 1 && q.axis == 1 && q.geometry == FPIC_LOAD_CYLINDER);
    CHECK(q.dens == block.data() && q.cum == block.data() + 3 && q.therm == block.data() + 6 && q.ur == block.data() + 8 && q.ut == block.data() + 12 && q.ua == block.data() + 14);
    CHECK(q.cum[0] == 0.0 && q.cum[2] > q.cum[1] && q.ua[2] == -0.03 && q.c_f[0] == 0.5 && q.rl[2] == 0.003 / 0.008);
    struct fpic_load_radial bare;
    std::memset(&bare, 0, sizeof bare);
    bare.geometry = FPIC_LOAD_SPHERE; bare.center[0] = bare.center[1] = bare.center[2] = 0.004; bare.r_max = 0.002;
    CHECK(fesload::check_radial(bare, kBox) == nullptr && fesload::radial_layout(bare, kBox, nullptr, nullptr, nullptr) == 4);
    fesload::radial_layout(bare, kBox, block.data(), block.data(), &q);
    CHECK(q.dk == 1 && q.dens[0] == 1.0 && q.dens[1] == 1.0 && q.cum[1] == 1.0 / 3.0 && q.needs_pos == 0 && q.lds_doubles == 4 && !q.therm && !q.ur && !q.ut && !q.ua);
}

static void refusals()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    static double big[FPIC_LOAD_TABLE_MAX + 1];
    for (double& v : big) v = 1.0;
    const uint32_t S = FPIC_LOAD_SPHERE, Cy = FPIC_LOAD_CYLINDER;
    struct fpic_load_radial p = good(S);
    CHECK(fesload::check_radial(p, kBox) == nullptr);
    p.geometry = 0; CHECK(names(fesload::check_radial(p, kBox), ".geometry <- "));
    p.geometry = 3; CHECK(names(fesload::check_radial(p, kBox), ".geometry <- "));
    for (int k = 0; k < 3; ++k) { p = good(Cy); p.reserved[k] = 1; CHECK(names(fesload::check_radial(p, kBox), ".reserved <- ")); }
    p = good(Cy); p.axis = 3; CHECK(names(fesload::check_radial(p, kBox), ".axis <- "));
    p = good(Cy); p.axis = -1; CHECK(names(fesload::check_radial(p, kBox), ".axis <- "));
    p = good(S); p.axis = 1; CHECK(names(fesload::check_radial(p, kBox), ".axis <- "));
    for (double bad : { 0.0, -0.001, inf, nan }) { p = good(S); p.r_max = bad; CHECK(names(fesload::check_radial(p, kBox), ".r_max <- ")); }
    p = good(S); p.r_max = 0.004; CHECK(fesload::check_radial(p, kBox) == nullptr);                            // 2 r_max = the shortest side
    p = good(S); p.r_max = 0.0041; CHECK(names(fesload::check_radial(p, kBox), ".r_max <- the diameter"));
    p = good(Cy); p.axis = 2; p.r_max = 0.006; CHECK(fesload::check_radial(p, kBox) == nullptr);               // the column's own axis does not count
    p = good(Cy); p.axis = 2; p.r_max = 0.0061; CHECK(names(fesload::check_radial(p, kBox), ".r_max <- the diameter"));
    p = good(Cy); p.axis = 1; p.r_max = 0.0041; CHECK(names(fesload::check_radial(p, kBox), ".r_max <- the diameter"));
    for (int k = 0; k < 3; ++k)
        for (double bad : { -1e-9, kBox[k] * 1.0001, inf, nan }) { p = good(Cy); p.center[k] = bad; CHECK(names(fesload::check_radial(p, kBox), ".center <- ")); }
    p = good(S); p.center[0] = 0.0; p.center[1] = kBox[1]; CHECK(fesload::check_radial(p, kBox) == nullptr);  // on the faces: the body wraps
    p = good(S); p.azimuthal_n = 2; p.azimuthal = kZ; CHECK(names(fesload::check_radial(p, kBox), ".azimuthal_n <- a sphere"));
    p = good(S); p.axial_n = 3; p.axial = kA; CHECK(names(fesload::check_radial(p, kBox), ".azimuthal_n <- a sphere"));
    p = good(Cy); p.density_n = 1; CHECK(names(fesload::check_radial(p, kBox), ".density_n <- "));
    p = good(Cy); p.density_n = FPIC_LOAD_TABLE_MAX + 1; p.density = big; CHECK(names(fesload::check_radial(p, kBox), ".density_n <- "));
    p = good(Cy); p.density_n = FPIC_LOAD_TABLE_MAX; p.density = big; CHECK(fesload::check_radial(p, kBox) == nullptr);
    p = good(Cy); p.thermal_n = 1; CHECK(names(fesload::check_radial(p, kBox), ".thermal_n <- "));
    p = good(Cy); p.radial_n = 0xFFFFFFFFu; CHECK(names(fesload::check_radial(p, kBox), ".radial_n <- "));
    p = good(Cy); p.azimuthal_n = 1; CHECK(names(fesload::check_radial(p, kBox), ".azimuthal_n <- "));
    p = good(Cy); p.axial_n = FPIC_LOAD_TABLE_MAX + 1; p.axial = big; CHECK(names(fesload::check_radial(p, kBox), ".axial_n <- "));
    p = good(Cy); p.density = nullptr; CHECK(names(fesload::check_radial(p, kBox), ".density <- the table is null"));
    p = good(Cy); p.thermal = nullptr; CHECK(names(fesload::check_radial(p, kBox), ".thermal <- the table is null"));
    p = good(Cy); p.radial = nullptr; CHECK(names(fesload::check_radial(p, kBox), ".radial <- the table is null"));
    p = good(Cy); p.azimuthal = nullptr; CHECK(names(fesload::check_radial(p, kBox), ".azimuthal <- the table is null"));
    p = good(Cy); p.axial = nullptr; CHECK(names(fesload::check_radial(p, kBox), ".axial <- the table is null"));
    p = good(S); p.azimuthal = kZ; CHECK(fesload::check_radial(p, kBox) == nullptr);                         // (a pointer without a count is not read)
    for (double bad : { inf, -inf, nan }) {
        double d[3] = { 0.0, bad, 0.5 }, t[2] = { bad, 1.0 }, r[4] = { 0.0, 0.0, 0.0, bad }, z[2] = { bad, 0.0 }, a[3] = { 0.0, bad, 0.0 };
        p = good(Cy); p.density = d; CHECK(names(fesload::check_radial(p, kBox), ".density <- values must be finite"));
        p = good(Cy); p.thermal = t; CHECK(names(fesload::check_radial(p, kBox), ".thermal <- values must be finite"));
        p = good(Cy); p.radial = r; CHECK(names(fesload::check_radial(p, kBox), ".radial <- values must be finite"));
        p = good(Cy); p.azimuthal = z; CHECK(names(fesload::check_radial(p, kBox), ".azimuthal <- values must be finite"));
        p = good(Cy); p.axial = a; CHECK(names(fesload::check_radial(p, kBox), ".axial <- values must be finite"));
    }
    double neg[3] = { 1.0, -1e-300, 1.0 }, zero[3] = { 0.0, 0.0, 0.0 }, huge[3] = { 1.7e308, 1.7e308, 1.7e308 }, tneg[2] = { 1.0, -0.5 }, tzero[2] = { 0.0, 0.0 };
    for (uint32_t g : { S, Cy }) {
        p = good(g); p.density = neg; CHECK(names(fesload::check_radial(p, kBox), ".density <- values must not be negative"));
        p = good(g); p.density = zero; CHECK(names(fesload::check_radial(p, kBox), ".density <- the table holds no mass"));
        p = good(g); p.density = huge; CHECK(names(fesload::check_radial(p, kBox), ".density <- the total of the table must be finite"));
        p = good(g); p.thermal = tneg; CHECK(names(fesload::check_radial(p, kBox), ".thermal <- values must not be negative"));
        p = good(g); p.thermal = tzero; CHECK(fesload::check_radial(p, kBox) == nullptr);                     // a cold body is allowed
    }
}

template <typename V>
static bool get(std::FILE* f, V* v, size_t n = 1) { return std::fread(v, sizeof(V), n, f) == n; }

static bool cases(const char* in_path, const char* out_path)
{
    std::FILE* in = std::fopen(in_path, "rb");
    std::FILE* out = std::fopen(out_path, "wb");
    bool ok = in && out;
    uint32_t ncases = 0;
    ok = ok && get(in, &ncases);
    for (uint32_t c = 0; ok && c < ncases; ++c) {
        uint32_t kind = 0, geometry = 0, n = 0, m = 0;
        ok = get(in, &kind) && get(in, &geometry) && (geometry == FPIC_LOAD_SPHERE || geometry == FPIC_LOAD_CYLINDER);
        const bool sphere = geometry == FPIC_LOAD_SPHERE;
        std::vector<double> res;
        if (ok && kind == 1) {
            ok = get(in, &n) && get(in, &m) && n >= 2 && n <= FPIC_LOAD_TABLE_MAX;
            std::vector<double> tab(ok ? n : 0), C(ok ? n : 0);
            std::vector<uint32_t> w(ok ? m : 0);
            ok = ok && get(in, tab.data(), n) && get(in, w.data(), m);
            if (!ok) break;
            fesload::radial_cumulative(sphere, tab.data(), n, C.data());
            for (uint32_t k = 0; k < m; ++k) {
                uint32_t j;
                double s;
                const double v = fesload::radius_of(sphere, tab.data(), C.data(), n - 1, fesload::fraction_of(w[k]), j, s);
                res.insert(res.end(), { v, static_cast<double>(j), s });
            }
        } else if (ok && kind == 3) {
            fpic_load_spec s;
            std::memset(&s, 0, sizeof s);
            struct fpic_load_radial p;
            std::memset(&p, 0, sizeof p);
            p.geometry = geometry;
            double L[3];
            uint32_t lattice = 0, counts[5] = {};
            ok = get(in, &p.axis) && get(in, &lattice) && get(in, &s.seed) && get(in, &s.stream) && get(in, L, 3) && get(in, s.lo, 3) && get(in, s.hi, 3) &&
                 get(in, s.drift, 3) && get(in, p.center, 3) && get(in, &p.r_max) && get(in, counts, 5);
            std::vector<double> tabs[5];
            for (int t = 0; ok && t < 5; ++t) {
                ok = counts[t] <= FPIC_LOAD_TABLE_MAX;
                if (ok) tabs[t].resize(counts[t]);
                ok = ok && get(in, tabs[t].data(), counts[t]);
            }
            ok = ok && get(in, &m);
            std::vector<uint32_t> idx(ok ? m : 0);
            ok = ok && get(in, idx.data(), m);
            if (!ok) break;
            s.flags = FPIC_LOAD_POS | FPIC_LOAD_VEL | (lattice ? FPIC_LOAD_LATTICE : 0u);
            s.count = 1;
            p.density_n = counts[0]; p.density = counts[0] ? tabs[0].data() : nullptr;
            p.thermal_n = counts[1]; p.thermal = counts[1] ? tabs[1].data() : nullptr;
            p.radial_n = counts[2]; p.radial = counts[2] ? tabs[2].data() : nullptr;
            p.azimuthal_n = counts[3]; p.azimuthal = counts[3] ? tabs[3].data() : nullptr;
            p.axial_n = counts[4]; p.axial = counts[4] ? tabs[4].data() : nullptr;
            const double box[3] = { L[0], L[1], L[2] };
            CHECK(fesload::check(s, 1, ~0ull, box, true) == nullptr);
            CHECK(fesload::check_radial(p, box) == nullptr);
            if (failures) { ok = false; break; }
            const fesload::Rule r = fesload::rule_of(s, ~0ull, box);
            std::vector<double> block(fesload::radial_layout(p, box, nullptr, nullptr, nullptr));
            fesload::Radial q;
            fesload::radial_layout(p, box, block.data(), block.data(), &q);
            const int exact = sphere ? 2 : p.axis;
            for (uint32_t k = 0; k < m; ++k) {
                double pos[3], dir[3], v[3], theta, rho, mu = 0.0, qq = 0.0;
                fesload::radial_base_of(r, q, idx[k], pos, theta, rho, dir);
                fesload::radial_velocity_of(r, q, idx[k], theta, rho, dir, v);     // (vth = 0: the drift and the flows alone)
                if (sphere) {
                    uint32_t w[4];
                    if (lattice) w[1] = fesload::lattice_word(idx[k], r.mult[1], r.shift[1]);
                    else fesload::philox(idx[k], r.stream, 0u, fesload::kTag, r.seed_lo, r.seed_hi, w);
                    fesload::polar_of(fesload::fraction_of(w[1]), mu, qq);
                    CHECK(dir[2] == mu);
                }
                res.insert(res.end(), { rho, pos[exact], mu, qq, v[exact], q.tk ? fesload::lookup(q.therm, q.tk, rho) : 0.0, q.rk ? fesload::lookup(q.ur, q.rk, rho) : 0.0,
                                        q.zk ? fesload::lookup(q.ut, q.zk, rho) : 0.0, q.ak ? fesload::lookup(q.ua, q.ak, rho) : 0.0 });
            }
        } else {
            ok = false;
        }
        ok = ok && std::fwrite(res.data(), sizeof(double), res.size(), out) == res.size();
    }
    if (in) std::fclose(in);
    if (out) ok = std::fclose(out) == 0 && ok;
    return ok;
}

int main(int argc, char** argv)
{
    closed_forms();
    layout_of_the_tables();
    refusals();
    if (argc == 3) CHECK(cases(argv[1], argv[2]));
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
