// fes_force_core.hpp — the rule of the prescribed external forces of a CART3D handle (fpic_force; the kernels are
// fes_force_kernels.hpp, the orchestration fes_force.inc.hpp): the host-side numbers of an application, the window, the
// tapers, the waves and the kick of one particle, and the checks of a request.  Plain C++ that compiles for the host and the
// device, shared with a host test (tests/native/force_core_test.cpp, g++).
//
// What happens to a particle depends on the request, s = sub-step count + epoch and its own stored state alone.  All
// arithmetic is double, every operation rounded once (build with -ffp-contract=off, as the library is); the stored T state is
// converted to double and the new velocity is cast back to T.  Positions are box fractions, velocities in units of c.
//
//   numbers    (rule_of, on the host) kq = (charge dt) / (mass c) (FIELD), dt / c (ACCEL); lo_f = lo / L, hi_f = hi / L,
//              w = hi_f - lo_f; per wave tw = nu (double) s, tfrac = tw - floor(tw); active iff start <= s <= stop;
//              g = ((double)(s - start) K) / (double)(stop - start), j = min((int) g, K - 1), r = g - j,
//              env = tab[j] + (tab[j+1] - tab[j]) r (no table: 1); scale = kq env.
//   window     inside iff lo_f[a] <= p[a] < hi_f[a] on the three axes.
//   taper      f = (p[a] - lo_f[a]) / w[a]; fesload::lookup (g = f K, j = min((int) g, K - 1), s = g - j,
//              tab[j] + (tab[j+1] - tab[j]) s); taper = (tx ty) tz over the tables present.
//   waves      theta = (m0 p0 + m1 p1) + m2 p2; arg = (theta - tfrac_k) + phase_k; c_k = cospi_(2 arg).
//   kick       e[a] = amp_0[a] c_0, e[a] = e[a] + amp_k[a] c_k; sc = scale or scale taper; d[a] = sc e[a]; v'[a] = v[a] + d[a].
//
// Where the kick sits: the hook runs after the move, at the new position and time.  Without B that equals adding the field
// to the two half-kicks of the next push (leapfrog with the total field); with B the external kick comes wholly before the
// Boris rotation instead of straddling it — an operator-splitting term of order (omega_c dt) times the kick.
#ifndef FES_FORCE_CORE_HPP
#define FES_FORCE_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_load_profile_core.hpp"

namespace fesforce {

constexpr double kC = 2.998e8;            // the box's c (fes_host_push.inc.hpp)
constexpr int kWords = 10;                // the device words of a request: kicked | work (lo, hi) | impulse x, y, z (lo, hi) | out-of-range bits

struct Wave {
    double amp[3], m[3];
    double tfrac, phase;
};

// an application as the kernels read it
struct Rule {
    int nwaves, tapered, whole;           // tapered: any taper table; whole: the window is the box
    double lo_f[3], hi_f[3], w[3];
    uint32_t tk[3];                       // the INTERVALS of the taper tables (nodes - 1), 0: no table
    const double* tab[3];
    double scale;
    Wave wave[FPIC_FORCE_MAX_WAVES];
};

FES_HIST_HD bool inside(const Rule& r, const double (&p)[3])
{
    bool in = true;
    for (int a = 0; a < 3; ++a) in = in && r.lo_f[a] <= p[a] && p[a] < r.hi_f[a];
    return in;
}

// the product of the taper tables at p (the caller has found p inside); tab: where the tables are read (r.tab, or a
// workgroup's copies of them)
FES_HIST_HD double taper_of(const Rule& r, const double* const (&tab)[3], const double (&p)[3])
{
    double t = 1.0;
    bool first = true;
    for (int a = 0; a < 3; ++a) {
        if (!r.tk[a]) continue;
        const double off = p[a] - r.lo_f[a];
        const double f = off / r.w[a];
        const double val = fesload::lookup(tab[a], r.tk[a], f);
        t = first ? val : t * val;
        first = false;
    }
    return t;
}

// the kick of an inside particle: v is read and rewritten (still double: the caller casts)
template <bool TAPER>
FES_HIST_HD void kick(const Rule& r, const double* const (&tab)[3], const double (&p)[3], double (&v)[3])
{
    double e[3] = { 0, 0, 0 };
    const double p0 = p[0], p1 = p[1], p2 = p[2];
    for (int k = 0; k < r.nwaves; ++k) {
        const Wave& q = r.wave[k];
        const double tx = q.m[0] * p0, ty = q.m[1] * p1, tz = q.m[2] * p2;
        const double txy = tx + ty;
        const double theta = txy + tz;
        const double back = theta - q.tfrac;
        const double arg = back + q.phase;
        const double c = fesload::cospi_(2.0 * arg);
        for (int a = 0; a < 3; ++a) {
            const double t = q.amp[a] * c;
            e[a] = k ? e[a] + t : t;
        }
    }
    double sc = r.scale;
    if (TAPER) sc = r.scale * taper_of(r, tab, p);
    for (int a = 0; a < 3; ++a) {
        const double d = sc * e[a];
        v[a] = v[a] + d;
    }
}

// the whole rule for one live particle (the host test's form): true if it is inside, v then holds v'
inline bool apply(const Rule& r, const double (&p)[3], double (&v)[3])
{
    if (!inside(r, p)) return false;
    const double* const tab[3] = { r.tab[0], r.tab[1], r.tab[2] };
    if (r.tapered) kick<true>(r, tab, p, v);
    else kick<false>(r, tab, p, v);
    return true;
}

// ---- the tally terms of a particle whose velocity a pass changed (the forces' and fpic_gas's).  floor(d 2^80) exactly for
// |d| < kFixRange, as a 128-bit two's complement integer: fes::to_fix (fes_diag_kernels.hpp) restated for the host and the
// device, so that the host tests run what the kernels run.
using Fix = unsigned __int128;
constexpr double kFixRange = 0x1p15;      // = fes::kFixRange
FES_HIST_HD Fix floor_fix(double d)
{
    const double y = fabs(d) * 0x1p80;
    const double h = floor(y * 0x1p-64);
    const double r = y - h * 0x1p64;
    const unsigned long long lo = static_cast<unsigned long long>(r);
    const Fix mag = (static_cast<Fix>(static_cast<unsigned long long>(h)) << 64) + lo;
    if (!(d < 0)) return mag;
    return ~mag + (static_cast<double>(lo) != r ? 0 : 1);
}
// after - before into `sum`, or — either outside the range — the bit into `out`
FES_HIST_HD void fix_diff(Fix& sum, unsigned long long& out, double before, double after, int bit)
{
    if (fabs(before) < kFixRange && fabs(after) < kFixRange) sum += floor_fix(after) - floor_fix(before);
    else out |= 1ull << bit;
}
// u0 the stored velocity before, w the stored velocity after, both as doubles.  sum[0] energy (|w|^2 - |u0|^2: the work),
// sum[1 .. 3] momentum (the impulse); out: bit 0 energy, bits 1 .. 3 momentum
FES_HIST_HD void tally(const double (&u0)[3], const double (&w)[3], Fix (&sum)[4], unsigned long long& out)
{
    for (int a = 0; a < 3; ++a) fix_diff(sum[1 + a], out, u0[a], w[a], 1 + a);
    const double b00 = u0[0] * u0[0], b11 = u0[1] * u0[1], b22 = u0[2] * u0[2];
    const double a00 = w[0] * w[0], a11 = w[1] * w[1], a22 = w[2] * w[2];
    const double b01 = b00 + b11, a01 = a00 + a11;
    fix_diff(sum[0], out, b01 + b22, a01 + a22, 0);
}

// ---- the host-side numbers
inline bool active(const fpic_force_spec& s, uint64_t at) { return s.start <= at && at <= s.stop; }

inline double tfrac_of(double nu, uint64_t at)
{
    const double tw = nu * static_cast<double>(at);
    return tw - std::floor(tw);
}

// the envelope at `at` (the request is active there): tab has s.envelope_n nodes, or none
inline double envelope_of(const fpic_force_spec& s, const double* tab, uint64_t at)
{
    if (!s.envelope_n) return 1.0;
    const uint32_t K = s.envelope_n - 1;
    const double num = static_cast<double>(at - s.start) * static_cast<double>(K);
    const double g = num / static_cast<double>(s.stop - s.start);
    uint32_t j = static_cast<uint32_t>(static_cast<int>(g));
    if (j > K - 1) j = K - 1;
    const double r = g - static_cast<double>(j);
    const double rise = tab[j + 1] - tab[j];
    const double part = rise * r;
    return tab[j] + part;
}

inline double kq_of(int kind, double charge, double mass, double dt)
{
    if (kind == FPIC_FORCE_ACCEL) return dt / kC;
    const double num = charge * dt, den = mass * kC;
    return num / den;
}

// the kernels' form of a checked, active request at `at`: envelope = the host's copy of the envelope table, taper[a] = where
// the kernels read the taper tables (device pointers in the library)
inline Rule rule_of(const fpic_force_spec& s, const double (&L)[3], double charge, double mass, double dt, uint64_t at, const double* envelope,
                    const double* const* taper)
{
    Rule r{};
    r.nwaves = s.nwaves;
    r.whole = 1;
    for (int a = 0; a < 3; ++a) {
        r.lo_f[a] = s.lo[a] / L[a];
        r.hi_f[a] = s.hi[a] / L[a];
        r.w[a] = r.hi_f[a] - r.lo_f[a];
        r.tk[a] = s.taper_n[a] ? s.taper_n[a] - 1 : 0;
        r.tab[a] = s.taper_n[a] ? taper[a] : nullptr;
        if (s.taper_n[a]) r.tapered = 1;
        if (!(r.lo_f[a] == 0.0 && r.hi_f[a] == 1.0)) r.whole = 0;
    }
    for (int k = 0; k < s.nwaves; ++k) {
        for (int a = 0; a < 3; ++a) {
            r.wave[k].amp[a] = s.wave[k].amp[a];
            r.wave[k].m[a] = static_cast<double>(s.wave[k].mode[a]);
        }
        r.wave[k].tfrac = tfrac_of(s.wave[k].nu, at);
        r.wave[k].phase = s.wave[k].phase;
    }
    r.scale = kq_of(s.kind, charge, mass, dt) * envelope_of(s, envelope, at);
    return r;
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style,
// ".property <- what is wrong").  nspecies: the species the handle has; L: the box in metres.
inline const char* check(const fpic_force_spec* p, int nspecies, const double (&L)[3])
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    const fpic_force_spec& s = *p;
    if (s.kind != FPIC_FORCE_FIELD && s.kind != FPIC_FORCE_ACCEL) return ".kind <- must be 0 (field) or 1 (accel)";
    if (s.species < 0 || s.species >= nspecies) return ".species <- no such species";
    if (s.nwaves < 1 || s.nwaves > FPIC_FORCE_MAX_WAVES) return ".nwaves <- must be 1 .. FPIC_FORCE_MAX_WAVES (4)";
    if (s.reserved_i32 != 0) return ".reserved <- must be zero";
    for (double z : s.reserved)
        if (!(z == 0)) return ".reserved <- must be zero";
    for (int k = 0; k < FPIC_FORCE_MAX_WAVES; ++k)
        if (s.wave[k].reserved != 0) return ".reserved <- must be zero";
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(s.lo[a]) || !std::isfinite(s.hi[a])) return ".lo, .hi <- must be finite";
        if (!(0 <= s.lo[a] && s.lo[a] < s.hi[a] && s.hi[a] <= L[a])) return ".lo, .hi <- the window must lie within 0 <= lo < hi <= L";
    }
    for (int k = 0; k < s.nwaves; ++k) {
        const fpic_force_wave& q = s.wave[k];
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(q.amp[a])) return ".amp <- must be finite";
            if (q.mode[a] > 32768 || q.mode[a] < -32768) return ".mode <- components must lie within +-2^15";
        }
        if (!std::isfinite(q.nu)) return ".nu <- must be finite";
        if (!std::isfinite(q.phase)) return ".phase <- must be finite";
    }
    auto nodes_bad = [](uint32_t n) { return n == 1 || n > FPIC_FORCE_TABLE_MAX; };
    for (int a = 0; a < 3; ++a) {
        if (nodes_bad(s.taper_n[a])) return ".taper_n <- a table has 2 .. FPIC_FORCE_TABLE_MAX nodes (0: none)";
        if (s.taper_n[a] && !s.taper[a]) return ".taper <- a table is null but its node count is not zero";
    }
    if (nodes_bad(s.envelope_n)) return ".envelope_n <- a table has 2 .. FPIC_FORCE_TABLE_MAX nodes (0: none)";
    if (s.envelope_n && !s.envelope) return ".envelope <- the table is null but its node count is not zero";
    if (s.start > s.stop) return ".start <- must not lie after stop";
    if (s.envelope_n && (s.stop == s.start || s.stop == FPIC_FORCE_FOREVER)) return ".stop <- an envelope table needs start < stop < FPIC_FORCE_FOREVER";
    for (int a = 0; a < 3; ++a)
        for (uint32_t k = 0; k < s.taper_n[a]; ++k)
            if (!std::isfinite(s.taper[a][k])) return ".taper <- the nodes must be finite";
    for (uint32_t k = 0; k < s.envelope_n; ++k)
        if (!std::isfinite(s.envelope[k])) return ".envelope <- the nodes must be finite";
    return nullptr;
}

// ---- the tallies on the host
// the double nearest to s 2^-80 (ties to even) of a 128-bit two's complement sum: from_fix of fes_diag_kernels.hpp
inline double fixed_to_double(uint64_t lo, uint64_t hi)
{
    using U = unsigned __int128;
    const U s = (static_cast<U>(hi) << 64) | lo;
    const bool neg = hi >> 63;
    const U m = neg ? ~s + 1 : s;
    const uint64_t top64 = static_cast<uint64_t>(m >> 64);
    double r;
    if (!top64) {
        r = static_cast<double>(static_cast<uint64_t>(m));
    } else {
        const int sh = 64 - __builtin_clzll(top64);
        const uint64_t top = static_cast<uint64_t>(m >> sh) | ((m & ((static_cast<U>(1) << sh) - 1)) != 0 ? 1u : 0u);
        r = std::ldexp(static_cast<double>(top), sh);
    }
    return (neg ? -r : r) * 0x1p-80;
}

// the device words of a request (kWords of them) -> the result but `applications`; mass, W: the species' and the box's
inline void result_of(const uint64_t* w, double mass, double W, fpic_force_result* out)
{
    const double ke = 0.5 * mass * W * kC * kC, pm = mass * W * kC;   // the scales of the energy diagnostics
    out->kicked = w[0];
    out->work_fixed[0] = w[1];
    out->work_fixed[1] = w[2];
    out->work = (w[9] & 1u) ? std::nan("") : ke * fixed_to_double(w[1], w[2]);
    for (int a = 0; a < 3; ++a) {
        out->impulse_fixed[a][0] = w[3 + 2 * a];
        out->impulse_fixed[a][1] = w[4 + 2 * a];
        out->impulse[a] = (w[9] >> (1 + a) & 1u) ? std::nan("") : pm * fixed_to_double(w[3 + 2 * a], w[4 + 2 * a]);
    }
}

// The words of several ranks added exactly: a 128-bit sum as four 32-bit limbs and every out-of-range bit as a word of its
// own, so that the shared rank-sum (which adds 64-bit words independently) loses no carry.  kSumWords words.
constexpr int kSumWords = 1 + 4 * 4 + 4;
inline void split_words(const uint64_t* w, uint64_t* s)
{
    s[0] = w[0];
    for (int q = 0; q < 4; ++q) {
        s[1 + 4 * q] = w[1 + 2 * q] & 0xFFFFFFFFull;
        s[2 + 4 * q] = w[1 + 2 * q] >> 32;
        s[3 + 4 * q] = w[2 + 2 * q] & 0xFFFFFFFFull;
        s[4 + 4 * q] = w[2 + 2 * q] >> 32;
    }
    for (int b = 0; b < 4; ++b) s[17 + b] = w[9] >> b & 1u;
}
inline void join_words(const uint64_t* s, uint64_t* w)
{
    using U = unsigned __int128;
    w[0] = s[0];
    for (int q = 0; q < 4; ++q) {
        const U v = static_cast<U>(s[1 + 4 * q]) + (static_cast<U>(s[2 + 4 * q]) << 32) + (static_cast<U>(s[3 + 4 * q]) << 64) + (static_cast<U>(s[4 + 4 * q]) << 96);
        w[1 + 2 * q] = static_cast<uint64_t>(v);
        w[2 + 2 * q] = static_cast<uint64_t>(v >> 64);
    }
    w[9] = 0;
    for (int b = 0; b < 4; ++b) w[9] |= s[17 + b] ? uint64_t(1) << b : 0;
}

} // namespace fesforce
#endif
