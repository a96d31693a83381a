// fes_inject_core.hpp — the rule of the particle sources of a CART3D handle (fpic_inject, fpic_reserve; the kernels are
// fes_inject_kernels.hpp, the orchestration fes_inject.inc.hpp): the sequence numbers of an application, the state of
// sequence number j under both kinds, the checks of a request, and the totals' conversion to the result.  Plain C++ that
// compiles for the host and the device, shared with a host test (tests/native/inject_core_test.cpp, g++).  The state of a
// VOLUME particle is the loader's (fesload::base_of, displace, velocity_of), the embedded request's checks are the loader's
// (fesload::check), the result's scales are the sinks' (fesrem::result_of): nothing of them is restated here.
#ifndef FES_INJECT_CORE_HPP
#define FES_INJECT_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_load_core.hpp"
#include "fes_remove_core.hpp"

namespace fesinj {

constexpr int kRowWords = fesrem::kRowWords;   // a row of totals: the energy diagnostics' partial row, as the sinks'
constexpr double kSpeedOfLight = 2.998e8;      // the push's (fes_host_push.inc.hpp)
constexpr uint64_t kIdEnd = 0xFFFFFFFFull;    // one past the largest sequence number and id a source gives: the loader's bound on 32-bit ids (fesload::check)
constexpr uint64_t kCapacityEnd = 0xFFFFFFFFull - 4096;   // fpic_add_species's bound on a species' particles

// a request as the kernel reads it: the loader's form, and for FLUX the plane and the step in box fractions
struct Rule {
    fesload::Rule r;          // FLUX: lo_f[axis] = 0, w_f[axis] = 1 — base_of's p[axis] is then the time fraction itself
    int kind, axis, t1, t2;   // FLUX: the normal axis and the two others, ascending
    double side;              // +1 or -1
    double plane_f, step_f;   // plane / L_axis; dt c / L_axis
};

// the first sequence number of application k (k counts from the epoch on); false: first + count would pass 2^32 - 1, the
// bound fesload::check holds application 0 to
inline bool first_of(const fpic_inject_spec& s, uint64_t k, uint64_t* first)
{
    const unsigned __int128 at = static_cast<unsigned __int128>(s.load.first) + (static_cast<unsigned __int128>(s.epoch) + k) * s.load.count;
    if (at + s.load.count > kIdEnd) return false;
    *first = static_cast<uint64_t>(at);
    return true;
}

// whether `count` more particles fit a species of n particles, capacity cap and id span `span`
inline bool fits(uint64_t n, uint64_t cap, uint64_t span, uint64_t count) { return count <= cap - (n < cap ? n : cap) && span <= kIdEnd && count <= kIdEnd - span; }

// the state of sequence number j before the cast to the handle's precision (and the wrap of the position)
FES_HIST_HD void state_of(const Rule& q, uint32_t j, double (&p)[3], double (&v)[3])
{
    double theta;
    fesload::base_of(q.r, j, p, theta);
    if (q.kind == FPIC_INJECT_VOLUME) {
        fesload::velocity_of(q.r, j, theta, v);
        fesload::displace(q.r, theta, p);
        return;
    }
    uint32_t w[4];
    fesload::philox(j, q.r.stream, 1u, fesload::kTag, q.r.seed_lo, q.r.seed_hi, w);
    double n[3];
    fesload::normals_from(w, n);
    const double u3 = (static_cast<double>(w[2]) + 0.5) * fesload::kTwoM32;
    const double s = sqrt(-2.0 * log(u3));                 // the radius of normals_from's n[2]: a Rayleigh deviate
    // (every index below is a constant after unrolling: the axis picks by comparison, so that a kernel keeps p and v in registers)
    double vn = 0, ft = 0;
    for (int a = 0; a < 3; ++a) {
        const bool normal = a == q.axis;
        const double dev = normal ? s : (a == q.t1 ? n[0] : n[1]);
        const double th = q.r.vth[a] * dev;
        const double tangential = q.r.drift[a] + th;
        v[a] = normal ? q.side * th : tangential;
        vn = normal ? v[a] : vn;
        ft = normal ? p[a] : ft;                           // (0 + f 1: the fraction, exactly)
    }
    const double d = vn * q.step_f;
    const double e = d * ft;
    const double pn = q.plane_f + e;
    for (int a = 0; a < 3; ++a) p[a] = a == q.axis ? pn : p[a];
}

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style).
inline const char* check(const fpic_inject_spec* p, int nspecies, const double (&L)[3])
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    const fpic_load_spec& l = p->load;
    if ((l.flags & (FPIC_LOAD_POS | FPIC_LOAD_VEL)) != (FPIC_LOAD_POS | FPIC_LOAD_VEL)) return ".flags <- a source needs FPIC_LOAD_POS and FPIC_LOAD_VEL both";
    if (l.flags & FPIC_LOAD_APPEND) return ".flags <- FPIC_LOAD_APPEND is for a rank of a decomposition: a source always appends";
    if (l.count == ~0ull) return ".count <- a source has no end of the species to run to: give the particles per application";
    // the rest of the embedded request: the loader's own checks, in the form that takes the indices as 32-bit ids
    if (const char* why = fesload::check(l, nspecies, ~0ull, L, true)) return why;
    if (p->kind != FPIC_INJECT_VOLUME && p->kind != FPIC_INJECT_FLUX) return ".kind <- must be FPIC_INJECT_VOLUME (0) or FPIC_INJECT_FLUX (1)";
    if (p->reserved_i != 0) return ".reserved <- must be zero";
    for (int k = 0; k < 4; ++k)
        if (!(p->reserved[k] == 0)) return ".reserved <- must be zero";
    if (p->kind == FPIC_INJECT_VOLUME) {
        if (p->axis != 0 || p->side != 0 || !(p->plane == 0)) return ".axis <- axis, side and plane belong to FPIC_INJECT_FLUX: zero for a volume source";
        return nullptr;
    }
    if (p->axis < 0 || p->axis > 2) return ".axis <- must be 0, 1 or 2";
    if (p->side != 1 && p->side != -1) return ".side <- must be +1 or -1";
    if (!std::isfinite(p->plane) || !(p->plane >= 0) || !(p->plane <= L[p->axis])) return ".plane <- must lie within [0, the box length along the axis]";
    if (l.drift[p->axis] != 0) return ".drift <- a flux source has no drift along its axis (a drifting flux is not the half-Maxwellian this draws)";
    if (l.flags & FPIC_LOAD_PAIRED) return ".flags <- FPIC_LOAD_PAIRED with a flux source: the negated partner would fly back through the plane";
    for (int a = 0; a < 3; ++a) {
        if (l.xamp[a] != 0) return ".xamp <- a flux source takes no perturbation";
        if (l.vamp[a] != 0) return ".vamp <- a flux source takes no perturbation";
        if (l.mode[a] != 0) return ".mode <- a flux source takes no perturbation";
    }
    return nullptr;
}

inline const char* check_capacity(uint64_t capacity)
{
    if (capacity >= kCapacityEnd) return ".capacity <- at most 2^32 particles per species and device: the ids are 32-bit";
    return nullptr;
}

// the kernel's form of a checked request whose application starts at sequence number `first`; dt: the handle's step
inline Rule rule_of(const fpic_inject_spec& s, uint64_t first, const double (&L)[3], double dt)
{
    Rule q{};
    fpic_load_spec l = s.load;
    l.first = first;
    q.r = fesload::rule_of(l, ~0ull, L);
    q.kind = s.kind;
    if (s.kind == FPIC_INJECT_FLUX) {
        q.axis = s.axis;
        q.t1 = s.axis == 0 ? 1 : 0;
        q.t2 = s.axis == 2 ? 1 : 2;
        q.side = static_cast<double>(s.side);
        q.plane_f = s.plane / L[s.axis];
        const double step = dt * kSpeedOfLight;
        q.step_f = step / L[s.axis];
        q.r.lo_f[s.axis] = 0.0;
        q.r.w_f[s.axis] = 1.0;
    }
    return q;
}

// a row of totals -> the result but `applications`: the sinks' conversion (the same scales), what the species GAINED
inline void result_of(const uint64_t* w, double mass, double charge, double W, fpic_inject_result* out)
{
    fpic_remove_result r{};
    fesrem::result_of(w, mass, charge, W, &r);
    out->injected = r.removed;
    for (int k = 0; k < 2; ++k) out->energy_fixed[k] = r.energy_fixed[k];
    out->energy = r.energy;
    for (int a = 0; a < 3; ++a) {
        out->momentum_fixed[a][0] = r.momentum_fixed[a][0];
        out->momentum_fixed[a][1] = r.momentum_fixed[a][1];
        out->momentum[a] = r.momentum[a];
    }
    out->charge = r.charge;
}

} // namespace fesinj
#endif
