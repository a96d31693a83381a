// fes_remove_core.hpp — the rule of the absorbing particle sinks of a CART3D handle (fpic_remove, fpic_renumber; the passes
// are fes_remove_kernels.hpp, the orchestration fes_remove.inc.hpp): the request as the selection's request, which particles
// leave, the checks of a request, and the totals' conversion to the result.  Plain C++ that compiles for the host and the
// device, shared with a host test (tests/native/remove_core_test.cpp, g++).  The predicate is the selection's
// (fessel::inside, id_passes, check; the axis values feshist::v2_of): nothing of it is restated here.
#ifndef FES_REMOVE_CORE_HPP
#define FES_REMOVE_CORE_HPP
#include <cmath>
#include <cstdint>

#include "fes_force_core.hpp"
#include "fes_select_core.hpp"

namespace fesrem {

// a row of totals on the device, 64-bit words, in the layout of the energy diagnostics' partial row (fes::kDiagWords):
// removed | sum |v|^2 (lo, hi) | sum vx, vy, vz (lo, hi) | (the diagnostics' maximum: not read) | the out-of-range bits
// (bit 0: |v|^2, bits 1..3: vx, vy, vz)
constexpr int kRowWords = 11;
constexpr uint32_t kFlags = FPIC_REMOVE_OUTSIDE;

// the predicate of a request as the selection's request
inline fpic_select_spec select_of(const fpic_remove_spec& s)
{
    fpic_select_spec q{};
    q.species = s.species;
    q.nterms = s.nterms;
    for (int t = 0; t < 8; ++t) {
        q.axis[t] = s.axis[t];
        q.lo[t] = s.lo[t];
        q.hi[t] = s.hi[t];
    }
    q.id_mod = s.id_mod;
    q.id_rem = s.id_rem;
    for (int k = 0; k < 4; ++k) q.reserved[k] = s.reserved[k];
    return q;
}

// whether a live particle leaves: in_terms = it matches every term, id_ok = it passes the id rule
FES_HIST_HD bool removes(bool in_terms, bool id_ok, uint32_t flags) { return id_ok && ((flags & FPIC_REMOVE_OUTSIDE) ? !in_terms : in_terms); }

// a checked request that can remove nothing whatever the particles are (no term is never missed): nothing is launched
inline bool never(const fpic_remove_spec& s) { return (s.flags & FPIC_REMOVE_OUTSIDE) && s.nterms == 0; }

// A request's checks, in the order the messages name them: nullptr if it is good, else the message (house style).
inline const char* check(const fpic_remove_spec* p, int nspecies)
{
    if (!p) return ".spec <- Non-optional property is undefined!";
    if (const char* why = fessel::check(select_of(*p), nspecies, 0, false, FPIC_F32)) return why;
    if (p->flags & ~kFlags) return ".flags <- unknown flag (FPIC_REMOVE_OUTSIDE is the only one)";
    if (p->reserved_u != 0) return ".reserved <- must be zero";
    return nullptr;
}

// a row of totals -> the result but `applications` and `scanned`; mass, charge: the species'; W: the box's macro-weight
inline void result_of(const uint64_t* w, double mass, double charge, double W, fpic_remove_result* out)
{
    const double ke = 0.5 * mass * W * fesforce::kC * fesforce::kC, pm = mass * W * fesforce::kC;   // the scales of the energy diagnostics
    out->removed = w[0];
    out->energy_fixed[0] = w[1];
    out->energy_fixed[1] = w[2];
    out->energy = (w[10] & 1u) ? std::nan("") : ke * fesforce::fixed_to_double(w[1], w[2]);
    for (int a = 0; a < 3; ++a) {
        out->momentum_fixed[a][0] = w[3 + 2 * a];
        out->momentum_fixed[a][1] = w[4 + 2 * a];
        out->momentum[a] = (w[10] >> (1 + a) & 1u) ? std::nan("") : pm * fesforce::fixed_to_double(w[3 + 2 * a], w[4 + 2 * a]);
    }
    const double q = static_cast<double>(w[0]) * charge;
    out->charge = q * W;
}

} // namespace fesrem
#endif
