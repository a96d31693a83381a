// fes_ops_core.hpp — what the registered operators of a CART3D handle share before anything touches the device (the
// orchestration is fes_ops.inc.hpp): the families in the order of the sub-step hook, the two checks of a registration and of
// an index, and the families' messages.  Plain C++ that compiles for the host, shared with a host test
// (tests/native/ops_core_test.cpp, g++).  A family's own checks of a request stay in its fes_*_core.hpp.
#ifndef FES_OPS_CORE_HPP
#define FES_OPS_CORE_HPP
#include "../../include/fusionpic.h"

namespace fesops {

// the families, in the order in which the hook runs them (fes_api.hip, diag_after_substep)
enum Family { kForce, kCollide, kGas, kPair, kFusion, kFspec, kRemove, kInject, kFamilies };

// what a family says when it is full and when an index names nothing, and how many it holds
struct Messages {
    int max;
    const char* full;
    const char* index;
};
inline const Messages& messages(int family)
{
    static const Messages table[kFamilies] = {
        { FPIC_FORCE_MAX_OPS, ".spec <- FPIC_FORCE_MAX_OPS (8) requests are registered already", ".index <- no such registered request" },
        { FPIC_COLLIDE_MAX_OPS, ".spec <- FPIC_COLLIDE_MAX_OPS (8) operators are registered already", ".index <- no such registered operator" },
        { FPIC_GAS_MAX_OPS, ".spec <- FPIC_GAS_MAX_OPS (8) operators are registered already", ".index <- no such registered operator" },
        { FPIC_PAIR_MAX_OPS, ".spec <- FPIC_PAIR_MAX_OPS (8) operators are registered already", ".index <- no such registered operator" },
        { FPIC_FUSION_MAX_OPS, ".spec <- FPIC_FUSION_MAX_OPS (4) operators are registered already", ".index <- no such registered operator" },
        { FPIC_FUSION_SPECTRUM_MAX_OPS, ".spec <- FPIC_FUSION_SPECTRUM_MAX_OPS (4) operators are registered already", ".index <- no such registered operator" },
        { FPIC_REMOVE_MAX_OPS, ".spec <- FPIC_REMOVE_MAX_OPS (8) operators are registered already", ".index <- no such registered operator" },
        { FPIC_INJECT_MAX_OPS, ".spec <- FPIC_INJECT_MAX_OPS (8) sources are registered already", ".index <- no such registered source" },
    };
    return table[family];
}

// a registration with the period `every` (a family without one passes 1): `registered` are held already, `max` fit
inline const char* check_register(int every, int registered, int max, const char* message)
{
    if (every < 1) return ".every <- must be at least 1";
    if (registered >= max) return message;
    return nullptr;
}
inline const char* check_index(int index, int registered, const char* message)
{
    if (index < 0 || index >= registered) return message;
    return nullptr;
}

} // namespace fesops
#endif
