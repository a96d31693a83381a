// Host test of fusion-sim_amd/csrc/fes_ops_core.hpp (what the registered operators of the box share): per family the
// registration and index checks by their whole messages, the boundaries of what they accept, and that the table's order is the
// hook's.  Built with g++ by tests/test_ops_host.py; prints "ok" and exits 0, or names the first failed check and exits 1.
#include <cstdio>
#include <cstring>

#include "../../fusion-sim_amd/csrc/fes_ops_core.hpp"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static bool says(const char* msg, const char* want) { return msg && std::strcmp(msg, want) == 0; }

struct Want {
    int family, max;
    const char* full;
    const char* index;
};
// the strings as the callers have always seen them: written out here, not taken from the table under test
static const Want kWant[] = {
    { fesops::kForce, 8, ".spec <- FPIC_FORCE_MAX_OPS (8) requests are registered already", ".index <- no such registered request" },
    { fesops::kCollide, 8, ".spec <- FPIC_COLLIDE_MAX_OPS (8) operators are registered already", ".index <- no such registered operator" },
    { fesops::kGas, 8, ".spec <- FPIC_GAS_MAX_OPS (8) operators are registered already", ".index <- no such registered operator" },
    { fesops::kPair, 8, ".spec <- FPIC_PAIR_MAX_OPS (8) operators are registered already", ".index <- no such registered operator" },
    { fesops::kFusion, 4, ".spec <- FPIC_FUSION_MAX_OPS (4) operators are registered already", ".index <- no such registered operator" },
    { fesops::kFspec, 4, ".spec <- FPIC_FUSION_SPECTRUM_MAX_OPS (4) operators are registered already", ".index <- no such registered operator" },
    { fesops::kRemove, 8, ".spec <- FPIC_REMOVE_MAX_OPS (8) operators are registered already", ".index <- no such registered operator" },
    { fesops::kInject, 8, ".spec <- FPIC_INJECT_MAX_OPS (8) sources are registered already", ".index <- no such registered source" },
};

static void families()
{
    CHECK(fesops::kFamilies == 8 && sizeof kWant / sizeof kWant[0] == 8);
    // the hook's order: the forces first, the background operators, the binary ones, the tallies, the sinks, the sources last
    CHECK(fesops::kForce == 0 && fesops::kCollide == 1 && fesops::kGas == 2 && fesops::kPair == 3 && fesops::kFusion == 4 && fesops::kFspec == 5 &&
          fesops::kRemove == 6 && fesops::kInject == 7);
    CHECK(FPIC_FORCE_MAX_OPS == 8 && FPIC_COLLIDE_MAX_OPS == 8 && FPIC_GAS_MAX_OPS == 8 && FPIC_PAIR_MAX_OPS == 8 && FPIC_FUSION_MAX_OPS == 4 &&
          FPIC_FUSION_SPECTRUM_MAX_OPS == 4 && FPIC_REMOVE_MAX_OPS == 8 && FPIC_INJECT_MAX_OPS == 8);
}

static void checks()
{
    const char* every = ".every <- must be at least 1";
    for (const Want& w : kWant) {
        const fesops::Messages& m = fesops::messages(w.family);
        CHECK(m.max == w.max && says(m.full, w.full) && says(m.index, w.index));
        // a registration: any period from 1 on while there is room; the period is looked at first
        CHECK(fesops::check_register(1, 0, m.max, m.full) == nullptr && fesops::check_register(1000000, m.max - 1, m.max, m.full) == nullptr);
        CHECK(fesops::check_register(2147483647, 0, m.max, m.full) == nullptr);
        CHECK(says(fesops::check_register(0, 0, m.max, m.full), every) && says(fesops::check_register(-3, 0, m.max, m.full), every));
        CHECK(says(fesops::check_register(0, m.max, m.max, m.full), every));
        CHECK(says(fesops::check_register(1, m.max, m.max, m.full), w.full) && says(fesops::check_register(1, m.max + 1, m.max, m.full), w.full));
        // an index: 0 .. registered - 1
        CHECK(fesops::check_index(0, 1, m.index) == nullptr && fesops::check_index(m.max - 1, m.max, m.index) == nullptr);
        CHECK(says(fesops::check_index(0, 0, m.index), w.index) && says(fesops::check_index(-1, 3, m.index), w.index) && says(fesops::check_index(3, 3, m.index), w.index) &&
              says(fesops::check_index(1, 1, m.index), w.index) && says(fesops::check_index(m.max, m.max, m.index), w.index));
    }
}

int main()
{
    families();
    checks();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
