// bands_host.hpp -- the host-side checks of the plan bands (rn_plan_quantiles, rn_plan_paths; plan_bands.inc): the cap on a stage's width and
// the order of the levels.  Host-only code, tested without a GPU (tests/cpp/test_bands_host.cpp).
#pragma once
#include <cstddef>

namespace rn {
namespace bands {

constexpr int MAX_WIDTH = 4096;    // nodes of one stage: the sort's (value, index) keys of a stage fill 48 KB of LDS (k_plan_bands, k_plan.hpp)
constexpr int MAX_LEVELS = 16;     // levels of one call: they travel in the kernel's argument struct

// the largest number of nodes a stage holds; cum = nodesPerStageCumul [N + 1]
inline int widest_stage(const int *cum, int N) {
    int w = 0;
    for (int k = 0; k < N; k++) if (cum[k + 1] - cum[k] > w) w = cum[k + 1] - cum[k];
    return w;
}
inline bool width_ok(const int *cum, int N) { return N >= 1 && N <= MAX_WIDTH && widest_stage(cum, N) <= MAX_WIDTH; }

enum { LEVELS_OK = 0, LEVELS_COUNT = 1, LEVELS_VALUE = 2 };
// The levels in ascending order (equal levels keep the caller's order) and the caller's position of each: the kernel picks them in one walk
// and writes result l to slot[l].  LEVELS_COUNT: nq outside [1, MAX_LEVELS]; LEVELS_VALUE: a level outside [0, 1] or NaN.
inline int sort_levels(size_t nq, const double *q, double *sorted, int *slot) {
    if (nq < 1 || nq > (size_t)MAX_LEVELS) return LEVELS_COUNT;
    for (size_t i = 0; i < nq; i++) if (!(q[i] >= 0.0 && q[i] <= 1.0)) return LEVELS_VALUE;
    for (size_t i = 0; i < nq; i++) {      // insertion sort: at most 16 entries
        size_t j = i;
        while (j > 0 && sorted[j - 1] > q[i]) { sorted[j] = sorted[j - 1]; slot[j] = slot[j - 1]; j--; }
        sorted[j] = q[i]; slot[j] = (int)i;
    }
    return LEVELS_OK;
}

}  // namespace bands
}  // namespace rn
