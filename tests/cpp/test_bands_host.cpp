// The host-side checks of the plan bands (rapidnet_amd/csrc/bands_host.hpp), without a GPU: the cap on a stage's width -- a tree of 4097
// nodes in one stage is refused here and never built on a device -- and the order of the levels with the caller's positions.
#include <cmath>
#include <iostream>
#include <limits>
#include <vector>

#include "bands_host.hpp"

static int g_failures = 0;
#define CHECK(c) do { if (!(c)) { std::cerr << "CHECK failed at line " << __LINE__ << ": " #c "\n"; g_failures++; } } while (0)

int main() {
    using namespace rn::bands;
    CHECK(MAX_WIDTH == 4096 && MAX_LEVELS == 16);
    {   // stage widths 1, 70, 4096: allowed; 4097: refused; one node per stage: allowed
        const std::vector<int> ok = {0, 1, 71, 71 + 4096}, wide = {0, 1, 71, 71 + 4097}, chain = {0, 1, 2, 3, 4};
        CHECK(widest_stage(ok.data(), 3) == 4096 && width_ok(ok.data(), 3));
        CHECK(widest_stage(wide.data(), 3) == 4097 && !width_ok(wide.data(), 3));
        CHECK(widest_stage(chain.data(), 4) == 1 && width_ok(chain.data(), 4));
        CHECK(!width_ok(chain.data(), 0));
    }
    double s[MAX_LEVELS];
    int slot[MAX_LEVELS];
    {
        const double q[5] = {0.95, 0.0, 1.0, 0.5, 0.05};
        CHECK(sort_levels(5, q, s, slot) == LEVELS_OK);
        const double want[5] = {0.0, 0.05, 0.5, 0.95, 1.0};
        const int pos[5] = {1, 4, 3, 0, 2};
        for (int i = 0; i < 5; i++) CHECK(s[i] == want[i] && slot[i] == pos[i]);
    }
    {   // equal levels keep the caller's order; every position appears once
        const double q[4] = {0.5, 0.2, 0.5, 0.2};
        CHECK(sort_levels(4, q, s, slot) == LEVELS_OK);
        CHECK(s[0] == 0.2 && s[1] == 0.2 && s[2] == 0.5 && s[3] == 0.5 && slot[0] == 1 && slot[1] == 3 && slot[2] == 0 && slot[3] == 2);
    }
    {
        std::vector<double> q(17, 0.5);
        CHECK(sort_levels(0, q.data(), s, slot) == LEVELS_COUNT && sort_levels(17, q.data(), s, slot) == LEVELS_COUNT);
        CHECK(sort_levels(16, q.data(), s, slot) == LEVELS_OK && sort_levels(1, q.data(), s, slot) == LEVELS_OK);
        for (double bad : {-1e-300, 1.0000000000000002, std::nan(""), std::numeric_limits<double>::infinity(), -0.5}) {
            q[3] = bad;
            CHECK(sort_levels(5, q.data(), s, slot) == LEVELS_VALUE);
        }
        q[3] = 0.0; q[4] = 1.0;
        CHECK(sort_levels(5, q.data(), s, slot) == LEVELS_OK);
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "bands host: all checks passed\n";
    return 0;
}
