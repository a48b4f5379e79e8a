// The plan bands through the host classes (rapidnet.h, rn_plan_quantiles / rn_plan_paths; Engine::planQuantiles / planPaths,
// SmpcController::getPlanBands / writePlanBands).
//   test_plan_bands <dir>        two controllers built from <dir>/controllerConfig.json run the same control step into <dir>/plain.json and
//                                <dir>/bands.json; the second also writes its plan bands.  Checked: before a solve the bands are refused; the
//                                tables have the tree's shape and are those of the C-ABI route, bit for bit; the levels are ordered within
//                                every (stage, component) and bracketed by q = 0 and q = 1; every path starts at the root's row; the first
//                                call allocates outside the window of controlAction's leak check, so the next control step still returns 1.
//                                tests/test_host_plan_bands.py reads the two files: the control output is unchanged byte for byte and the
//                                "planBands" entry is a JSON object holding the printed figures.
#include <cmath>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <vector>

#include "../../include/rapidnet.h"
#include "../../rapidnet_amd/csrc/host/SmpcController.hpp"

static int g_failures = 0;
#define CHECK(c) do { if (!(c)) { std::cerr << "CHECK failed at line " << __LINE__ << ": " #c "\n"; g_failures++; } } while (0)

static void start(SmpcController &c) {
    c.getForecaster()->predictDemand(0);
    c.getForecaster()->predictPrices(0);
}
static bool same(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

int main(int argc, char **argv) {
    if (argc < 2) { std::cerr << "usage: test_plan_bands <dir>\n"; return 2; }
    const string dir = argv[1];
    try {
        SmpcController a(dir + "/controllerConfig.json"), b(dir + "/controllerConfig.json");
        for (SmpcController *s : {&a, &b}) { start(*s); s->initialiseSmpcController(); }
        const std::vector<real_t> levels = {0.95, 0.0, 0.5, 1.0, 0.05};      // the caller's order is kept
        bool refused = false;
        try { b.getPlanBands(levels); } catch (const std::runtime_error &) { refused = true; }
        CHECK(refused);                                          // no sweep yet: RN_E_STATE through the host class
        std::fstream fa(dir + "/plain.json", std::ios::out | std::ios::trunc), fb(dir + "/bands.json", std::ios::out | std::ios::trunc);
        CHECK(a.controlAction(fa) == 1 && b.controlAction(fb) == 1);
        CHECK(b.writePlanBands(fb) == 1);
        const SmpcController::PlanBands r = b.getPlanBands(levels);      // (a copy)
        ScenarioTree *t = b.getScenarioTree();
        const size_t N = r.stages, L = r.scenarios, nx = r.nx, nu = r.nu, nq = levels.size();
        CHECK(N == (size_t)t->getPredHorizon() && L == (size_t)t->getNumScenarios() && nx == b.getSmpcConfiguration()->getNX() && nu == b.getSmpcConfiguration()->getNU());
        CHECK(r.xQuantiles.size() == N * nx * nq && r.uQuantiles.size() == N * nu * nq && r.xPaths.size() == L * N * nx && r.uPaths.size() == L * N * nu && r.leafNode.size() == L);
        // the C-ABI route on the same context: the same bits, twice
        rn_ctx *x = b.getEngine()->getContext();
        std::vector<double> qx(r.xQuantiles.size()), qu(r.uQuantiles.size()), px(r.xPaths.size()), pu(r.uPaths.size());
        std::vector<int> ln(L);
        CHECK(rn_plan_quantiles(x, RN_BAND_X, nq, levels.data(), N, qx.data()) == RN_OK && rn_plan_quantiles(x, RN_BAND_U, nq, levels.data(), N, qu.data()) == RN_OK);
        CHECK(rn_plan_paths(x, RN_BAND_X, L, px.data(), ln.data()) == RN_OK && rn_plan_paths(x, RN_BAND_U, L, pu.data(), nullptr) == RN_OK);
        CHECK(same(qx, r.xQuantiles) && same(qu, r.uQuantiles) && same(px, r.xPaths) && same(pu, r.uPaths) && ln == r.leafNode);
        CHECK(same(b.getPlanBands(levels).xQuantiles, r.xQuantiles) && same(b.getPlanBands(levels).uPaths, r.uPaths));
        CHECK(rn_plan_quantiles(x, RN_BAND_X, nq, levels.data(), N + 1, qx.data()) == RN_E_ARG && rn_plan_quantiles(x, 2, nq, levels.data(), N, qx.data()) == RN_E_ARG);
        CHECK(rn_plan_quantiles(x, RN_BAND_X, 0, levels.data(), N, qx.data()) == RN_E_ARG && rn_plan_paths(x, RN_BAND_X, L + 1, px.data(), nullptr) == RN_E_ARG);
        CHECK(rn_plan_quantiles(nullptr, RN_BAND_X, nq, levels.data(), N, qx.data()) == RN_E_ARG);
        // levels 0.95, 0, 0.5, 1, 0.05 at positions 0 .. 4: min <= 5 % <= median <= 95 % <= max in every (stage, component)
        for (size_t i = 0; i < N * nx; i++) {
            const double *v = &r.xQuantiles[i * nq];
            CHECK(v[1] <= v[4] && v[4] <= v[2] && v[2] <= v[0] && v[0] <= v[3]);
        }
        // the rows are those of the last stage in ascending order; every path starts at the root's row, which every quantile of stage 0 equals
        const uint_t nodes = t->getNumNodes();
        std::vector<real_t> x0(nx);
        b.getEngine()->getBufferRange(RN_BUF_X, 0, nx, x0.data());
        for (size_t l = 0; l < L; l++) {
            CHECK(r.leafNode[l] == (int)(nodes - L + l));
            CHECK(std::memcmp(&r.xPaths[l * N * nx], x0.data(), nx * sizeof(double)) == 0);
        }
        for (size_t c = 0; c < nx; c++) for (size_t l = 0; l < nq; l++) CHECK(r.xQuantiles[c * nq + l] == x0[c]);
        // a path's last row is the leaf's own
        std::vector<real_t> xl(nx);
        b.getEngine()->getBufferRange(RN_BUF_X, (size_t)(nodes - 1) * nx, nx, xl.data());
        CHECK(std::memcmp(&r.xPaths[((L - 1) * N + (N - 1)) * nx], xl.data(), nx * sizeof(double)) == 0);
        std::cout << std::setprecision(17) << "median: x " << r.xQuantiles[((N - 1) * nx) * nq + 2] << " u " << r.uQuantiles[((N - 1) * nu) * nq + 2] << "\n";
        std::cout << "shape: " << N << " stages, " << L << " scenarios, " << nx << " nx, " << nu << " nu\n";
        // the tables were allocated outside the leak check's window: the next control steps pass it
        real_t u[4096];
        CHECK(nu <= 4096);
        CHECK(b.controlAction(u) == 1);
        CHECK(b.controlAction(fb) == 1);
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "plan bands: all checks passed\n";
    return 0;
}
