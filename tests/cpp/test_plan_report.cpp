// The plan report through the host classes (rapidnet.h, rn_plan_report; Engine::evaluatePlan, SmpcController::getPlanReport / writePlanReport).
//   test_plan_report <dir>       two controllers built from <dir>/controllerConfig.json run the same control step into <dir>/plain.json and
//                                <dir>/report.json; the second also writes its plan report.  Checked: before a solve the report is refused;
//                                the tables have the tree's shape and are those of the C-ABI route, bit for bit; the first report allocates
//                                outside the window of controlAction's leak check, so the next control step still returns 1; a second
//                                report returns the same bits.  tests/test_host_plan_report.py reads the two files: the control output is
//                                unchanged byte for byte and the "planReport" entry is a JSON object holding the printed figures.
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

int main(int argc, char **argv) {
    if (argc < 2) { std::cerr << "usage: test_plan_report <dir>\n"; return 2; }
    const string dir = argv[1];
    try {
        SmpcController a(dir + "/controllerConfig.json"), b(dir + "/controllerConfig.json");
        for (SmpcController *s : {&a, &b}) { start(*s); s->initialiseSmpcController(); }
        bool refused = false;
        try { b.getPlanReport(); } catch (const std::runtime_error &) { refused = true; }
        CHECK(refused);                                          // no sweep yet: RN_E_STATE through the host class
        {
            double row[RN_PLAN_COLS];
            CHECK(rn_plan_report(b.getEngine()->getContext(), 1, row) == RN_E_ARG || rn_plan_report(b.getEngine()->getContext(), 1, row) == RN_E_STATE);
            CHECK(rn_plan_report(nullptr, 1, row) == RN_E_ARG);
        }
        std::fstream fa(dir + "/plain.json", std::ios::out | std::ios::trunc), fb(dir + "/report.json", std::ios::out | std::ios::trunc);
        CHECK(a.controlAction(fa) == 1 && b.controlAction(fb) == 1);
        CHECK(b.writePlanReport(fb) == 1);
        Engine::PlanReport r = b.getPlanReport();               // (a copy: the second report)
        ScenarioTree *t = b.getScenarioTree();
        CHECK(r.stages == (size_t)t->getPredHorizon() && r.scenarios == (size_t)t->getNumScenarios() && r.scenarios == b.getEngine()->getNumLocalScenarios());
        CHECK(r.perStage.size() == r.stages * RN_PLAN_COLS && r.perScenario.size() == r.scenarios * RN_PLAN_COLS && r.leafNode.size() == r.scenarios);
        // the C-ABI route on the same context: the same bits
        std::vector<double> st(r.perStage.size()), sc(r.perScenario.size());
        std::vector<int> ln(r.scenarios);
        rn_ctx *x = b.getEngine()->getContext();
        CHECK(rn_plan_report(x, r.stages, st.data()) == RN_OK && rn_plan_report_scenarios(x, r.scenarios, sc.data(), ln.data()) == RN_OK);
        CHECK(std::memcmp(st.data(), r.perStage.data(), st.size() * sizeof(double)) == 0);
        CHECK(std::memcmp(sc.data(), r.perScenario.data(), sc.size() * sizeof(double)) == 0 && ln == r.leafNode);
        CHECK(rn_plan_report(x, r.stages + 1, st.data()) == RN_E_ARG && rn_plan_report(x, r.stages, nullptr) == RN_E_ARG);
        CHECK(rn_plan_report_scenarios(x, r.scenarios + 1, sc.data(), nullptr) == RN_E_ARG);
        // the rows are those of the last stage, in ascending order, and the stored volume is positive at every stage
        const uint_t nodes = t->getNumNodes();
        for (size_t l = 0; l < r.scenarios; l++) CHECK(r.leafNode[l] == (int)(nodes - r.scenarios + l));
        for (size_t k = 0; k < r.stages; k++) CHECK(r.stage(k, RN_PLAN_STORED) > 0 && r.stage(k, RN_PLAN_SMOOTH) >= 0 && r.stage(k, RN_PLAN_SHORT_MAX) >= 0);
        // the stored volume of the root is that of x_0, which the stage-0 row holds with p_0 = 1
        std::vector<real_t> x0(b.getSmpcConfiguration()->getNX());
        b.getEngine()->getBufferRange(RN_BUF_X, 0, x0.size(), x0.data());
        real_t sum = 0;
        for (real_t v : x0) sum += v;
        CHECK(std::fabs(r.stage(0, RN_PLAN_STORED) - sum) <= 1e-12 * std::fabs(sum));
        std::cout << std::setprecision(17) << "stage0: econ " << r.stage(0, RN_PLAN_ECON) << " stored " << r.stage(0, RN_PLAN_STORED) << "\n";
        std::cout << "shape: " << r.stages << " stages, " << r.scenarios << " scenarios\n";
        // the report's buffers were allocated outside the leak check's window: the next control steps pass it
        real_t u[4096];
        CHECK(b.getSmpcConfiguration()->getNU() <= 4096);
        CHECK(b.controlAction(u) == 1);
        CHECK(b.controlAction(fb) == 1);
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "plan report: all checks passed\n";
    return 0;
}
