// The "stopTolerance" / "stopCheckEvery" keys of the controller configuration through the host classes (rapidnet.h, rn_set_stop_tolerance).
//   test_stop_tolerance <dir> parse     no GPU: loads <dir>/controllerConfig.json (no keys) and <dir>/controllerTolConfig.json (both keys) and
//                                       prints what SmpcConfiguration read
//   test_stop_tolerance <dir>           a controller built from the file with the keys stops its control step early, reports the count
//                                       (SmpcController::getIterationsRun) and gives bit for bit the control of a controller built from the plain
//                                       file and told the same through Engine::setStopTolerance; the plain file runs maxIterations
#include <cstring>
#include <iostream>
#include <vector>

#include "../../include/rapidnet.h"
#include "../../rapidnet_amd/csrc/host/SmpcController.hpp"

static int g_failures = 0;
#define CHECK(c) do { if (!(c)) { std::cerr << "CHECK failed at line " << __LINE__ << ": " #c "\n"; g_failures++; } } while (0)

static void start(SmpcController &c) {
    c.getForecaster()->predictDemand(1);
    c.getForecaster()->predictPrices(1);
}

int main(int argc, char **argv) {
    if (argc < 2) { std::cerr << "usage: test_stop_tolerance <dir> [parse]\n"; return 2; }
    const string dir = argv[1];
    try {
        if (argc > 2 && string(argv[2]) == "parse") {
            SmpcConfiguration plain(dir + "/controllerConfig.json"), tol(dir + "/controllerTolConfig.json");
            std::cout << "plain: stopTolerance " << plain.getStopTolerance() << " stopCheckEvery " << plain.getStopCheckEvery() << "\n";
            std::cout << "keys: stopTolerance " << tol.getStopTolerance() << " stopCheckEvery " << tol.getStopCheckEvery() << "\n";
            return 0;
        }
        SmpcController t(dir + "/controllerTolConfig.json"), n(dir + "/controllerConfig.json"), c(dir + "/controllerConfig.json");
        const real_t tol = t.getSmpcConfiguration()->getStopTolerance();
        const int every = (int)t.getSmpcConfiguration()->getStopCheckEvery();
        const uint_t maxIt = t.getSmpcConfiguration()->getMaxIterations(), nu = t.getSmpcConfiguration()->getNU();
        CHECK(tol > 0 && every > 0 && n.getSmpcConfiguration()->getStopTolerance() == 0);
        int e = -1;
        CHECK(t.getEngine()->getStopTolerance(&e) == tol && e == every);
        CHECK(n.getEngine()->getStopTolerance(&e) == 0 && e == 20);
        c.getEngine()->setStopTolerance(tol, every);
        CHECK(rn_set_stop_tolerance(c.getEngine()->getContext(), -1.0, 0) == RN_E_ARG);
        CHECK(c.getEngine()->getStopTolerance(&e) == tol && e == every);
        for (SmpcController *s : {&t, &n, &c}) { start(*s); s->initialiseSmpcController(); }
        std::vector<real_t> ut(nu), un(nu), uc(nu);
        CHECK(t.controlAction(ut.data()) == 1 && n.controlAction(un.data()) == 1 && c.controlAction(uc.data()) == 1);
        std::cout << "iterations: keys " << t.getIterationsRun() << ", plain " << n.getIterationsRun() << " of " << maxIt << "\n";
        CHECK(n.getIterationsRun() == maxIt);
        CHECK(t.getIterationsRun() <= maxIt && t.getIterationsRun() % every == 0 && t.getIterationsRun() == c.getIterationsRun());
        long ls[4] = {0, 0, 0, 0};
        CHECK(rn_get_last_solve(t.getEngine()->getContext(), ls) == RN_OK && ls[0] == (long)t.getIterationsRun() && ls[3] == ls[0] / every);
        CHECK(t.getIterationsRun() < maxIt ? ls[1] == 1 : true);
        CHECK(std::memcmp(ut.data(), uc.data(), nu * sizeof(real_t)) == 0);      // the file's keys and the setter: the same solve, bit for bit
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "stop tolerance: all checks passed\n";
    return 0;
}
