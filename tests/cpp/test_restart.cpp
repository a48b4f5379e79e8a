// The "momentumRestart" key of the controller configuration through the host classes (rapidnet.h, rn_set_restart).
//   test_restart <dir> parse     no GPU: loads <dir>/controllerConfig.json (no key) and <dir>/controllerRestartConfig.json (the key) and prints
//                                what SmpcConfiguration read
//   test_restart <dir>           a controller built from the file with "momentumRestart": "gradient" restarts the momentum of its control step,
//                                reports the count (SmpcController::getRestartsRun) and gives bit for bit the control of a controller built
//                                from the plain file and told the same through Engine::setRestart, which is also the control of the C-ABI
//                                route (rn_set_restart + rn_control_action on a third controller's context); the plain file never restarts
#include <cstring>
#include <iostream>
#include <vector>

#include "../../include/rapidnet.h"
#include "../../include/rapidnet_debug.h"
#include "../../rapidnet_amd/csrc/host/SmpcController.hpp"

static int g_failures = 0;
#define CHECK(c) do { if (!(c)) { std::cerr << "CHECK failed at line " << __LINE__ << ": " #c "\n"; g_failures++; } } while (0)

static void start(SmpcController &c) {
    c.getForecaster()->predictDemand(0);
    c.getForecaster()->predictPrices(0);
}

int main(int argc, char **argv) {
    if (argc < 2) { std::cerr << "usage: test_restart <dir> [parse]\n"; return 2; }
    const string dir = argv[1];
    try {
        if (argc > 2 && string(argv[2]) == "parse") {
            SmpcConfiguration plain(dir + "/controllerConfig.json"), key(dir + "/controllerRestartConfig.json");
            std::cout << "plain: momentumRestart " << plain.getMomentumRestart() << "\n";
            std::cout << "key: momentumRestart " << key.getMomentumRestart() << "\n";
            return 0;
        }
        SmpcController g(dir + "/controllerRestartConfig.json"), n(dir + "/controllerConfig.json"), c(dir + "/controllerConfig.json"),
            a(dir + "/controllerConfig.json");
        const uint_t maxIt = g.getSmpcConfiguration()->getMaxIterations(), nu = g.getSmpcConfiguration()->getNU();
        CHECK(g.getSmpcConfiguration()->getMomentumRestart() == "gradient" && n.getSmpcConfiguration()->getMomentumRestart() == "off");
        CHECK(g.getEngine()->getRestart() == RN_RESTART_GRADIENT && n.getEngine()->getRestart() == RN_RESTART_OFF);
        c.getEngine()->setRestart(RN_RESTART_GRADIENT);
        CHECK(c.getEngine()->getRestart() == RN_RESTART_GRADIENT);
        CHECK(rn_set_restart(c.getEngine()->getContext(), 7) == RN_E_ARG && c.getEngine()->getRestart() == RN_RESTART_GRADIENT);
        CHECK(rn_set_restart(n.getEngine()->getContext(), -1) == RN_E_ARG && n.getEngine()->getRestart() == RN_RESTART_OFF);
        {   // NULL outputs on a live context: refused, nothing written, the setting as it was
            long cnt[4] = {77, 77, 77, 77};
            double lst[3] = {77, 77, 77};
            rn_ctx *x = c.getEngine()->getContext();
            CHECK(rn_get_restart(x, nullptr) == RN_E_ARG);
            CHECK(rn_get_restart_info(x, nullptr, lst) == RN_E_ARG && rn_get_restart_info(x, cnt, nullptr) == RN_E_ARG);
            CHECK(cnt[0] == 77 && cnt[3] == 77 && lst[0] == 77 && lst[2] == 77);
            CHECK(rn_debug_restart_test(x, nullptr) == RN_E_ARG);
            CHECK(c.getEngine()->getRestart() == RN_RESTART_GRADIENT);
        }
        CHECK(rn_set_restart(a.getEngine()->getContext(), RN_RESTART_GRADIENT) == RN_OK);
        for (SmpcController *s : {&g, &n, &c, &a}) { start(*s); s->initialiseSmpcController(); }
        std::vector<real_t> ug(nu), un(nu), uc(nu), ua(nu);
        CHECK(g.controlAction(ug.data()) == 1 && n.controlAction(un.data()) == 1 && c.controlAction(uc.data()) == 1);
        // the C-ABI route: the same control step through rn_control_action on the fourth controller's context
        SmpcConfiguration *cf = a.getSmpcConfiguration();
        CHECK(rn_control_action(a.getEngine()->getContext(), cf->getCurrentX(), cf->getPrevU(), cf->getPrevDemand(), a.getForecaster()->getNominalDemand(),
                                a.getForecaster()->getNominalPrices(), (int)maxIt, 0, ua.data()) == RN_OK);
        std::cout << "restarts: key " << g.getRestartsRun() << ", plain " << n.getRestartsRun() << " in " << g.getIterationsRun() << " of " << maxIt << " iterations\n";
        CHECK(n.getRestartsRun() == 0 && n.getIterationsRun() == maxIt);
        CHECK(g.getIterationsRun() == maxIt);                    // no tolerance: a restart does not end the solve
        CHECK(g.getRestartsRun() >= 1 && g.getRestartsRun() == c.getRestartsRun());
        long counts[4] = {0, 0, 0, 0}, ls[4] = {0, 0, 0, 0};
        double last[3] = {0, 0, 0};
        CHECK(rn_get_restart_info(g.getEngine()->getContext(), counts, last) == RN_OK && counts[0] == (long)g.getRestartsRun() && counts[3] == 0);
        CHECK(rn_get_last_solve(g.getEngine()->getContext(), ls) == RN_OK && counts[2] == ls[3] && ls[0] == (long)maxIt);
        CHECK(counts[1] > 0 && counts[1] <= (long)maxIt && counts[1] % 20 == 0);
        CHECK(last[1] >= 0 && last[2] >= 0 && last[0] * last[0] <= last[1] * last[2] * (1 + 1e-12));      // Cauchy-Schwarz
        CHECK(rn_get_restart_info(a.getEngine()->getContext(), counts, last) == RN_OK && counts[0] == (long)g.getRestartsRun());
        CHECK(std::memcmp(ug.data(), uc.data(), nu * sizeof(real_t)) == 0);      // the file's key and the setter: the same solve, bit for bit
        CHECK(std::memcmp(ug.data(), ua.data(), nu * sizeof(real_t)) == 0);      // ... and the C-ABI route
        CHECK(std::memcmp(ug.data(), un.data(), nu * sizeof(real_t)) != 0);      // the restart changed the solve
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "momentum restart: all checks passed\n";
    return 0;
}
