// The dual Lipschitz estimate and the step rule through the host classes (rapidnet.h, rn_estimate_lipschitz / rn_set_step_rule;
// Engine::estimateLipschitz / setStepRule, SmpcController::getStepSizeInForce; the configuration's optional "stepSizeRule", "stepSizeMargin"
// and "lipschitzIterations" keys).
//   test_lipschitz <dir> parse   reads <dir>/controllerConfig.json (no key) and <dir>/controllerLipConfig.json and prints what it read;
//                                a bad value throws (exit code 3).  No GPU.
//   test_lipschitz <dir>         two controllers: the plain one and the one with "stepSizeRule": "lipschitz".  Checked: the plain one's step size
//                                in force is the file's and it holds no estimate; the keyed one's first controlAction passes the leak check
//                                (the first estimate ran in front of its window) and its step size in force is margin / norm of the estimate it
//                                holds; Engine::estimateLipschitz is the C-ABI route bit for bit, twice; a controller given that step size by
//                                hand computes the same control, bit for bit; setStepRule(RN_STEP_FIXED) returns the file's figure.
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
    if (argc < 2) { std::cerr << "usage: test_lipschitz <dir> [parse]\n"; return 2; }
    const string dir = argv[1];
    try {
        if (argc > 2 && string(argv[2]) == "parse") {
            for (const char *f : {"controllerConfig.json", "controllerLipConfig.json"}) {
                SmpcConfiguration c(dir + "/" + f);
                std::cout << f << ": stepSizeRule " << c.getStepSizeRule() << " margin " << c.getStepSizeMargin() << " iterations " << c.getLipschitzIterations() << "\n";
            }
            return 0;
        }
        SmpcController plain(dir + "/controllerConfig.json"), lip(dir + "/controllerLipConfig.json"), hand(dir + "/controllerConfig.json");
        for (SmpcController *s : {&plain, &lip, &hand}) { start(*s); s->initialiseSmpcController(); }
        SmpcConfiguration *cfg = lip.getSmpcConfiguration();
        const uint_t nu = cfg->getNU();
        std::vector<real_t> u0(nu), u1(nu), u2(nu);
        Engine::LipschitzEstimate held;
        CHECK(plain.getStepSizeInForce() == plain.getSmpcConfiguration()->getStepSize());
        CHECK(!plain.getEngine()->getLipschitz(held));
        CHECK(plain.controlAction(u0.data()) == 1);
        CHECK(!plain.getEngine()->getLipschitz(held));                   // the rule off: nothing was estimated
        real_t margin = 0; int its = 0;
        CHECK(lip.getEngine()->getStepRule(&margin, &its) == RN_STEP_LIPSCHITZ && margin == cfg->getStepSizeMargin() && its == (int)cfg->getLipschitzIterations());
        CHECK(lip.controlAction(u1.data()) == 1);                        // the first estimate allocated in front of the leak check's window
        CHECK(lip.getEngine()->getLipschitz(held) && !held.stale && held.iterations == cfg->getLipschitzIterations() && held.norm > 0);
        CHECK(held.rayleigh <= held.norm * (1 + 1e-12) && held.residual >= 0);
        const real_t step = margin / held.norm;
        CHECK(lip.getStepSizeInForce() == step);
        CHECK(lip.controlAction(u1.data()) == 1);                        // ... and the second step holds what it needs
        // the host class is the C-ABI route, bit for bit, twice
        double out[RN_LIP_COLS];
        std::vector<double> hist((size_t)its * 3);
        CHECK(rn_estimate_lipschitz(lip.getEngine()->getContext(), its, 0.0, 0, nullptr, nullptr, 0, out, hist.data()) == RN_OK);
        const Engine::LipschitzEstimate e = lip.getEngine()->estimateLipschitz(its, 0, 0, std::vector<real_t>(), 0, true);
        CHECK(e.norm == out[RN_LIP_NORM] && e.rayleigh == out[RN_LIP_RAYLEIGH] && e.residual == out[RN_LIP_RESIDUAL] && e.iterations == (uint_t)its);
        CHECK(e.history.size() == hist.size() && std::memcmp(e.history.data(), hist.data(), hist.size() * sizeof(double)) == 0);
        CHECK(e.norm == held.norm);
        bool refused = false;
        try { lip.getEngine()->estimateLipschitz(0); } catch (const std::runtime_error &) { refused = true; }
        CHECK(refused);
        // that step size by hand: the same control, bit for bit
        CHECK(rn_set_parameters(hand.getEngine()->getContext(), step, cfg->getPenaltyState(), cfg->getPenaltySafety()) == RN_OK);
        CHECK(hand.controlAction(u2.data()) == 1);
        CHECK(std::memcmp(u1.data(), u2.data(), nu * sizeof(real_t)) == 0);
        CHECK(std::memcmp(u0.data(), u1.data(), nu * sizeof(real_t)) != 0 || step == plain.getStepSizeInForce());
        lip.getEngine()->setStepRule(RN_STEP_FIXED);
        CHECK(lip.getStepSizeInForce() == cfg->getStepSize());
        std::cout << std::setprecision(17) << "norm " << held.norm << " step " << step << " file " << cfg->getStepSize() << "\n";
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "lipschitz: all checks passed\n";
    return 0;
}
