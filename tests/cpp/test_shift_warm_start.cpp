// The shifted warm start through the host classes (rapidnet.h, rn_shift_warm_start; Engine::shiftWarmStart / setShiftMap / getShiftMap,
// SmpcController::shiftWarmStart, the "warmStart" key of the controller configuration).
//   test_shift_warm_start <dir> parse   no GPU: loads <dir>/controllerConfig.json (no key), <dir>/controllerKeepConfig.json and
//                                       <dir>/controllerShiftConfig.json and prints what SmpcConfiguration read
//   test_shift_warm_start <dir>         three control steps of a closed loop (controlAction, moveForewardInTime) on five controllers: the file
//                                       with "warmStart": "shift"; the plain file told the same by hand (Engine::setWarmStart + a
//                                       SmpcController::shiftWarmStart between the steps); the file with "keep"; the plain file with
//                                       setWarmStart and the identity as its own map; the plain file.  Checked: key and hand give the same
//                                       controls bit for bit, the identity map is "keep" bit for bit, shift, keep and cold differ from the
//                                       second step on, every controlAction passes its leak check (the first shift allocates in front of its
//                                       window), the map of the rule starts at the root's most probable child, and the C-ABI's refusals.
#include <cstring>
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
static bool same(const std::vector<real_t> &a, const std::vector<real_t> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(real_t)) == 0; }

int main(int argc, char **argv) {
    if (argc < 2) { std::cerr << "usage: test_shift_warm_start <dir> [parse]\n"; return 2; }
    const string dir = argv[1];
    try {
        if (argc > 2 && string(argv[2]) == "parse") {
            SmpcConfiguration plain(dir + "/controllerConfig.json"), keep(dir + "/controllerKeepConfig.json"), shift(dir + "/controllerShiftConfig.json");
            std::cout << "plain: warmStart " << plain.getWarmStart() << "\n";
            std::cout << "keep: warmStart " << keep.getWarmStart() << "\n";
            std::cout << "shift: warmStart " << shift.getWarmStart() << "\n";
            return 0;
        }
        SmpcController s(dir + "/controllerShiftConfig.json"), h(dir + "/controllerConfig.json"), k(dir + "/controllerKeepConfig.json"),
            id(dir + "/controllerConfig.json"), n(dir + "/controllerConfig.json");
        SmpcController *all[5] = {&s, &h, &k, &id, &n};
        const uint_t nu = s.getSmpcConfiguration()->getNU();
        const int nodes = (int)s.getScenarioTree()->getNumNodes();
        CHECK(s.getSmpcConfiguration()->getWarmStart() == "shift" && k.getSmpcConfiguration()->getWarmStart() == "keep" && n.getSmpcConfiguration()->getWarmStart() == "off");
        h.getEngine()->setWarmStart(true);
        id.getEngine()->setWarmStart(true);
        for (SmpcController *c : all) { start(*c); c->initialiseSmpcController(); }
        rn_ctx *x = h.getEngine()->getContext();
        CHECK(rn_shift_warm_start(x, 0) == RN_E_STATE);                       // no solve yet: there are no duals to shift
        CHECK(rn_shift_warm_start(nullptr, 0) == RN_E_ARG);
        // the rule's map: a node one stage down, the root onto its most probable child (ties to the lowest index)
        std::vector<int> map, first;
        h.getEngine()->getShiftMap(-1, map);
        h.getEngine()->getShiftMap(0, first);
        CHECK((int)map.size() == nodes && first[0] == 1 && map[0] >= 1);
        {
            std::vector<real_t> p((size_t)nodes), ed((size_t)nodes * s.getSmpcConfiguration()->getND()), ep((size_t)nodes * nu);
            CHECK(rn_get_tree_data(x, (size_t)nodes, p.data(), ed.data(), ep.data()) == RN_OK);
            int nc = 0, best = 1;      // the root's children are nodes 1 .. nc: child number r is accepted exactly for r < nc
            while (nc < nodes && rn_get_shift_map(x, nc, (size_t)nodes, first.data()) == RN_OK) { CHECK(first[0] == 1 + nc); nc++; }
            for (int r = 1; r < nc; r++) if (p[1 + r] > p[best]) best = 1 + r;
            CHECK(nc >= 1 && map[0] == best);
            CHECK(rn_get_shift_map(x, nc, (size_t)nodes, first.data()) == RN_E_ARG && rn_get_shift_map(x, -2, (size_t)nodes, first.data()) == RN_E_ARG);
            CHECK(rn_get_shift_map(x, 0, (size_t)nodes + 1, first.data()) == RN_E_ARG && rn_get_shift_map(x, 0, (size_t)nodes, nullptr) == RN_E_ARG);
            std::cout << "root children: " << nc << ", most probable: " << best - 1 << "\n";
        }
        std::vector<int> identity((size_t)nodes);
        for (int i = 0; i < nodes; i++) identity[i] = i;
        id.getEngine()->setShiftMap(identity);
        std::vector<int> back;
        id.getEngine()->getShiftMap(0, back);
        CHECK(back == identity);
        {
            std::vector<int> bad(identity);
            bad[1] = nodes;
            CHECK(rn_set_shift_map(x, (size_t)nodes, bad.data()) == RN_E_ARG && rn_set_shift_map(x, (size_t)nodes - 1, identity.data()) == RN_E_ARG);
        }
        std::vector<std::vector<real_t>> u[5];
        for (int step = 0; step < 3; step++) {
            for (int c = 0; c < 5; c++) {
                if (step > 0 && (all[c] == &h || all[c] == &id)) all[c]->shiftWarmStart(-1);      // by hand, between two steps
                std::vector<real_t> uc(nu);
                CHECK(all[c]->controlAction(uc.data()) == 1);          // (with the leak check: the shift's arrays came before its window)
                u[c].push_back(uc);
                all[c]->moveForewardInTime();
            }
            if (step == 0) CHECK(rn_shift_warm_start(x, 1 << 20) == RN_E_ARG);      // a solve has run: now the argument is looked at
        }
        CHECK(same(u[0][0], u[4][0]) && same(u[1][0], u[4][0]) && same(u[2][0], u[4][0]) && same(u[3][0], u[4][0]));      // the first step is cold everywhere
        for (int step = 1; step < 3; step++) {
            CHECK(same(u[0][step], u[1][step]));       // the key and the calls by hand
            CHECK(same(u[2][step], u[3][step]));       // "keep" and the identity as the caller's map
            CHECK(!same(u[0][step], u[2][step]) && !same(u[0][step], u[4][step]) && !same(u[2][step], u[4][step]));
        }
        std::cout << "controls of step 2, component 0: shift " << u[0][2][0] << ", keep " << u[2][2][0] << ", cold " << u[4][2][0] << "\n";
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "shift warm start: all checks passed\n";
    return 0;
}
