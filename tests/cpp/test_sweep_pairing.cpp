// The "sweepPairing" key of the controller configuration and Engine::setSweepPairing / getSweepPairing (rapidnet.h, rn_set_sweep_pairing: NAMA's
// two Hessian sweeps in one pass over the dense blocks).
//   test_sweep_pairing parse <dir>     no GPU: the loader alone.  dir holds controllerConfig.json (no key), controllerOnConfig.json ("on"),
//                                      controllerOffConfig.json ("off"), controllerAutoConfig.json ("auto") and controllerBadConfig.json, whose
//                                      value must be refused (exit status 3)
//   test_sweep_pairing engine <dir>    the engines of the first three files: what the constructor took from the key, the accessor's round trip
#include <cstring>
#include <iostream>

#include "../../include/rapidnet.h"
#include "../../rapidnet_amd/csrc/host/SmpcController.hpp"

static int g_failures = 0;
#define CHECK(c) do { if (!(c)) { std::cerr << "CHECK failed at line " << __LINE__ << ": " #c "\n"; g_failures++; } } while (0)

int main(int argc, char **argv) {
    if (argc < 3) { std::cerr << "usage: test_sweep_pairing parse|engine <dir>\n"; return 2; }
    const string mode = argv[1], dir = argv[2];
    try {
        if (mode == "parse") {
            SmpcConfiguration plain(dir + "/controllerConfig.json"), on(dir + "/controllerOnConfig.json"), off(dir + "/controllerOffConfig.json"),
                autoKey(dir + "/controllerAutoConfig.json");
            CHECK(plain.getSweepPairing() == "auto");      // the default: every file of the reference
            CHECK(on.getSweepPairing() == "on" && off.getSweepPairing() == "off" && autoKey.getSweepPairing() == "auto");
            std::cout << "pairing keys: " << plain.getSweepPairing() << " " << on.getSweepPairing() << " " << off.getSweepPairing() << " "
                      << autoKey.getSweepPairing() << "\n";
            SmpcConfiguration bad(dir + "/controllerBadConfig.json");      // throws
            CHECK(false);
        } else {
            SmpcController plain(dir + "/controllerConfig.json"), on(dir + "/controllerOnConfig.json"), off(dir + "/controllerOffConfig.json");
            int active = -1;
            CHECK(plain.getEngine()->getSweepPairing(&active) == RN_PAIR_AUTO && active == 0);      // no NAMA selected
            CHECK(on.getEngine()->getSweepPairing() == RN_PAIR_ON && off.getEngine()->getSweepPairing() == RN_PAIR_OFF);
            Engine *e = plain.getEngine();
            for (int m : {RN_PAIR_ON, RN_PAIR_OFF, RN_PAIR_AUTO}) { e->setSweepPairing(m); CHECK(e->getSweepPairing() == m); }
            bool refused = false;
            try { e->setSweepPairing(7); } catch (const std::exception &) { refused = true; }
            CHECK(refused && e->getSweepPairing() == RN_PAIR_AUTO);
            CHECK(rn_set_sweep_pairing(e->getContext(), 7) == RN_E_ARG);
        }
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "sweep pairing: all checks passed\n";
    return 0;
}
