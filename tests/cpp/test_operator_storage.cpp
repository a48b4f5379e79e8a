// The "operatorStorage" key of the controller configuration through the host classes: a configuration with "operatorStorage": "f32" and
// "operatorMode": "dense" gives a controller whose engine holds fp32 blocks under fp64 iterates (rapidnet.h, rn_set_operator_storage), its blocks
// are fp32-representable, and its control action is bit for bit that of a context that was given the same setting through the C ABI; a
// configuration without the key keeps the engine's own element type.
//   test_operator_storage <dir>     dir holds controllerConfig.json (dense, no key) and controllerF32Config.json (dense, "operatorStorage": "f32")
#include <cmath>
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
    if (argc < 2) { std::cerr << "usage: test_operator_storage <dir>\n"; return 2; }
    const string dir = argv[1];
    try {
        SmpcController f(dir + "/controllerF32Config.json"), n(dir + "/controllerConfig.json"), c(dir + "/controllerConfig.json");
        CHECK(f.getSmpcConfiguration()->getOperatorStorage() == "f32" && n.getSmpcConfiguration()->getOperatorStorage() == "native");
        // the third controller: the plain configuration, the setting made through the C ABI before the factor step
        CHECK(rn_set_operator_storage(c.getEngine()->getContext(), RN_STORE_F32) == RN_OK);
        int req = -1, act = -1;
        CHECK(rn_get_operator_storage(f.getEngine()->getContext(), &req, &act) == RN_OK && req == RN_STORE_F32 && act == RN_STORE_NATIVE);   // no blocks yet
        for (SmpcController *s : {&f, &n, &c}) { start(*s); s->initialiseSmpcController(); }
        CHECK(f.getEngine()->getOperatorMode() == RN_OPS_DENSE && n.getEngine()->getOperatorMode() == RN_OPS_DENSE);
        CHECK(f.getEngine()->getOperatorStorage() == RN_STORE_F32);
        CHECK(c.getEngine()->getOperatorStorage() == RN_STORE_F32);
        CHECK(n.getEngine()->getOperatorStorage() == RN_STORE_NATIVE);
        CHECK(rn_get_operator_storage(n.getEngine()->getContext(), &req, &act) == RN_OK && req == RN_STORE_NATIVE && act == RN_STORE_NATIVE);
        std::cout << "storage: f32 config -> " << (f.getEngine()->getOperatorStorage() == RN_STORE_F32 ? "f32" : "native") << ", plain config -> "
                  << (n.getEngine()->getOperatorStorage() == RN_STORE_F32 ? "f32" : "native") << "\n";
        CHECK(rn_set_operator_storage(f.getEngine()->getContext(), RN_STORE_NATIVE) == RN_E_STATE);      // after the factor step
        const uint_t nu = f.getSmpcConfiguration()->getNU(), nx = f.getSmpcConfiguration()->getNX(), nv = f.getSmpcConfiguration()->getNV();
        const uint_t nodes = f.getScenarioTree()->getNumNodes();
        // every block of the f32 engine is fp32-representable and within one fp32 rounding of the native engine's; the native engine's are not all floats
        size_t notFloat = 0;
        for (uint_t node = 0; node < nodes; node++)
            for (int op : {RN_OP_PHI, RN_OP_PSI, RN_OP_D, RN_OP_F}) {
                const size_t len = (size_t)nv * ((op == RN_OP_PHI || op == RN_OP_D) ? 2 * nx : nu);
                std::vector<real_t> a(len), b(len);
                f.getEngine()->getOperator(op, node, a.data(), len);
                n.getEngine()->getOperator(op, node, b.data(), len);
                for (size_t i = 0; i < len; i++) {
                    if ((double)(float)a[i] != a[i]) g_failures++;
                    if (std::fabs(a[i] - b[i]) > std::ldexp(std::fabs(b[i]), -23)) g_failures++;
                    if ((double)(float)b[i] != b[i]) notFloat++;
                }
            }
        CHECK(g_failures == 0);
        CHECK(notFloat > 0);
        std::vector<real_t> uf(nu), uc(nu), un(nu);
        CHECK(f.controlAction(uf.data()) == 1 && c.controlAction(uc.data()) == 1 && n.controlAction(un.data()) == 1);
        CHECK(std::memcmp(uf.data(), uc.data(), nu * sizeof(real_t)) == 0);        // bit for bit the C-ABI context's
        real_t diff = 0, mag = 0;
        for (uint_t i = 0; i < nu; i++) { diff = std::max(diff, std::fabs(uf[i] - un[i])); mag = std::max(mag, std::fabs(un[i])); }
        std::cout << "u0: fp32 blocks against native blocks, max difference " << diff / mag << " (relative)\n";
        CHECK(std::isfinite(diff) && diff <= 2e-4 * mag);      // the project's tolerance for fp32 storage
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "operator storage: all checks passed\n";
    return 0;
}
