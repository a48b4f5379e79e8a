// All per-node operator blocks in one call through the host classes: Engine::setOperators / getOperators (host arrays) and
// setOperatorsDevice / getOperatorsDevice (device arrays) against the per-node Engine::setOperator / getOperator, bit for bit
// (rapidnet.h, rn_set_operators; the reference: Engine.cuh getMatPhi() ... getMatF() as whole arrays).
//   test_operator_bulk <dir>     dir holds controllerConfig.json (dense, no key) and controllerF32Config.json (dense, "operatorStorage": "f32")
// The device arrays come from the HIP runtime that librapidnet_hip.so has loaded (looked up by name: this program is built without HIP headers).
#include <cmath>
#include <cstring>
#include <dlfcn.h>
#include <iostream>
#include <vector>

#include "../../include/rapidnet.h"
#include "../../rapidnet_amd/csrc/host/SmpcController.hpp"

static int g_failures = 0;
#define CHECK(c) do { if (!(c)) { std::cerr << "CHECK failed at line " << __LINE__ << ": " #c "\n"; g_failures++; } } while (0)

typedef int (*hip_malloc_t)(void **, size_t);
typedef int (*hip_free_t)(void *);
typedef int (*hip_memcpy_t)(void *, const void *, size_t, int);
static hip_malloc_t p_malloc;
static hip_free_t p_free;
static hip_memcpy_t p_memcpy;
enum { H2D = 1, D2H = 2 };   // hipMemcpyHostToDevice, hipMemcpyDeviceToHost

struct Ops { std::vector<real_t> a[4]; };   // phi, psi, D, F as [node][cols][nv]
static const int OP_ID[4] = {RN_OP_PHI, RN_OP_PSI, RN_OP_D, RN_OP_F};

static Ops per_node(Engine *e, uint_t nodes, const size_t len[4]) {
    Ops o;
    for (int i = 0; i < 4; i++) {
        o.a[i].resize(nodes * len[i]);
        for (uint_t node = 0; node < nodes; node++) e->getOperator(OP_ID[i], node, o.a[i].data() + node * len[i], len[i]);
    }
    return o;
}
static Ops bulk(Engine *e, uint_t nodes, const size_t len[4]) {
    Ops o;
    for (int i = 0; i < 4; i++) o.a[i].assign(nodes * len[i], -7.0);
    e->getOperators(o.a[0].data(), o.a[1].data(), o.a[2].data(), o.a[3].data());
    return o;
}
static bool same(const std::vector<real_t> &x, const std::vector<real_t> &y) { return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(real_t)) == 0; }
static bool same(const Ops &x, const Ops &y) { return same(x.a[0], y.a[0]) && same(x.a[1], y.a[1]) && same(x.a[2], y.a[2]) && same(x.a[3], y.a[3]); }

int main(int argc, char **argv) {
    if (argc < 2) { std::cerr << "usage: test_operator_bulk <dir>\n"; return 2; }
    const string dir = argv[1];
    try {
        SmpcController n(dir + "/controllerConfig.json"), f(dir + "/controllerF32Config.json");
        Engine *en = n.getEngine(), *ef = f.getEngine();
        const uint_t nu = n.getSmpcConfiguration()->getNU(), nx = n.getSmpcConfiguration()->getNX(), nv = n.getSmpcConfiguration()->getNV();
        const uint_t nodes = n.getScenarioTree()->getNumNodes();
        const size_t len[4] = {(size_t)nv * 2 * nx, (size_t)nv * nu, (size_t)nv * 2 * nx, (size_t)nv * nu};
        std::vector<real_t> one(len[0] * nodes);
        CHECK(rn_set_operators(en->getContext(), nodes, one.data(), nullptr, nullptr, nullptr) == RN_E_STATE);      // before the factor step
        for (SmpcController *s : {&n, &f}) { s->getForecaster()->predictDemand(1); s->getForecaster()->predictPrices(1); s->initialiseSmpcController(); }
        CHECK(en->getOperatorStorage() == RN_STORE_NATIVE && ef->getOperatorStorage() == RN_STORE_F32);
        p_malloc = (hip_malloc_t)dlsym(RTLD_DEFAULT, "hipMalloc"); p_free = (hip_free_t)dlsym(RTLD_DEFAULT, "hipFree"); p_memcpy = (hip_memcpy_t)dlsym(RTLD_DEFAULT, "hipMemcpy");
        CHECK(p_malloc && p_free && p_memcpy);
        if (!p_malloc || !p_free || !p_memcpy) return 1;

        // read: bulk == per node
        const Ops own = per_node(en, nodes, len);
        CHECK(same(bulk(en, nodes, len), own));
        CHECK(same(bulk(ef, nodes, len), per_node(ef, nodes, len)));
        // write: blocks of the caller's (not fp32-representable), all four, host form
        Ops mine;
        size_t notFloat = 0;
        for (int i = 0; i < 4; i++) {
            mine.a[i].resize(own.a[i].size());
            for (size_t k = 0; k < mine.a[i].size(); k++) {
                mine.a[i][k] = own.a[i][k] * (1.0 + 0.3 * std::sin(0.37 * (double)k + i)) + 1e-3 * std::cos((double)k);
                if ((double)(float)mine.a[i][k] != mine.a[i][k]) notFloat++;
            }
        }
        CHECK(notFloat > mine.a[0].size());
        en->setOperators(mine.a[0].data(), mine.a[1].data(), mine.a[2].data(), mine.a[3].data());
        CHECK(same(per_node(en, nodes, len), mine) && same(bulk(en, nodes, len), mine));
        // fp32 storage: the values rounded to nearest, exactly what the per-node call stores
        Ops rounded = mine;
        for (int i = 0; i < 4; i++) for (real_t &v : rounded.a[i]) v = (double)(float)v;
        ef->setOperators(mine.a[0].data(), mine.a[1].data(), mine.a[2].data(), mine.a[3].data());
        CHECK(same(per_node(ef, nodes, len), rounded) && same(bulk(ef, nodes, len), rounded));
        SmpcController g(dir + "/controllerF32Config.json");
        g.getForecaster()->predictDemand(1); g.getForecaster()->predictPrices(1); g.initialiseSmpcController();
        for (int i = 0; i < 4; i++) for (uint_t node = 0; node < nodes; node++) g.getEngine()->setOperator(OP_ID[i], node, mine.a[i].data() + node * len[i], len[i]);
        CHECK(same(per_node(g.getEngine(), nodes, len), rounded));
        // partial: Phi and F back to the engine's own, Psi and D keep the caller's
        en->setOperators(own.a[0].data(), nullptr, nullptr, own.a[3].data());
        {
            const Ops now = bulk(en, nodes, len);
            CHECK(same(now.a[0], own.a[0]) && same(now.a[3], own.a[3]) && same(now.a[1], mine.a[1]) && same(now.a[2], mine.a[2]));
            CHECK(same(per_node(en, nodes, len), now));
        }
        // device arrays, fp64 elements: set all four, read all four back
        void *dv[4] = {nullptr, nullptr, nullptr, nullptr}, *back[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < 4; i++) {
            CHECK(p_malloc(&dv[i], mine.a[i].size() * sizeof(double)) == 0 && p_malloc(&back[i], mine.a[i].size() * sizeof(double)) == 0);
            CHECK(p_memcpy(dv[i], own.a[i].data(), own.a[i].size() * sizeof(double), H2D) == 0);     // (blocking: the producer is done before the call)
        }
        if (g_failures) return 1;
        en->setOperatorsDevice(RN_F64, dv[0], dv[1], dv[2], dv[3]);
        en->getOperatorsDevice(RN_F64, back[0], back[1], back[2], back[3]);
        CHECK(rn_synchronize(en->getContext()) == RN_OK);
        Ops fromDev;
        for (int i = 0; i < 4; i++) {
            fromDev.a[i].resize(own.a[i].size());
            CHECK(p_memcpy(fromDev.a[i].data(), back[i], own.a[i].size() * sizeof(double), D2H) == 0);
        }
        CHECK(same(fromDev, own) && same(bulk(en, nodes, len), own) && same(per_node(en, nodes, len), own));
        // refused calls
        rn_ctx *c = en->getContext();
        CHECK(rn_set_operators(c, nodes + 1, own.a[0].data(), nullptr, nullptr, nullptr) == RN_E_ARG);
        CHECK(rn_get_operators(c, nodes - 1, fromDev.a[0].data(), nullptr, nullptr, nullptr) == RN_E_ARG);
        CHECK(rn_set_operators(c, nodes, nullptr, nullptr, nullptr, nullptr) == RN_E_ARG);
        CHECK(rn_set_operators_device(c, nodes, 7, dv[0], nullptr, nullptr, nullptr) == RN_E_ARG);
        CHECK(rn_get_operators_device(c, nodes, -1, back[0], nullptr, nullptr, nullptr) == RN_E_ARG);
        bool threw = false;
        try { en->setOperators(nullptr, nullptr, nullptr, nullptr); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
        CHECK(same(bulk(en, nodes, len), own));      // ... and none of them changed a block
        for (int i = 0; i < 4; i++) { p_free(dv[i]); p_free(back[i]); }
        std::cout << "bulk operators: " << nodes << " nodes, nv " << nv << ", 2nx " << 2 * nx << ", nu " << nu << "\n";
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "operator bulk: all checks passed\n";
    return 0;
}
