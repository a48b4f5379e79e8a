// A re-weighted scenario tree through the host classes (rapidnet.h, rn_set_tree_data; the reference loads devTreeProb once, Engine.cu:263-286):
// SmpcController::updateScenarioTree(path) between two controlAction calls against a fresh controller on the new files, bit for bit;
// ScenarioTree::reload of another topology throws and changes nothing; Engine::setTreeDataDevice round-trips through getTreeData.
//   test_tree_data <dirOld> <dirNew> <badTree.json>
//     dirOld / dirNew hold the four files of one problem with the old and the re-weighted scenarioTree.json (same topology);
//     badTree.json is the old tree with another `ancestor`.
// The device arrays come from the HIP runtime that librapidnet_hip.so has loaded (looked up by name: this program is built without HIP headers).
#include <cstring>
#include <dlfcn.h>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "../../include/rapidnet.h"
#include "../../rapidnet_amd/csrc/host/SmpcController.hpp"

static int g_failures = 0;
#define CHECK(c) do { if (!(c)) { std::cerr << "CHECK failed at line " << __LINE__ << ": " #c "\n"; g_failures++; } } while (0)

typedef int (*hip_malloc_t)(void **, size_t);
typedef int (*hip_free_t)(void *);
typedef int (*hip_memcpy_t)(void *, const void *, size_t, int);
enum { H2D = 1 };   // hipMemcpyHostToDevice

static bool same(const std::vector<real_t> &x, const std::vector<real_t> &y) { return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(real_t)) == 0; }
static bool same(const real_t *x, const std::vector<real_t> &y) { return std::memcmp(x, y.data(), y.size() * sizeof(real_t)) == 0; }

struct TreeData { std::vector<real_t> p, ed, ep; };
static TreeData held(Engine *e, uint_t nodes, uint_t nd, uint_t nu) {
    TreeData t;
    t.p.assign(nodes, -7.0); t.ed.assign((size_t)nodes * nd, -7.0); t.ep.assign((size_t)nodes * nu, -7.0);
    e->getTreeData(t.p.data(), t.ed.data(), t.ep.data());
    return t;
}

int main(int argc, char **argv) {
    if (argc < 4) { std::cerr << "usage: test_tree_data <dirOld> <dirNew> <badTree.json>\n"; return 2; }
    const string dirOld = argv[1], dirNew = argv[2], badTree = argv[3];
    try {
        SmpcController a(dirOld + "/controllerConfig.json"), b(dirNew + "/controllerConfig.json");
        const uint_t nu = a.getSmpcConfiguration()->getNU(), nd = a.getSmpcConfiguration()->getND();
        const uint_t nodes = a.getScenarioTree()->getNumNodes();
        for (SmpcController *s : {&a, &b}) { s->getForecaster()->predictDemand(0); s->getForecaster()->predictPrices(0); }
        std::vector<real_t> ua(nu), ub(nu), ua2(nu);
        CHECK(a.controlAction(ua.data()) == 1);
        // another topology: refused, and neither the host arrays nor the device's change
        ScenarioTree *ta = a.getScenarioTree();
        const std::vector<real_t> p0(ta->getProbArray(), ta->getProbArray() + nodes);
        const std::vector<uint_t> anc0(ta->getAncestorArray(), ta->getAncestorArray() + nodes);
        bool threw = false;
        try { a.updateScenarioTree(badTree); } catch (const std::invalid_argument &) { threw = true; }
        CHECK(threw);
        CHECK(same(ta->getProbArray(), p0) && std::memcmp(ta->getAncestorArray(), anc0.data(), nodes * sizeof(uint_t)) == 0);
        CHECK(same(held(a.getEngine(), nodes, nd, nu).p, p0));
        threw = false;
        try { ta->setProbArray(p0.data(), nodes - 1); } catch (const std::invalid_argument &) { threw = true; }
        CHECK(threw);
        // the re-weighted tree between two control steps == a fresh controller on the new files
        a.updateScenarioTree(dirNew + "/scenarioTree.json");
        size_t differ = 0;
        for (uint_t i = 0; i < nodes; i++) if (ta->getProbArray()[i] != p0[i]) differ++;
        CHECK(differ * 2 >= (size_t)nodes);
        CHECK(a.controlAction(ua2.data()) == 1);
        CHECK(b.controlAction(ub.data()) == 1);
        CHECK(same(ua2, ub));
        CHECK(!same(ua2, ua));
        const TreeData ha = held(a.getEngine(), nodes, nd, nu), hb = held(b.getEngine(), nodes, nd, nu);
        CHECK(same(ha.p, hb.p) && same(ha.ed, hb.ed) && same(ha.ep, hb.ep));
        CHECK(same(b.getScenarioTree()->getProbArray(), ha.p));
        // device arrays: the old tree's values back into `a`, read back through getTreeData
        hip_malloc_t p_malloc = (hip_malloc_t)dlsym(RTLD_DEFAULT, "hipMalloc");
        hip_free_t p_free = (hip_free_t)dlsym(RTLD_DEFAULT, "hipFree");
        hip_memcpy_t p_memcpy = (hip_memcpy_t)dlsym(RTLD_DEFAULT, "hipMemcpy");
        CHECK(p_malloc && p_free && p_memcpy);
        if (!p_malloc || !p_free || !p_memcpy) return 1;
        ScenarioTree told(dirOld + "/scenarioTree.json");
        const std::vector<real_t> ed0(told.getErrorDemandArray(), told.getErrorDemandArray() + (size_t)nodes * nd);
        void *dp = nullptr, *de = nullptr;
        CHECK(p_malloc(&dp, nodes * sizeof(double)) == 0 && p_malloc(&de, ed0.size() * sizeof(double)) == 0);
        if (g_failures) return 1;
        CHECK(p_memcpy(dp, p0.data(), nodes * sizeof(double), H2D) == 0 && p_memcpy(de, ed0.data(), ed0.size() * sizeof(double), H2D) == 0);   // (blocking: the producer is done)
        a.getEngine()->setTreeDataDevice(RN_F64, dp, de, nullptr);
        CHECK(rn_apg_iterate(a.getEngine()->getContext(), 1, nullptr) == RN_E_STATE);       // the affine terms are the old probabilities'
        const TreeData back = held(a.getEngine(), nodes, nd, nu);       // (synchronises)
        CHECK(same(back.p, p0) && same(back.ed, ed0) && same(back.ep, ha.ep));
        rn_ctx *c = a.getEngine()->getContext();
        CHECK(rn_set_tree_data_device(c, nodes, 7, dp, nullptr, nullptr) == RN_E_ARG);
        CHECK(rn_set_tree_data_device(c, nodes + 1, RN_F64, dp, nullptr, nullptr) == RN_E_ARG);
        CHECK(rn_set_tree_data_device(c, nodes, RN_F64, p0.data(), nullptr, nullptr) == RN_E_ARG);     // a host pointer
        CHECK(rn_set_tree_data(c, nodes, nullptr, nullptr, nullptr) == RN_E_ARG);
        CHECK(same(held(a.getEngine(), nodes, nd, nu).p, p0));
        p_free(dp); p_free(de);
        std::cout << "tree data: " << nodes << " nodes, " << differ << " re-weighted\n";
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "tree data: all checks passed\n";
    return 0;
}
