// Bounds per stage through the host classes (rapidnet.h, rn_set_bounds; the reference's callers write through getSysXmin() ... getSysUmax(),
// Engine.cuh:294-314): SmpcController::updateBounds between two controlAction calls against a controller that set the same bounds before its
// first step, bit for bit; Engine::setBoundsDevice round-trips through getBounds; a factor step returns to the network's vectors.
//   test_bounds <dir>        dir holds the four files of one problem
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

struct Bounds {
    std::vector<real_t> xmin, xmax, xsafe, umin, umax;
    Bounds(size_t rows, uint_t nx, uint_t nu, real_t v = -7.0) : xmin(rows * nx, v), xmax(rows * nx, v), xsafe(rows * nx, v), umin(rows * nu, v), umax(rows * nu, v) {}
};
static Bounds held(Engine *e, uint_t nx, uint_t nu) {
    size_t rows = 0;
    e->getBoundsLayout(&rows);
    Bounds b(rows, nx, nu);
    e->getBounds(rows, b.xmin.data(), b.xmax.data(), b.xsafe.data(), b.umin.data(), b.umax.data());
    return b;
}
static bool same(const Bounds &a, const Bounds &b) { return same(a.xmin, b.xmin) && same(a.xmax, b.xmax) && same(a.xsafe, b.xsafe) && same(a.umin, b.umin) && same(a.umax, b.umax); }

int main(int argc, char **argv) {
    if (argc < 2) { std::cerr << "usage: test_bounds <dir>\n"; return 2; }
    const string dir = argv[1];
    try {
        SmpcController a(dir + "/controllerConfig.json"), b(dir + "/controllerConfig.json");
        const uint_t nx = a.getSmpcConfiguration()->getNX(), nu = a.getSmpcConfiguration()->getNU();
        const uint_t N = a.getScenarioTree()->getPredHorizon();
        for (SmpcController *s : {&a, &b}) { s->getForecaster()->predictDemand(0); s->getForecaster()->predictPrices(0); }
        // a row per stage: the safety volume grows and the pumps lose capacity along the horizon
        DwnNetwork *net = a.getDwnNetwork();
        Bounds rows(N, nx, nu);
        for (uint_t s = 0; s < N; s++) {
            const real_t t = N > 1 ? (real_t)s / (real_t)(N - 1) : 0.0;
            for (uint_t j = 0; j < nx; j++) {
                rows.xmin[s * nx + j] = net->getXmin()[j]; rows.xmax[s * nx + j] = net->getXmax()[j] * (1.0 - 0.2 * t);
                rows.xsafe[s * nx + j] = net->getXsafe()[j] * (1.0 + 0.5 * t);
            }
            for (uint_t j = 0; j < nu; j++) { rows.umin[s * nu + j] = net->getUmin()[j]; rows.umax[s * nu + j] = net->getUmax()[j] * (1.0 - 0.4 * (real_t)(s % 3) / 2.0); }
        }
        std::vector<real_t> ua(nu), ua2(nu), ub(nu);
        CHECK(a.controlAction(ua.data()) == 1);
        size_t r = 0;
        CHECK(a.getEngine()->getBoundsLayout(&r) == RN_BOUNDS_SHARED && r == 1);
        const Bounds own = held(a.getEngine(), nx, nu);
        CHECK(std::memcmp(own.xsafe.data(), net->getXsafe(), nx * sizeof(real_t)) == 0 && std::memcmp(own.umax.data(), net->getUmax(), nu * sizeof(real_t)) == 0);
        // between two control steps == before the first step
        a.updateBounds(RN_BOUNDS_PER_STAGE, N, rows.xmin.data(), rows.xmax.data(), rows.xsafe.data(), rows.umin.data(), rows.umax.data());
        CHECK(a.controlAction(ua2.data()) == 1);
        b.updateBounds(RN_BOUNDS_PER_STAGE, N, rows.xmin.data(), rows.xmax.data(), rows.xsafe.data(), rows.umin.data(), rows.umax.data());
        CHECK(b.controlAction(ub.data()) == 1);
        CHECK(same(ua2, ub));
        CHECK(!same(ua2, ua));
        CHECK(a.getEngine()->getBoundsLayout(&r) == RN_BOUNDS_PER_STAGE && r == (size_t)N);
        CHECK(same(held(a.getEngine(), nx, nu), rows) && same(held(b.getEngine(), nx, nu), rows));
        // refused calls change nothing
        rn_ctx *c = a.getEngine()->getContext();
        CHECK(rn_set_bounds(c, RN_BOUNDS_PER_STAGE, N + 1, rows.xmin.data(), rows.xmax.data(), rows.xsafe.data(), rows.umin.data(), rows.umax.data()) == RN_E_ARG);
        CHECK(rn_set_bounds(c, RN_BOUNDS_SHARED, 1, rows.xmin.data(), nullptr, rows.xsafe.data(), rows.umin.data(), rows.umax.data()) == RN_E_ARG);
        CHECK(rn_set_bounds(c, RN_BOUNDS_PER_STAGE, N, nullptr, nullptr, nullptr, nullptr, nullptr) == RN_E_ARG);
        CHECK(rn_set_bounds(c, RN_BOUNDS_PER_STAGE, N, rows.xmax.data(), rows.xmin.data(), nullptr, nullptr, nullptr) == RN_E_ARG);      // xmin > xmax
        bool threw = false;
        try { a.getEngine()->setBounds(RN_BOUNDS_PER_NODE, N, rows.xmin.data(), rows.xmax.data(), rows.xsafe.data(), rows.umin.data(), rows.umax.data()); }
        catch (const std::exception &) { threw = true; }
        CHECK(threw);
        CHECK(same(held(a.getEngine(), nx, nu), rows));
        // device arrays: xsafe alone, read back through getBounds
        hip_malloc_t p_malloc = (hip_malloc_t)dlsym(RTLD_DEFAULT, "hipMalloc");
        hip_free_t p_free = (hip_free_t)dlsym(RTLD_DEFAULT, "hipFree");
        hip_memcpy_t p_memcpy = (hip_memcpy_t)dlsym(RTLD_DEFAULT, "hipMemcpy");
        CHECK(p_malloc && p_free && p_memcpy);
        if (!p_malloc || !p_free || !p_memcpy) return 1;
        Bounds want = rows;
        for (real_t &v : want.xsafe) v *= 1.25;
        void *dx = nullptr;
        CHECK(p_malloc(&dx, want.xsafe.size() * sizeof(double)) == 0);
        if (g_failures) return 1;
        CHECK(p_memcpy(dx, want.xsafe.data(), want.xsafe.size() * sizeof(double), H2D) == 0);   // (blocking: the producer is done)
        a.getEngine()->setBoundsDevice(RN_BOUNDS_PER_STAGE, N, RN_F64, nullptr, nullptr, dx, nullptr, nullptr);
        CHECK(same(held(a.getEngine(), nx, nu), want));       // (synchronises)
        CHECK(rn_set_bounds_device(c, RN_BOUNDS_PER_STAGE, N, 7, nullptr, nullptr, dx, nullptr, nullptr) == RN_E_ARG);
        CHECK(rn_set_bounds_device(c, RN_BOUNDS_PER_STAGE, N, RN_F64, nullptr, nullptr, want.xsafe.data(), nullptr, nullptr) == RN_E_ARG);     // a host pointer
        CHECK(rn_set_bounds_device(c, RN_BOUNDS_SHARED, 1, RN_F64, nullptr, nullptr, dx, nullptr, nullptr) == RN_E_ARG);                       // a new granularity wants all five
        CHECK(same(held(a.getEngine(), nx, nu), want));
        p_free(dx);
        // the factor step returns to the network's vectors
        a.getEngine()->factorStep();
        CHECK(a.getEngine()->getBoundsLayout(&r) == RN_BOUNDS_SHARED && r == 1);
        CHECK(same(held(a.getEngine(), nx, nu), own));
        std::cout << "bounds: " << N << " stages\n";
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "bounds: all checks passed\n";
    return 0;
}
