// The solve certificate through the host classes (rapidnet.h, rn_solve_certificate; Engine::solveCertificate, SmpcController::getSolveCertificate /
// writeSolveCertificate).
//   test_certificate <dir>       two controllers built from <dir>/controllerConfig.json run the same control step into <dir>/plain.json and
//                                <dir>/certificate.json; the second also writes its certificate.  Checked: before the affine terms the record
//                                is refused; the record is that of the C-ABI route, bit for bit, twice; its columns obey their definitions;
//                                the first certificate allocates outside the window of controlAction's leak check, so the next control steps
//                                still return 1 -- and return the controls of the controller that never asked, bit for bit.
//                                tests/test_host_certificate.py reads the two files: the control output is unchanged byte for byte and the
//                                "solveCertificate" entry is a JSON object holding the printed figures.
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
    if (argc < 2) { std::cerr << "usage: test_certificate <dir>\n"; return 2; }
    const string dir = argv[1];
    try {
        SmpcController a(dir + "/controllerConfig.json"), b(dir + "/controllerConfig.json");
        {
            double rec[RN_CERT_COLS];
            CHECK(rn_solve_certificate(b.getEngine()->getContext(), rec) == RN_E_STATE);      // no factor step, no affine terms
            CHECK(rn_solve_certificate(nullptr, rec) == RN_E_ARG);
            bool refused = false;
            try { b.getSolveCertificate(); } catch (const std::runtime_error &) { refused = true; }
            CHECK(refused);
        }
        for (SmpcController *s : {&a, &b}) { start(*s); s->initialiseSmpcController(); }
        std::fstream fa(dir + "/plain.json", std::ios::out | std::ios::trunc), fb(dir + "/certificate.json", std::ios::out | std::ios::trunc);
        CHECK(a.controlAction(fa) == 1 && b.controlAction(fb) == 1);
        CHECK(b.writeSolveCertificate(fb) == 1);
        const std::vector<real_t> r = b.getSolveCertificate();      // (a copy: the second certificate)
        CHECK(r.size() == (size_t)RN_CERT_COLS);
        // the C-ABI route on the same context, host and device form: the same bits
        rn_ctx *x = b.getEngine()->getContext();
        double rec[RN_CERT_COLS], eng[RN_CERT_COLS];
        void *dev = nullptr;
        CHECK(rn_solve_certificate(x, rec) == RN_OK && std::memcmp(rec, r.data(), sizeof rec) == 0);
        b.getEngine()->solveCertificate(eng);
        CHECK(std::memcmp(eng, rec, sizeof rec) == 0);
        CHECK(rn_solve_certificate_device(x, &dev) == RN_OK && dev != nullptr && rn_synchronize(x) == RN_OK);
        CHECK(rn_solve_certificate(x, nullptr) == RN_E_ARG && rn_solve_certificate_device(x, nullptr) == RN_E_ARG);
        // the columns obey their definitions
        for (int c = 0; c < RN_CERT_COLS; c++) CHECK(std::isfinite(r[c]));
        CHECK(r[RN_CERT_GAP] == r[RN_CERT_PRIMAL] - r[RN_CERT_DUAL]);
        CHECK(r[RN_CERT_DUAL] == (r[RN_CERT_COST] + r[RN_CERT_INNER]) - r[RN_CERT_SUPPORT]);
        CHECK(r[RN_CERT_DIST_X] >= 0 && r[RN_CERT_DIST_S] >= 0 && r[RN_CERT_U_EXCESS] >= 0 && r[RN_CERT_NORM_X] >= 0 && r[RN_CERT_NORM_S] >= 0 && r[RN_CERT_XIS_POS] >= 0);
        CHECK(r[RN_CERT_ABS_TERMS] >= std::fabs(r[RN_CERT_DUAL]) * (1 - 1e-12) && (r[RN_CERT_VALID] == 0.0 || r[RN_CERT_VALID] == 1.0));
        CHECK(r[14] == 0.0 && r[15] == 0.0);
        CHECK(r[RN_CERT_NORM_X] <= b.getSmpcConfiguration()->getPenaltyState() * (1 + 1e-9) || r[RN_CERT_VALID] == 0.0);
        // x(y), u(y) are there and read-only
        const size_t nx = b.getSmpcConfiguration()->getNX();
        std::vector<real_t> x0(nx);
        b.getEngine()->getBufferRange(RN_BUF_CERT_X, 0, nx, x0.data());
        for (real_t v : x0) CHECK(std::isfinite(v));
        CHECK(rn_set_range(x, RN_BUF_CERT_X, 0, nx, x0.data()) == RN_E_ARG);
        std::cout << std::setprecision(17) << "record: dual " << r[RN_CERT_DUAL] << " primal " << r[RN_CERT_PRIMAL] << " uExcess " << r[RN_CERT_U_EXCESS] << " valid "
                  << r[RN_CERT_VALID] << "\n";
        // the certificate's buffers were allocated outside the leak check's window, and the solve went on as if nobody had asked
        const uint_t nu = b.getSmpcConfiguration()->getNU();
        std::vector<real_t> ua(nu), ub(nu);
        CHECK(a.controlAction(ua.data()) == 1 && b.controlAction(ub.data()) == 1);
        CHECK(std::memcmp(ua.data(), ub.data(), nu * sizeof(real_t)) == 0);
        CHECK(b.getSolveCertificate().size() == (size_t)RN_CERT_COLS);
        CHECK(b.controlAction(fb) == 1);
    } catch (const std::exception &e) {
        std::cerr << "EXCEPTION: " << e.what() << "\n";
        return 3;
    }
    if (g_failures) { std::cerr << g_failures << " check(s) failed\n"; return 1; }
    std::cout << "solve certificate: all checks passed\n";
    return 0;
}
