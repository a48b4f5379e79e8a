// AddressSanitizer / UBSan run of the host arithmetic behind rn_set_bounds / rn_get_bounds (rapidnet_amd/csrc/bounds.hpp, plain C++): rows and
// strides of every granularity on random shapes -- every (stage, node) of a tree lands in its own row, inside the table --, the validation of
// the caller's values (not finite, lower above upper, the missing half of a pair taken from what the context holds), and the y order of the
// tables against a pack written out here.  Arrays are allocated at their exact sizes, so an index one past a row is the sanitizer's to find.
// Built and run by tests/test_host_bounds_sanitized.py; exit code 0 = clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../../rapidnet_amd/csrc/bounds.hpp"

#define CHECK(c)                                                                                                        \
    do {                                                                                                                \
        if (!(c)) { std::fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); std::exit(2); }                \
    } while (0)

using namespace rn::bounds;

int main() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<double> u(0.1, 1.0);
    int runs = 0;
    CHECK(!known(-1) && !known(3) && rows_of(3, 5, 9) == 0 && rows_of(-1, 5, 9) == 0);
    CHECK(table_fits(1, 12) && table_fits(((size_t)1 << 31) / 16 - 1, 16) && !table_fits((size_t)1 << 31, 1) && !table_fits(((size_t)1 << 31) / 16, 16));
    for (int trial = 0; trial < 300; trial++) {
        const int nx = 1 + rng() % 9, nu = 1 + rng() % 14, ny = 2 * nx + nu, N = 1 + rng() % 12;
        // a tree: nodes per stage, stage of every node
        std::vector<int> stageOf;
        for (int s = 0, width = 1; s < N; s++) { for (int k = 0; k < width; k++) stageOf.push_back(s); width += (int)(rng() % 3); }
        const int nodes = (int)stageOf.size();
        for (int gran = SHARED; gran <= PER_NODE; gran++) {
            CHECK(known(gran));
            const size_t rows = rows_of(gran, N, nodes);
            CHECK(rows == (gran == SHARED ? 1u : (gran == PER_STAGE ? (size_t)N : (size_t)nodes)));
            int ss = -1, sn = -1;
            strides_of(gran, ny, &ss, &sn);
            CHECK((ss == 0 || ss == ny) && (sn == 0 || sn == ny) && !(ss && sn));
            // the caller's arrays at their exact sizes
            std::vector<double> arr[5];
            const double *b[5];
            for (int i = 0; i < 5; i++) {
                arr[i].resize(count_of(i, rows, nx, nu));
                CHECK(arr[i].size() == rows * (size_t)(i < 3 ? nx : nu));
                for (auto &v : arr[i]) v = (i == 0 || i == 3) ? -u(rng) : (i == 2 ? 0.5 * u(rng) : 1.0 + u(rng));
                b[i] = arr[i].data();
            }
            const double *none[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            CHECK(validate(rows, nx, nu, b, none) == OK);
            // the tables in y order, written out here, and every node's row through the strides
            const double big = 1e300;
            std::vector<double> lo(rows * ny), hi(rows * ny);
            for (size_t r = 0; r < rows; r++) {
                for (int t = 0; t < nx; t++) { lo[r * ny + t] = arr[0][r * nx + t]; hi[r * ny + t] = arr[1][r * nx + t]; lo[r * ny + nx + t] = arr[2][r * nx + t]; hi[r * ny + nx + t] = big; }
                for (int t = 0; t < nu; t++) { lo[r * ny + 2 * nx + t] = arr[3][r * nu + t]; hi[r * ny + 2 * nx + t] = arr[4][r * nu + t]; }
            }
            for (int node = 0; node < nodes; node++) {
                const size_t off = table_offset(stageOf[node], node, ss, sn);
                const size_t row = gran == SHARED ? 0 : (gran == PER_STAGE ? (size_t)stageOf[node] : (size_t)node);
                CHECK(off == row * ny && off + ny <= lo.size());
                CHECK(lo[off + nx] == arr[2][row * nx] && hi[off + ny - 1] == arr[4][row * nu + nu - 1]);      // first xsafe, last umax of the row
            }
            std::vector<double> back[5];
            double *out[5];
            for (int i = 0; i < 5; i++) { back[i].assign(arr[i].size(), -7.0); out[i] = back[i].data(); }
            unpack_tables(rows, nx, nu, lo.data(), hi.data(), out);
            for (int i = 0; i < 5; i++) CHECK(back[i] == arr[i]);
            double *only[5] = {nullptr, nullptr, back[2].data(), nullptr, nullptr};
            back[2].assign(arr[2].size(), -7.0);
            unpack_tables(rows, nx, nu, lo.data(), hi.data(), only);
            CHECK(back[2] == arr[2]);
            // bad values, each at the last element of its array
            for (int i = 0; i < 5; i++) {
                for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()}) {
                    const double keep = arr[i].back();
                    arr[i].back() = bad;
                    CHECK(validate(rows, nx, nu, b, none) == NOT_FINITE);
                    const double *one[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
                    one[i] = b[i];
                    CHECK(validate(rows, nx, nu, one, b) == NOT_FINITE);
                    arr[i].back() = keep;
                }
            }
            {   // lower above upper: both given, and either half alone against the context's
                const double keep = arr[0].back();
                arr[0].back() = arr[1].back() + 1.0;
                CHECK(validate(rows, nx, nu, b, none) == XMIN_ABOVE_XMAX);
                const double *lower[5] = {b[0], nullptr, nullptr, nullptr, nullptr}, *upper[5] = {nullptr, b[1], nullptr, nullptr, nullptr};
                CHECK(validate(rows, nx, nu, lower, b) == XMIN_ABOVE_XMAX && validate(rows, nx, nu, upper, b) == XMIN_ABOVE_XMAX);
                bool need[5];
                needed_from_context(lower, need);
                CHECK(!need[0] && need[1] && !need[2] && !need[3] && !need[4]);
                needed_from_context(upper, need);
                CHECK(need[0] && !need[1] && !need[2] && !need[3] && !need[4]);
                arr[0].back() = keep;
                arr[3][0] = arr[4][0] + 0.5;
                CHECK(validate(rows, nx, nu, b, none) == UMIN_ABOVE_UMAX);
                const double *ulow[5] = {nullptr, nullptr, nullptr, b[3], nullptr}, *xs[5] = {nullptr, nullptr, b[2], nullptr, nullptr};
                CHECK(validate(rows, nx, nu, ulow, b) == UMIN_ABOVE_UMAX);
                CHECK(validate(rows, nx, nu, xs, none) == OK);      // the safety volume has no partner
                needed_from_context(ulow, need);
                CHECK(!need[0] && !need[1] && !need[2] && !need[3] && need[4]);
                needed_from_context(xs, need);
                CHECK(!need[0] && !need[1] && !need[2] && !need[3] && !need[4]);
                needed_from_context(b, need);
                CHECK(!need[0] && !need[1] && !need[2] && !need[3] && !need[4]);
                arr[3][0] = arr[4][0];      // equal is allowed
                CHECK(validate(rows, nx, nu, b, none) == OK);
            }
            runs++;
        }
    }
    std::printf("bounds runs %d\n", runs);
    return 0;
}
