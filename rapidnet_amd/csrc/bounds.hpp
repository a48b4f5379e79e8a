// bounds.hpp -- host-only arithmetic of rn_set_bounds / rn_get_bounds (rapidnet_capi.hip): rows and strides of a granularity, validation of the
// caller's values, the y-order of the unscaled tables.  Plain C++ without a GPU call, so that tests/cpp/bounds_sanitize.cpp runs it under
// AddressSanitizer / UBSan on the CPU.
#pragma once
#include <cmath>
#include <cstddef>

namespace rn {
namespace bounds {

enum { SHARED = 0, PER_STAGE = 1, PER_NODE = 2 };      // RN_BOUNDS_* of rapidnet.h
enum { OK = 0, NOT_FINITE = 1, XMIN_ABOVE_XMAX = 2, UMIN_ABOVE_UMAX = 3 };

inline bool known(int gran) { return gran == SHARED || gran == PER_STAGE || gran == PER_NODE; }
// rows of a granularity: 1, the horizon, the context's (local) node count; 0: no such granularity
inline size_t rows_of(int gran, int N, int nodes) { return gran == SHARED ? 1 : (gran == PER_STAGE ? (size_t)N : (gran == PER_NODE ? (size_t)nodes : 0)); }
// element strides by which a kernel finds the row of (stage, node) in a [rows][ny] table: (0, 0), (ny, 0), (0, ny)
inline void strides_of(int gran, int ny, int *strideStage, int *strideNode) {
    *strideStage = gran == PER_STAGE ? ny : 0;
    *strideNode = gran == PER_NODE ? ny : 0;
}
inline size_t table_offset(int stage, int node, int strideStage, int strideNode) { return (size_t)stage * strideStage + (size_t)node * strideNode; }
// the kernels index the tables with 32-bit integers
inline bool table_fits(size_t rows, int ny) { return rows * (size_t)ny < ((size_t)1 << 31); }
inline size_t count_of(int i, size_t rows, int nx, int nu) { return rows * (size_t)(i < 3 ? nx : nu); }      // i: xmin, xmax, xsafe, umin, umax
// every given value finite; lower <= upper pair by pair, the half of a pair that is not given taken from cur (what the context holds; may be
// null where both halves are given or both are missing)
inline int validate(size_t rows, int nx, int nu, const double *const b[5], const double *const cur[5]) {
    for (int i = 0; i < 5; i++) {
        if (!b[i]) continue;
        const size_t n = count_of(i, rows, nx, nu);
        for (size_t k = 0; k < n; k++) if (!std::isfinite(b[i][k])) return NOT_FINITE;
    }
    const int pairs[2][2] = {{0, 1}, {3, 4}};
    for (int q = 0; q < 2; q++) {
        const int iLo = pairs[q][0], iHi = pairs[q][1];
        if (!b[iLo] && !b[iHi]) continue;
        const double *lo = b[iLo] ? b[iLo] : cur[iLo], *hi = b[iHi] ? b[iHi] : cur[iHi];
        if (!lo || !hi) continue;
        const size_t n = count_of(iLo, rows, nx, nu);
        for (size_t k = 0; k < n; k++) if (!(lo[k] <= hi[k])) return q == 0 ? XMIN_ABOVE_XMAX : UMIN_ABOVE_UMAX;
    }
    return OK;
}
// which half of a pair the validation needs from the context: need[i] = true for an array that is missing while its partner is given
inline void needed_from_context(const double *const b[5], bool need[5]) {
    for (int i = 0; i < 5; i++) need[i] = false;
    if (b[0] && !b[1]) need[1] = true;
    if (b[1] && !b[0]) need[0] = true;
    if (b[3] && !b[4]) need[4] = true;
    if (b[4] && !b[3]) need[3] = true;
}
// the tables in y order, lo = xmin|xsafe|umin and hi = xmax|+BIG|umax per row, back to the five arrays (a null output is skipped)
inline void unpack_tables(size_t rows, int nx, int nu, const double *lo, const double *hi, double *const out[5]) {
    const int ny = 2 * nx + nu;
    for (size_t r = 0; r < rows; r++) {
        const double *l = lo + r * ny, *h = hi + r * ny;
        for (int t = 0; t < nx; t++) {
            if (out[0]) out[0][r * nx + t] = l[t];
            if (out[1]) out[1][r * nx + t] = h[t];
            if (out[2]) out[2][r * nx + t] = l[nx + t];
        }
        for (int t = 0; t < nu; t++) {
            if (out[3]) out[3][r * nu + t] = l[2 * nx + t];
            if (out[4]) out[4][r * nu + t] = h[2 * nx + t];
        }
    }
}

}  // namespace bounds
}  // namespace rn
