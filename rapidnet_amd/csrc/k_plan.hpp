// k_plan.hpp -- the plan report: costs and bound violations of the plan a context holds, per stage and per scenario
// (part of the kernel sources of librapidnet_hip.so; k_misc.hip instantiates the one kernel, k_misc.hpp includes this header)
#pragma once
#include "common.hpp"

namespace rn {

// ------------------------------------------------------------------------------------------------------
// rn_plan_report / rn_plan_report_scenarios / rn_plan_report_device (include/rapidnet.h).  The reference's KPIs (SmpcController::updateKpi
// and the get*Kpi read-outs, SmpcController.cu:1819-1859) are closed-loop sums over ONE realised trajectory; this is their predictive
// counterpart over the scenario tree, evaluated on the physical x and u the last sweep stored.  For node i with parent a(i)
// (du_i = u_i - u_a(i), the root against prevU) the node table [nodes][PLAN_COLS] holds, NOT weighted,
//   ECON   alpha_i' u_i                    SMOOTH  du_i' W du_i               STORED  sum_j x_ij
//   SHORT  sum_j max(xs_j - x_ij, 0)       XBOX    sum_j max(xmin_j - x_ij, 0) + max(x_ij - xmax_j, 0)      UBOX  the same for u
//   SHORT_MAX, XBOX_MAX, UBOX_MAX          the largest single entry of the same three violations
// with the bounds row of the unscaled table in force (rn_set_bounds: row = stage * bStrideStage + node * bStrideNode, in elements).
// One kernel, two launches, the phase a run-time argument that is uniform over the grid (as the precision flag: one kernel instead of
// four, k_tree_data's and k_restart_test's idiom):
//   phase 0  node terms.  k_value_terms' shape: a workgroup takes PLAN_TILE nodes; every wave requests the parents of its rows first, then
//            all u / u_parent / alpha / umin / umax values of its rows in one batch, then all x / xmin / xs / xmax; du goes to LDS so that
//            every element of W fetched from L2 serves the whole tile.  Columns beyond 64 lanes are looped, tails are masked.
//   phase 1  folds.  Workgroup k < N folds the contiguous node rows of stage k -- sum columns weighted by p_i, maxima as they are -- into
//            stage[c * N + k]; the further workgroups take one leaf per thread and walk leaf -> root through `parent` (N dependent steps over
//            rows phase 0 has just left in L2): sums and maxima along the path, NOT weighted, STORED the leaf's own.
// Arithmetic: every loaded value is converted to double before the first operation, on fp32 contexts too.  Every sum has an order fixed by
// the tree and the launch shape -- a lane over its strided positions, the wave (wave_sum_f64), the waves in LDS in ascending order -- and
// there are no floating-point atomics: an unchanged context gives the same bits.  Violations are one IEEE subtraction and comparisons
// (contraction off), so the maxima are exact functions of the inputs.
// Sharded contexts: the stages [0, crownStages) are replicated on every rank.  Their node rows are computed everywhere (every leaf's path
// is complete on its rank); their SUM columns of the stage table are written as 0 unless countCrown (rank 0), so that the sum over the
// ranks counts them once; their maxima are the same on every rank.  The stage table is column-major ([PLAN_COLS][N]) so that the sum
// block (the first PLAN_SUMS * N doubles) and the maxima block behind it are each one contiguous payload of a collective.
constexpr int PLAN_ECON = 0, PLAN_SMOOTH = 1, PLAN_STORED = 2, PLAN_SHORT = 3, PLAN_XBOX = 4, PLAN_UBOX = 5, PLAN_SHORT_MAX = 6, PLAN_XBOX_MAX = 7,
              PLAN_UBOX_MAX = 8, PLAN_COLS = 9, PLAN_SUMS = 6;
constexpr int PLAN_THREADS = 128, PLAN_WAVES = PLAN_THREADS / 64, PLAN_TILE = 8, PLAN_RPW = PLAN_TILE / PLAN_WAVES, PLAN_JB = 8;
constexpr int PLAN_RED = PLAN_WAVES * PLAN_COLS > PLAN_WAVES * PLAN_TILE ? PLAN_WAVES * PLAN_COLS : PLAN_WAVES * PLAN_TILE;   // doubles of LDS behind du
struct PlanArgs {
    int phase, f64;
    int nodes, nx, nu, ny, N, leaves;
    const void *x, *u, *alpha, *prevU, *prob, *W, *blo, *bhi;   // of T (f64: doubles, else floats)
    int bStrideStage, bStrideNode;
    const int *parent, *stageOf, *stageCum;
    int crownStages, countCrown;
    double *node;      // [nodes][PLAN_COLS]
    double *stage;     // [PLAN_COLS][N]
    double *leaf;      // [leaves][PLAN_COLS]
    int *leafNode;     // [leaves]
};
inline size_t plan_lds_bytes(int nu) { return ((size_t)nu * PLAN_TILE + PLAN_RED) * sizeof(double); }

__device__ __forceinline__ double plan_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}
// the part of a difference that is above zero: one IEEE subtraction, one comparison
__device__ __forceinline__ double plan_excess(double a, double b) {
#pragma clang fp contract(off)
    const double d = a - b;
    return d > 0.0 ? d : 0.0;
}

template <typename T>
__device__ __forceinline__ void plan_nodes_body(const PlanArgs &a, double *du, double *red) {
#pragma clang fp contract(off)
    const T *const x = static_cast<const T *>(a.x), *const u = static_cast<const T *>(a.u), *const alpha = static_cast<const T *>(a.alpha);
    const T *const prevU = static_cast<const T *>(a.prevU), *const W = static_cast<const T *>(a.W);
    const T *const blo = static_cast<const T *>(a.blo), *const bhi = static_cast<const T *>(a.bhi);
    const int nx = a.nx, nu = a.nu;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tiles = (a.nodes + PLAN_TILE - 1) / PLAN_TILE;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // (uniform trip count: the barriers below)
        const int n0 = tile * PLAN_TILE;
        const int cnt = a.nodes - n0 < PLAN_TILE ? a.nodes - n0 : PLAN_TILE;
        {
            int nd[PLAN_RPW], par[PLAN_RPW];
            size_t brow[PLAN_RPW];
#pragma unroll
            for (int r = 0; r < PLAN_RPW; r++) {      // a row beyond the tile's end reads node n0 and is dropped
                const int n = wave * PLAN_RPW + r;
                nd[r] = n < cnt ? n0 + n : -1;
                const int nc = n < cnt ? n0 + n : n0;
                par[r] = a.parent[nc];
                brow[r] = (size_t)a.stageOf[nc] * a.bStrideStage + (size_t)nc * a.bStrideNode;
            }
            double econ[PLAN_RPW], ubox[PLAN_RPW], umax[PLAN_RPW], stored[PLAN_RPW], shrt[PLAN_RPW], xbox[PLAN_RPW], smax[PLAN_RPW], xmax[PLAN_RPW];
#pragma unroll
            for (int r = 0; r < PLAN_RPW; r++) econ[r] = ubox[r] = umax[r] = stored[r] = shrt[r] = xbox[r] = smax[r] = xmax[r] = 0.0;
            for (int t = lane; t < nu; t += 64) {
                T un[PLAN_RPW], up[PLAN_RPW], al[PLAN_RPW], lo[PLAN_RPW], hi[PLAN_RPW];
#pragma unroll
                for (int r = 0; r < PLAN_RPW; r++) {
                    const int nc = nd[r] >= 0 ? nd[r] : n0;
                    un[r] = u[(size_t)nc * nu + t];
                    up[r] = par[r] < 0 ? prevU[t] : u[(size_t)par[r] * nu + t];
                    al[r] = alpha[(size_t)nc * nu + t];
                    lo[r] = blo[brow[r] + 2 * nx + t];
                    hi[r] = bhi[brow[r] + 2 * nx + t];
                }
#pragma unroll
                for (int r = 0; r < PLAN_RPW; r++) {
                    const bool live = nd[r] >= 0;
                    const double uv = (double)un[r];
                    du[t * PLAN_TILE + wave * PLAN_RPW + r] = live ? uv - (double)up[r] : 0.0;
                    if (live) {
                        econ[r] = fma_rn((double)al[r], uv, econ[r]);
                        const double v1 = plan_excess((double)lo[r], uv), v2 = plan_excess(uv, (double)hi[r]);
                        ubox[r] += v1 + v2;
                        const double m = v1 > v2 ? v1 : v2;
                        umax[r] = m > umax[r] ? m : umax[r];
                    }
                }
            }
            for (int j = lane; j < nx; j += 64) {
                T xv[PLAN_RPW], lo[PLAN_RPW], xs[PLAN_RPW], hi[PLAN_RPW];
#pragma unroll
                for (int r = 0; r < PLAN_RPW; r++) {
                    const int nc = nd[r] >= 0 ? nd[r] : n0;
                    xv[r] = x[(size_t)nc * nx + j];
                    lo[r] = blo[brow[r] + j];
                    xs[r] = blo[brow[r] + nx + j];
                    hi[r] = bhi[brow[r] + j];
                }
#pragma unroll
                for (int r = 0; r < PLAN_RPW; r++) {
                    if (nd[r] >= 0) {
                        const double v = (double)xv[r];
                        stored[r] += v;
                        const double s = plan_excess((double)xs[r], v);
                        shrt[r] += s;
                        smax[r] = s > smax[r] ? s : smax[r];
                        const double v1 = plan_excess((double)lo[r], v), v2 = plan_excess(v, (double)hi[r]);
                        xbox[r] += v1 + v2;
                        const double m = v1 > v2 ? v1 : v2;
                        xmax[r] = m > xmax[r] ? m : xmax[r];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < PLAN_RPW; r++) {      // (every lane takes part: the loops above hold no wave-wide operation)
                const double e = wave_sum_f64(econ[r]), st = wave_sum_f64(stored[r]), sh = wave_sum_f64(shrt[r]), xb = wave_sum_f64(xbox[r]),
                             ub = wave_sum_f64(ubox[r]);
                const double sm = plan_wave_max(smax[r]), xm = plan_wave_max(xmax[r]), um = plan_wave_max(umax[r]);
                if (lane == 0 && nd[r] >= 0) {
                    double *row = a.node + (size_t)nd[r] * PLAN_COLS;
                    row[PLAN_ECON] = e; row[PLAN_STORED] = st; row[PLAN_SHORT] = sh; row[PLAN_XBOX] = xb; row[PLAN_UBOX] = ub;
                    row[PLAN_SHORT_MAX] = sm; row[PLAN_XBOX_MAX] = xm; row[PLAN_UBOX_MAX] = um;
                }
            }
        }
        __syncthreads();
        // du' W du of every node of the tile: thread t holds row t of W du for the whole tile, PLAN_JB columns of W requested together
        double q[PLAN_TILE];
#pragma unroll
        for (int n = 0; n < PLAN_TILE; n++) q[n] = 0.0;
        for (int t = threadIdx.x; t < nu; t += PLAN_THREADS) {
            double wd[PLAN_TILE];
#pragma unroll
            for (int n = 0; n < PLAN_TILE; n++) wd[n] = 0.0;
            for (int j0 = 0; j0 < nu; j0 += PLAN_JB) {
                T wv[PLAN_JB];
#pragma unroll
                for (int jj = 0; jj < PLAN_JB; jj++) wv[jj] = W[t + (size_t)(j0 + jj < nu ? j0 + jj : nu - 1) * nu];
#pragma unroll
                for (int jj = 0; jj < PLAN_JB; jj++) {
                    if (j0 + jj < nu) {
                        const double w = (double)wv[jj];
                        const double *dj = du + (size_t)(j0 + jj) * PLAN_TILE;
#pragma unroll
                        for (int n = 0; n < PLAN_TILE; n++) wd[n] = fma_rn(w, dj[n], wd[n]);
                    }
                }
            }
#pragma unroll
            for (int n = 0; n < PLAN_TILE; n++) q[n] = fma_rn(du[t * PLAN_TILE + n], wd[n], q[n]);
        }
#pragma unroll
        for (int n = 0; n < PLAN_TILE; n++) {
            const double s = wave_sum_f64(q[n]);
            if (lane == 0) red[wave * PLAN_TILE + n] = s;
        }
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            double s = red[threadIdx.x];
            for (int w = 1; w < PLAN_WAVES; w++) s += red[w * PLAN_TILE + threadIdx.x];
            a.node[(size_t)(n0 + threadIdx.x) * PLAN_COLS + PLAN_SMOOTH] = s;
        }
        __syncthreads();      // du and red belong to the next tile from here on
    }
}

template <typename T>
__device__ __forceinline__ void plan_folds_body(const PlanArgs &a, double *red) {
#pragma clang fp contract(off)
    const T *const prob = static_cast<const T *>(a.prob);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if ((int)blockIdx.x < a.N) {      // one stage: its node rows are contiguous
        const int k = blockIdx.x, s0 = a.stageCum[k], s1 = a.stageCum[k + 1];
        double acc[PLAN_COLS];
#pragma unroll
        for (int c = 0; c < PLAN_COLS; c++) acc[c] = 0.0;
        for (int i = s0 + threadIdx.x; i < s1; i += PLAN_THREADS) {
            const double p = (double)prob[i];
            const double *row = a.node + (size_t)i * PLAN_COLS;
#pragma unroll
            for (int c = 0; c < PLAN_SUMS; c++) acc[c] = fma_rn(p, row[c], acc[c]);
#pragma unroll
            for (int c = PLAN_SUMS; c < PLAN_COLS; c++) acc[c] = row[c] > acc[c] ? row[c] : acc[c];
        }
#pragma unroll
        for (int c = 0; c < PLAN_COLS; c++) {
            const double v = c < PLAN_SUMS ? wave_sum_f64(acc[c]) : plan_wave_max(acc[c]);
            if (lane == 0) red[wave * PLAN_COLS + c] = v;
        }
        __syncthreads();
        if (threadIdx.x < PLAN_COLS) {
            const int c = threadIdx.x;
            double v = red[c];
            for (int w = 1; w < PLAN_WAVES; w++) { const double o = red[w * PLAN_COLS + c]; v = c < PLAN_SUMS ? v + o : (o > v ? o : v); }
            const bool counted = a.countCrown || k >= a.crownStages;
            a.stage[(size_t)c * a.N + k] = (c < PLAN_SUMS && !counted) ? 0.0 : v;
        }
        return;
    }
    const int l = ((int)blockIdx.x - a.N) * PLAN_THREADS + threadIdx.x;      // one leaf per thread, leaf -> root
    if (l >= a.leaves) return;
    const int leafNode = a.stageCum[a.N - 1] + l;
    double acc[PLAN_COLS];
#pragma unroll
    for (int c = 0; c < PLAN_COLS; c++) acc[c] = 0.0;
    const double own = a.node[(size_t)leafNode * PLAN_COLS + PLAN_STORED];
    int i = leafNode;
    for (int step = 0; step < a.N && i >= 0; step++) {      // (a path has at most N nodes: a bad parent table cannot keep the loop alive)
        const double *row = a.node + (size_t)i * PLAN_COLS;
#pragma unroll
        for (int c = 0; c < PLAN_SUMS; c++) acc[c] += row[c];
#pragma unroll
        for (int c = PLAN_SUMS; c < PLAN_COLS; c++) acc[c] = row[c] > acc[c] ? row[c] : acc[c];
        i = a.parent[i];
    }
    acc[PLAN_STORED] = own;
    double *out = a.leaf + (size_t)l * PLAN_COLS;
#pragma unroll
    for (int c = 0; c < PLAN_COLS; c++) out[c] = acc[c];
    a.leafNode[l] = leafNode;
}

template <int PLAIN = 0>   // (a template so that one translation unit owns its code: instantiations/*.inc)
__global__ void __launch_bounds__(PLAN_THREADS) k_plan_report(PlanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char plan_smem[];
    double *du = reinterpret_cast<double *>(plan_smem);      // [nu][PLAN_TILE]: the tile's values of one column are contiguous
    double *red = du + (size_t)a.nu * PLAN_TILE;             // PLAN_RED doubles
    if (a.phase == 0) { if (a.f64) plan_nodes_body<double>(a, du, red); else plan_nodes_body<float>(a, du, red); }
    else { if (a.f64) plan_folds_body<double>(a, red); else plan_folds_body<float>(a, red); }
}

// ------------------------------------------------------------------------------------------------------
// rn_plan_quantiles / rn_plan_quantiles_device / rn_plan_paths (include/rapidnet.h): what the plan looks like across the tree -- weighted
// quantiles of every component of x or u per stage, and the rows along every leaf's path.  The reference has no counterpart.  One kernel,
// the phase a run-time argument uniform over the grid, the element type of `src` and `prob` a flag (k_plan_report's idiom):
//   phase 0  quantiles.  Workgroup (stage k, component c) loads the stage's contiguous rows of that component as (double value, node index)
//            into LDS, padded to the next power of two with (+inf, INT_MAX); a node with p <= 0 is keyed +inf, so it sorts behind every node
//            that can occur.  A bitonic network orders by (value, index).  Wave 0 then walks the `live` leading entries in chunks of 64:
//            every lane fetches the p of its entry, and the sum runs through the lanes ONE AFTER THE OTHER (c_j = c_{j-1} + p_(j), fp64):
//            once for c_m, once more to pick, for every level, the first j with c_j >= q * c_m (one product, nothing to contract).  The
//            order of the additions is part of the definition: any call on any rank gives the same bits.  Levels arrive ascending (q) with
//            the caller's position of each (slot).  Values that are not finite are counted into *flag, and their (stage, component) reads
//            NaN at every level.
//   phase 1  paths.  Workgroup l walks leaf l's ancestors into LDS once, then copies the N rows, two elements per thread where dim and the
//            row stride are even (16-byte stores): paths[l][k][c]; leafNode[l] = the leaf.
//   phase 2  pack (sharded contexts).  Local rows, widened, and the local p go to row gmap[i] of a zeroed [full nodes][dim + 1] table; the
//            replicated crown rows [0, crownNodes) only where writeCrown (rank 0), so that a sum over the ranks holds every entry once.
//            Phases 0 and 1 then read the summed table (f64 = 1, rowStride = probStride = dim + 1, prob = table + dim).
constexpr int BANDS_THREADS = 256, BANDS_WIDTH = 4096, BANDS_LEVELS = 16;
struct BandsArgs {
    int phase, f64;
    int nodes, dim, N, leaves, nq;
    int rowStride, probStride;        // in elements
    const void *src, *prob;           // of T (f64: doubles, else floats)
    const int *parent, *stageCum;
    double q[BANDS_LEVELS];           // ascending
    int slot[BANDS_LEVELS];           // the caller's position of q[l]
    double *quant;                    // [N][dim][nq]
    double *paths;                    // [leaves][N][dim]
    int *leafNode;                    // [leaves]
    int *flag;                        // values that are not finite
    const int *gmap;                  // phase 2: full-tree row of every local node
    int crownNodes, writeCrown;
    double *table;                    // phase 2: [full nodes][dim + 1]
};
static_assert(BANDS_WIDTH * (sizeof(double) + sizeof(int)) == 48 * 1024, "the sort's keys fill 48 KB of LDS");

__device__ __forceinline__ bool bands_less(double va, int ia, double vb, int ib) { return va < vb || (va == vb && ia < ib); }

template <typename T>
__device__ __forceinline__ void bands_quantiles_body(const BandsArgs &a, double *val, int *idx, int *cnt) {
#pragma clang fp contract(off)
    const T *const src = static_cast<const T *>(a.src), *const prob = static_cast<const T *>(a.prob);
    const int k = (int)blockIdx.x / a.dim, c = (int)blockIdx.x - k * a.dim;
    const int s0 = a.stageCum[k], m = a.stageCum[k + 1] - s0;
    if (m < 1 || m > BANDS_WIDTH) return;      // (refused on the host; uniform over the workgroup)
    int P = 1;
    while (P < m) P <<= 1;
    const double inf = __builtin_huge_val();
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    int live = 0, bad = 0;
    for (int i = threadIdx.x; i < P; i += BANDS_THREADS) {
        double v = inf;
        int id = 0x7fffffff;
        if (i < m) {
            id = s0 + i;
            const double x = (double)src[(size_t)id * a.rowStride + c];
            const double p = (double)prob[(size_t)id * a.probStride];
            if (!(fabs(x) < inf)) bad++;
            if (p > 0.0) { v = x; live++; }
        }
        val[i] = v; idx[i] = id;
    }
    if (live) atomicAdd(&cnt[0], live);
    if (bad) atomicAdd(&cnt[1], bad);
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {      // (uniform trip counts: the barriers)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += BANDS_THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const double vl = val[lo], vh = val[hi];
                const int il = idx[lo], ih = idx[hi];
                const bool swap = (lo & kk) == 0 ? bands_less(vh, ih, vl, il) : bands_less(vl, il, vh, ih);
                if (swap) { val[lo] = vh; idx[lo] = ih; val[hi] = vl; idx[hi] = il; }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    live = cnt[0];
    double *out = a.quant + ((size_t)k * a.dim + c) * a.nq;
    if (cnt[1] > 0 || live == 0) {
        if (lane < a.nq) out[lane] = __builtin_nan("");
        if (lane == 0 && cnt[1] > 0) atomicAdd(a.flag, cnt[1]);
        return;
    }
    // c_m: the p of a chunk's entries fetched together, added lane by lane (a lane beyond `live` adds +0.0, which changes no bit)
    double tot = 0.0;
    for (int base = 0; base < live; base += 64) {
        const int j = base + lane;
        const double pj = j < live ? (double)prob[(size_t)idx[j] * a.probStride] : 0.0;
#pragma unroll
        for (int t = 0; t < 64; t++) tot += __shfl(pj, t);
    }
    int l = 0;
    double cum = 0.0;
    for (int base = 0; base < live && l < a.nq; base += 64) {
        const int j = base + lane;
        const double pj = j < live ? (double)prob[(size_t)idx[j] * a.probStride] : 0.0;
        double mine = 0.0;
#pragma unroll
        for (int t = 0; t < 64; t++) { cum += __shfl(pj, t); if (lane == t) mine = cum; }
        while (l < a.nq) {      // (l is uniform over the wave)
            const double thr = a.q[l] * tot;
            const unsigned long long hit = __ballot(j < live && mine >= thr);
            if (!hit) break;
            if (lane == 0) out[a.slot[l]] = val[base + __ffsll(hit) - 1];
            l++;
        }
    }
}

template <typename T, typename T2>
__device__ __forceinline__ void bands_paths_body(const BandsArgs &a, int *anc) {
    const T *const src = static_cast<const T *>(a.src);
    const int l = blockIdx.x, N = a.N < BANDS_WIDTH ? a.N : BANDS_WIDTH, dim = a.dim;
    const int leafNode = a.stageCum[a.N - 1] + l;
    if (threadIdx.x == 0) {
        int i = leafNode;
        for (int k = N - 1; k >= 0; k--) {      // (N steps at most, and an index that stays in range whatever `parent` holds)
            anc[k] = i;
            i = a.parent[i];
            if (i < 0 || i >= a.nodes) i = 0;
        }
        a.leafNode[l] = leafNode;
    }
    __syncthreads();
    double *out = a.paths + (size_t)l * N * dim;
    const int total = N * dim;
    if (((dim | a.rowStride) & 1) == 0) {
        for (int e = threadIdx.x * 2; e < total; e += BANDS_THREADS * 2) {
            const int k = e / dim, c = e - k * dim;
            const T2 v = *reinterpret_cast<const T2 *>(src + (size_t)anc[k] * a.rowStride + c);
            *reinterpret_cast<double2 *>(out + e) = make_double2((double)v.x, (double)v.y);
        }
    } else {
        for (int e = threadIdx.x; e < total; e += BANDS_THREADS) {
            const int k = e / dim, c = e - k * dim;
            out[e] = (double)src[(size_t)anc[k] * a.rowStride + c];
        }
    }
}

template <typename T>
__device__ __forceinline__ void bands_pack_body(const BandsArgs &a) {
    const T *const src = static_cast<const T *>(a.src), *const prob = static_cast<const T *>(a.prob);
    const int w = a.dim + 1;
    const long long n = (long long)a.nodes * w;
    for (long long i = (long long)blockIdx.x * BANDS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * BANDS_THREADS) {
        const int node = (int)(i / w), c = (int)(i - (long long)node * w);
        if (node < a.crownNodes && !a.writeCrown) continue;
        a.table[(size_t)a.gmap[node] * w + c] = c < a.dim ? (double)src[(size_t)node * a.rowStride + c] : (double)prob[(size_t)node * a.probStride];
    }
}

template <int PLAIN = 0>   // (a template so that one translation unit owns its code: instantiations/*.inc)
__global__ void __launch_bounds__(BANDS_THREADS) k_plan_bands(BandsArgs a) {
    __shared__ double val[BANDS_WIDTH];
    __shared__ int idx[BANDS_WIDTH];
    __shared__ int cnt[2];
    if (a.phase == 0) { if (a.f64) bands_quantiles_body<double>(a, val, idx, cnt); else bands_quantiles_body<float>(a, val, idx, cnt); }
    else if (a.phase == 1) { if (a.f64) bands_paths_body<double, double2>(a, idx); else bands_paths_body<float, float2>(a, idx); }
    else { if (a.f64) bands_pack_body<double>(a); else bands_pack_body<float>(a); }
}

// ------------------------------------------------------------------------------------------------------
// rn_solve_certificate / rn_solve_certificate_device (include/rapidnet.h; DESIGN.md "the solve certificate"): the value of the dual function at
// the multiplier y = (xi_b, xi_s, psi) a context would warm-start from, and the penalised primal value of the minimiser z(y) of the Lagrangian
// there.  The reference has no counterpart (its computeValueFbe, SmpcController.cu:1066-1146, is the envelope of the FBE line search).  The host
// runs one sweep at y into buffers of the certificate's own and k_plan_report's node phase on its x(y), u(y); this kernel then makes ONE flat
// pass over y, Hz(y) = (F x, G u) and the bounds, and one pass over the node rows:
//   element (node i, column c), k = sqrt(p_i) d_c in the context's type, lo = k blo_c, hi = k bhi_c as the dual update rebuilds them (k_dual_fused,
//   regen: the prox and the certificate see the same bits), everything below in double:
//     INNER    y h                       SUPPORT  box and psi columns max(y lo, y hi), safety columns y lo     (and the |.| of both)
//     DIST2_X  (h - clamp(h, lo, hi))^2  DIST2_S  max(lo - h, 0)^2       NORM2_X, NORM2_S  y^2 of the two xi halves       XIS_POS  max(y, 0), safety
//   node i, row = k_plan_report's node table: ECON p_i row[ECON], SMOOTH p_i row[SMOOTH], COST_ABS the |.| of both, U_EXCESS max row[UBOX_MAX].
// COST's summation order is therefore: a node's alpha' u and du' W du as k_plan_report's node phase sums them, the nodes as below.
// 16 bytes per lane and stream with a scalar tail.  Every product is formed and summed in double whatever the element type is, in a fixed
// order -- a lane over its grid-stride positions, the wave (wave_sum_f64), the workgroup's waves in LDS, the workgroups' partials by the
// workgroup that arrives last (agent-scope release -> ticket -> acquire: k_restart_test's reduction) -- and there are no floating-point atomics:
// two calls give the same bits.  Sharded contexts: the leading crownElems elements / crownNodes rows are replicated on every rank and enter the
// sums on ONE rank (countCrown); the maxima are the same everywhere.  The host sums the sum block over the ranks and takes the maxima's MAX, then
// phase 1 derives the record; an unsharded context's last arriver derives it in the same launch (finish).
// The element type arrives as a flag and not as a template parameter (k_restart_test's idiom); the branch is uniform over the grid.
constexpr int CERT_INNER = 0, CERT_INNER_ABS = 1, CERT_SUPPORT = 2, CERT_SUPPORT_ABS = 3, CERT_DIST2_X = 4, CERT_DIST2_S = 5, CERT_NORM2_X = 6, CERT_NORM2_S = 7,
              CERT_ECON = 8, CERT_SMOOTH = 9, CERT_COST_ABS = 10, CERT_COUNT = 11, CERT_SUMS = 12, CERT_UEXC = 12, CERT_XISPOS = 13, CERT_PART = 14;
constexpr int CERT_REC = 16;       // columns of the record: RN_CERT_COLS
struct CertArgs {
    int phase, f64;
    const void *y, *hz;                               // [node][ny] of T
    const void *sqrtp, *dy, *blo, *bhi, *prob;        // of T
    const int *stageOf;
    int bStrideStage, bStrideNode;
    int nx, ny, nodes;
    long long n, crownElems;
    int crownNodes, countCrown;
    const double *node;           // [nodes][PLAN_COLS]: k_plan_report's node phase on x(y), u(y)
    double gammaX, gammaS;
    double count;                 // entries of one xi half this rank counts
    double *partials;             // [gridDim.x][CERT_PART]
    unsigned int *ticket;         // arrival counter: the host zeroes it on the stream in front of every launch
    double *sums;                 // [CERT_PART]: the sum block, the two maxima behind it
    double *rec;                  // [CERT_REC]
    int finish;                   // phase 0: the last arriver derives the record as well
};
template <typename T>
__device__ __forceinline__ void cert_elem(const CertArgs &a, T yv, T hv, int node, int c, bool counted, double *s, double &xisPos) {
#pragma clang fp contract(off)
    const T *const sqrtp = static_cast<const T *>(a.sqrtp), *const dy = static_cast<const T *>(a.dy);
    const T *const blo = static_cast<const T *>(a.blo), *const bhi = static_cast<const T *>(a.bhi);
    const int stg = a.stageOf[node], bc = stg * a.bStrideStage + node * a.bStrideNode + c;
    const bool box = c < a.nx, safe = !box && c < 2 * a.nx;
    const T k = sqrtp[node] * dy[(size_t)stg * a.ny + c];
    const T loT = k * blo[bc], hiT = safe ? (T)0 : k * bhi[bc];      // (the safety half has no upper bound)
    const double lo = (double)loT, hi = (double)hiT, y = (double)yv, h = (double)hv;
    const double ti = y * h, tl = y * lo, th = y * hi;
    const double ts = safe ? tl : (tl > th ? tl : th);
    double d = 0.0;
    if (box) d = h < lo ? lo - h : (h > hi ? h - hi : 0.0);
    else if (safe) d = h < lo ? lo - h : 0.0;
    const double d2 = d * d, y2 = y * y;
    if (counted) {
        s[CERT_INNER] += ti; s[CERT_INNER_ABS] += fabs(ti); s[CERT_SUPPORT] += ts; s[CERT_SUPPORT_ABS] += fabs(ts);
        s[CERT_DIST2_X] += box ? d2 : 0.0; s[CERT_DIST2_S] += safe ? d2 : 0.0;
        s[CERT_NORM2_X] += box ? y2 : 0.0; s[CERT_NORM2_S] += safe ? y2 : 0.0;
    }
    if (safe && y > xisPos) xisPos = y;
}
// a lane's sums over its grid-stride positions of the flat range and of the node rows
template <typename T>
__device__ __forceinline__ void cert_lane_sums(const CertArgs &a, double *s, double &uExc, double &xisPos) {
#pragma clang fp contract(off)
    typedef typename VecOf<T>::type VT;
    constexpr int VN = VecOf<T>::N;
    const T *const ay = static_cast<const T *>(a.y), *const ah = static_cast<const T *>(a.hz), *const prob = static_cast<const T *>(a.prob);
    const long long stride = (long long)gridDim.x * ELT_THREADS, gid = (long long)blockIdx.x * ELT_THREADS + threadIdx.x;
    const long long nvec = a.n / VN;
    for (long long iv = gid; iv < nvec; iv += stride) {
        const VT y = reinterpret_cast<const VT *>(ay)[iv], h = reinterpret_cast<const VT *>(ah)[iv];
        int node = (int)(iv * VN / a.ny), c = (int)(iv * VN - (long long)node * a.ny);
#pragma unroll
        for (int e = 0; e < VN; e++) {
            cert_elem<T>(a, y[e], h[e], node, c, a.countCrown || iv * VN + e >= a.crownElems, s, xisPos);
            if (++c == a.ny) { c = 0; node++; }
        }
    }
    for (long long i = nvec * VN + gid; i < a.n; i += stride) {   // at most VN-1 tail elements
        const int node = (int)(i / a.ny), c = (int)(i - (long long)node * a.ny);
        cert_elem<T>(a, ay[i], ah[i], node, c, a.countCrown || i >= a.crownElems, s, xisPos);
    }
    for (long long i = gid; i < a.nodes; i += stride) {
        const double *row = a.node + (size_t)i * PLAN_COLS;
        const double p = (double)prob[i], te = p * row[PLAN_ECON], tq = p * row[PLAN_SMOOTH];
        if (a.countCrown || i >= a.crownNodes) { s[CERT_ECON] += te; s[CERT_SMOOTH] += tq; s[CERT_COST_ABS] += fabs(te) + fabs(tq); }
        uExc = row[PLAN_UBOX_MAX] > uExc ? row[PLAN_UBOX_MAX] : uExc;
    }
}
// the record from the (all-rank) sums and maxima: one thread
__device__ __forceinline__ void cert_finish(const CertArgs &a) {
#pragma clang fp contract(off)
    const double *s = a.sums;
    const double cost = s[CERT_ECON] + s[CERT_SMOOTH], inner = s[CERT_INNER], support = s[CERT_SUPPORT];
    const double dual = (cost + inner) - support;
    const double distX = sqrt(s[CERT_DIST2_X]), distS = sqrt(s[CERT_DIST2_S]), normX = sqrt(s[CERT_NORM2_X]), normS = sqrt(s[CERT_NORM2_S]);
    const double primal = (cost + a.gammaX * distX) + a.gammaS * distS;
    const double u = 1.1102230246251565e-16;      // 2^-53
    const double slack = 1.0 + 4.0 * u * sqrt(s[CERT_COUNT]);
    const bool valid = normX <= a.gammaX * slack && normS <= a.gammaS * slack && s[CERT_XISPOS] <= u * normS;
    double *r = a.rec;
    r[0] = dual; r[1] = primal; r[2] = primal - dual; r[3] = cost; r[4] = inner; r[5] = support; r[6] = distX; r[7] = distS;
    r[8] = s[CERT_UEXC]; r[9] = normX; r[10] = normS; r[11] = s[CERT_XISPOS];
    r[12] = (s[CERT_COST_ABS] + s[CERT_INNER_ABS]) + s[CERT_SUPPORT_ABS];
    r[13] = valid ? 1.0 : 0.0; r[14] = 0.0; r[15] = 0.0;
}
template <int PLAIN = 0>   // (a template so that one translation unit owns its code: instantiations/*.inc)
__global__ void __launch_bounds__(ELT_THREADS) k_certificate(CertArgs a) {
    constexpr int NW = ELT_THREADS / 64, FLAG = NW * CERT_PART;
    __shared__ double sh[NW * CERT_PART + 1];   // the waves' sums and maxima; sh[FLAG] != 0: this workgroup arrived last
    if (a.phase == 1) { if (blockIdx.x == 0 && threadIdx.x == 0) cert_finish(a); return; }
    double s[CERT_PART];
#pragma unroll
    for (int k = 0; k < CERT_PART; k++) s[k] = 0.0;
    if (a.f64) cert_lane_sums<double>(a, s, s[CERT_UEXC], s[CERT_XISPOS]); else cert_lane_sums<float>(a, s, s[CERT_UEXC], s[CERT_XISPOS]);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < CERT_PART; k++) {
        const double v = k < CERT_SUMS ? wave_sum_f64(s[k]) : plan_wave_max(s[k]);
        if (lane == 0) sh[wave * CERT_PART + k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *out = a.partials + (size_t)blockIdx.x * CERT_PART;
        for (int k = 0; k < CERT_PART; k++) {
            double t = sh[k];
            for (int v = 1; v < NW; v++) { const double o = sh[v * CERT_PART + k]; t = k < CERT_SUMS ? t + o : (o > t ? o : t); }
            out[k] = t;
        }
        // publish the partial, then draw a ticket: the last arriver folds (release -> ticket -> acquire, as k_restart_test)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        sh[FLAG] = last ? 1.0 : 0.0;
    }
    __syncthreads();
    if (sh[FLAG] == 0.0) return;
#pragma unroll
    for (int k = 0; k < CERT_PART; k++) s[k] = 0.0;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += ELT_THREADS) {   // ascending per lane: a fixed order
        const double *q = a.partials + (size_t)b * CERT_PART;
#pragma unroll
        for (int k = 0; k < CERT_SUMS; k++) s[k] += q[k];
#pragma unroll
        for (int k = CERT_SUMS; k < CERT_PART; k++) s[k] = q[k] > s[k] ? q[k] : s[k];
    }
    __syncthreads();      // (sh is read above by thread 0 only, before the barrier in front of the flag; written again from here)
#pragma unroll
    for (int k = 0; k < CERT_PART; k++) {
        const double v = k < CERT_SUMS ? wave_sum_f64(s[k]) : plan_wave_max(s[k]);
        if (lane == 0) sh[wave * CERT_PART + k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < CERT_PART; k++) {
            double t = sh[k];
            for (int v = 1; v < NW; v++) { const double o = sh[v * CERT_PART + k]; t = k < CERT_SUMS ? t + o : (o > t ? o : t); }
            a.sums[k] = t;
        }
        a.sums[CERT_COUNT] = a.count;
        if (a.finish) cert_finish(a);
    }
}

}  // namespace rn
