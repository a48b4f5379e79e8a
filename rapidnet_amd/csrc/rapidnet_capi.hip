// rapidnet_capi.hip -- implementation of include/rapidnet.h (librapidnet_hip.so).
//
// Host side of the boundary: owns every device allocation, drives the kernels of kernels.hpp on one HIP
// stream, never synchronises inside the APG loop.  No torch types, no cuBLAS/rocBLAS: the only external
// libraries are the HIP runtime and (lazily, for multi-GPU) RCCL.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <memory>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rapidnet.h"
#include "../../include/rapidnet_debug.h"
#include "kernels.hpp"
#include "fbe_kernels.hpp"
#include "partition.hpp"
#include "bounds.hpp"
#include "bands_host.hpp"
#include "shift_map.hpp"

// Every kernel this file launches is compiled in ONE of the units k_stream.hip ... k_fbe.hip; here the instantiations are only declared.
// (RN_NO_EXTERN_TEMPLATES: the one-unit build tools/gen_instantiations.py uses to find out what is launched.)
#ifndef RN_NO_EXTERN_TEMPLATES
#define RN_LINKAGE extern
#include "instantiations/stream.inc"
#include "instantiations/walks.inc"
#include "instantiations/slab.inc"
#include "instantiations/dual.inc"
#include "instantiations/misc.inc"
#include "instantiations/fbe.inc"
#undef RN_LINKAGE
#endif

#ifndef RN_FIXUP_BLOCKS
#define RN_FIXUP_BLOCKS 64
#endif
#ifndef RN_FOLD_CROWN_DOWN
#define RN_FOLD_CROWN_DOWN 1
#endif
#ifndef RN_OPT_LOCAL_MIN
#define RN_OPT_LOCAL_MIN 16   // shortest rn_apg_iterate batch that takes the optimistic single-GPU path
#define RN_LIP_CHECK_EVERY 20     // rn_estimate_lipschitz: iterations between two looks at the residual when the caller names none
#define RN_LIP_RULE_ITERATIONS 40 // rn_set_step_rule: applications per estimate when the caller names none
#define RN_STOP_CHECK_EVERY 20   // rn_apg_solve / rn_set_stop_tolerance: iterations per batch when the caller names none
#endif
#ifndef RN_OPT_BACKOFF
#define RN_OPT_BACKOFF 8      // exact batches after an optimistic batch had to be replayed
#endif
#ifndef RN_DUAL_REGEN
#define RN_DUAL_REGEN 1
#endif
#ifndef RN_DOWN_PF_UNSC
#define RN_DOWN_PF_UNSC 12   // stages per batch of loads of the unscaled walk (24: one batch, 212 registers, two waves per SIMD: 16.6 -> 16.8 us)
#endif
#ifndef RN_FOLD_ROOT
#define RN_FOLD_ROOT 1
#endif
#ifndef RN_DUAL_STAGE
#define RN_DUAL_STAGE 1   // 1: stage-tiled main pass of the fused dual update (k_dual_stage) whenever the shape allows it
#endif
#ifndef RN_DUAL_STAGE_MAX_BLOCKS
#define RN_DUAL_STAGE_MAX_BLOCKS 16384
#endif
#ifndef RN_GEMM_SLAB
#define RN_GEMM_SLAB 1   // 1: slab kernels (k_gemm_slab / fused k_gemm_vlv); 0: always the tile kernel k_gemm_shared
#endif
#ifndef RN_GEMM_KS
#define RN_GEMM_KS 3   // k-steps whose operands a wave requests at once in k_gemm_shared (tuning knob)
#endif

namespace rn {

#define RN_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            char b_[512];                                                                              \
            snprintf(b_, sizeof b_, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #call); \
            err = b_;                                                                                  \
            return RN_E_HIP;                                                                           \
        }                                                                                              \
    } while (0)

#define RN_CHECK(cond, code, msg)  \
    do {                           \
        if (!(cond)) {             \
            err = (msg);           \
            return (code);         \
        }                          \
    } while (0)

// ---- minimal RCCL binding, resolved at run time (so single-GPU users never load it) ---------------------
struct UniqueId128 { char b[128]; };
struct NcclApi {
    void *h = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommCount)(void *, int *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*InitRank)(void **, int, struct UniqueId128, int) = nullptr;
    int (*GetAsyncError)(void *, int *) = nullptr;
    int (*CommAbort)(void *) = nullptr;
    std::string path;   // file the bound image was loaded from (rn_comm_library)
    bool load() {
        if (h) return true;
        // an RCCL image that is already part of the process (PyTorch links one under the soname librccl.so.1) is reused:
        // RTLD_NOLOAD only returns a handle to a loaded object; a second image of the library is never mapped
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD); if (h) break; }
        if (!h) for (const char *n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
        if (!h) return false;
        GetUniqueId = (int (*)(void *))dlsym(h, "ncclGetUniqueId");
        AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(h, "ncclAllReduce");
        CommDestroy = (int (*)(void *))dlsym(h, "ncclCommDestroy");
        CommCount = (int (*)(void *, int *))dlsym(h, "ncclCommCount");
        GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
        InitRank = (int (*)(void **, int, UniqueId128, int))dlsym(h, "ncclCommInitRank");
        GetAsyncError = (int (*)(void *, int *))dlsym(h, "ncclCommGetAsyncError");
        CommAbort = (int (*)(void *))dlsym(h, "ncclCommAbort");
        Dl_info info;
        if (AllReduce && dladdr((void *)AllReduce, &info) && info.dli_fname) path = info.dli_fname;
        return GetUniqueId && AllReduce && InitRank;
    }
};
static NcclApi g_nccl;
constexpr int NCCL_IN_PROGRESS = 7;   // ncclInProgress
static std::atomic<long> g_guardContexts{0}, g_guardBadBytes{0};   // guard mode: contexts checked when they were destroyed / red-zone bytes found overwritten
static std::atomic<long> g_liveContexts{0};   // contexts of this process (rn_device_memory_info: a device-wide figure is only the caller's own while this is 1)

struct CtxBase {
    std::string err;
    virtual ~CtxBase() {}
    virtual int factor_step(const rn_system *) = 0;
    virtual int set_tree_errors(const double *, const double *) = 0;
    virtual int set_uncertainty(int, int, double) = 0;
    virtual int update_state_control(const double *, const double *, const double *) = 0;
    virtual int eliminate(const double *, const double *) = 0;
    virtual int set_parameters(double, double, double) = 0;
    virtual int apg_reset() = 0;
    virtual int apg_iterate(int, double *) = 0;
    virtual int apg_run(int, double *) = 0;
    virtual int apg_solve(int, double, int, int *, double *) = 0;
    virtual int set_stop_tolerance(double, int) = 0;
    virtual int get_stop_tolerance(double *, int *) = 0;
    virtual int last_solve(long *) = 0;
    virtual int set_restart(int) = 0;
    virtual int get_restart(int *) = 0;
    virtual int restart_info(long *, double *) = 0;
    virtual int debug_restart_test(double *) = 0;
    virtual int control_action(const double *, const double *, const double *, const double *, const double *, int, int,
                               double *) = 0;
    virtual int extrapolate(double) = 0;
    virtual int solve_step() = 0;
    virtual int prox() = 0;
    virtual int residual() = 0;
    virtual int dual_update() = 0;
    virtual int primal_infeasibility(double *) = 0;
    virtual int prox_distances(double *, double *) = 0;
    virtual size_t buffer_size(int) const = 0;
    virtual int get(int, double *, size_t) = 0;
    virtual int set(int, const double *, size_t) = 0;
    virtual int get_operator(int, int, double *, size_t) = 0;
    virtual int device_pointer(int, void **, size_t *, int *) = 0;
    virtual int get_range(int, size_t, size_t, double *) = 0;
    virtual int set_range(int, size_t, size_t, const double *) = 0;
    virtual int profile_enable(int) = 0;
    virtual int profile_reset() = 0;
    virtual int profile_read(double *, long *) = 0;
    virtual int algorithmic_bytes(double *, double *) const = 0;
    virtual int stream_live(long long *) = 0;
    virtual int stream_units(long long *) = 0;
    virtual int stream_product(int, double *, double *, double *) = 0;
    virtual int dual_update_alone(const rn_dual_update_args *, double *) = 0;
    virtual int slab_product(const rn_slab_product_args *, int *) = 0;
    virtual int synchronize() = 0;
    virtual void *stream_handle() = 0;
    virtual int comm_init(int, int, const void *, double timeoutSeconds = -1.0) = 0;
    virtual int comm_check() = 0;
    virtual int set_cut_stage(int) = 0;
    virtual int hist_parts(int, int, double *) = 0;
    virtual int counters(long *) = 0;
    virtual int kernel_info(int *) = 0;
    virtual int sweep_phase(int) = 0;
    virtual int set_operator_mode(int) = 0;
    virtual int get_operator_mode(int *, int *) = 0;
    virtual int set_operator(int, int, const double *, size_t) = 0;
    virtual int set_operators(size_t, int, bool, const void *const *) = 0;
    virtual int get_operators(size_t, int, bool, void *const *) = 0;
    virtual int set_warm_start(int) = 0;
    virtual int set_exchange_mode(int) = 0;
    virtual int set_cut_moments(const double *, const double *, size_t) = 0;
    virtual int cut_buffer(int, double *, size_t) = 0;
    virtual int measure_hbm(size_t, int, double *, double *) = 0;
    // global FBE / NAMA
    virtual int set_algorithm(int, int) = 0;
    virtual int fbe_reset() = 0;
    virtual int hessian_oracle() = 0;
    virtual int gradient_fbe() = 0;
    virtual int nama_residual() = 0;
    virtual int lbfgs_direction() = 0;
    virtual int lbfgs_update_buffer() = 0;
    virtual int lbfgs_two_loop() = 0;
    virtual int value_fbe(double *) = 0;
    virtual int line_search_fbe(double, double *) = 0;
    virtual int line_search_ame(double, double *) = 0;
    virtual int algorithm_fbe_nama(int, double *, double *, double *) = 0;
    virtual int lbfgs_state(int, int *, int *, double *, double *) = 0;
    virtual int lbfgs_column(int, int, int, double *, size_t) = 0;
    // multi-GPU through the boundary
    virtual int set_allreduce(rn_allreduce_fn, void *) = 0;
    virtual int shard_info(int *) = 0;
    virtual int shard_global_nodes(int *, size_t) = 0;
    virtual void set_global_nodes(const int *, int, int) = 0;
    virtual int device_ordinal() const = 0;
    virtual int join_local_group(struct LocalGroup *, int) = 0;
    virtual int guard_check(long *) = 0;
    virtual int memory_info(size_t *) = 0;
    virtual int reserve_iterations(int) = 0;
    virtual int profile_read_collective(double *, long *) = 0;
    virtual int inject_allocation(size_t) = 0;
    virtual int guard_poke(int) = 0;
    virtual int peer_inbox_create(void *) = 0;
    virtual int peer_inbox_connect(const void *, int) = 0;
    virtual int peer_inbox_connect_local(CtxBase **, int) = 0;
    virtual unsigned long long *peer_inbox_ptr() = 0;
    virtual int set_exchange_transport(int) = 0;
    virtual int exchange_autotune_api(int, double *) = 0;
    virtual int exchange_prepare_api() = 0;
    virtual int set_fused_walk_dual(int) = 0;
    virtual int set_knob(int, int) = 0;
    virtual int stream_info(int *) = 0;
    virtual int debug_peer_seq(unsigned int) = 0;
    virtual int fbe_counters(long *) = 0;
    virtual int set_operator_storage(int) = 0;
    virtual int get_operator_storage(int *, int *) = 0;
    virtual int set_sweep_pairing(int) = 0;
    virtual int get_sweep_pairing(int *, int *) = 0;
    virtual int set_tree_data(size_t, int, bool, const void *, const void *, const void *) = 0;
    virtual int get_tree_data(size_t, double *, double *, double *) = 0;
    virtual int set_bounds(int, size_t, int, bool, const void *const *) = 0;
    virtual int get_bounds_layout(int *, size_t *) = 0;
    virtual int get_bounds(size_t, double *const *) = 0;
    virtual int set_cut_children(const int *, const int *, int, bool, int, int, const double *, const double *) = 0;
    virtual int cut_moments(double *, double *, size_t) = 0;
    virtual int plan_report(size_t, double *) = 0;
    virtual int plan_report_scenarios(size_t, double *, int *) = 0;
    virtual int plan_report_device(void **, void **, size_t *) = 0;
    virtual int plan_quantiles(int, size_t, const double *, size_t, double *) = 0;
    virtual int plan_quantiles_device(int, size_t, const double *, void **) = 0;
    virtual int plan_paths(int, size_t, double *, int *) = 0;
    virtual void set_full_tree(const int *, const int *, int, int) = 0;
    virtual int shift_warm_start(int) = 0;
    virtual int set_shift_map(size_t, const int *) = 0;
    virtual int get_shift_map(int, size_t, int *) = 0;
    virtual int estimate_lipschitz(int, double, int, const double *, const double *, unsigned long long, double *, double *) = 0;
    virtual int get_lipschitz(double *, int *) = 0;
    virtual int set_step_rule(int, double, int) = 0;
    virtual int get_step_rule(int *, double *, int *, double *) = 0;
    virtual int solve_certificate(double *) = 0;
    virtual int solve_certificate_device(void **) = 0;
    virtual int certificate_hz(double *, double *) = 0;
};

// ---- in-process stand-in for the communicator (rn_debug_local_group_*): `n` contexts of one process, one host thread each ----
struct LocalGroup {
    int n = 0;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    long gen = 0;
    bool broken = false;
    int timeoutSeconds = 120;   // $RAPIDNET_GROUP_TIMEOUT_S at creation (tests of the failure path use a short one)
    std::vector<void *> bufs;
    std::vector<size_t> counts;
    std::vector<int> f64;
    // false: a rank did not arrive in time (or the group is already broken) -- every waiter gives up with an error
    bool barrier() {
        std::unique_lock<std::mutex> lk(m);
        if (broken) return false;
        const long g = gen;
        if (++arrived == n) { arrived = 0; gen++; cv.notify_all(); return true; }
        if (!cv.wait_for(lk, std::chrono::seconds(timeoutSeconds), [&] { return gen != g || broken; })) { broken = true; cv.notify_all(); return false; }
        return !broken;
    }
};
struct LocalMember { LocalGroup *g = nullptr; int rank = 0; void *recv = nullptr; size_t recvBytes = 0; };
constexpr int LOCAL_GROUP_MAX = 16;
struct PeerPtrs { const void *p[LOCAL_GROUP_MAX]; };
template <typename T>
__global__ void k_sum_ranks(T *out, PeerPtrs peers, int n, size_t count, int op) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        T s = reinterpret_cast<const T *>(peers.p[0])[i];
        for (int r = 1; r < n; r++) {                                    // rank order: the same bits on every rank
            const T v = reinterpret_cast<const T *>(peers.p[r])[i];
            s = op == 2 ? (v > s ? v : s) : s + v;
        }
        out[i] = s;
    }
}
static int local_allreduce(void *user, void *devBuf, size_t count, int isF64, int op, void *streamHandle) {
    LocalMember *me = static_cast<LocalMember *>(user);
    LocalGroup *g = me->g;
    hipStream_t stream = (hipStream_t)streamHandle;
    if (hipStreamSynchronize(stream) != hipSuccess) return 1;          // this rank's payload is complete
    g->bufs[me->rank] = devBuf; g->counts[me->rank] = count; g->f64[me->rank] = isF64;
    if (!g->barrier()) return 2;                                        // ... and so is everybody else's
    for (int r = 0; r < g->n; r++)
        if (g->counts[r] != count || g->f64[r] != isF64) { std::lock_guard<std::mutex> lk(g->m); g->broken = true; g->cv.notify_all(); return 3; }
    const size_t bytes = count * (isF64 ? 8 : 4);
    if (bytes > me->recvBytes) {
        if (me->recv) (void)hipFree(me->recv);
        me->recv = nullptr; me->recvBytes = 0;
        if (hipMalloc(&me->recv, bytes * 2) != hipSuccess) return 4;
        me->recvBytes = bytes * 2;
    }
    PeerPtrs pp{};
    for (int r = 0; r < g->n; r++) pp.p[r] = g->bufs[r];
    const int blocks = (int)std::min<size_t>(256, (count + 255) / 256);
    if (isF64) hipLaunchKernelGGL(k_sum_ranks<double>, dim3(blocks), dim3(256), 0, stream, (double *)me->recv, pp, g->n, count, op);
    else hipLaunchKernelGGL(k_sum_ranks<float>, dim3(blocks), dim3(256), 0, stream, (float *)me->recv, pp, g->n, count, op);
    if (hipStreamSynchronize(stream) != hipSuccess) return 5;
    if (!g->barrier()) return 6;                                        // nobody still reads this rank's payload
    if (hipMemcpyAsync(devBuf, me->recv, bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess) return 7;
    return 0;
}

// dense host helpers (fp64, column-major) ---------------------------------------------------------------
static void h_gemm(bool ta, bool tb, int m, int n, int k, const double *A, int lda, const double *B, int ldb, double *C) {
    for (int j = 0; j < n; j++)
        for (int i = 0; i < m; i++) {
            double s = 0;
            for (int p = 0; p < k; p++)
                s += (ta ? A[p + (size_t)i * lda] : A[i + (size_t)p * lda]) * (tb ? B[j + (size_t)p * ldb] : B[p + (size_t)j * ldb]);
            C[i + (size_t)j * m] = s;
        }
}
static int h_inverse(int n, std::vector<double> A, double *Ainv) {  // LU with partial pivoting
    std::vector<int> piv(n);
    for (int k = 0; k < n; k++) {
        int p = k; double mx = std::fabs(A[k + (size_t)k * n]);
        for (int i = k + 1; i < n; i++) if (std::fabs(A[i + (size_t)k * n]) > mx) { mx = std::fabs(A[i + (size_t)k * n]); p = i; }
        piv[k] = p;
        if (mx == 0.0 || !std::isfinite(mx)) return k + 1;
        if (p != k) for (int j = 0; j < n; j++) std::swap(A[k + (size_t)j * n], A[p + (size_t)j * n]);
        const double d = A[k + (size_t)k * n];
        for (int i = k + 1; i < n; i++) A[i + (size_t)k * n] /= d;
        for (int j = k + 1; j < n; j++) { const double akj = A[k + (size_t)j * n]; for (int i = k + 1; i < n; i++) A[i + (size_t)j * n] -= A[i + (size_t)k * n] * akj; }
    }
    std::vector<double> b(n);
    for (int c = 0; c < n; c++) {
        for (int i = 0; i < n; i++) b[i] = (i == c) ? 1.0 : 0.0;
        for (int k = 0; k < n; k++) if (piv[k] != k) std::swap(b[k], b[piv[k]]);
        for (int k = 0; k < n; k++) { const double bk = b[k]; for (int i = k + 1; i < n; i++) b[i] -= A[i + (size_t)k * n] * bk; }
        for (int k = n - 1; k >= 0; k--) { b[k] /= A[k + (size_t)k * n]; const double bk = b[k]; for (int i = 0; i < k; i++) b[i] -= A[i + (size_t)k * n] * bk; }
        for (int i = 0; i < n; i++) Ainv[i + (size_t)c * n] = b[i];
    }
    return 0;
}

template <typename T>
struct Ctx : CtxBase {
    rn_dims d{};
    int ny = 0, LD = 0, device = 0, numCUs = 256;
    size_t strideA = 0;      // values between the operator blocks of consecutive nodes (>= ny * LD, whole cache lines)
    hipStream_t stream = nullptr;
    bool factored = false, affine_ready = false;
    // host copies of the tree and of the shared factors (fp64)
    std::vector<int> h_stageCum, h_parent, h_childStart, h_childCount, h_stageOf;
    std::vector<double> h_prob, h_Rinv, h_Bbt, h_diag /* [N][nu|nx|nx] as given */;
    // device allocations
    std::vector<void *> allocs;
    int *d_stageCum = nullptr, *d_parent = nullptr, *d_childStart = nullptr, *d_childCount = nullptr, *d_stageOf = nullptr;
    T *d_sqrtp = nullptr, *d_prob = nullptr, *d_dy = nullptr;
    T *d_A = nullptr, *d_Rinv = nullptr, *d_Bbt = nullptr, *d_L = nullptr, *d_B = nullptr, *d_Lt = nullptr, *d_WLt = nullptr;
    T *d_T1 = nullptr, *d_T2 = nullptr, *d_Gd = nullptr, *d_Lhat = nullptr, *d_alpha1 = nullptr, *d_blo = nullptr, *d_bhi = nullptr;
    T *d_errD = nullptr, *d_errP = nullptr, *d_dhat = nullptr, *d_ahat = nullptr;
    T *d_curX = nullptr, *d_prevU = nullptr, *d_prevUhat = nullptr, *d_prevD = nullptr;
    T *d_beta = nullptr, *d_uhat = nullptr, *d_e = nullptr, *d_alpha = nullptr;
    T *d_x = nullptr, *d_u = nullptr, *d_v = nullptr, *d_hx = nullptr;
    T *d_my = nullptr, *d_qa = nullptr, *d_sk = nullptr, *d_rkq = nullptr, *d_lvb = nullptr, *d_eb = nullptr, *d_bw0 = nullptr, *d_bw = nullptr;
    T *d_LBLp = nullptr;
    bool aux_dirty = true;   // eb = e + B uhat and bw0 = B (prevU - prevUhat) must be refreshed before the next sweep
    T *d_RTp = nullptr, *d_Lp = nullptr, *d_Bp = nullptr, *d_BLp = nullptr, *d_ab = nullptr;
    // Operator storage (rn_set_operator_mode).  opsMode is what the caller asked for, `structured` what the context runs: RN_OPS_AUTO
    // (the default) is structured for as long as every block is the factor step's own -- block = shared matrix x stage diagonal x power
    // of p_i, Engine.cu:721-745 -- and becomes dense the moment a caller hands in a block of its own (rn_set_operator: materialise_dense)
    int opsMode = RN_OPS_AUTO, structured = 1, warmStart = 0;
    // Element type of the dense blocks (rn_set_operator_storage).  RN_STORE_F32 on an fp64 context: the blocks live in d_A32 as floats -- LD,
    // strideA and the streaming kernel's span follow the 4-byte element -- and k_stream_gemv<double, ..., float> accumulates them in fp64; every other buffer
    // and every other kernel is the fp64 context's.  On an fp32 context the request changes nothing (its blocks are floats already).
    int storeReq = RN_STORE_NATIVE;
    float *d_A32 = nullptr;
    bool store32() const { return sizeof(T) == 8 && storeReq == RN_STORE_F32; }
    int block_elem() const { return store32() ? 4 : (int)sizeof(T); }      // bytes of one stored block entry
    void block_layout() {   // columns are whole 16-byte slots, node blocks whole 128-byte lines (k_stream_gemv walks a block in slots and
                            // its spans are only line-aligned if the block is)
        const int vps = 16 / block_elem(), vpl = 128 / block_elem();
        LD = (2 * d.nv + vps - 1) / vps * vps;
        strideA = ((size_t)ny * LD + vpl - 1) / vpl * vpl;
    }
    struct SavedSystem { std::vector<double> B, Gd, L, Lhat, W, diag, xmin, xmax, xsafe, umin, umax, alpha1; } h_sys;   // the factor step's inputs (AUTO: for the dense re-factor)
    int optimistic = 1;      // multi-GPU: 1 = one collective per iteration + verification, 0 = exact two-collective path
    // What one iteration of an rn_apg_iterate batch hands to the next: run_batch owns it, launch_sweep and launch_dual_main read and consume
    // it (nullptr: a sweep outside a batch -- the step-wise API, the FBE / NAMA Hessian sweeps, rn_debug_sweep_phase).  A value-initialised
    // Batch is the state between batches: every flag is false at each batch boundary on the success path (checked below, flag by flag),
    // so whatever a batch abandoned half-way held goes away with it.
    struct Batch {
        bool optimistic = false;  // prox as a pure projection, verified once per batch (and the walk may leave Hx unscaled); else exact
        bool sharded = false;     // has_comm() && cutStage > 0: the cut payload is all-reduced (or sent one-shot) every iteration
        // the previous iteration's bookkeeping rides in this sweep's first chain / cut launch.  Set after every iteration but the last,
        // whose bookkeeping has a launch of its own (k_finalize_optimistic): false at the end of a batch
        bool pendingFin = false;
        // the chain walk of the NEXT sweep was done by the last fused launch (k_down_chain_dual UPLIN).  Set only when !fuseMat, i.e. never
        // by the last iteration, and cleared by every sweep: false at the end of a batch
        bool upDone = false;
        // d_hx holds the primal values of every node (k_down_chain UNSC): the dual update applies sqrt(p_i) d_k (k_dual_stage SCALE).  Set
        // only by a sweep that writes no primal (not the last iteration), cleared by the same iteration's launch_dual_main
        bool hxUnscaled = false;
        // the fused walk + dual update (k_down_chain_dual): requested before a sweep and cleared after it; fuseDone is the sweep's answer,
        // cleared by the iteration that reads it.  fuseMat / fuseArgs / fuseLn are the request's arguments, read only while fuseReq is set
        bool fuseReq = false, fuseDone = false, fuseMat = false;
        DualArgs<T> fuseArgs{};
        double fuseLn = 0.0;
        // an optimistic sharded batch: the cut payload carries 2 extra reals (rank-local dist^2 of the previous iteration)
        bool carry_tail() const { return optimistic && sharded; }
    };
    T *d_ck[3] = {nullptr, nullptr, nullptr};   // checkpoint of (y, y+, w) for the exact fallback
    long fallbacks = 0;          // optimistic batches that had to be replayed through the exact path
    long optBatches = 0, exactBatches = 0;
    int optHold = 0;             // batches still to run through the exact path after a replay (back-off: a state that violates its
                                 // soft bounds would otherwise pay checkpoint + replay on every batch of every control step)
    std::vector<double> h_T1, h_T2, h_Lt;   // zero-padded (rows % 16, cols % 4) copies for the MFMA GEMMs
    int chainStage = 0;
    // host-mapped copy of the batch record (common.hpp, BatchRecord) that the closing launch of a single-GPU batch writes: the verdict of an
    // optimistic batch and what a stop tolerance needs, read behind the batch's one synchronisation (nullptr: not granted -- a copy is used)
    BatchRecord *h_rec = nullptr;
    BatchRecord lastRec{0, -1, 0.0};   // of the batch run last, as the host read it (valid when that batch was run under a tolerance)
    // rn_set_stop_tolerance: what rn_control_action and rn_algorithm_apg do (stopTol == 0: one batch of maxIterations, as ever)
    double stopTol = 0.0;
    int stopEvery = RN_STOP_CHECK_EVERY;
    long lastSolve[4] = {0, 0, -1, 0};   // rn_get_last_solve
    // rn_set_restart: RN_RESTART_GRADIENT -- the APG loops run in batches (solve_loop) and every batch end evaluates the gradient test
    // (k_restart_test, k_dual.hpp).  d_rt: the kernel's per-workgroup partials ([ELT_MAX_BLOCKS][6]) and, behind them, its arrival counter;
    // allocated by the first rn_set_restart(RN_RESTART_GRADIENT) / rn_debug_restart_test, never by a context that leaves the mode off.
    // lamBase: iteration at which the lambda sequence started last (0 after a reset; h_it at a restart inside a solve): iteration t takes
    // h_lam[t - lamBase], while the iteration count, the history and the device's counter run on.
    int restartMode = RN_RESTART_OFF;
    double *d_rt = nullptr;
    int lamBase = 0;
    long restartCounts[4] = {0, -1, 0, 0};     // rn_get_restart_info: restarts, iteration of the last one, batches tested, 0
    double restartLast[3] = {0.0, 0.0, 0.0};   // g, na2, nb2 of the last test
    bool unscaled_on() const { return knob[RN_KNOB_UNSCALED_WALK] != 0; }   // inner iterations of optimistic batches take that pair of kernels (default on)
    // rn_debug_set_knob (include/rapidnet_debug.h): launch-shape choices the library otherwise makes by problem size, forced by tests and A/B tools
    // on trees that would not take them by themselves; -1 = the library's own choice.  Before the factor step only.
    int knob[RN_KNOB_COUNT];
    int set_knob(int k, int v) override {
        RN_CHECK(k >= 0 && k < RN_KNOB_COUNT, RN_E_ARG, "rn_debug_set_knob: unknown knob");
        RN_CHECK(!factored, RN_E_STATE, "rn_debug_set_knob must precede rn_factor_step");
        knob[k] = v;
        if (k == RN_KNOB_DUAL_TRIPS || k == RN_KNOB_DUAL_PIPE) dual_stage_setup();
        return RN_OK;
    }
    void hx_scale_now(T *hx) {   // (safety net: a consumer of Hx other than k_dual_stage SCALE behind an unscaled walk)
        const long long total = ntot();
        const int blocks = (int)std::min<long long>((total + ELT_THREADS - 1) / ELT_THREADS, (long long)numCUs * 16);
        hipLaunchKernelGGL(k_hx_scale<>, dim3(blocks), dim3(ELT_THREADS), 0, stream, (void *)hx, (const void *)d_sqrtp, (const void *)d_dy, (const int *)d_stageOf, ny, total,
                           sizeof(T) == 8 ? 1 : 0);
    }
    T *d_lo = nullptr, *d_hi = nullptr, *d_z = nullptr, *d_res = nullptr;
    // rn_set_bounds: d_blo / d_bhi point at the unscaled table of the granularity in force ([rows][ny]; one table per granularity, allocated by
    // the first set at that granularity and kept); the element strides by which the kernels find a node's row: k_dual.hpp, DualArgs
    T *d_bloG[3] = {nullptr, nullptr, nullptr}, *d_bhiG[3] = {nullptr, nullptr, nullptr};
    int boundsGran = RN_BOUNDS_SHARED;
    bool keepBounds = false;      // materialise_dense re-runs the factor step: the bounds stay the caller's
    size_t bounds_rows(int g) const { return bounds::rows_of(g, d.N, d.nodes); }
    int b_stride_stage() const { int s, n; bounds::strides_of(boundsGran, ny, &s, &n); return s; }
    int b_stride_node() const { int s, n; bounds::strides_of(boundsGran, ny, &s, &n); return n; }
    T *d_ybuf[2] = {nullptr, nullptr}, *d_wbuf[2] = {nullptr, nullptr};
    T *d_tmp = nullptr;  // nodes*max(2nx,nu) staging for reference-layout get/set
    T *d_cut = nullptr;  // multi-GPU all-reduce payload
    T *d_momE = nullptr, *d_momP = nullptr;  // multi-GPU: children moments of the cut parents (static tree data)
    bool moments_set = false;
    // rn_set_tree_data (k_tree_data): the per-workgroup counts of bad probabilities of the last device-form set and whether the host has still
    // to read them (eliminate does, behind its uploads' synchronisation); treeBad: the last set held bad entries -- the context refuses the
    // affine terms until a valid one; hProbStale: h_prob is older than d_prob (a device-form set) and is read back by whoever needs it
    int *d_treeBad = nullptr;
    double *d_prob64 = nullptr;         // fp32 contexts: the probabilities as given (doubles), for rn_get_tree_data and the host copy
    bool treeCheckPending = false, treeBad = false, hProbStale = false;
    long treeBadCount = 0;
    // a context made by rn_create_sharded: the full-tree row of every local node on the device, the contiguous full-tree child range of every
    // cut parent (build_partition) and the full-tree p and errorDemand of the cut stage's nodes, from which k_tree_data recomputes the moments
    int *d_gmap = nullptr, *d_cutC0 = nullptr, *d_cutNc = nullptr;
    double *d_fullP = nullptr, *d_fullE = nullptr;
    int nCutPar = 0, cutFirstFull = 0;
    bool cutContiguous = true;
    // logical views (see DESIGN.md "iterate buffers")
    T *p_xi = nullptr, *p_upd = nullptr, *p_acc = nullptr, *p_acc_other = nullptr, *p_acc_view = nullptr;
    bool acc_ready = false;
    IterState *d_state = nullptr;
    Partial *d_partials = nullptr, *d_partials2 = nullptr;   // main pass / fix-up pass
    double *d_lam = nullptr, *d_hist = nullptr, *d_histParts = nullptr, *d_dist2 = nullptr;
    double *d_histGlob = nullptr;   // sharded: payload of the per-batch MAX all-reduce (verdict + the batch's history entries)
    int lamCap = 0, histCap = 0;
    int h_it = 0;
    double theta0 = 1, theta1 = 1;
    std::vector<double> h_lam;
    double stepSize = 1e-4, penX = 1e6, penXs = 1e4, wEco = 1.0;
    int useErrD = 1, useErrP = 1;
    int eltBlocks = 1;
    DualStageShape dshape{};   // k_dual_stage launch shape (dual_stage_setup)
    int dualU = 0;             // vectors a k_dual_stage thread keeps in flight; 0: shape not eligible, the flat k_dual_fused runs
    int dualBlocks = 1;        // workgroups (= partials) of the main pass of the fused dual update
    int mainPartials = 1;      // partials the most recent main pass left in d_partials (k_dual_stage or k_dual_fused)
    // profiling
    int prof = 0;
    struct EvPair { int cls; hipEvent_t a, b; };
    std::vector<EvPair> pending;
    std::vector<hipEvent_t> freeEvents;
    double prof_ms[5] = {0, 0, 0, 0, 0};   // classes 0-3 as in rn_profile_read; 4 = the collectives (rn_profile_read_collective)
    long prof_n[5] = {0, 0, 0, 0, 0};
    // multi-GPU
    void *comm = nullptr;
    int rank = 0, nranks = 1, cutStage = -1;
    rn_allreduce_fn arHook = nullptr;   // rn_debug_set_allreduce: called in place of ncclAllReduce
    void *arUser = nullptr;
    LocalMember *localMember = nullptr; // rn_debug_local_group_join (owned)
    std::vector<int> globalNode;        // sharded through rn_create_sharded: index of every local node in the full tree
    int fullNodes = 0;
    bool has_comm() const { return comm != nullptr || arHook != nullptr; }
    // sum all-reduce, in place, on the solver's stream: the library's RCCL communicator, or the installed stand-in
    int all_reduce(void *buf, size_t count, bool f64, const char *what, int op = 0 /* ncclSum; 2 = ncclMax */) {
        if (arHook) {
            hipEvent_t ev = prof_begin(4);
            const int rc = arHook(arUser, buf, count, f64 ? 1 : 0, op, (void *)stream);
            prof_end(ev);
            RN_CHECK(rc == 0, RN_E_COMM, std::string(what) + ": the installed all-reduce callback failed (" + std::to_string(rc) + ")");
            return RN_OK;
        }
        RN_CHECK(comm != nullptr, RN_E_STATE, std::string(what) + ": no communicator");
        hipEvent_t ev = prof_begin(4);
        const int rc = g_nccl.AllReduce(buf, buf, count, f64 ? 8 /*ncclFloat64*/ : 7 /*ncclFloat32*/, op, comm, stream);
        prof_end(ev);
        RN_CHECK(rc == 0, RN_E_COMM, std::string(what) + " failed: " + (g_nccl.GetErrorString ? g_nccl.GetErrorString(rc) : "?"));
        return RN_OK;
    }

    ~Ctx() override {
        g_liveContexts--;
        if (commJob) { std::lock_guard<std::mutex> lk(commJob->m); commJob->abandoned = true; }   // a helper still inside ncclCommInitRank destroys what it gets
        if (comm && g_nccl.CommDestroy) g_nccl.CommDestroy(comm);
        (void)hipSetDevice(device);
        if (guardMode && stream) {   // guard mode: a context never goes away with an overwritten red zone unnoticed
            long bad = 0;
            if (guard_check(&bad) == RN_OK) { g_guardContexts++; g_guardBadBytes += bad; if (bad) fprintf(stderr, "librapidnet_hip: %s\n", err.c_str()); }
        }
        if (localMember) { if (localMember->recv) (void)hipFree(localMember->recv); delete localMember; }
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto &p : pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        for (auto e : freeEvents) (void)hipEventDestroy(e);
        for (void *p : ipcOpened) (void)hipIpcCloseMemHandle(p);
        if (h_rec) (void)hipHostFree(h_rec);
        if (d_inbox) (void)hipFree(d_inbox);
        for (void *p : allocs) (void)hipFree(p);
        if (evFork) (void)hipEventDestroy(evFork);
        if (evJoin) (void)hipEventDestroy(evJoin);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // ---- device allocations ---------------------------------------------------------------------------------
    // Every buffer of the context comes from here.  RAPIDNET_GUARD=1 (read when the context is created) is the library's
    // stand-in for a GPU address sanitizer, which this pool does not offer: every buffer gets a red zone of GUARD_BYTES on both
    // sides, and red zones AND payload of floating-point buffers start out as 0xFF bytes -- a NaN in fp64 and in fp32 -- so a
    // kernel that reads outside its buffer, or reads what nobody has written, carries a NaN into the iterates (the parity
    // tests then fail); integer tables get zero red zones (an index read from one stays in range).  A kernel that WRITES
    // outside its buffer changes a red zone: rn_guard_check / rn_destroy compare them with the pattern.
    static constexpr size_t GUARD_BYTES = 128 * 1024;
    struct GuardRec { void *base; size_t bytes; unsigned char pat; };
    std::vector<GuardRec> guards;
    bool guardMode = false;
    size_t allocatedBytes = 0;   // payload bytes of all live allocations of this context (rn_device_memory_info)
    template <typename U> int dalloc(U **p, size_t n) {
        void *q = nullptr;
        const size_t bytes = (n ? n : 1) * sizeof(U);
        if (!guardMode) {
            RN_HIP(hipMalloc(&q, bytes));
            allocs.push_back(q);
            allocatedBytes += bytes;
            *p = (U *)q;
            return RN_OK;
        }
        const size_t padded = (bytes + 255) / 256 * 256;
        RN_HIP(hipMalloc(&q, padded + 2 * GUARD_BYTES));
        allocs.push_back(q);
        allocatedBytes += bytes;
        const unsigned char pat = std::is_floating_point<U>::value || std::is_class<U>::value ? 0xFF : 0x00;
        // filled on the context's OWN stream and waited for: the stream is non-blocking (no implicit ordering with the null
        // stream), and everything that touches the buffer afterwards -- uploads on either stream, kernels -- must come after the fill
        RN_HIP(hipMemsetAsync(q, pat, padded + 2 * GUARD_BYTES, stream));
        RN_HIP(hipStreamSynchronize(stream));
        guards.push_back(GuardRec{q, bytes, pat});
        *p = (U *)((char *)q + GUARD_BYTES);
        return RN_OK;
    }
    // number of red-zone bytes that no longer hold their pattern (0 outside guard mode)
    int guard_check(long *bad) override {
        RN_CHECK(bad, RN_E_ARG, "rn_guard_check: null output");
        *bad = 0;
        if (!guardMode) return RN_OK;
        RN_HIP(hipSetDevice(device));
        RN_HIP(hipStreamSynchronize(stream));
        std::vector<unsigned char> h(GUARD_BYTES + 256);
        for (const GuardRec &g : guards) {
            const size_t padded = (g.bytes + 255) / 256 * 256;
            RN_HIP(hipMemcpy(h.data(), g.base, GUARD_BYTES, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < GUARD_BYTES; i++) if (h[i] != g.pat) (*bad)++;
            // the back red zone starts right behind the payload (the round-up to 256 bytes belongs to it)
            const size_t back = GUARD_BYTES + (padded - g.bytes);
            RN_HIP(hipMemcpy(h.data(), (char *)g.base + GUARD_BYTES + g.bytes, back, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < back; i++) if (h[i] != g.pat) (*bad)++;
        }
        if (*bad) err = "rn_guard_check: " + std::to_string(*bad) + " red-zone bytes were overwritten (a kernel wrote outside its buffer)";
        return RN_OK;
    }
    // test of the detector: `n` bytes right behind the payload of the context's first buffer are overwritten
    int guard_poke(int n) override {
        RN_CHECK(guardMode && !guards.empty(), RN_E_STATE, "rn_debug_guard_poke: the context was not created under RAPIDNET_GUARD=1");
        RN_CHECK(n >= 1 && n <= 256, RN_E_ARG, "rn_debug_guard_poke: 1 .. 256 bytes");
        RN_HIP(hipSetDevice(device));
        RN_HIP(hipStreamSynchronize(stream));
        RN_HIP(hipMemset((char *)guards[0].base + GUARD_BYTES + guards[0].bytes, 0xA5, (size_t)n));
        return RN_OK;
    }
    // free / total bytes of the device and the bytes this context holds: what cudaMemGetInfo reports in the reference's leak check
    // (SmpcController.cu:1612, :1619) plus a figure that other contexts on the same device cannot disturb
    int memory_info(size_t *out) override {
        RN_CHECK(out, RN_E_ARG, "rn_device_memory_info: null output");
        RN_HIP(hipSetDevice(device));
        size_t fr = 0, tot = 0;
        RN_HIP(hipMemGetInfo(&fr, &tot));
        out[0] = fr; out[1] = tot; out[2] = allocatedBytes; out[3] = (size_t)g_liveContexts.load();
        return RN_OK;
    }
    int upload(T *dst, const double *src, size_t n) {
        std::vector<T> tmp(n);
        for (size_t i = 0; i < n; i++) tmp[i] = (T)src[i];
        RN_HIP(hipMemcpyAsync(dst, tmp.data(), n * sizeof(T), hipMemcpyHostToDevice, stream));
        RN_HIP(hipStreamSynchronize(stream));  // tmp goes out of scope
        return RN_OK;
    }
    int download(double *dst, const T *src, size_t n) {
        std::vector<T> tmp(n);
        RN_HIP(hipMemcpyAsync(tmp.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < n; i++) dst[i] = (double)tmp[i];
        return RN_OK;
    }
    // one node's block [ny][LD] in the element type it is stored in (fp32 storage: rounded to nearest on the way in)
    int upload_block(int node, const double *src) {
        const size_t n = (size_t)ny * LD;
        if (!store32()) return upload(d_A + (size_t)node * strideA, src, n);
        std::vector<float> tmp(n);
        for (size_t i = 0; i < n; i++) tmp[i] = (float)src[i];
        RN_HIP(hipMemcpyAsync(d_A32 + (size_t)node * strideA, tmp.data(), n * sizeof(float), hipMemcpyHostToDevice, stream));
        RN_HIP(hipStreamSynchronize(stream));
        return RN_OK;
    }
    int download_block(int node, double *dst) {
        const size_t n = (size_t)ny * LD;
        if (!store32()) return download(dst, d_A + (size_t)node * strideA, n);
        std::vector<float> tmp(n);
        RN_HIP(hipMemcpyAsync(tmp.data(), d_A32 + (size_t)node * strideA, n * sizeof(float), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < n; i++) dst[i] = (double)tmp[i];
        return RN_OK;
    }
    int upload_int(int *dst, const std::vector<int> &v) {
        RN_HIP(hipMemcpy(dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
        return RN_OK;
    }

    static int pad16(int v) { return (v + 63) / 64 * 64; }   // rows padded to one wave tile (GEMM_RT * 16)
    static int pad4(int v) { return (v + 4 * RN_SLAB_KU - 1) / (4 * RN_SLAB_KU) * (4 * RN_SLAB_KU); }   // pad_k: K of the shared operators in whole groups of the MFMA loop (zero columns)
    int upload_padded(T *dst, const double *src, int m, int k) {   // col-major m x k -> zero-padded pad16(m) x pad4(k)
        const int mp = pad16(m), kp = pad4(k);
        std::vector<double> tmp((size_t)mp * kp, 0.0);
        for (int j = 0; j < k; j++) for (int i = 0; i < m; i++) tmp[i + (size_t)j * mp] = src[i + (size_t)j * m];
        return upload(dst, tmp.data(), tmp.size());
    }
    // the shared operators of the slab products once more in MFMA fragment order (kernels.hpp, GemmArgs::Mf): [16-row tile][pair of k-steps][lane][2],
    // zero-padded like the column-major copies (pad16(m) rows, pad4(k) columns): a wave's A operands of two k-steps are one contiguous request
    T *d_RTf = nullptr, *d_LBLf = nullptr, *d_BLf = nullptr;
    // structured mode, linear form of the leaf-to-root recursion (k_walks.hpp, k_up_chain_lin): the operator [Rinv | T1 | T2] of the v product
    // (column-major padded, and in fragment order) and the running sums' buffers; allocated by the factor step of a structured context
    T *d_RT2p = nullptr, *d_RT2f = nullptr, *d_sk2 = nullptr, *d_rkq2 = nullptr;
    // Bs_i = beta_i + sum_c Bs_c only changes with the affine terms (once per control step): its term of v_i, c_i = -Rinv Bs_i / (2 p_i), is computed by
    // lin_const_refresh when they change and enters the v product as its epilogue operand -- the product itself is [T1 | T2] [q_i + kappa_i ; Bu_i],
    // K = nx + nu instead of nv + nx + nu, and the walks leave the Bs columns alone.  rn_debug_set_knob(RN_KNOB_STRUCT_LINEAR, 3): Bs in every iteration's product.
    T *d_T12p = nullptr, *d_T12f = nullptr, *d_vconst = nullptr;
    bool linConstValid = false;
    bool lin_const() const { return knob[RN_KNOB_STRUCT_LINEAR] != 3; }
    // ... and since v_i then only feeds [L v_i ; B L v_i], the two products are one with the composite operator MC = [L ; B L] [T1 | T2] (k_gemm_comp);
    // d_lvconst = [L ; B L] c_i.  RN_KNOB_STRUCT_LINEAR 4: the two products kept apart.
    T *d_MCp = nullptr, *d_MCf = nullptr, *d_lvconst = nullptr;
    bool lin_comp() const { return lin_const() && knob[RN_KNOB_STRUCT_LINEAR] != 4 && d_MCp != nullptr; }
    // ... and the forward walk's affine terms (uhat_i - uhat_anc, eb_i - eb_anc) join that constant (k_fold_affine), so the walk requests neither
    // uhat nor eb (SweepArgs::lin bit 2).  RN_KNOB_STRUCT_LINEAR 5: the composite operator without them.
    bool lin_fold() const { return lin_comp() && knob[RN_KNOB_STRUCT_LINEAR] != 5; }
    // v_i is an output only in this form (nothing of the sweep reads it): the sweeps that store the primal iterates leave it PENDING and the product
    // runs when somebody asks for RN_BUF_V (rn_get / rn_set / rn_get_range / rn_set_range) -- from the product's input of that very sweep, which is
    // still in place: a later sweep drops the pending product (its state is no longer observable) or, a Hessian sweep, runs it first.  A context
    // whose raw v pointer has been handed out (rn_device_pointer) computes v with every such sweep, as the pointer's contract says.
    bool vPending = false, vEager = false;
    int v_flush() {
        if (!vPending) return RN_OK;
        vPending = false;
        launch_gemm<EPI_V>(d_T12p, d.nv, d.nx + d.nu, d_sk2 + d.nv, d.nv + d.nx + d.nu, d_v, d.nv, d_vconst, d.nv);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // the form applies to unsharded structured sweeps whose v / Lv slab (16 nodes x (nv + nx + nu) and 16 x nv values) fits a workgroup's 64 KB;
    // otherwise (the wide fp32 network) the structured sweep keeps its first product k_gemm_prep_m2
    bool lin_fits() const { return (size_t)16 * (slab_stride(pad4(d.nv + d.nx + d.nu)) + slab_stride(pad4(d.nv))) * sizeof(T) <= 64 * 1024; }
    bool lin_on() const { return structured && d_sk2 != nullptr && knob[RN_KNOB_STRUCT_LINEAR] != 0; }
    bool frag_on() const { return knob[RN_KNOB_SLAB_FRAG] != 0; }   // the slab products take their A operands from the fragment-ordered copies (default on)
    int upload_fragments(T *dst, const double *src, int m, int k) {
        const int mp = pad16(m), kp = pad4(k), tiles = mp / 16, pairs = kp / 8;
        std::vector<double> tmp((size_t)mp * kp, 0.0);
        for (int t = 0; t < tiles; t++)
            for (int p2 = 0; p2 < pairs; p2++)
                for (int l = 0; l < 64; l++)
                    for (int e = 0; e < 2; e++) {
                        const int row = t * 16 + (l & 15), col = 4 * (2 * p2 + e) + (l >> 4);
                        if (row < m && col < k) tmp[(((size_t)t * pairs + p2) * 64 + l) * 2 + e] = src[row + (size_t)col * m];
                    }
        return upload(dst, tmp.data(), tmp.size());
    }
    TreeDev<T> tree_dev() const { return TreeDev<T>{d_stageCum, d_parent, d_childStart, d_childCount, d_stageOf, d_sqrtp, d_prob, d_dy}; }
    SweepArgs<T> sweep_args(const Batch &b) const {
        SweepArgs<T> a{};
        a.tr = tree_dev();
        a.nx = d.nx; a.nu = d.nu; a.nv = d.nv; a.ny = ny; a.LD = LD; a.strideA = strideA; a.N = d.N; a.nodes = d.nodes;
        a.cutSums = (cutStage > 0) ? d_cut : nullptr;
        a.s1 = h_stageCum.size() > 1 ? h_stageCum[1] : d.nodes; a.e1 = h_stageCum.size() > 2 ? h_stageCum[2] : d.nodes;
        a.rootC0 = h_childStart.empty() ? 0 : h_childStart[0]; a.rootNc = h_childCount.empty() ? 0 : h_childCount[0];
        a.cutStage = cutStage;
        a.chainStage = a.cutSums ? std::max(chainStage, cutStage) : chainStage;
        a.K = h_stageCum[a.chainStage + 1] - h_stageCum[a.chainStage];
        a.A = store32() ? reinterpret_cast<const T *>(d_A32) : d_A; a.RT = d_RTp; a.L = d_L; a.B = d_B; a.structured = structured; a.ab = d_ab;
        a.lin = (lin_on() && cutStage <= 0) ? 1 : 0; a.sk2 = d_sk2; a.rkq2 = d_rkq2;
        a.beta = d_beta; a.uhat = d_uhat; a.e = d_e; a.curX = d_curX; a.prevU = d_prevU; a.prevUhat = d_prevUhat;
        a.w = p_acc;
        a.my = d_my; a.my2 = d_my2; a.splitFirst = (splitFirst >= 0 && !structured) ? splitFirst : d.nodes; a.qa = d_qa; a.sk = d_sk; a.rkq = d_rkq; a.v = d_v; a.lvb = d_lvb; a.eb = d_eb; a.bw0 = d_bw0; a.bw = d_bw;
        a.x = d_x; a.u = d_u; a.hx = d_hx;
        a.distTail = (b.carry_tail() && a.cutSums) ? d_cut + cut_tail_offset() : nullptr;
        a.thrX = penX / stepSize; a.thrS = penXs / stepSize; a.iterState = d_state;
        a.writePrimal = 1;
        a.chain0 = h_stageCum[a.chainStage]; a.chainAnc = chainAncStage == a.chainStage ? d_chainAnc : nullptr;
        a.cut0 = cutStage > 0 ? h_stageCum[cutStage - 1] : 0;
        return a;
    }
    // The crown path of every chain as a table (SweepArgs::chainAnc; k_down_chain / k_down_chain_dual with foldCrown): built for the stage the chains
    // start at -- the tree's own, or the cut stage of a shard -- the first time a sweep folds the crown into the forward walk, and again if that stage changes.
    int *d_chainAnc = nullptr;
    int chainAncStage = -1;
    int ensure_chain_anc(int cs) {
        if (chainAncStage == cs && d_chainAnc) return RN_OK;
        RN_CHECK(cs >= 0 && cs <= CROWN_MAX_DEPTH && cs + 1 < (int)h_stageCum.size(), RN_E_STATE, "ensure_chain_anc: the crown is deeper than the folded walk supports");
        const int K = h_stageCum[cs + 1] - h_stageCum[cs];
        std::vector<int> tab((size_t)K * CROWN_MAX_DEPTH, 0);
        for (int c = 0; c < K; c++) {
            int n = h_stageCum[cs] + c;
            bool first = true;
            for (int dd = 0; dd < cs; dd++) {
                const int p = h_parent[n];
                first = first && h_childStart[p] == n;
                tab[(size_t)c * CROWN_MAX_DEPTH + dd] = p | (first ? (1 << 30) : 0);
                n = p;
            }
        }
        if (!d_chainAnc) {      // room for the widest stage, once (rn_create): a control step never allocates (the reference's leak check, SmpcController.cu:1593-1667)
            int widest = 1;
            for (size_t k = 0; k + 1 < h_stageCum.size(); k++) widest = std::max(widest, h_stageCum[k + 1] - h_stageCum[k]);
            if (int rc = dalloc(&d_chainAnc, (size_t)widest * CROWN_MAX_DEPTH)) return rc;
        }
        RN_HIP(hipStreamSynchronize(stream));   // (a sweep in flight may still read the previous table)
        RN_HIP(hipMemcpy(d_chainAnc, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
        chainAncStage = cs;
        return RN_OK;
    }
    long long ntot() const { return (long long)d.nodes * ny; }

    // ---- construction --------------------------------------------------------------------------------
    int init(const rn_dims *dims, const rn_tree *tr, int dev) {
        d = *dims; device = dev;
        g_liveContexts++;
        for (int &k : knob) k = -1;
        if (const char *e = std::getenv("RAPIDNET_EXCHANGE")) {   // default transport of new contexts: collective | oneshot | auto
            const std::string v(e);
            if (v == "collective" || v == "rccl") { transportReq = RN_EXCHANGE_COLLECTIVE; tuned = true; }
            else if (v == "oneshot") { transportReq = RN_EXCHANGE_ONESHOT; tuned = true; }      // (takes effect once the inboxes are connected: exchange_prepare)
        }
        { const char *e = std::getenv("RAPIDNET_GUARD"); guardMode = e && std::atoi(e) != 0; }
        RN_CHECK(d.nx > 0 && d.nu > 0 && d.nv > 0 && d.nd > 0 && d.N > 0 && d.K > 0 && d.nodes > 0, RN_E_ARG, "rn_create: non-positive dimension");
        RN_CHECK(d.nv <= d.nu, RN_E_ARG, "rn_create: nv must not exceed nu");
        ny = 2 * d.nx + d.nu;
        block_layout();
        RN_HIP(hipSetDevice(device));
        RN_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        { int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cu > 0) numCUs = cu; }
        if (hipHostMalloc((void **)&h_rec, sizeof(BatchRecord), hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); h_rec = nullptr; } else *h_rec = BatchRecord{0, -1, 0.0};
        {   // The library's device code is six code objects (one per kernel unit) and the HIP runtime loads a code object when its first kernel is
            // looked up: asked for here, so that no later call -- a control step under the caller's leak check (SmpcController.cu:1612-1623) --
            // is the one during which the device's free memory shrinks by a code object
            hipFuncAttributes fa;
            for (const void *fn : {(const void *)k_stream_gemv<T, 1, false>, (const void *)k_dual_fused<T, false, false>, (const void *)k_up_chain<T, false>,
                                   (const void *)k_gemm_slab<T, EPI_Z, false>, (const void *)k_pack<T>, (const void *)k_dots<T>})
                if (hipFuncGetAttributes(&fa, fn) != hipSuccess) (void)hipGetLastError();
        }
        const int N = d.N, nodes = d.nodes;
        // validate and convert the tree (reference conventions -> 0-based parent/children ranges)
        h_stageCum.assign(tr->nodesPerStageCumul, tr->nodesPerStageCumul + N + 1);
        RN_CHECK(h_stageCum[0] == 0 && h_stageCum[N] == nodes, RN_E_ARG, "rn_create: nodesPerStageCumul inconsistent with nodes");
        h_parent.resize(nodes); h_childStart.assign(nodes, 0); h_childCount.assign(nodes, 0); h_stageOf.resize(nodes); h_prob.resize(nodes);
        for (int k = 0; k < N; k++) {
            RN_CHECK(tr->nodesPerStage[k] == h_stageCum[k + 1] - h_stageCum[k] && tr->nodesPerStage[k] > 0, RN_E_ARG, "rn_create: nodesPerStage inconsistent");
            for (int i = h_stageCum[k]; i < h_stageCum[k + 1]; i++) {
                RN_CHECK(tr->stages[i] == k, RN_E_ARG, "rn_create: nodes are not numbered stage by stage");
                h_stageOf[i] = k;
            }
        }
        RN_CHECK(h_stageCum[1] == 1 && tr->ancestor[0] == 0, RN_E_ARG, "rn_create: node 0 must be the only root");
        h_parent[0] = -1;
        for (int i = 0; i < nodes; i++) {
            h_prob[i] = tr->probNode[i];
            RN_CHECK(h_prob[i] > 0.0 && std::isfinite(h_prob[i]), RN_E_ARG, "rn_create: probNode must be positive");
            if (i == 0) continue;
            const int par = tr->ancestor[i] - 1;
            RN_CHECK(par >= 0 && par < i && h_stageOf[par] == h_stageOf[i] - 1, RN_E_ARG, "rn_create: ancestor must be a node of the previous stage");
            RN_CHECK(par >= h_parent[i - 1] || h_stageOf[i - 1] != h_stageOf[i], RN_E_ARG, "rn_create: children of a node must be contiguous");
            h_parent[i] = par;
            if (h_childCount[par] == 0) h_childStart[par] = i;
            RN_CHECK(h_childStart[par] + h_childCount[par] == i, RN_E_ARG, "rn_create: children of a node must be contiguous");
            h_childCount[par]++;
        }
        int leaves = 0, nonleaf = 0;
        for (int i = 0; i < nodes; i++) (h_childCount[i] == 0 ? leaves : nonleaf)++;
        RN_CHECK(nonleaf == d.nNonLeafNodes, RN_E_ARG, "rn_create: nNonLeafNodes inconsistent with ancestor[]");
        (void)leaves;
        // c*: first stage from which the tree is K parallel chains (every node has exactly one child, same position)
        chainStage = N - 1;
        while (chainStage > 0) {
            const int k = chainStage - 1;
            bool chain = (h_stageCum[k + 1] - h_stageCum[k]) == (h_stageCum[k + 2] - h_stageCum[k + 1]);
            for (int i = h_stageCum[k]; chain && i < h_stageCum[k + 1]; i++) chain = (h_childCount[i] == 1);
            if (!chain) break;
            chainStage--;
        }
        if (int rc = dalloc(&d_stageCum, N + 1)) return rc;
        if (int rc = dalloc(&d_parent, nodes)) return rc;
        if (int rc = dalloc(&d_childStart, nodes)) return rc;
        if (int rc = dalloc(&d_childCount, nodes)) return rc;
        if (int rc = dalloc(&d_stageOf, nodes)) return rc;
        if (int rc = upload_int(d_stageCum, h_stageCum)) return rc;
        if (int rc = upload_int(d_parent, h_parent)) return rc;
        if (int rc = upload_int(d_childStart, h_childStart)) return rc;
        if (int rc = upload_int(d_childCount, h_childCount)) return rc;
        if (int rc = upload_int(d_stageOf, h_stageOf)) return rc;
        if (chainStage <= CROWN_MAX_DEPTH) { if (int rc = ensure_chain_anc(chainStage)) return rc; }
        const size_t n = nodes;
        const int nx = d.nx, nu = d.nu, nv = d.nv, nd = d.nd;
#define DA(ptr, cnt) if (int rc = dalloc(&ptr, (size_t)(cnt))) return rc;
        DA(d_sqrtp, n) DA(d_prob, n) DA(d_dy, (size_t)N * ny)
        DA(d_Rinv, nv * nv) DA(d_Bbt, nv * nx) DA(d_L, nu * nv) DA(d_B, nx * nu) DA(d_Lt, nv * nu) DA(d_WLt, nv * nu) DA(d_W, nu * nu)
        DA(d_T1, nv * nx) DA(d_T2, nv * nu) DA(d_Gd, nx * nd) DA(d_Lhat, nu * nd) DA(d_alpha1, nu) DA(d_blo, ny) DA(d_bhi, ny)
        DA(d_errD, n * nd) DA(d_errP, n * nu) DA(d_dhat, (size_t)N * nd) DA(d_ahat, (size_t)N * nu)
        DA(d_curX, nx) DA(d_prevU, nu) DA(d_prevUhat, nu) DA(d_prevD, nd)
        DA(d_beta, n * nv) DA(d_uhat, n * nu) DA(d_e, n * nx) DA(d_alpha, n * nu)
        DA(d_x, n * nx) DA(d_u, n * nu) DA(d_v, n * nv) DA(d_hx, n * ny)
        DA(d_my, n * 2 * nv) DA(d_qa, n * nx) DA(d_sk, n * (nv + nx)) DA(d_rkq, n * (nv + 2 * nx)) DA(d_lvb, n * (nu + nx)) DA(d_eb, n * nx) DA(d_bw0, nx) DA(d_bw, n * nx)
        DA(d_LBLp, (size_t)pad16(nu + nx) * pad4(nv))
        DA(d_LBLf, (size_t)pad16(nu + nx) * pad4(nv)) DA(d_BLf, (size_t)pad16(nv) * pad4(nx + nu)) DA(d_RTf, (size_t)pad16(nv) * pad4(nv + nx))
        DA(d_BLp, (size_t)pad16(nv) * pad4(nx + nu)) DA(d_ab, n * (nx + nu))
        DA(d_RTp, (size_t)pad16(nv) * pad4(nv + nx)) DA(d_Lp, (size_t)pad16(nu) * pad4(nv)) DA(d_Bp, (size_t)pad16(nx) * pad4(nu))
        DA(d_lo, n * ny) DA(d_hi, n * ny) DA(d_z, n * ny) DA(d_res, n * ny)
        DA(d_ybuf[0], n * ny) DA(d_ybuf[1], n * ny) DA(d_wbuf[0], n * ny) DA(d_wbuf[1], n * ny)
        DA(d_tmp, n * (size_t)std::max(2 * nx, std::max(nu, nv)))
        DA(d_cut, (size_t)nodes * (nv + 2 * nx))  // upper bound on cut parents
        DA(d_treeBad, TREE_MAX_BLOCKS)
        if (sizeof(T) == 4) { DA(d_prob64, n) }
        DA(d_tune, 8) DA(d_state, 1) DA(d_partials, std::max(ELT_MAX_BLOCKS, RN_DUAL_STAGE_MAX_BLOCKS)) DA(d_partials2, ELT_MAX_BLOCKS) DA(d_dist2, 2)
#undef DA
        std::vector<double> sq(nodes);
        for (int i = 0; i < nodes; i++) sq[i] = std::sqrt(h_prob[i]);
        if (int rc = upload(d_sqrtp, sq.data(), nodes)) return rc;
        if (int rc = upload(d_prob, h_prob.data(), nodes)) return rc;
        if (d_prob64) RN_HIP(hipMemcpy(d_prob64, h_prob.data(), n * sizeof(double), hipMemcpyHostToDevice));
        RN_HIP(hipMemsetAsync(d_treeBad, 0, TREE_MAX_BLOCKS * sizeof(int), stream));
        RN_HIP(hipMemsetAsync(d_errD, 0, n * nd * sizeof(T), stream));
        RN_HIP(hipMemsetAsync(d_errP, 0, n * nu * sizeof(T), stream));
        RN_HIP(hipMemsetAsync(d_z, 0, n * ny * sizeof(T), stream));
        RN_HIP(hipMemsetAsync(d_res, 0, n * ny * sizeof(T), stream));
        RN_HIP(hipMemsetAsync(d_x, 0, n * nx * sizeof(T), stream));
        RN_HIP(hipMemsetAsync(d_u, 0, n * nu * sizeof(T), stream));
        RN_HIP(hipMemsetAsync(d_v, 0, n * nv * sizeof(T), stream));
        RN_HIP(hipMemsetAsync(d_hx, 0, n * ny * sizeof(T), stream));
        const long long want = (ntot() + ELT_THREADS * 4 - 1) / (ELT_THREADS * 4);
        eltBlocks = (int)std::max<long long>(1, std::min<long long>(ELT_MAX_BLOCKS, want));
        dual_stage_setup();
        p_xi = d_ybuf[0]; p_upd = d_ybuf[1]; p_acc = d_wbuf[0]; p_acc_other = d_wbuf[1]; p_acc_view = p_acc;
        return apg_reset();
    }

    // ---- Engine ----------------------------------------------------------------------------------------
    int factor_step(const rn_system *s) override {
        RN_CHECK(s && s->matB && s->matGd && s->matL && s->matLhat && s->costW && s->matDiagPrecnd && s->vecXmin && s->vecXmax &&
                     s->vecXsafe && s->vecUmin && s->vecUmax && s->costAlpha1, RN_E_ARG, "rn_factor_step: null input");
        RN_HIP(hipSetDevice(device));
        if (int rc = v_flush()) return rc;       // (a pending v is the previous operators')
        const int nx = d.nx, nu = d.nu, nv = d.nv, nd = d.nd, N = d.N;
        if (opsMode == RN_OPS_AUTO && s->matB != h_sys.B.data()) {   // (not when materialise_dense re-runs the step on the saved copy)
            h_sys.B.assign(s->matB, s->matB + (size_t)nx * nu); h_sys.Gd.assign(s->matGd, s->matGd + (size_t)nx * nd);
            h_sys.L.assign(s->matL, s->matL + (size_t)nu * nv); h_sys.Lhat.assign(s->matLhat, s->matLhat + (size_t)nu * nd);
            h_sys.W.assign(s->costW, s->costW + (size_t)nu * nu); h_sys.diag.assign(s->matDiagPrecnd, s->matDiagPrecnd + (size_t)N * (2 * nx + nu));
            h_sys.xmin.assign(s->vecXmin, s->vecXmin + nx); h_sys.xmax.assign(s->vecXmax, s->vecXmax + nx); h_sys.xsafe.assign(s->vecXsafe, s->vecXsafe + nx);
            h_sys.umin.assign(s->vecUmin, s->vecUmin + nu); h_sys.umax.assign(s->vecUmax, s->vecUmax + nu); h_sys.alpha1.assign(s->costAlpha1, s->costAlpha1 + nu);
        }
        // Rbar = L' W L  (Engine.cu:412-416), inverse once: Omega_i = Rbar^-1 / p_i (Engine.cu:707-714)
        std::vector<double> WL((size_t)nu * nv), Rbar((size_t)nv * nv), Lt((size_t)nv * nu), WLt((size_t)nv * nu);
        h_gemm(false, false, nu, nv, nu, s->costW, nu, s->matL, nu, WL.data());
        h_gemm(true, false, nv, nv, nu, s->matL, nu, WL.data(), nu, Rbar.data());
        h_Rinv.assign((size_t)nv * nv, 0.0);
        RN_CHECK(h_inverse(nv, Rbar, h_Rinv.data()) == 0, RN_E_SINGULAR, "rn_factor_step: L'WL is singular");
        h_Bbt.assign((size_t)nv * nx, 0.0);
        h_gemm(true, true, nv, nx, nu, s->matL, nu, s->matB, nx, h_Bbt.data());  // Bbar' = L'B' (Engine.cu:702-705)
        std::vector<double> T1((size_t)nv * nx), T2((size_t)nv * nu);
        for (int i = 0; i < nu; i++) for (int j = 0; j < nv; j++) { Lt[j + (size_t)i * nv] = s->matL[i + (size_t)j * nu]; WLt[j + (size_t)i * nv] = WL[i + (size_t)j * nu]; }
        h_gemm(false, false, nv, nx, nv, h_Rinv.data(), nv, h_Bbt.data(), nv, T1.data());
        h_gemm(false, false, nv, nu, nv, h_Rinv.data(), nv, Lt.data(), nv, T2.data());
        // preconditioner diagonal re-ordered to y order: (d_x | d_xs | d_u) per stage
        h_diag.assign(s->matDiagPrecnd, s->matDiagPrecnd + (size_t)N * (2 * nx + nu));
        std::vector<double> dy((size_t)N * ny), blo(ny), bhi(ny);
        for (int k = 0; k < N; k++) {
            const double *dk = s->matDiagPrecnd + (size_t)k * (2 * nx + nu);
            for (int t = 0; t < 2 * nx; t++) dy[(size_t)k * ny + t] = dk[nu + t];
            for (int t = 0; t < nu; t++) dy[(size_t)k * ny + 2 * nx + t] = dk[t];
        }
        // "no upper bound" on the safety half: the reference memsets bytes 0x7F (Engine.cu:454-455)
        T big; std::memset(&big, 0x7F, sizeof(T));
        for (int t = 0; t < nx; t++) { blo[t] = s->vecXmin[t]; bhi[t] = s->vecXmax[t]; blo[nx + t] = s->vecXsafe[t]; bhi[nx + t] = (double)big; }
        for (int t = 0; t < nu; t++) { blo[2 * nx + t] = s->vecUmin[t]; bhi[2 * nx + t] = s->vecUmax[t]; }
#define UP(dst, src, cnt) if (int rc = upload(dst, src, (size_t)(cnt))) return rc;
        h_T1 = T1; h_T2 = T2; h_Lt = Lt;
        {   // [Bbt | L'] for the structured m2 GEMM
            std::vector<double> BL((size_t)nv * (nx + nu));
            std::copy(h_Bbt.begin(), h_Bbt.end(), BL.begin());
            std::copy(Lt.begin(), Lt.end(), BL.begin() + (size_t)nv * nx);
            if (int rc = upload_padded(d_BLp, BL.data(), nv, nx + nu)) return rc;
            if (int rc = upload_fragments(d_BLf, BL.data(), nv, nx + nu)) return rc;
        }
        std::vector<double> LBL((size_t)(nu + nx) * nv);
        {   // [L ; B L]  ((nu+nx) x nv) for the forward GEMM
            std::vector<double> BLm((size_t)nx * nv);
            h_gemm(false, false, nx, nv, nu, s->matB, nx, s->matL, nu, BLm.data());
            for (int j = 0; j < nv; j++) {
                for (int i = 0; i < nu; i++) LBL[i + (size_t)j * (nu + nx)] = s->matL[i + (size_t)j * nu];
                for (int i = 0; i < nx; i++) LBL[nu + i + (size_t)j * (nu + nx)] = BLm[i + (size_t)j * nx];
            }
            if (int rc = upload_padded(d_LBLp, LBL.data(), nu + nx, nv)) return rc;
            if (int rc = upload_fragments(d_LBLf, LBL.data(), nu + nx, nv)) return rc;
        }
        std::vector<double> RTm((size_t)nv * (nv + nx));
        std::copy(h_Rinv.begin(), h_Rinv.end(), RTm.begin());
        std::copy(T1.begin(), T1.end(), RTm.begin() + (size_t)nv * nv);
        if (int rc = upload_padded(d_RTp, RTm.data(), nv, nv + nx)) return rc;
        if (int rc = upload_fragments(d_RTf, RTm.data(), nv, nv + nx)) return rc;
        if (structured && lin_fits()) {   // [Rinv | T1 | T2]: nv x (nv + nx + nu)
            const size_t no = (size_t)pad16(nv) * pad4(nv + nx + nu);
            if (!d_RT2p) {
                if (int rc = dalloc(&d_RT2p, no)) return rc;
                if (int rc = dalloc(&d_RT2f, no)) return rc;
                if (int rc = dalloc(&d_sk2, (size_t)d.nodes * (nv + nx + nu))) return rc;
                if (int rc = dalloc(&d_rkq2, (size_t)d.nodes * (nv + 2 * nx + nu))) return rc;
                if (int rc = dalloc(&d_T12p, (size_t)pad16(nv) * pad4(nx + nu))) return rc;
                if (int rc = dalloc(&d_T12f, (size_t)pad16(nv) * pad4(nx + nu))) return rc;
                if (int rc = dalloc(&d_vconst, (size_t)d.nodes * nv)) return rc;
                if (int rc = dalloc(&d_MCp, (size_t)pad16(nu + nx) * pad4(nx + nu))) return rc;
                if (int rc = dalloc(&d_MCf, (size_t)pad16(nu + nx) * pad4(nx + nu))) return rc;
                if (int rc = dalloc(&d_lvconst, (size_t)d.nodes * (nu + nx))) return rc;
            }
            std::vector<double> RT2((size_t)nv * (nv + nx + nu));
            std::copy(RTm.begin(), RTm.end(), RT2.begin());
            std::copy(T2.begin(), T2.end(), RT2.begin() + (size_t)nv * (nv + nx));
            if (int rc = upload_padded(d_RT2p, RT2.data(), nv, nv + nx + nu)) return rc;
            if (int rc = upload_fragments(d_RT2f, RT2.data(), nv, nv + nx + nu)) return rc;
            if (int rc = upload_padded(d_T12p, RT2.data() + (size_t)nv * nv, nv, nx + nu)) return rc;       // [T1 | T2]: the columns behind Rinv
            if (int rc = upload_fragments(d_T12f, RT2.data() + (size_t)nv * nv, nv, nx + nu)) return rc;
            {   // MC = [L ; B L] [T1 | T2]: (nu + nx) x (nx + nu)
                std::vector<double> MC((size_t)(nu + nx) * (nx + nu));
                h_gemm(false, false, nu + nx, nx + nu, nv, LBL.data(), nu + nx, RT2.data() + (size_t)nv * nv, nv, MC.data());
                if (int rc = upload_padded(d_MCp, MC.data(), nu + nx, nx + nu)) return rc;
                if (int rc = upload_fragments(d_MCf, MC.data(), nu + nx, nx + nu)) return rc;
            }
            linConstValid = false;
        }
        if (int rc = upload_padded(d_Lp, s->matL, nu, nv)) return rc;
        if (int rc = upload_padded(d_Bp, s->matB, nx, nu)) return rc;
        UP(d_Rinv, h_Rinv.data(), nv * nv) UP(d_Bbt, h_Bbt.data(), nv * nx) UP(d_L, s->matL, nu * nv) UP(d_B, s->matB, nx * nu)
        UP(d_Lt, Lt.data(), nv * nu) UP(d_WLt, WLt.data(), nv * nu) UP(d_T1, T1.data(), nv * nx) UP(d_T2, T2.data(), nv * nu)
        UP(d_Gd, s->matGd, nx * nd) UP(d_Lhat, s->matLhat, nu * nd) UP(d_alpha1, s->costAlpha1, nu) UP(d_W, s->costW, nu * nu)
        UP(d_dy, dy.data(), (size_t)N * ny)
        if (!keepBounds) {      // back to one row for the whole tree (rn_set_bounds)
            if (!d_bloG[0]) { d_bloG[0] = d_blo; d_bhiG[0] = d_bhi; }
            d_blo = d_bloG[0]; d_bhi = d_bhiG[0]; boundsGran = RN_BOUNDS_SHARED;
            UP(d_blo, blo.data(), ny) UP(d_bhi, bhi.data(), ny)
        }
#undef UP
        if (d_Wp) { if (int rc = upload_padded(d_Wp, s->costW, nu, nu)) return rc; }   // k_value_mfma's copy of W (rn_set_algorithm may come before the factor step)
        if (int rc = stream_split_setup()) return rc;
        if (!structured && !d_A && !d_A32) {   // the dense per-node blocks are only allocated when they are used
            if (store32()) { if (int rc = dalloc(&d_A32, (size_t)d.nodes * strideA)) return rc; }
            else if (int rc = dalloc(&d_A, (size_t)d.nodes * strideA)) return rc;
        }
        RN_HIP(hipMemsetAsync(d_my, 0, (size_t)d.nodes * 2 * nv * sizeof(T), stream));   // structured mode never writes m1
        if (int rc = launch_expand()) return rc;
        factored = true;
        lip_invalidate();
        if (int rc = refresh_bounds_copies()) return rc;
        RN_HIP(hipStreamSynchronize(stream));
        return RN_OK;
    }
    // the part of the factor step that depends on p_i: the scaled bounds and, where the context holds dense blocks, the blocks themselves
    // (Engine.cu:721-745), in the storage type in force.  One launch on the context's stream (rn_factor_step, rn_set_tree_data)
    int launch_expand() {
        const int nx = d.nx, nu = d.nu, nv = d.nv;
        ExpandArgs<T> ea{};
        ea.tr = tree_dev(); ea.nx = nx; ea.nu = nu; ea.nv = nv; ea.ny = ny; ea.LD = LD; ea.strideA = strideA; ea.nodes = d.nodes;
        ea.T1 = d_T1; ea.T2 = d_T2; ea.Bbt = d_Bbt; ea.Lt = d_Lt; ea.A = d_A; ea.skipBlocks = structured; ea.blo = d_blo; ea.bhi = d_bhi; ea.lo = d_lo; ea.hi = d_hi;
        ea.bStrideStage = b_stride_stage(); ea.bStrideNode = b_stride_node();
        const int colChunks = std::min(ny, 8);
        bool expanded = false;
        if constexpr (sizeof(T) == 8) {
            if (store32() && !structured) {   // the same formulas evaluated in double, every entry rounded once on its way into the fp32 block
                ExpandArgs<double, float> ef{};
                ef.tr = ea.tr; ef.nx = nx; ef.nu = nu; ef.nv = nv; ef.ny = ny; ef.LD = LD; ef.strideA = strideA; ef.nodes = d.nodes;
                ef.T1 = d_T1; ef.T2 = d_T2; ef.Bbt = d_Bbt; ef.Lt = d_Lt; ef.A = d_A32; ef.skipBlocks = structured; ef.blo = d_blo; ef.bhi = d_bhi; ef.lo = d_lo; ef.hi = d_hi;
                ef.bStrideStage = ea.bStrideStage; ef.bStrideNode = ea.bStrideNode;
                hipLaunchKernelGGL((k_expand_operators<double, float>), dim3(d.nodes, colChunks), dim3(LD >= 192 ? 256 : (LD >= 96 ? 128 : 64)), 0, stream, ef);
                expanded = true;
            }
        }
        if (!expanded) hipLaunchKernelGGL(k_expand_operators<T>, dim3(d.nodes, colChunks), dim3(LD >= 192 ? 256 : (LD >= 96 ? 128 : 64)), 0, stream, ea);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    int set_tree_errors(const double *ed, const double *ep) override {
        RN_CHECK(ed && ep, RN_E_ARG, "rn_set_tree_errors: null input");
        RN_HIP(hipSetDevice(device));
        if (int rc = upload(d_errD, ed, (size_t)d.nodes * d.nd)) return rc;
        return upload(d_errP, ep, (size_t)d.nodes * d.nu);
    }
    int set_uncertainty(int dflag, int pflag, double w) override { useErrD = dflag ? 1 : 0; useErrP = pflag ? 1 : 0; wEco = w; return RN_OK; }
    int update_state_control(const double *x0, const double *up, const double *dp) override {
        RN_CHECK(factored, RN_E_STATE, "rn_update_state_control before rn_factor_step");
        RN_CHECK(x0 && up && dp, RN_E_ARG, "rn_update_state_control: null input");
        RN_HIP(hipSetDevice(device));
        if (int rc = upload(d_curX, x0, d.nx)) return rc;
        if (int rc = upload(d_prevU, up, d.nu)) return rc;
        if (int rc = upload(d_prevD, dp, d.nd)) return rc;
        hipLaunchKernelGGL(k_gemv_small<T>, dim3(1), dim3(128), 0, stream, d_Lhat, d.nu, d.nd, d_prevD, d_prevUhat);  // Engine.cu:1314
        RN_HIP(hipGetLastError());
        aux_dirty = true;
        return RN_OK;
    }
    int eliminate(const double *dhat, const double *ahat) override {
        RN_CHECK(factored, RN_E_STATE, "rn_eliminate_input_disturbance_coupling before rn_factor_step");
        RN_CHECK(dhat && ahat, RN_E_ARG, "rn_eliminate_input_disturbance_coupling: null input");
        RN_HIP(hipSetDevice(device));
        if (int rc = upload(d_dhat, dhat, (size_t)d.N * d.nd)) return rc;
        if (int rc = upload(d_ahat, ahat, (size_t)d.N * d.nu)) return rc;
        if (treeCheckPending) {   // (the uploads above have synchronised the stream: the counts of the last rn_set_tree_data_device are complete)
            int cnt[TREE_MAX_BLOCKS];
            RN_HIP(hipMemcpyAsync(cnt, d_treeBad, sizeof cnt, hipMemcpyDeviceToHost, stream));
            RN_HIP(hipStreamSynchronize(stream));
            treeBadCount = 0;
            for (int v : cnt) treeBadCount += v;
            treeCheckPending = false; treeBad = treeBadCount > 0;
        }
        RN_CHECK(!treeBad, RN_E_ARG, "rn_eliminate_input_disturbance_coupling: rn_set_tree_data_device was given " + std::to_string(treeBadCount) +
                 " probNode entries that are not positive and finite; set valid probabilities first");
        AffineArgs<T> a{};
        a.tr = tree_dev(); a.nx = d.nx; a.nu = d.nu; a.nv = d.nv; a.nd = d.nd;
        a.Gd = d_Gd; a.Lhat = d_Lhat; a.WLt = d_WLt; a.Lt = d_Lt; a.errD = d_errD; a.errP = d_errP; a.dhat = d_dhat; a.ahat = d_ahat;
        a.alpha1 = d_alpha1; a.prevUhat = d_prevUhat; a.wEco = (T)wEco; a.useErrD = useErrD; a.useErrP = useErrP;
        a.e = d_e; a.uhat = d_uhat; a.alpha = d_alpha; a.beta = d_beta;
        RN_CHECK(cutStage <= 0 || nranks == 1 || moments_set, RN_E_STATE, "sharded context: rn_set_cut_children_moments must be called before the affine terms");
        a.momE = (cutStage > 0 && moments_set) ? d_momE : nullptr; a.momP = d_momP; a.cutStage = cutStage;
        const size_t sh1 = (size_t)(((d.nd + 3) & ~3) + ((std::max(d.nx, d.nu) + 3) & ~3) + AFF_THREADS) * sizeof(T);
        const size_t sh2 = (size_t)(2 * ((d.nu + 3) & ~3) + ((std::max(d.nv, d.nu) + 3) & ~3) + ((d.nv + 3) & ~3) + ((d.nd + 3) & ~3) + AFF_THREADS) * sizeof(T);
        hipEvent_t e0 = prof_begin(3);
        hipLaunchKernelGGL(k_affine_demand<T>, dim3(d.nodes), dim3(AFF_THREADS), sh1, stream, a);
        hipLaunchKernelGGL(k_affine_beta<T>, dim3(d.nodes), dim3(AFF_THREADS), sh2, stream, a);
        prof_end(e0);
        RN_HIP(hipGetLastError());
        affine_ready = true; aux_dirty = true;
        return RN_OK;
    }
    int set_parameters(double step, double px, double pxs) override {
        RN_CHECK(step > 0 && std::isfinite(step), RN_E_ARG, "rn_set_parameters: stepSize must be positive");
        stepFixed = step; apply_step_size(step); penX = px; penXs = pxs;      // (under RN_STEP_LIPSCHITZ the next solve replaces the step size on entry)
        return RN_OK;
    }

    // ---- profiling helpers -----------------------------------------------------------------------------
    hipEvent_t get_event() {
        if (!freeEvents.empty()) { hipEvent_t e = freeEvents.back(); freeEvents.pop_back(); return e; }
        hipEvent_t e; (void)hipEventCreate(&e); return e;
    }
    // returns the closing event of the interval (a handle: intervals nest -- the collectives sit inside class 1 -- and `pending`
    // may grow in between), nullptr while profiling is off
    int profOpen = 0;
    hipEvent_t prof_begin(int cls) {
        if (!prof) return nullptr;
        if (pending.size() >= 60000 && profOpen == 0) (void)prof_flush();
        pending.push_back(EvPair{cls, get_event(), get_event()});
        (void)hipEventRecord(pending.back().a, stream);
        profOpen++;
        return pending.back().b;
    }
    void prof_end(hipEvent_t e) { if (e) { (void)hipEventRecord(e, stream); profOpen--; } }
    int prof_flush() {
        if (pending.empty()) return RN_OK;
        RN_HIP(hipStreamSynchronize(stream));
        for (auto &p : pending) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { prof_ms[p.cls] += ms; prof_n[p.cls]++; }
            freeEvents.push_back(p.a); freeEvents.push_back(p.b);
        }
        pending.clear();
        profOpen = 0;
        return RN_OK;
    }
    int profile_enable(int on) override { if (!on) { int rc = prof_flush(); prof = 0; return rc; } prof = on; return RN_OK; }
    int profile_reset() override { int rc = prof_flush(); for (int i = 0; i < 5; i++) { prof_ms[i] = 0; prof_n[i] = 0; } return rc; }
    int profile_read(double *ms, long *n) override {
        int rc = prof_flush();
        for (int i = 0; i < 4; i++) { ms[i] = prof_ms[i]; n[i] = prof_n[i]; }
        return rc;
    }
    // time between hipEvents recorded on the solver's stream around every all-reduce (RCCL or the installed stand-in) while
    // profiling is on: from the end of the kernel in front of the collective to the end of the collective, i.e. wire latency
    // AND the wait for the slowest peer.  The launches of class 1 (recursion + shared products) contain these intervals.
    int profile_read_collective(double *ms, long *n) override {
        RN_CHECK(ms && n, RN_E_ARG, "rn_profile_read_collective: null output");
        int rc = prof_flush();
        *ms = prof_ms[4]; *n = prof_n[4];
        return rc;
    }
    int algorithmic_bytes(double *bwd, double *dual) const override {
        // k_stream_gemv, one launch = the whole tree: A_i (2nv x ny, unpadded) read once + y_i read + m1,m2,a_i written
        // (fp32 storage under fp64 iterates: the block at 4 bytes per entry, the vectors at 8)
        // With the skip (stream_walk, stream_walk_half) the block bytes are those of the units the MOST RECENT launch walked: whole spans at G * LD entries, the
        // ragged last span at its ny % G columns -- or, where the launch skips half-spans by themselves (stream_half_on), live halves at G / 2 columns and
        // those of a ragged span at the columns they have; before any launch and with RN_KNOB_STREAM_SKIP = 0 the dense figure
        const double s = sizeof(T), n = d.nodes, sa = block_elem();
        if (bwd) {
            *bwd = structured ? 0.0 : n * ((double)2 * d.nv * ny * sa + (ny + 2.0 * d.nv + d.nx) * s);
            if (!structured && stream_skip() && lastStreamGrid > 0) {
                int G, NL;
                stream_shape(&G, &NL);
                if (stream_half_on(G, NL)) {
                    long long units = 0, ragUnits = 0, ragCols = 0;
                    if (int rc = const_cast<Ctx *>(this)->stream_units_sum(&units, &ragUnits, &ragCols)) return rc;
                    *bwd = ((double)(units - ragUnits) * (G / 2) + (double)ragCols) * LD * sa + n * (ny + 2.0 * d.nv + d.nx) * s;
                } else {
                    long long live[4], ragged = 0;
                    if (int rc = const_cast<Ctx *>(this)->stream_live_sum(live, &ragged)) return rc;      // (a copy from the device: changes nothing the context computes)
                    *bwd = ((double)(live[0] - ragged) * G + (double)ragged * (ny % G)) * LD * sa + n * (ny + 2.0 * d.nv + d.nx) * s;
                }
            }
        }
        // fused dual update: Hx, w, y+prev read, y+, w_next written (+ the two scaled-bound streams unless they are regenerated)
        // (RN_BOUNDS_PER_NODE, rn_set_bounds: the unscaled tables are two streams of their own again)
        if (dual) *dual = (RN_DUAL_REGEN && boundsGran != RN_BOUNDS_PER_NODE ? 5.0 : 7.0) * (double)ntot() * s;
        return RN_OK;
    }
    int synchronize() override { RN_HIP(hipSetDevice(device)); RN_HIP(hipStreamSynchronize(stream)); return RN_OK; }
    void *stream_handle() override { return (void *)stream; }

    // ---- the sweep: launch shapes, kernel selectors, plan, steps, and the main pass of the dual update --------
#include "sweep.inc"
    int main_partials() const { return mainPartials; }
    DualArgs<T> dual_args() const {
        DualArgs<T> a{};
        a.hx = d_hx; a.w = p_acc; a.yprev = p_upd; a.lo = d_lo; a.hi = d_hi;
        a.ynew = p_xi; a.wnext = p_acc_other; a.z = d_z; a.res = d_res;
        a.n = ntot(); a.nx = d.nx; a.ny = ny;
        a.lambda = (T)stepSize; a.invLambda = (T)(1.0 / stepSize);
        // the kernels index it by iteration: lamNext[t + 1] = entry t + 1 - lamBase of the sequence.  With lamBase > 0 the pointer stands IN
        // FRONT of the allocation; the invariant that keeps every access inside it: the only read is lamNext[t + 1] of the iteration t being
        // run (k_dual_fused), and t >= lamBase for every iteration behind a restart (lamBase is h_it at the restart, the device's counter runs
        // with h_it), t + 1 - lamBase <= lamCap - 1 by ensure_tables.  A kernel that read lamNext[t] with t < lamBase would read outside.
        a.lamNext = d_lam - lamBase;
        a.thrX = penX / stepSize; a.thrS = penXs / stepSize;
        a.st = d_state; a.partials = d_partials;
        a.crownElems = 0; a.countCrown = 1;
        a.finalizedEarly = 0; a.hist = d_hist; a.histParts = d_histParts; a.histCap = histCap;
        if (cutStage > 0) { a.crownElems = h_stageCum[cutStage] * ny; a.countCrown = (rank == 0); }
        a.recN = -1;   // (only the launch that closes a batch publishes a record: run_batch)
        a.regen = RN_DUAL_REGEN; a.stageOf = d_stageOf; a.sqrtp = d_sqrtp; a.dy = d_dy; a.blo = d_blo; a.bhi = d_bhi;
        a.bStrideStage = b_stride_stage(); a.bStrideNode = b_stride_node();
        return a;
    }
    int lamUploaded = 0;   // leading entries of h_lam that are on the device (kept across restarts: the theta recursion always starts at (1, 1))
    int ensure_tables(int upto) {  // lambda table and history capacity for iterations [0, upto]
        if (upto + 2 > lamCap) {
            const int cap = std::max(1024, 2 * (upto + 2));
            double *nl = nullptr, *nh = nullptr, *np = nullptr;
            if (int rc = dalloc(&nl, cap)) return rc;
            if (int rc = dalloc(&nh, cap)) return rc;
            if (int rc = dalloc(&np, (size_t)4 * cap)) return rc;
            if (int rc = dalloc(&d_histGlob, (size_t)4 * cap + 2)) return rc;
            RN_HIP(hipStreamSynchronize(stream));
            if (d_hist && histCap) {
                RN_HIP(hipMemcpy(nh, d_hist, histCap * sizeof(double), hipMemcpyDeviceToDevice));
                RN_HIP(hipMemcpy(np, d_histParts, (size_t)4 * histCap * sizeof(double), hipMemcpyDeviceToDevice));
            }
            d_lam = nl; d_hist = nh; d_histParts = np; lamCap = cap; histCap = cap;   // old arrays are freed with the context
            lamUploaded = 0;
        }
        // the theta recursion (SmpcController.cu:1513-1520) is a fixed sequence: the table is filled up to the device array's capacity at once
        // and uploaded ONCE per capacity, so that a batch in steady state starts without a copy and a host sync of its own
        while ((int)h_lam.size() < lamCap) {
            h_lam.push_back(theta1 * (1.0 / theta0 - 1.0));
            theta0 = theta1;
            theta1 = 0.5 * (std::sqrt(std::pow(theta1, 4) + 4 * std::pow(theta1, 2)) - std::pow(theta1, 2));
        }
        if (lamUploaded >= upto + 2) return RN_OK;
        RN_HIP(hipMemcpyAsync(d_lam, h_lam.data(), (size_t)lamCap * sizeof(double), hipMemcpyHostToDevice, stream));
        RN_HIP(hipStreamSynchronize(stream));   // (pageable source)
        lamUploaded = lamCap;
        return RN_OK;
    }
    int apg_reset() override {
        RN_HIP(hipSetDevice(device));
        // the optimistic paths' checkpoint buffers: allocated here, not inside a (possibly timed) rn_apg_iterate
        if (optimistic) for (int i = 0; i < 3; i++) if (!d_ck[i]) { if (int rc = dalloc(&d_ck[i], (size_t)ntot())) return rc; }
        const size_t bytes = (size_t)ntot() * sizeof(T);
        for (int i = 0; i < 2; i++) { RN_HIP(hipMemsetAsync(d_ybuf[i], 0, bytes, stream)); RN_HIP(hipMemsetAsync(d_wbuf[i], 0, bytes, stream)); }
        RN_HIP(hipMemsetAsync(d_hx, 0, bytes, stream));
        RN_HIP(hipMemsetAsync(d_z, 0, bytes, stream));
        RN_HIP(hipMemsetAsync(d_state, 0, sizeof(IterState), stream));
        p_xi = d_ybuf[0]; p_upd = d_ybuf[1]; p_acc = d_wbuf[0]; p_acc_other = d_wbuf[1]; p_acc_view = p_acc;
        acc_ready = true;  // w_0 = (1+l) 0 - l 0 = 0
        poisoned = false;
        h_it = 0;      // (the lambda table is the same fixed sequence after every restart: kept, with its device copy)
        lamBase = 0;
        return ensure_tables(0);
    }
    // warm start: keep the duals of the previous control step, restart the momentum (theta = {1,1} => w_0 = y+)
    int apg_restart_keep_duals() {
        RN_HIP(hipSetDevice(device));
        RN_HIP(hipMemcpyAsync(p_xi, p_upd, (size_t)ntot() * sizeof(T), hipMemcpyDeviceToDevice, stream));   // y := y+
        RN_HIP(hipMemsetAsync(d_state, 0, sizeof(IterState), stream));
        h_it = 0;
        lamBase = 0;
        acc_ready = false;   // the first iteration re-derives w_0 = (1 + 0) y+ - 0 y
        return ensure_tables(0);
    }
    // The restart INSIDE a solve (rn_set_restart, decided at a batch end by solve_loop): y := y+, the next iteration re-derives w = y+ from
    // the first entry of the lambda sequence (0) -- and nothing else moves: the iteration count, the history, the device's iteration state
    // (its counter indexes the history; tripped / scale / dist are rewritten by every iteration, the verdict flag by every batch opening)
    // and the batch counters are the solve's.
    int momentum_restart() {
        RN_HIP(hipMemcpyAsync(p_xi, p_upd, (size_t)ntot() * sizeof(T), hipMemcpyDeviceToDevice, stream));   // y := y+
        acc_ready = false;
        lamBase = h_it;
        return RN_OK;
    }
    int restart_buffers() {
        if (d_rt) return RN_OK;
        RN_HIP(hipSetDevice(device));
        if (int rc = dalloc(&d_rt, (size_t)6 * ELT_MAX_BLOCKS + 1)) return rc;
        RN_HIP(hipMemsetAsync(d_rt, 0, ((size_t)6 * ELT_MAX_BLOCKS + 1) * sizeof(double), stream));
        return RN_OK;
    }
    // k_restart_test on (w_k, y_{k+1}, y_k) = (p_acc_view, p_upd, p_xi) as they stand behind a batch's rotation; the result lands in the batch
    // record (d_state->rec; single GPU: also in the host-mapped copy).  Sharded: every rank's sum counts its own subtree rows, rank 0's the
    // replicated crown as well; the three doubles are summed over the ranks, then passed through a MAX all-reduce so that every rank holds
    // the same bits -- hence takes the same decision -- whatever order a collective added them in.
    int launch_restart_test(bool sharded) {
        RestartArgs a{};
        a.f64 = sizeof(T) == 8 ? 1 : 0;
        a.w = p_acc_view; a.yp = p_upd; a.y = p_xi; a.n = ntot();
        a.crownElems = 0; a.countCrown = 1;
        if (cutStage > 0) { a.crownElems = (long long)h_stageCum[cutStage] * ny; a.countCrown = (rank == 0); }
        a.partials = d_rt; a.ticket = reinterpret_cast<unsigned int *>(d_rt + (size_t)6 * ELT_MAX_BLOCKS);
        a.st = d_state; a.hostRec = sharded ? nullptr : h_rec;
        RN_HIP(hipMemsetAsync(a.ticket, 0, sizeof(double), stream));
        hipEvent_t e3 = prof_begin(3);
        hipLaunchKernelGGL(k_restart_test<>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, a);
        prof_end(e3);
        RN_HIP(hipGetLastError());
        if (sharded) {
            if (int rc = all_reduce(&d_state->rec.g, 3, true, "ncclAllReduce(restart test)")) return rc;
            if (int rc = all_reduce(&d_state->rec.g, 3, true, "ncclAllReduce(restart test, agreement)", 2 /* ncclMax */)) return rc;
        }
        return RN_OK;
    }
    int set_warm_start(int on) override { warmStart = on ? 1 : 0; return RN_OK; }
    size_t cut_tail_offset() const { return (size_t)(h_stageCum[cutStage] - h_stageCum[cutStage - 1]) * (d.nv + 2 * d.nx); }
    // The iterate state a batch starts from, as far as it is not in the checkpoint buffers (d_ck: y, y+, w -- written by batch_open):
    // which buffer plays which role, and the iteration count.  restore_iterates puts a context back there (the replay of a tripped batch;
    // the timing runs of the exchange auto-tuner).
    struct IterSave { T *xi, *upd, *acc, *other; bool ready; int it; };
    IterSave save_iterates() const { return IterSave{p_xi, p_upd, p_acc, p_acc_other, acc_ready, h_it}; }
    int restore_iterates(const IterSave &sv) {
        const size_t bytes = (size_t)ntot() * sizeof(T);
        p_xi = sv.xi; p_upd = sv.upd; p_acc = sv.acc; p_acc_other = sv.other; p_acc_view = p_acc; acc_ready = sv.ready;
        RN_HIP(hipMemcpyAsync(p_xi, d_ck[0], bytes, hipMemcpyDeviceToDevice, stream));
        RN_HIP(hipMemcpyAsync(p_upd, d_ck[1], bytes, hipMemcpyDeviceToDevice, stream));
        RN_HIP(hipMemcpyAsync(p_acc, d_ck[2], bytes, hipMemcpyDeviceToDevice, stream));
        h_it = sv.it;
        RN_HIP(hipMemcpyAsync(&d_state->it, &sv.it, sizeof(int), hipMemcpyHostToDevice, stream));
        RN_HIP(hipStreamSynchronize(stream));   // (sv.it is the caller's)
        return RN_OK;
    }
    int batch_open(T *tail) {
        const long long n = ntot();
        const int blocks = (int)std::max<long long>(1, std::min<long long>((n / (16 / (long long)sizeof(T)) + ELT_THREADS - 1) / ELT_THREADS, (long long)numCUs * 8));
        hipLaunchKernelGGL(k_batch_open<T>, dim3(blocks), dim3(ELT_THREADS), 0, stream, (const T *)p_xi, (const T *)p_upd, (const T *)p_acc, d_ck[0], d_ck[1], d_ck[2], n, d_state, tail);
        RN_HIP(hipGetLastError());   // a checkpoint that was not taken must not be replayed from
        return RN_OK;
    }
    // One rn_apg_iterate batch of n iterations.  Exact: every iteration decides on the prox before it finishes its dual update -- single
    // GPU in the small fix-up launch (decideHere), sharded after an all-reduce of the ranks' dist^2.  Optimistic: the prox runs as a pure
    // projection (what happens unless a tree-global distance exceeds gamma/lambda, SmpcController.cu:793/811), and instead of a decision
    // after every iteration the fold of its partials, its history entry and its distance check ride in the next iteration's first chain
    // launch (single GPU) or cut launch (sharded: every rank's dist^2 rides in the tail of the cut payload -- ONE collective per iteration).
    // If a threshold was exceeded anywhere in the batch, the batch is replayed from its checkpoint as an exact batch: the result is exact
    // either way.
    // recTol >= 0: the batch is run under a stop tolerance -- its closing launch scans the batch's history entries for recTol, and the host
    // reads the batch record (lastRec) behind the batch's synchronisation: the one an optimistic batch has anyway, one of its own for an exact
    // batch.  recTol < 0: nobody asked, nothing is scanned and an exact batch does not synchronise.  A replayed batch is judged on the replay's record.
    // rtest (with recTol >= 0): the gradient restart test is evaluated on the batch's final iterates, in front of the same synchronisation.
    int run_batch(int n, double *primalInfs, bool optimistic, double recTol = -1.0, bool rtest = false) {
        Batch b{};
        b.optimistic = optimistic; b.sharded = has_comm() && cutStage > 0;
        const int first = h_it;
        if (b.optimistic) for (int i = 0; i < 3; i++) if (!d_ck[i]) { if (int rc = dalloc(&d_ck[i], (size_t)ntot())) return rc; }
        if (int rc = ensure_tables(h_it + n)) return rc;
        T *const tail = b.carry_tail() ? d_cut + cut_tail_offset() : nullptr;
        IterSave saved{};
        if (b.optimistic) {   // checkpoint of (y, y+, w), the payload's dist^2 tail (sharded) and the verdict flag cleared: one launch
            if (int rc = batch_open(tail)) return fail_batch(rc);
            saved = save_iterates();
        }
        for (int k = 0; k < n; k++) {
            const bool last = k == n - 1;
            if (!acc_ready) {   // re-derive w_t after manual buffer edits (SmpcController.cu:1514)
                launch_extrapolate(h_lam[h_it - lamBase]);
                acc_ready = true;
            }
            b.fuseReq = b.optimistic && fuse_want();
            if (b.fuseReq) { b.fuseArgs = dual_args(); b.fuseMat = last; b.fuseLn = h_lam[h_it + 1 - lamBase]; }
            if (int rc = launch_sweep(&b, 0, nullptr, last)) return fail_batch(rc);
            b.fuseReq = false;
            DualArgs<T> a = dual_args();
            hipEvent_t e2 = prof_begin(2);
            if (!std::exchange(b.fuseDone, false)) launch_dual_main(b, a, last);
            prof_end(e2);
            if (b.optimistic && !last) b.pendingFin = true;   // this iteration's bookkeeping rides in the next sweep
            else {
                hipEvent_t e3 = prof_begin(3);
                if (b.optimistic) {   // the batch's last bookkeeping gets a launch of its own
                    run_close_optimistic(a, main_partials(), tail, b.sharded, first, recTol >= 0 ? n : 0, recTol, h_rec);
                } else if (b.sharded) {   // tree-global distances: sum the ranks' dist^2 (2 doubles) before deciding
                    if (int rc = run_close_exact_sharded(a, last, d_dist2)) return fail_batch(rc);
                } else {   // single GPU: the (small) fix-up launch also decides and does the bookkeeping (kernels.hpp, decideHere)
                    a = exact_fixup_args(a, h_it, main_partials(), d_partials2);
                    if (last && recTol >= 0) { a.recFirst = first; a.recN = n; a.recTol = recTol; a.hostRec = h_rec; }   // the launch that closes the batch
                    run_exact_fixup(a, last);
                }
                prof_end(e3);
            }
            // rotate: y_t := y+_{t-1} (old upd), y+_t := buffer just written; w_{t+1} becomes the sweep input
            std::swap(p_xi, p_upd);
            p_acc_view = p_acc;
            std::swap(p_acc, p_acc_other);
            h_it++;
        }
        if (b.sharded && n > 0) {
            // optimistic: the last iteration's distances, one 2-element all-reduce per BATCH.  Then one more all-reduce per batch (MAX): the
            // batch's history entries become tree-global (vecPrimalInfs, SmpcController.cu:1521) and the ranks agree on the verdict (every
            // rank takes the same replay decision even if an all-reduce algorithm ever delivered sums that differ in the last bit between ranks)
            if (tail) { if (int rc = all_reduce(tail, 2, sizeof(T) == 8, "ncclAllReduce(dist tail)")) return fail_batch(rc); }
            if (int rc = globalize_history(first, n, tail, recTol)) return fail_batch(rc);
        }
        RN_HIP(hipGetLastError());
        if (rtest && n > 0 && recTol >= 0) { if (int rc = launch_restart_test(b.sharded)) return fail_batch(rc); }
        int violated = 0;
        const bool synced = n > 0 && (b.optimistic || recTol >= 0);
        if (synced) {   // the batch record: the verdict of an optimistic batch, and what a stop tolerance asks about
            if (!b.sharded && h_rec) {   // written by the batch's last launch (k_finalize_optimistic / the fix-up launch): no copy, one synchronisation
                RN_HIP(hipStreamSynchronize(stream));
                const volatile BatchRecord *r = h_rec;
                lastRec.verdict = r->verdict; lastRec.firstBelow = r->firstBelow; lastRec.lastResidual = r->lastResidual;
                lastRec.g = r->g; lastRec.na2 = r->na2; lastRec.nb2 = r->nb2;
            } else {   // sharded (k_batch_close_unpack: tree-global values, the same bits on every rank), or no mapped memory: one copy
                RN_HIP(hipMemcpyAsync(&lastRec, &d_state->rec, sizeof(BatchRecord), hipMemcpyDeviceToHost, stream));
                RN_HIP(hipStreamSynchronize(stream));
            }
            violated = b.optimistic ? lastRec.verdict : 0;
        }
        if (b.sharded && n > 0 && transport == 1 && peerReady) { if (int rc = check_comm_fail()) return fail_batch(rc); }
        if (violated) {   // the same n iterations once more from the checkpoint, as an exact batch; so are the next RN_OPT_BACKOFF batches
            fallbacks++;
            if (int rc = restore_iterates(saved)) return fail_batch(rc);
            optHold = RN_OPT_BACKOFF;
            return run_batch(n, primalInfs, false, recTol, rtest);
        }
        if (primalInfs && n > 0) {
            if (!synced) RN_HIP(hipStreamSynchronize(stream));   // (an optimistic batch has synchronised for its verdict, a batch under a tolerance for its record)
            RN_HIP(hipMemcpy(primalInfs, d_hist + first, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        }
        return RN_OK;
    }
    // SmpcController::allocateApgAlgorithm sizes its per-iteration storage by maxIterations once (SmpcController.cu:124-151):
    // the iteration tables (lambda_k, vecPrimalInfs and its parts) and the optimistic paths' checkpoint buffers for `n` iterations
    // are allocated here, so that no control step allocates device memory (the reference's leak check, :1612-1623, would flag it)
    // ---- one-shot exchange at the cut (kernels.hpp, PeerTable) -----------------------------------------------------------------
    // The inbox of this rank: 2 buffers x nranks sources x slots elements of 8-byte packets, in UNCACHED device memory (no L2 of
    // either side may hold a packet back), exported as a hipIpcMemHandle_t; peers map it and write into it from their kernels.
    unsigned long long *d_inbox = nullptr;
    size_t inboxBytes = 0;
    PeerTable h_peer{};   // handed to the kernels by value (SweepArgs::peer)
    std::vector<void *> ipcOpened;
    bool peerReady = false;
    // Transport of the per-iteration exchange at the cut.  transportReq is what the caller asked for (RN_EXCHANGE_AUTO unless told:
    // rn_set_exchange_transport, $RAPIDNET_EXCHANGE), `transport` what the batches run: 0 = the communicator's all-reduce on the solver's
    // stream, 1 = one-shot peer writes.  AUTO is resolved by exchange_autotune -- by the first device-resident batch, or when the caller
    // asks (rn_exchange_autotune): both candidates run the context's own iterations, the ranks agree on the faster one.
    int transportReq = RN_EXCHANGE_AUTO, transport = 0;
    bool tuned = false, oneShotBroken = false;
    double tuneInfo[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // rn_exchange_autotune: {chosen, candidates, us/it collective (max over ranks), us/it one-shot (max), own collective, own one-shot, iterations, tunes run}
    double *d_tune = nullptr;    // 8 doubles: the ranks' agreement on the timings (allocated with the context: a control step never allocates)
    T *d_ckView = nullptr;       // the tuner's copy of the accelerated dual a getter would show (allocated when the one-shot transport becomes a candidate)
    // The forward walk and the dual update of the nodes it has walked in ONE launch (k_down_chain_dual): the optimistic batches ask for
    // it per iteration (Batch::fuseReq + the dual update's arguments), the sweep says whether it happened (Batch::fuseDone).
    // Default (round 6): on, with the number of workgroups per chain BY SHAPE (fuse_split) -- one where the chains (nearly) fill the chip: the whole
    // 493-scenario tree -2.2 % per iteration dense, -5.6 % structured, a 1/2 shard -0.7 %; several on small trees and smaller shards (with one, the 62
    // workgroups of a 1/8 shard cannot keep as many bytes in flight as the stage-tiled kernel's grid: +2.7 %; profiles/r06_ab_fuse_by_shape.txt).  rn_set_fused_walk_dual(ctx, 0 / 1) or
    // $RAPIDNET_FUSE_DOWN_DUAL = 0 / 1 (read when the context runs its first batch) force it either way; while the per-launch profiling
    // of rn_profile_enable is on, the dual update always runs as a launch of its own (the kernel north_star's roofline target names).
    int fuseMode = -2;     // -2: not decided yet ($RAPIDNET_FUSE_DOWN_DUAL, else by shape), -1: by shape, 0 / 1: forced
    int set_fused_walk_dual(int on) override { RN_CHECK(on >= -1 && on <= 1, RN_E_ARG, "rn_set_fused_walk_dual: 0, 1 or -1 (by shape)"); fuseMode = on; return RN_OK; }
    bool fuse_by_shape() const {      // (profiles/r06_ab_fuse_by_shape.txt: 493 chains -2.2 % dense / -5.6 % structured, 247 chains of a 1/2 shard -0.7 %, 124 chains: a tie,
        const int cs = chainStage, K = h_stageCum[cs + 1] - h_stageCum[cs];      //  62 and 31 chains: +3-4 % with ONE workgroup per chain)
        return 4 * K >= 3 * numCUs;
    }
    // workgroups per chain of the fused launch: one where the chains (nearly) fill the chip; otherwise up to four, as many as give every CU a
    // workgroup, each updating the dual of its own slice of the chain's rows (k_down_chain_dual, P) -- the dual update of a 1/8 shard's 62 chains
    // then runs on 248 workgroups instead of 62.  With that the one launch is never slower than the two (profiles/r06_ab_fuse_split.txt: 31-scenario
    // tree -1 ... -3 % dense, -4.4 % structured; 1/4 shard -1.1 %; 1/8 shard -0.5 %; more than four redo too much of the walk).
    // rn_debug_set_knob(RN_KNOB_FUSE_SPLIT): n > 0 forces n, 0 = one per chain and only by fuse_by_shape() (the rule before the split existed).
    int fuse_split() const {
        const int cs = chainStage, K = h_stageCum[cs + 1] - h_stageCum[cs], L = d.N - cs;
        if (knob[RN_KNOB_FUSE_SPLIT] > 0) return std::max(1, std::min(knob[RN_KNOB_FUSE_SPLIT], L));
        if (knob[RN_KNOB_FUSE_SPLIT] == 0 || fuse_by_shape()) return 1;
        return std::max(1, std::min(std::min(L, 4), numCUs / std::max(K, 1)));
    }
    bool fuse_want() {
        if (fuseMode == -2) { const char *e = std::getenv("RAPIDNET_FUSE_DOWN_DUAL"); fuseMode = e ? (std::atoi(e) != 0 ? 1 : 0) : -1; }
        const bool shapeSaysYes = knob[RN_KNOB_FUSE_SPLIT] == 0 ? fuse_by_shape() : true;
        return (fuseMode == 1 || (fuseMode == -1 && shapeSaysYes)) && dualU != 0 && !prof;
    }
    unsigned int peerSeq = 0;     // sequence number of the last one-shot exchange (the same on every rank: they issue the same exchanges)
    unsigned int peer_slots() const { return (unsigned int)((size_t)(h_stageCum[cutStage] - h_stageCum[cutStage - 1]) * (d.nv + 2 * d.nx) + 2); }
    int peer_inbox_create(void *handle64) override {
        RN_CHECK(handle64, RN_E_ARG, "rn_peer_inbox_create: null output");
        // (one rank: the context writes to and reads from its own inbox -- what a rank executes except the wire, for timing runs)
        RN_CHECK(cutStage > 0 && nranks >= 1 && nranks <= PEER_MAX, RN_E_STATE, "rn_peer_inbox_create: a sharded context (cut stage set) of at most 16 ranks is required");
        RN_HIP(hipSetDevice(device));
        if (!d_inbox) {
            inboxBytes = (size_t)2 * nranks * peer_slots() * PeerPk<T>::N * sizeof(unsigned long long);
            RN_HIP(hipExtMallocWithFlags((void **)&d_inbox, inboxBytes, hipDeviceMallocUncached));
            RN_HIP(hipMemset(d_inbox, 0, inboxBytes));      // tag 0 = "never written" (sequence numbers start at 1)
            RN_HIP(hipDeviceSynchronize());
        }
        hipIpcMemHandle_t h;
        static_assert(sizeof(hipIpcMemHandle_t) == 64, "rn_peer_inbox_create hands out 64-byte handles");
        RN_HIP(hipIpcGetMemHandle(&h, d_inbox));
        std::memcpy(handle64, &h, sizeof h);
        return RN_OK;
    }
    unsigned long long *peer_inbox_ptr() override { return d_inbox; }
    int peer_table_install() {
        h_peer.nranks = nranks; h_peer.rank = rank; h_peer.slots = peer_slots();
        double ms = 2000.0;   // a reader waits at most this long for a peer's packets, then gives up with RN_E_COMM
        if (const char *e = std::getenv("RAPIDNET_ONESHOT_TIMEOUT_MS")) { const double v = std::atof(e); if (v > 0) ms = v; }
        h_peer.timeoutTicks = (unsigned long long)(ms * 1e5);   // 100 MHz wall clock
        h_peer.own = h_peer.inbox[rank];
        peerReady = true; peerSeq = 0;
        return RN_OK;
    }
    int peer_inbox_connect(const void *handles, int n) override {
        RN_CHECK(handles && n == nranks, RN_E_ARG, "rn_peer_inbox_connect: one 64-byte handle per rank expected");
        RN_CHECK(d_inbox != nullptr, RN_E_STATE, "rn_peer_inbox_connect before rn_peer_inbox_create");
        // once per context: the sequence numbers of the ranks advance together from the connect on, and a second connect of one rank
        // would restart its tags over packets its peers still hold (a new set of peers needs a new context)
        RN_CHECK(!peerReady, RN_E_STATE, "rn_peer_inbox_connect: the inboxes of this context are already connected");
        RN_HIP(hipSetDevice(device));
        for (int r = 0; r < nranks; r++) {
            if (r == rank) { h_peer.inbox[r] = d_inbox; continue; }
            hipIpcMemHandle_t h;
            std::memcpy(&h, (const char *)handles + (size_t)64 * r, sizeof h);
            void *ptr = nullptr;
            RN_HIP(hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess));
            ipcOpened.push_back(ptr);
            h_peer.inbox[r] = (unsigned long long *)ptr;
        }
        return peer_table_install();
    }
    // the ranks are contexts of ONE process (tests): a peer's inbox is an ordinary device pointer of the same address space
    int peer_inbox_connect_local(CtxBase **peers, int n) override {
        RN_CHECK(peers && n == nranks, RN_E_ARG, "rn_debug_peer_inbox_connect_local: one context per rank expected");
        for (int r = 0; r < nranks; r++) {
            RN_CHECK(peers[r] && peers[r]->peer_inbox_ptr(), RN_E_STATE, "rn_debug_peer_inbox_connect_local: a rank has no inbox (rn_peer_inbox_create)");
            RN_CHECK(!peerReady, RN_E_STATE, "rn_debug_peer_inbox_connect_local: the inboxes of this context are already connected");
            h_peer.inbox[r] = peers[r]->peer_inbox_ptr();
        }
        RN_CHECK(h_peer.inbox[rank] == d_inbox, RN_E_ARG, "rn_debug_peer_inbox_connect_local: contexts must be given in rank order");
        RN_HIP(hipSetDevice(device));
        return peer_table_install();
    }
    int debug_peer_seq(unsigned int seq) override {      // test hook: the next exchange gets sequence number seq + 1 (all ranks alike)
        RN_CHECK(peerReady, RN_E_STATE, "rn_debug_peer_seq: connect the inboxes first");
        peerSeq = seq;
        return RN_OK;
    }
    int set_exchange_transport(int t) override {
        RN_CHECK(t == RN_EXCHANGE_COLLECTIVE || t == RN_EXCHANGE_ONESHOT || t == RN_EXCHANGE_AUTO, RN_E_ARG,
                 "rn_set_exchange_transport: RN_EXCHANGE_COLLECTIVE, RN_EXCHANGE_ONESHOT or RN_EXCHANGE_AUTO");
        if (t == RN_EXCHANGE_ONESHOT && !peerReady) { if (int rc = exchange_prepare()) return rc; }   // (a real communicator: the library wires the inboxes itself)
        RN_CHECK(t != RN_EXCHANGE_ONESHOT || peerReady, RN_E_STATE, "rn_set_exchange_transport: the peers' inboxes are not connected (rn_peer_inbox_connect, or a communicator over which the library can exchange the handles)");
        transportReq = t;
        transport = t == RN_EXCHANGE_ONESHOT ? 1 : 0;
        tuned = t != RN_EXCHANGE_AUTO;
        return RN_OK;
    }
    // ---- the exchange chooses itself (round 6) ----------------------------------------------------------------------------------
    // all-reduce of raw integers over the library's own communicator (the IPC handles travel this way: every rank fills its own slot of a
    // zeroed buffer, the sum is the gather)
    int all_reduce_bytes(void *buf, size_t count, const char *what) {
        RN_CHECK(comm != nullptr, RN_E_STATE, std::string(what) + ": no communicator");
        const int rc = g_nccl.AllReduce(buf, buf, count, 1 /* ncclUint8 */, 0 /* ncclSum */, comm, stream);
        RN_CHECK(rc == 0, RN_E_COMM, std::string(what) + " failed: " + (g_nccl.GetErrorString ? g_nccl.GetErrorString(rc) : "?"));
        return RN_OK;
    }
    // One-shot transport made available WITHOUT the caller's help: the inbox of this rank, its IPC handle gathered over the RCCL
    // communicator, the peers' inboxes mapped.  Collective (every rank of the communicator calls it at the same point: rn_comm_init /
    // rn_create_sharded / rn_set_exchange_transport(ONESHOT) do).  A rank that cannot create or map an inbox makes EVERY rank give the
    // transport up (a MAX all-reduce of the failure flags): returns RN_OK with peerReady == false, and AUTO then has one candidate.
    bool prepared = false;
    int exchange_prepare() {
        if (prepared || peerReady || oneShotBroken) return RN_OK;
        // (stand-in communicators: the test wires the inboxes.  A ONE-rank communicator goes through all of it too -- the rank's own inbox, the
        //  gather, the agreement: what a one-GPU box can exercise of this path)
        if (comm == nullptr || nranks < 1 || nranks > PEER_MAX || cutStage <= 0) return RN_OK;
        prepared = true;
        RN_HIP(hipSetDevice(device));
        unsigned char handle[64] = {0};
        int bad = peer_inbox_create(handle) != RN_OK ? 1 : 0;
        unsigned char *d_h = nullptr;
        const size_t hb = (size_t)64 * nranks + 8;      // + the failure flags' slot
        if (hipMalloc((void **)&d_h, hb) != hipSuccess) { (void)hipGetLastError(); d_h = nullptr; bad = 1; }
        std::vector<unsigned char> all(hb, 0);
        if (d_h) {
            std::memcpy(all.data() + (size_t)64 * rank, handle, 64);
            all[(size_t)64 * nranks] = (unsigned char)(bad ? 1 : 0);      // (sum over <= 16 ranks: no overflow)
            if (hipMemcpyAsync(d_h, all.data(), hb, hipMemcpyHostToDevice, stream) != hipSuccess) bad = 1;
        }
        // every rank MUST issue the same collectives whatever happened to it: a rank without a buffer contributes through a fallback slot
        int rc = RN_OK;
        if (d_h) rc = all_reduce_bytes(d_h, hb, "ncclAllReduce(inbox handles)");
        else { err = "exchange_prepare: no device memory for the handle exchange"; rc = RN_E_HIP; }
        if (rc == RN_OK && (hipMemcpyAsync(all.data(), d_h, hb, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)) { (void)hipGetLastError(); rc = RN_E_HIP; }
        if (d_h) (void)hipFree(d_h);
        if (rc != RN_OK) { oneShotBroken = true; return rc; }      // the communicator itself failed: the caller must know
        if (all[(size_t)64 * nranks] == 0) {
            if (peer_inbox_connect(all.data(), nranks) != RN_OK) { (void)hipGetLastError(); bad = 1; }
        } else bad = 1;
        // second agreement: did every rank map every peer?
        double flag = bad ? 1.0 : 0.0;
        RN_HIP(hipMemcpyAsync(d_tune, &flag, sizeof flag, hipMemcpyHostToDevice, stream));
        if (int rc2 = all_reduce(d_tune, 1, true, "ncclAllReduce(inbox set-up verdict)", 2 /* ncclMax */)) { oneShotBroken = true; peerReady = false; return rc2; }
        RN_HIP(hipMemcpyAsync(&flag, d_tune, sizeof flag, hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        if (flag != 0.0) { peerReady = false; oneShotBroken = true; }      // somebody could not: nobody uses the transport (err keeps this rank's reason, if it was this rank)
        else if (transportReq == RN_EXCHANGE_ONESHOT) transport = 1;
        if (peerReady && transportReq == RN_EXCHANGE_AUTO && !d_ckView) { if (int rc3 = dalloc(&d_ckView, (size_t)ntot())) return rc3; }   // the tuner will run: its buffer now, not inside a control step
        return RN_OK;
    }
    // Times the candidates on THIS context's own iterations and keeps the faster: `iters` device-resident iterations per candidate (after
    // a warm-up run of half as many) from the current iterate state, which is restored afterwards -- iterates, iteration count, batch
    // counters: a caller cannot tell that the runs happened, except by the clock.  The ranks' times are combined by a MAX all-reduce, so
    // every rank takes the same decision.  Collective: every rank calls it at the same point (rn_apg_iterate does, in its first batch).
    int exchange_autotune(int iters) {
        RN_CHECK(factored && affine_ready, RN_E_STATE, "rn_exchange_autotune before the factor step / affine terms");
        RN_CHECK(!poisoned, RN_E_STATE, "rn_exchange_autotune: an earlier batch failed half-way; call rn_apg_reset first");
        RN_CHECK(iters >= 1, RN_E_ARG, "rn_exchange_autotune: iterations >= 1");
        RN_HIP(hipSetDevice(device));
        tuned = true;
        const bool sharded = has_comm() && cutStage > 0 && nranks >= 1 && optimistic;
        if (sharded && !peerReady) { if (int rc = exchange_prepare()) return rc; }
        const bool canOne = sharded && peerReady && !oneShotBroken;
        tuneInfo[1] = 1.0 + (canOne ? 2.0 : 0.0); tuneInfo[6] = 0; tuneInfo[2] = tuneInfo[3] = tuneInfo[4] = tuneInfo[5] = 0.0;
        if (!canOne) { transport = 0; tuneInfo[0] = 0; return RN_OK; }     // one candidate: nothing to time
        for (int i = 0; i < 3; i++) if (!d_ck[i]) { if (int rc = dalloc(&d_ck[i], (size_t)ntot())) return rc; }
        // what the timing runs must leave as they found it: the iterates, in a checkpoint taken here (each pass's own batch_open copies
        // the same values over it again: the passes start from the restored state), ...
        const IterSave sv = save_iterates();
        if (int rc = batch_open(nullptr)) return rc;
        const long kOpt = optBatches, kExact = exactBatches, kFall = fallbacks; const int kHold = optHold;
        // ... the counters, and what RN_BUF_ACC_* shows: after a batch that is w_t, in the buffer the timing runs are about to reuse (the checkpoint holds w_{t+1}, the next input)
        T *const view = p_acc_view;
        const size_t vbytes = (size_t)ntot() * sizeof(T);
        if (view != sv.acc) {
            if (!d_ckView) { if (int rc = dalloc(&d_ckView, (size_t)ntot())) return rc; }
            RN_HIP(hipMemcpyAsync(d_ckView, view, vbytes, hipMemcpyDeviceToDevice, stream));
        }
        double own[2] = {0, 0};
        int failed[2] = {0, 0};
        for (int cand = 0; cand < 2; cand++) {
            transport = cand;
            for (int pass = 0; pass < 2 && !failed[cand]; pass++) {
                const int n = pass == 0 ? std::max(iters / 2, 8) : iters;
                optHold = 0;
                const auto t0 = std::chrono::steady_clock::now();
                const int rc = run_batch(n, nullptr, true);     // ends with a synchronisation
                const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
                if (rc != RN_OK) {      // (a one-shot reader's time-out is every rank's RN_E_COMM: all ranks come here together)
                    failed[cand] = 1; poisoned = false;
                    (void)hipMemsetAsync(&d_state->commFail, 0, sizeof(int), stream);
                }
                if (pass == 1 && rc == RN_OK) own[cand] = us / n;
                if (int rc2 = restore_iterates(sv)) return fail_batch(rc2);
            }
        }
        optBatches = kOpt; exactBatches = kExact; fallbacks = kFall; optHold = kHold;
        if (view != sv.acc) { RN_HIP(hipMemcpyAsync(view, d_ckView, vbytes, hipMemcpyDeviceToDevice, stream)); p_acc_view = view; }
        if (knob[RN_KNOB_TUNE_BIAS_US] != -1) own[1] += (double)knob[RN_KNOB_TUNE_BIAS_US];      // test of the selection: this rank's one-shot time, biased
        // every rank the same figures: MAX over the ranks of {time collective, time one-shot, failed collective, failed one-shot}
        double h[4] = {own[0], own[1], (double)failed[0], (double)failed[1]};
        RN_HIP(hipMemcpyAsync(d_tune, h, sizeof h, hipMemcpyHostToDevice, stream));
        transport = 0;
        if (int rc = all_reduce(d_tune, 4, true, "ncclAllReduce(exchange timings)", 2 /* ncclMax */)) return rc;
        RN_HIP(hipMemcpyAsync(h, d_tune, sizeof h, hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        RN_CHECK(h[2] == 0.0, RN_E_COMM, "rn_exchange_autotune: the collective exchange failed on a rank (" + err + ")");
        if (h[3] != 0.0) oneShotBroken = true;
        transport = (h[3] == 0.0 && h[1] < h[0]) ? 1 : 0;
        tuneInfo[0] = transport; tuneInfo[2] = h[0]; tuneInfo[3] = h[3] != 0.0 ? -1.0 : h[1]; tuneInfo[4] = own[0]; tuneInfo[5] = own[1]; tuneInfo[6] = iters; tuneInfo[7] += 1.0;
        return RN_OK;
    }
    int exchange_prepare_api() override { return transportReq == RN_EXCHANGE_COLLECTIVE ? RN_OK : exchange_prepare(); }
    int exchange_autotune_api(int iters, double *out) override {
        RN_CHECK(iters >= 0, RN_E_ARG, "rn_exchange_autotune: iterations >= 0");
        if (iters > 0) {
            RN_CHECK(transportReq == RN_EXCHANGE_AUTO, RN_E_STATE, "rn_exchange_autotune: the transport was fixed by rn_set_exchange_transport");
            if (int rc = exchange_autotune(iters)) return rc;
        }
        if (out) { for (int i = 0; i < 8; i++) out[i] = tuneInfo[i]; out[0] = transport; }
        return RN_OK;
    }
    // after a batch in one-shot mode: did a reader give up waiting?  (one 4-byte read-back; the stream has been synchronised)
    int check_comm_fail() {
        int f = 0;
        RN_HIP(hipMemcpyAsync(&f, &d_state->commFail, sizeof(int), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        RN_CHECK(f == 0, RN_E_COMM, "one-shot exchange: a peer's packets did not arrive within the time-out (a rank is missing or far behind)");
        return RN_OK;
    }
    size_t injectBytes = 0;
    int inject_allocation(size_t bytes) override { injectBytes = bytes; return RN_OK; }
    int reserve_iterations(int n) override {
        RN_CHECK(n >= 0, RN_E_ARG, "rn_reserve_iterations: negative iteration count");
        RN_HIP(hipSetDevice(device));
        for (int i = 0; i < 3; i++) if (!d_ck[i]) { if (int rc = dalloc(&d_ck[i], (size_t)ntot())) return rc; }
        if (n + 2 > lamCap) return ensure_tables(n);
        return RN_OK;
    }
    int set_exchange_mode(int mode) override {
        RN_CHECK(mode == 0 || mode == 1, RN_E_ARG, "rn_set_exchange_mode: 0 exact, 1 optimistic");
        optimistic = mode; optHold = 0;
        return RN_OK;
    }
    int apg_iterate(int n, double *primalInfs) override { return apg_iterate(n, primalInfs, -1.0); }
    int apg_iterate(int n, double *primalInfs, double recTol, bool rtest = false) {
        RN_CHECK(factored && affine_ready, RN_E_STATE, "rn_apg_iterate before the factor step / affine terms");
        RN_CHECK(n >= 0, RN_E_ARG, "rn_apg_iterate: negative iteration count");
        RN_CHECK(!poisoned, RN_E_STATE, "rn_apg_iterate: an earlier batch failed half-way; call rn_apg_reset first");
        RN_HIP(hipSetDevice(device));
        // optimistic batches (prox as a pure projection, verified afterwards); after a replay the next RN_OPT_BACKOFF batches
        // go straight through the exact path (every rank sees the same verdicts, so sharded ranks stay in step)
        const bool wantOptSharded = has_comm() && cutStage > 0 && optimistic && n > 0;
        // single GPU: worth a checkpoint (3 vector copies) and a read-back per batch once the batch is long enough
        const bool wantOptLocal = !has_comm() && cutStage <= 0 && optimistic && n >= RN_OPT_LOCAL_MIN;
        if (wantOptSharded && transportReq == RN_EXCHANGE_AUTO && !tuned) {   // the exchange chooses itself, once
            if (int rc = exchange_autotune(std::min(std::max(n, 20), 100))) return rc;
        }
        bool opt = wantOptSharded || wantOptLocal;
        if (opt && optHold > 0) { optHold--; opt = false; }
        if (opt) optBatches++;
        else if (n > 0) exactBatches++;
        return run_batch(n, primalInfs, opt, recTol, rtest);
    }
    // The loop of rn_apg_solve (the reset, or the warm restart, is the caller's): batches of `every` iterations through apg_iterate -- so the
    // iterates are those of the same sequence of rn_apg_iterate calls, bit for bit -- until the residual of a batch's LAST iteration is <= tol
    // or maxIt iterations have run (SmpcController::algorithmApg runs maxIterations whatever the residual, SmpcController.cu:1500-1525).  The
    // decision is the host's and is taken where the host synchronises anyway: behind the launch that closes the batch, which has published the
    // batch record (common.hpp, BatchRecord).  Sharded: the record is built from the all-reduced history, the same bits on every rank, so all
    // ranks stop together.  tol == 0 never stops early.
    // rn_set_restart(RN_RESTART_GRADIENT): behind the tolerance check -- a solve that stops does not restart -- the batch's gradient test
    // decides whether the momentum starts again (g > 0: momentum_restart).  A replayed batch is judged on the replay; sharded ranks hold the
    // same bits of g and decide alike.
    int solve_loop(int maxIt, double tol, int every, double *primalInfs) {
        lastSolve[0] = 0; lastSolve[1] = 0; lastSolve[2] = -1; lastSolve[3] = 0;
        const bool rtest = restartMode == RN_RESTART_GRADIENT;
        restartCounts[0] = 0; restartCounts[1] = -1; restartCounts[2] = 0; restartCounts[3] = 0;
        restartLast[0] = restartLast[1] = restartLast[2] = 0.0;
        for (int done = 0; done < maxIt;) {
            const int n = std::min(every, maxIt - done);
            if (int rc = apg_iterate(n, primalInfs ? primalInfs + done : nullptr, tol, rtest)) return rc;
            if (lastSolve[2] < 0 && lastRec.firstBelow >= 0) lastSolve[2] = done + lastRec.firstBelow;
            done += n;
            lastSolve[0] = done; lastSolve[3]++;
            if (tol > 0 && lastRec.lastResidual <= tol) { lastSolve[1] = 1; break; }
            if (rtest) {
                restartCounts[2]++;
                restartLast[0] = lastRec.g; restartLast[1] = lastRec.na2; restartLast[2] = lastRec.nb2;
                if (lastRec.g > 0 && !poisoned) {
                    if (int rc = momentum_restart()) return rc;
                    restartCounts[0]++; restartCounts[1] = done;
                }
            }
        }
        return RN_OK;
    }
    // what rn_algorithm_apg and rn_control_action run after their reset: one batch of maxIt iterations -- today's path, untouched -- unless
    // rn_set_stop_tolerance named a tolerance
    int apg_run(int maxIt, double *primalInfs) override {
        if (stepRule != RN_STEP_FIXED) { RN_CHECK(factored && affine_ready, RN_E_STATE, "rn_apg_iterate before the factor step / affine terms"); if (int rc = step_rule_on_entry()) return rc; }
        if (stopTol > 0 || restartMode == RN_RESTART_GRADIENT) {   // (restart without a tolerance: batches of stopEvery, never stopping early)
            RN_CHECK(factored && affine_ready, RN_E_STATE, "rn_apg_iterate before the factor step / affine terms");
            RN_CHECK(maxIt >= 0, RN_E_ARG, "rn_apg_iterate: negative iteration count");
            const int rc = solve_loop(maxIt, stopTol, stopEvery, primalInfs);
            // no tolerance was set (the batches are the restart's): rn_get_last_solve promises -1 -- the closing launches scanned for
            // entries <= 0, and vecPrimalInfs can be exactly 0 (`small`: over its first 140 iterations)
            if (stopTol <= 0) lastSolve[2] = -1;
            return rc;
        }
        if (int rc = apg_iterate(maxIt, primalInfs)) return rc;
        lastSolve[0] = maxIt; lastSolve[1] = 0; lastSolve[2] = -1; lastSolve[3] = maxIt > 0 ? 1 : 0;
        restartCounts[0] = 0; restartCounts[1] = -1; restartCounts[2] = 0; restartCounts[3] = 0;
        restartLast[0] = restartLast[1] = restartLast[2] = 0.0;
        return RN_OK;
    }
    int apg_solve(int maxIt, double tol, int every, int *iterationsRun, double *primalInfs) override {
        RN_CHECK(iterationsRun, RN_E_ARG, "rn_apg_solve: null iterationsRun");
        RN_CHECK(maxIt >= 0, RN_E_ARG, "rn_apg_solve: negative iteration count");
        RN_CHECK(std::isfinite(tol) && tol >= 0, RN_E_ARG, "rn_apg_solve: the tolerance must be finite and >= 0");
        RN_CHECK(factored && affine_ready, RN_E_STATE, "rn_apg_solve before the factor step / affine terms");
        *iterationsRun = 0;
        if (int rc = apg_reset()) return rc;
        if (int rc = step_rule_on_entry()) return rc;
        const int rc = solve_loop(maxIt, tol, every > 0 ? every : RN_STOP_CHECK_EVERY, primalInfs);
        *iterationsRun = (int)lastSolve[0];
        return rc;
    }
    int set_stop_tolerance(double tol, int every) override {
        RN_CHECK(std::isfinite(tol) && tol >= 0, RN_E_ARG, "rn_set_stop_tolerance: the tolerance must be finite and >= 0");
        stopTol = tol; stopEvery = every > 0 ? every : RN_STOP_CHECK_EVERY;
        return RN_OK;
    }
    int get_stop_tolerance(double *tol, int *every) override {
        if (tol) *tol = stopTol;
        if (every) *every = stopEvery;
        return RN_OK;
    }
    int set_restart(int mode) override {
        RN_CHECK(mode == RN_RESTART_OFF || mode == RN_RESTART_GRADIENT, RN_E_ARG, "rn_set_restart: RN_RESTART_OFF or RN_RESTART_GRADIENT");
        if (mode == RN_RESTART_GRADIENT) { if (int rc = restart_buffers()) return rc; }   // here, not inside a control step
        restartMode = mode;
        return RN_OK;
    }
    int get_restart(int *mode) override {
        RN_CHECK(mode, RN_E_ARG, "rn_get_restart: null output");
        *mode = restartMode;
        return RN_OK;
    }
    int restart_info(long *counts, double *last) override {
        RN_CHECK(counts && last, RN_E_ARG, "rn_get_restart_info: null output");
        for (int i = 0; i < 4; i++) counts[i] = restartCounts[i];
        for (int i = 0; i < 3; i++) last[i] = restartLast[i];
        return RN_OK;
    }
    // rn_debug_restart_test (include/rapidnet_debug.h): the kernel alone, on the iterates as they stand (sharded contexts: collective)
    int debug_restart_test(double *out) override {
        RN_CHECK(out, RN_E_ARG, "rn_debug_restart_test: null output");
        RN_CHECK(p_acc_view && p_upd && p_xi, RN_E_STATE, "rn_debug_restart_test before the factor step");
        RN_CHECK(!poisoned, RN_E_STATE, "rn_debug_restart_test: an earlier batch failed half-way; call rn_apg_reset first");
        RN_HIP(hipSetDevice(device));
        if (int rc = restart_buffers()) return rc;
        if (int rc = launch_restart_test(has_comm() && cutStage > 0)) return rc;
        RN_HIP(hipMemcpyAsync(out, &d_state->rec.g, 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        return RN_OK;
    }
    int last_solve(long *out) override {
        RN_CHECK(out, RN_E_ARG, "rn_get_last_solve: null output");
        for (int i = 0; i < 4; i++) out[i] = lastSolve[i];
        return RN_OK;
    }
    // Sharded contexts, once per batch: vecPrimalInfs[first .. first + n) of this rank (arg-max over its own nodes) -> the
    // tree-global values, on every rank (SmpcController.cu:1480-1496, :1521); element 0 of the payload carries the ranks'
    // verdict on the optimistic batch (tail = the all-reduced dist^2 of its last iteration; nullptr: no verdict).
    int globalize_history(int first, int n, T *tail, double recTol) {
        hipLaunchKernelGGL(k_batch_close_pack<T>, dim3(1), dim3(ELT_THREADS), 0, stream, (const T *)tail, d_state, penX / stepSize, penXs / stepSize,
                           (const double *)d_histParts, first, n, d_histGlob);
        // (the last element: one-shot exchange, "a reader of this rank gave up waiting" -- the MAX makes it every rank's verdict, so all
        //  ranks return RN_E_COMM for the batch together instead of the late one alone)
        if (int rc = all_reduce(d_histGlob, (size_t)4 * n + 2, true, "ncclAllReduce(verdict + primal infeasibilities)", 2 /* ncclMax */)) return rc;
        hipLaunchKernelGGL(k_batch_close_unpack<>, dim3(1), dim3(ELT_THREADS), 0, stream, (const double *)d_histGlob, d_hist, first, n, d_state, recTol, recTol >= 0 ? 1 : 0);
        if (int rc = comm_check()) return rc;
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    // A batch that fails half-way (a launch or a collective returned an error after some of its iterations were enqueued) leaves
    // the rotating iterate buffers, the device-side iteration counter and the host's view of them out of step: the context
    // refuses further iterations until rn_apg_reset / rn_fbe_reset (or rn_control_action, which resets) instead of continuing
    // from an inconsistent accelerated dual.
    bool poisoned = false;
    int fail_batch(int rc) {
        poisoned = true;
        err += " -- the batch was abandoned half-way: call rn_apg_reset before iterating again";
        return rc;
    }
    // which kernels a batch of this context launches (bench.py names them in its JSON line instead of assuming)
    int kernel_info(int *out) override {
        RN_CHECK(out, RN_E_ARG, "rn_get_kernel_info: null output");
        int G = 0, NL = 0;
        stream_shape(&G, &NL);
        const bool flat = dual_main_flat(optimistic != 0);
        out[0] = flat ? 0 : 1;   // 1: k_dual_stage is the main pass of the fused dual update, 0: the flat k_dual_fused
        out[1] = flat ? eltBlocks : dualBlocks;
        out[2] = dualU > 0 ? dshape.trips : 0;
        out[3] = dualU;                                  // 2: double-buffered variant
        out[4] = G; out[5] = NL;                         // k_stream_gemv: columns per span, 16-byte slots per thread and span
        out[6] = chainStage;
        out[7] = v_lv_is_slab() ? (wideCt >= 2 ? wideCt : 1) : 0;   // 1: k_gemm_vlv (slab), 0: two k_gemm_shared launches; 2 / 3: a sweep has chosen k_gemm_vlv_wide with that many slabs per workgroup
        return RN_OK;
    }
    // rn_debug_stream_info (include/rapidnet_debug.h): what stream_split_setup() decided, for the tests of the split last round
    int stream_info(int *out) override {
        RN_CHECK(out, RN_E_ARG, "rn_debug_stream_info: null output");
        out[0] = splitFirst; out[1] = splitFirst >= 0 && splitFirst < d.nodes ? splitSpanHalf : 0;
        out[2] = streamTwoPerCU ? 1 : 0; out[3] = numCUs;
        return RN_OK;
    }
    // {live spans, spans, live columns, columns} of the most recent streaming launch, summed over its workgroups' records; ragged: how many of the
    // live spans were ragged last spans (ny % G columns)
    int stream_live_sum(long long *out, long long *ragged) {
        RN_HIP(hipSetDevice(device));
        RN_HIP(hipStreamSynchronize(stream));
        std::vector<int2> h((size_t)lastStreamGrid);
        RN_HIP(hipMemcpy(h.data(), d_streamLive, h.size() * sizeof(int2), hipMemcpyDeviceToHost));
        int G, NL;
        stream_shape(&G, &NL);
        long long ls = 0, lc = 0, rg = 0;
        for (const int2 &e : h) { ls += e.x; lc += e.y & ((1 << 30) - 1); rg += (e.y >> 30) & 1; }
        out[0] = ls; out[1] = (long long)d.nodes * ((ny + G - 1) / G); out[2] = lc; out[3] = (long long)d.nodes * ny;
        if (ragged) *ragged = rg;
        return RN_OK;
    }
    // the units records of the most recent launch summed (stream_walk_half: live units, those of ragged last spans among them, and the columns of those)
    int stream_units_sum(long long *units, long long *ragUnits, long long *ragCols) {
        RN_HIP(hipSetDevice(device));
        RN_HIP(hipStreamSynchronize(stream));
        std::vector<int> h((size_t)lastStreamGrid);
        RN_HIP(hipMemcpy(h.data(), d_streamUnits, h.size() * sizeof(int), hipMemcpyDeviceToHost));
        long long u = 0, ru = 0, rc = 0;
        for (int e : h) { u += e & 0xffff; ru += (e >> 16) & 0xf; rc += e >> 20; }
        *units = u;
        if (ragUnits) *ragUnits = ru;
        if (ragCols) *ragCols = rc;
        return RN_OK;
    }
    // {live units, units, columns per unit} of the most recent streaming launch: half-spans where the launch skipped them by themselves
    // (stream_half_on), whole spans otherwise
    int stream_units(long long *out) override {
        RN_CHECK(out, RN_E_ARG, "rn_debug_stream_units: null output");
        RN_CHECK(!structured && lastStreamGrid > 0 && d_streamLive && d_streamUnits, RN_E_STATE, "rn_debug_stream_units: no streaming launch yet");
        int G, NL;
        stream_shape(&G, &NL);
        if (!stream_half_on()) {
            long long live[4];
            if (int rc = stream_live_sum(live, nullptr)) return rc;
            out[0] = live[0]; out[1] = live[1]; out[2] = G;
            return RN_OK;
        }
        long long lu = 0;
        if (int rc = stream_units_sum(&lu, nullptr, nullptr)) return rc;
        out[0] = lu; out[1] = (long long)d.nodes * ((ny + G / 2 - 1) / (G / 2)); out[2] = G / 2;
        return RN_OK;
    }
    int stream_live(long long *out) override {
        RN_CHECK(out, RN_E_ARG, "rn_debug_stream_live: null output");
        RN_CHECK(!structured && lastStreamGrid > 0 && d_streamLive, RN_E_STATE, "rn_debug_stream_live: no streaming launch yet");
        return stream_live_sum(out, nullptr);
    }
    // rn_debug_stream_product (include/rapidnet_debug.h): launch_stream alone, with the arguments a sweep of this context would give it at the
    // accelerated dual RN_BUF_ACC_* shows; pair: the context's y (RN_BUF_XI / RN_BUF_PSI) as the second right-hand side of an NR = 2 launch,
    // unsplit as launch_sweep runs a pair.  The products are scratch of the next sweep's: no iterate changes.
    int stream_product(int pair, double *my, double *my2, double *myB) override {
        RN_CHECK(my && (pair == 0 || pair == 1) && (!pair || myB), RN_E_ARG, "rn_debug_stream_product: my is required, pair is 0 or 1, and pair = 1 needs myB");
        RN_CHECK(factored && !structured && p_acc_view && p_xi, RN_E_STATE, "rn_debug_stream_product: dense per-node blocks exist after rn_factor_step on a context that is not structured");
        RN_CHECK(!pair || pair_active(), RN_E_STATE, "rn_debug_stream_product: pair = 1 needs the pair buffers and a launch that can run unsplit (rn_get_sweep_pairing: active)");
        RN_HIP(hipSetDevice(device));
        SweepArgs<T> a = sweep_args(Batch{});
        a.w = p_acc_view;
        if (pair && store32()) a.splitFirst = d.nodes;
        RN_CHECK(!my2 || a.splitFirst < d.nodes, RN_E_ARG, "rn_debug_stream_product: my2 belongs to a launch with a split last round");
        const StreamRhs2<T> r2{p_xi, d_myB, d_qaB};
        if (int rc = launch_stream(a, pair ? &r2 : nullptr)) return rc;
        RN_HIP(hipGetLastError());
        if (int rc = download(my, d_my, (size_t)d.nodes * 2 * d.nv)) return rc;
        if (my2) { if (int rc = download(my2, d_my2, (size_t)(d.nodes - a.splitFirst) * 2 * d.nv)) return rc; }
        if (pair) { if (int rc = download(myB, d_myB, (size_t)d.nodes * 2 * d.nv)) return rc; }
        return RN_OK;
    }
    // rn_debug_dual_update (include/rapidnet_debug.h): the dual update of one iteration alone, through the batch loop's own launch steps (sweep.inc),
    // with outputs, partials, iteration state and history slot in scratch of the hook's own
    struct DualScratch { T *yn = nullptr, *wn = nullptr, *z = nullptr, *res = nullptr, *hx = nullptr; Partial *parts = nullptr, *parts2 = nullptr;
                         IterState *st = nullptr; double *hist = nullptr, *dist2 = nullptr; bool ready = false; };
    DualScratch dsx;
    int dual_scratch() {
        if (dsx.ready) return RN_OK;
        const size_t n = (size_t)ntot();
        if (int rc = dalloc(&dsx.yn, n)) return rc;
        if (int rc = dalloc(&dsx.wn, n)) return rc;
        if (int rc = dalloc(&dsx.z, n)) return rc;
        if (int rc = dalloc(&dsx.res, n)) return rc;
        if (int rc = dalloc(&dsx.hx, n)) return rc;
        if (int rc = dalloc(&dsx.parts, (size_t)std::max(ELT_MAX_BLOCKS, RN_DUAL_STAGE_MAX_BLOCKS))) return rc;
        if (int rc = dalloc(&dsx.parts2, (size_t)ELT_MAX_BLOCKS)) return rc;
        if (int rc = dalloc(&dsx.st, 1)) return rc;
        if (int rc = dalloc(&dsx.hist, 5)) return rc;      // the history entry and its four parts
        if (int rc = dalloc(&dsx.dist2, 2)) return rc;
        dsx.ready = true;
        return RN_OK;
    }
    int dual_update_alone(const rn_dual_update_args *p, double *info) override {
        RN_CHECK(p && info, RN_E_ARG, "rn_debug_dual_update: null arguments");
        RN_CHECK(factored && d_hx && p_acc_view && p_upd, RN_E_STATE, "rn_debug_dual_update before the factor step");
        RN_CHECK(algorithm == RN_ALG_APG, RN_E_STATE, "rn_debug_dual_update: the dual update of global FBE / NAMA is another one (fbe_methods.inc)");
        RN_CHECK(!poisoned, RN_E_STATE, "rn_debug_dual_update: an earlier batch failed half-way; call rn_apg_reset first");
        RN_CHECK(p->form >= RN_DUALP_MAIN && p->form <= RN_DUALP_NEXT_W, RN_E_ARG, "rn_debug_dual_update: unknown form");
        RN_CHECK(p->iteration >= 0 && p->iteration < (1 << 24), RN_E_ARG, "rn_debug_dual_update: iteration out of range");
        RN_HIP(hipSetDevice(device));
        const size_t n = (size_t)ntot();
        if (p->form == RN_DUALP_NEXT_W) {
            RN_CHECK(p->wnext, RN_E_ARG, "rn_debug_dual_update: NEXT_W needs wnext");
            RN_CHECK(acc_ready, RN_E_STATE, "rn_debug_dual_update: the next sweep would re-derive w (the iterates were edited)");
            return download(p->wnext, p_acc, n);
        }
        const bool launches = p->form != RN_DUALP_INFO;
        const bool mat = p->materialize != 0, unscaled = p->unscaled != 0, sharded = p->form == RN_DUALP_EXACT_SHARDED;
        const bool exact = p->form == RN_DUALP_EXACT || sharded;
        // the flat kernel: where the shape is not eligible, on request, and in the exact sharded form (whose fix-up and k_finalize fold eltBlocks partials)
        const bool flat = dualU == 0 || p->flat != 0 || sharded;
        RN_CHECK(!(unscaled && exact), RN_E_ARG, "rn_debug_dual_update: only optimistic batches walk unscaled; an exact form never meets an unscaled Hx");
        RN_CHECK(!(unscaled && mat && !flat), RN_E_ARG, "rn_debug_dual_update: k_dual_stage has no instantiation with SCALE and MATERIALIZE (the batch's last sweep walks scaled)");
        RN_CHECK(!launches || (p->ynew && p->wnext), RN_E_ARG, "rn_debug_dual_update: ynew and wnext are required");
        RN_CHECK(!launches || !mat || (p->z && p->res), RN_E_ARG, "rn_debug_dual_update: a materialising pass needs z and res");
        const int t = p->iteration;
        if (int rc = ensure_tables(t + 1)) return rc;
        if (int rc = dual_scratch()) return rc;
        DualArgs<T> a = dual_args();
        a.w = p_acc_view;
        a.ynew = dsx.yn; a.wnext = dsx.wn; a.z = dsx.z; a.res = dsx.res;
        a.st = dsx.st; a.partials = dsx.parts;
        // the kernels index the history and the lambda table by iteration: slot t of both views is the hook's scratch entry / the table's entry t
        a.lamNext = d_lam; a.hist = dsx.hist - t; a.histParts = dsx.hist + 1 - 4 * (ptrdiff_t)t; a.histCap = t + 1;
        const DualMainLaunch m = dual_main_args(flat, unscaled, mat, h_lam[t + 1]);
        RN_CHECK(!p->partials || !launches || p->nPartials >= (size_t)m.blocks, RN_E_ARG, "rn_debug_dual_update: the main pass leaves more partials than the caller's array holds");
        const DualArgs<T> fx = exact_fixup_args(a, t, m.blocks, dsx.parts2);
        for (int i = 0; i < RN_DUAL_INFO_COUNT; i++) info[i] = 0.0;
        info[0] = (double)a.lambda; info[1] = (double)a.invLambda; info[2] = (double)(T)h_lam[t + 1]; info[3] = a.thrX; info[4] = a.thrS;
        for (int i = 5; i < 20; i++) info[i] = std::nan("");
        info[20] = flat ? 0 : 1; info[21] = m.blocks; info[22] = flat ? 0 : m.g.trips; info[23] = m.pipe; info[24] = flat ? 0 : m.g.crownBlocks;
        info[25] = flat ? 0 : m.g.bps; info[26] = flat ? 0 : m.g.vpn; info[27] = flat ? 0 : m.g.cs; info[28] = flat ? 0 : m.g.K; info[29] = flat ? 0 : m.g.node0;
        info[30] = eltBlocks; info[31] = exact_fixup_blocks(); info[32] = a.crownElems; info[33] = a.countCrown; info[34] = m.scale ? 1 : 0;
        info[35] = a.bStrideStage; info[36] = a.bStrideNode; info[37] = (double)bounds_rows(boundsGran); info[38] = m.preScale ? 1 : 0;
        if (p->lo) { if (int rc = download(p->lo, d_lo, n)) return rc; }
        if (p->hi) { if (int rc = download(p->hi, d_hi, n)) return rc; }
        if (p->sqrtp) { if (int rc = download(p->sqrtp, d_sqrtp, (size_t)d.nodes)) return rc; }
        if (p->dy) { if (int rc = download(p->dy, d_dy, (size_t)d.N * ny)) return rc; }
        if (p->blo) { if (int rc = download(p->blo, d_blo, bounds_rows(boundsGran) * ny)) return rc; }
        if (p->bhi) { if (int rc = download(p->bhi, d_bhi, bounds_rows(boundsGran) * ny)) return rc; }
        if (p->stageOf) RN_HIP(hipMemcpy(p->stageOf, d_stageOf, (size_t)d.nodes * sizeof(int), hipMemcpyDeviceToHost));
        if (!launches) return RN_OK;
        // the caller's fill under the outputs, the scratch state at iteration t
        if (int rc = upload(dsx.yn, p->ynew, n)) return rc;
        if (int rc = upload(dsx.wn, p->wnext, n)) return rc;
        if (p->z) { if (int rc = upload(dsx.z, p->z, n)) return rc; }
        if (p->res) { if (int rc = upload(dsx.res, p->res, n)) return rc; }
        IterState st0{};
        st0.it = t;
        RN_HIP(hipMemcpyAsync(dsx.st, &st0, sizeof st0, hipMemcpyHostToDevice, stream));
        const double nanv = std::nan("");
        const double h0[5] = {nanv, nanv, nanv, nanv, nanv};
        RN_HIP(hipMemcpyAsync(dsx.hist, h0, sizeof h0, hipMemcpyHostToDevice, stream));
        RN_HIP(hipStreamSynchronize(stream));   // (st0, h0 are locals)
        if (m.preScale) {   // as hx_scale_now in launch_dual_main, on a copy: the context's Hx stays what it is
            RN_HIP(hipMemcpyAsync(dsx.hx, d_hx, n * sizeof(T), hipMemcpyDeviceToDevice, stream));
            hx_scale_now(dsx.hx);
            a.hx = dsx.hx;
        }
        run_dual_main(m, a, mat);
        // (the fold the record reports: fold_partials over the main pass's partials, into scratch; reads only)
        hipLaunchKernelGGL(k_reduce_dist<>, dim3(1), dim3(ELT_THREADS), 0, stream, (const Partial *)dsx.parts, m.blocks, dsx.dist2);
        double d2main[2] = {0, 0};
        RN_HIP(hipMemcpyAsync(d2main, dsx.dist2, sizeof d2main, hipMemcpyDeviceToHost, stream));
        if (p->form == RN_DUALP_EXACT) run_exact_fixup(fx, mat);
        else if (sharded) { if (int rc = run_close_exact_sharded(a, mat, dsx.dist2)) return rc; }
        else if (p->form == RN_DUALP_OPTIMISTIC_CLOSE) run_close_optimistic(a, m.blocks, nullptr, false, 0, -1, -1.0, nullptr);
        RN_HIP(hipGetLastError());
        IterState st1{};
        double h1[5];
        std::vector<Partial> hp((size_t)m.blocks), hp2;
        RN_HIP(hipMemcpyAsync(&st1, dsx.st, sizeof st1, hipMemcpyDeviceToHost, stream));
        RN_HIP(hipMemcpyAsync(h1, dsx.hist, sizeof h1, hipMemcpyDeviceToHost, stream));
        RN_HIP(hipMemcpyAsync(hp.data(), dsx.parts, hp.size() * sizeof(Partial), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        info[5] = d2main[0]; info[6] = d2main[1];
        if (p->form != RN_DUALP_MAIN) { info[7] = st1.distX; info[8] = st1.distS; info[9] = st1.tripped; info[10] = st1.scaleX; info[11] = st1.scaleS; }
        info[12] = st1.violated; info[39] = st1.it;
        // which partials decided the arg-max: the fix-up's when it ran to the end (EXACT: its own array; EXACT_SHARDED: it overwrote the main pass's, read
        // back above, so the raw main partials the caller gets are then the fix-up's -- the sharded form has one array, as in the batch loop)
        const std::vector<Partial> *dec = &hp;
        if (p->form == RN_DUALP_EXACT && st1.tripped) {
            hp2.resize((size_t)exact_fixup_blocks());
            RN_HIP(hipMemcpy(hp2.data(), dsx.parts2, hp2.size() * sizeof(Partial), hipMemcpyDeviceToHost));
            dec = &hp2;
        }
        double aX = -1, aP = -1; long long iX = 0x7fffffffffffffffLL, iP = iX;
        for (const Partial &q : *dec) {
            if (q.absXi > aX || (q.absXi == aX && q.idxXi < iX)) { aX = q.absXi; iX = q.idxXi; }
            if (q.absPsi > aP || (q.absPsi == aP && q.idxPsi < iP)) { aP = q.absPsi; iP = q.idxPsi; }
        }
        info[13] = h1[1]; info[14] = h1[2]; info[15] = iX == 0x7fffffffffffffffLL ? -1.0 : (double)iX;
        info[16] = h1[3]; info[17] = h1[4]; info[18] = iP == 0x7fffffffffffffffLL ? -1.0 : (double)iP;
        info[19] = h1[0];
        if (p->partials)
            for (size_t b = 0; b < hp.size(); b++) {
                const Partial &q = hp[b];
                double *o = p->partials + 8 * b;
                o[0] = q.d2x; o[1] = q.d2s; o[2] = q.absXi; o[3] = q.valXi; o[4] = q.absPsi; o[5] = q.valPsi;
                o[6] = q.idxXi == 0x7fffffffffffffffLL ? -1.0 : (double)q.idxXi; o[7] = q.idxPsi == 0x7fffffffffffffffLL ? -1.0 : (double)q.idxPsi;
            }
        if (int rc = download(p->ynew, dsx.yn, n)) return rc;
        if (int rc = download(p->wnext, dsx.wn, n)) return rc;
        if (p->z) { if (int rc = download(p->z, dsx.z, n)) return rc; }
        if (p->res) { if (int rc = download(p->res, dsx.res, n)) return rc; }
        return RN_OK;
    }
    // rn_debug_slab_product (include/rapidnet_debug.h): one launch step of the shared-operator products (sweep.inc: run_v_lv, run_comp, run_prep_m2,
    // run_gemm) over scratch buffers of the hook's own, with the arguments v_lv_args / prep_m2_args / gemm_args shape for a sweep of this context.
    struct SlabScratch { T *MA = nullptr, *MAf = nullptr, *MB = nullptr, *MBf = nullptr, *in = nullptr, *aux = nullptr, *aux2 = nullptr, *prob = nullptr, *outA = nullptr, *outB = nullptr; bool ready = false; };
    SlabScratch ss;
    int slab_out_nodes() const { return ((d.nodes + 47) / 48 + 1) * 48; }
    int slab_scratch() {
        if (ss.ready) return RN_OK;
        const int nx = d.nx, nu = d.nu, nv = d.nv;
        const size_t nA = (size_t)pad16(std::max(nv, nu + nx)) * pad4(nv + nx + nu), nB = (size_t)pad16(nu + nx) * pad4(nv);
        const size_t rowsAux = (size_t)std::max(2 * nv, nu + nx), on = (size_t)slab_out_nodes();
        if (int rc = dalloc(&ss.MA, nA)) return rc;
        if (int rc = dalloc(&ss.MAf, nA)) return rc;
        if (int rc = dalloc(&ss.MB, nB)) return rc;
        if (int rc = dalloc(&ss.MBf, nB)) return rc;
        if (int rc = dalloc(&ss.in, (size_t)d.nodes * (nv + nx + nu))) return rc;
        if (int rc = dalloc(&ss.aux, (size_t)d.nodes * rowsAux)) return rc;
        if (int rc = dalloc(&ss.aux2, (size_t)d.nodes * rowsAux)) return rc;
        if (int rc = dalloc(&ss.prob, (size_t)d.nodes)) return rc;
        if (int rc = dalloc(&ss.outA, on * rowsAux)) return rc;
        if (int rc = dalloc(&ss.outB, on * (nu + nx))) return rc;
        ss.ready = true;
        return RN_OK;
    }
    // caller's compact rows [nodes][k] into scratch rows of ld at column off; the other columns hold a value no product may read
    int slab_put_rows(T *dst, const double *src, int k, int ld, int off) {
        std::vector<double> tmp((size_t)d.nodes * ld, 7777.0);
        for (int i = 0; i < d.nodes; i++) for (int j = 0; j < k; j++) tmp[(size_t)i * ld + off + j] = src[(size_t)i * k + j];
        return upload(dst, tmp.data(), tmp.size());
    }
    static void slab_info_product(int *info, const GemmArgs<T> &g) { info[0] = g.m; info[1] = g.k; info[2] = g.kp; info[3] = g.ldin; }
    int slab_product(const rn_slab_product_args *p, int *info) override {
        RN_CHECK(p && info, RN_E_ARG, "rn_debug_slab_product: null arguments");
        RN_CHECK(factored, RN_E_STATE, "rn_debug_slab_product: the shared operators' launches are shaped by rn_factor_step");
        RN_CHECK(p->launch >= RN_SLABP_PAIR && p->launch <= RN_SLABP_SINGLE && p->MA, RN_E_ARG, "rn_debug_slab_product: unknown launch, or no operator");
        RN_HIP(hipSetDevice(device));
        const int nx = d.nx, nu = d.nu, nv = d.nv, nodes = d.nodes;
        const size_t on = (size_t)slab_out_nodes();
        if (int rc = slab_scratch()) return rc;
        SweepArgs<T> a = sweep_args(Batch{});
        a.w = p_acc_view ? p_acc_view : p_acc;
        a.lin = lin_bits(a.lin);
        a.sk = ss.in; a.sk2 = ss.in; a.ab = ss.in; a.v = ss.outA; a.lvb = ss.outB; a.my = ss.aux; a.my2 = ss.aux2; a.qa = ss.outB;
        GemmArgs<T> g1{}, g2{}, gC{};
        bool two = false;
        int epi = EPI_V;
        size_t needA = 0, needB = 0;
        if (p->launch == RN_SLABP_PAIR || p->launch == RN_SLABP_COMP) {
            a.writePrimal = p->storeV ? 1 : 0;
            if ((a.lin & 2) && !p->aux) a.beta = d_zero;      // (the form of a Hessian sweep: no constant operand)
            else if (a.beta == d_zero) a.beta = ss.aux;      // (any address but d_zero: only compared)
            const bool comp = v_lv_args(a, g1, g2, gC);
            RN_CHECK(comp == (p->launch == RN_SLABP_COMP), RN_E_ARG, "rn_debug_slab_product: this context's sweep runs the other form of the v / Lv products (RN_KNOB_STRUCT_LINEAR)");
            if (comp) {
                g1 = gC;
                RN_CHECK(!p->MB && !p->outA && p->outB, RN_E_ARG, "rn_debug_slab_product: the composite product has one operator and one output, outB");
                needB = on * (nu + nx);
            } else {
                two = true;
                RN_CHECK(p->MB && p->outA && p->outB, RN_E_ARG, "rn_debug_slab_product: the pair needs MB, outA and outB");
                needA = on * nv; needB = on * (nu + nx);
            }
        } else if (p->launch == RN_SLABP_PREP_M2) {
            RN_CHECK(structured, RN_E_ARG, "rn_debug_slab_product: k_gemm_prep_m2 belongs to structured contexts");
            RN_CHECK(!p->MB && !p->in && !p->aux && !p->aux2 && !p->prob && p->outA && p->outB, RN_E_ARG, "rn_debug_slab_product: k_gemm_prep_m2 reads the context's dual, not caller operands; outputs outA, outB");
            a.my = ss.outA;
            g1 = prep_m2_args(a);
            epi = EPI_LV;
            needA = on * 2 * nv; needB = on * nx;
        } else {
            RN_CHECK(!p->MB && p->outA && !p->outB, RN_E_ARG, "rn_debug_slab_product: a single product has one operator and one output, outA");
            switch (p->role) {
                case 0:
                    RN_CHECK(!structured, RN_E_ARG, "rn_debug_slab_product: role 0 is the dense contexts' v product");
                    g1 = gemm_args<EPI_V>(d_RTp, nv, nv + nx, a.sk, nv + nx, a.v, nv, a.my, 2 * nv, a.splitFirst); g1.aux2 = g1.aux2 ? ss.aux2 : nullptr; break;
                case 1: g1 = gemm_args<EPI_LV>(d_LBLp, nu + nx, nv, ss.in, nv, a.v, nu + nx, nullptr, 0); epi = EPI_LV; break;
                case 2: g1 = gemm_args<EPI_Z>(d_Bp, nx, nu, ss.in, nu, a.v, nx, ss.aux, nx); epi = EPI_Z; break;
                case 3: g1 = gemm_args<EPI_V>(d_T12p, nv, nx + nu, a.sk2 + nv, nv + nx + nu, a.v, nv, p->aux ? ss.aux : nullptr, nv); g1.aux2 = nullptr; g1.auxSplit = 0; break;
                default: RN_CHECK(false, RN_E_ARG, "rn_debug_slab_product: role 0 .. 3");
            }
            needA = on * g1.m;
        }
        const bool scaled = epi == EPI_V;
        const bool split = g1.aux2 != nullptr && g1.auxSplit < nodes;
        if (p->launch != RN_SLABP_PREP_M2) {
            RN_CHECK(p->in, RN_E_ARG, "rn_debug_slab_product: no input");
            RN_CHECK((p->prob != nullptr) == scaled, RN_E_ARG, "rn_debug_slab_product: prob belongs to the products that scale by -1 / (2 p)");
            RN_CHECK((p->aux != nullptr) == (g1.aux != nullptr), RN_E_ARG, "rn_debug_slab_product: aux given for a launch that reads none, or missing for one that does");
            RN_CHECK((p->aux2 != nullptr) == split, RN_E_ARG, "rn_debug_slab_product: aux2 belongs to a launch with a split last round, and that launch needs it");
        }
        RN_CHECK(p->nOutA == needA && p->nOutB == needB, RN_E_ARG, "rn_debug_slab_product: output sizes are outNodes * the sweep buffer's row length");
        // operators: through the context's own uploads
        if (int rc = upload_padded(ss.MA, p->MA, g1.m, g1.k)) return rc;
        if (int rc = upload_fragments(ss.MAf, p->MA, g1.m, g1.k)) return rc;
        g1.M = ss.MA; if (g1.Mf) g1.Mf = ss.MAf;
        if (two) {
            if (int rc = upload_padded(ss.MB, p->MB, g2.m, g2.k)) return rc;
            if (int rc = upload_fragments(ss.MBf, p->MB, g2.m, g2.k)) return rc;
            g2.M = ss.MB; if (g2.Mf) g2.Mf = ss.MBf;
        }
        if (p->launch != RN_SLABP_PREP_M2) {
            const int off = (int)(g1.in - ss.in);
            if (int rc = slab_put_rows(ss.in, p->in, g1.k, g1.ldin, off)) return rc;
            info[23] = off;
            if (p->aux) {
                // only the rows the launch reads are the caller's; in the sweep's m1 buffer each row has 2 nv entries and the product reads the first nv
                if (int rc = upload(ss.aux, p->aux, (size_t)nodes * g1.ldaux)) return rc;
                g1.aux = ss.aux;
            } else {
                // (a pair that runs as two launches on a structured context reads the m1 half of the sweep's buffer, which stays zero there)
                std::vector<double> z((size_t)nodes * std::max(2 * nv, nu + nx), 0.0);
                if (int rc = upload(ss.aux, z.data(), z.size())) return rc;
            }
            if (split) { if (int rc = upload(ss.aux2, p->aux2, (size_t)(nodes - g1.auxSplit) * g1.ldaux)) return rc; g1.aux2 = ss.aux2; }
            if (scaled) { if (int rc = upload(ss.prob, p->prob, (size_t)nodes)) return rc; g1.prob = ss.prob; }
        } else info[23] = 0;
        if (needA) { if (int rc = upload(ss.outA, p->outA, needA)) return rc; }
        if (needB) { if (int rc = upload(ss.outB, p->outB, needB)) return rc; }
        SlabReport rep{};
        slabRep = &rep;
        if (p->launch == RN_SLABP_COMP) run_comp(g1, a, 0);
        else if (p->launch == RN_SLABP_PAIR) run_v_lv(g1, g2, a, 0);
        else if (p->launch == RN_SLABP_PREP_M2) run_prep_m2(g1, a);
        else if (epi == EPI_V) run_gemm<EPI_V>(g1);
        else if (epi == EPI_LV) run_gemm<EPI_LV>(g1);
        else run_gemm<EPI_Z>(g1);
        slabRep = nullptr;
        RN_HIP(hipGetLastError());
        RN_HIP(hipStreamSynchronize(stream));
        if (needA) { if (int rc = download(p->outA, ss.outA, needA)) return rc; }
        if (needB) { if (int rc = download(p->outB, ss.outB, needB)) return rc; }
        info[0] = rep.kernel[0]; info[1] = rep.kernel[1]; info[2] = rep.nw[0]; info[3] = rep.pipe; info[4] = rep.frag; info[5] = rep.ct;
        info[6] = rep.grid[0]; info[7] = (int)rep.lds[0];
        slab_info_product(info + 8, g1);
        if (two) slab_info_product(info + 12, g2); else info[12] = info[13] = info[14] = info[15] = 0;
        info[16] = rep.nw[1]; info[17] = rep.grid[1]; info[18] = (int)rep.lds[1];
        info[19] = split ? g1.auxSplit : nodes; info[20] = numCUs; info[21] = rep.pre; info[22] = (int)on;
        return RN_OK;
    }
    int counters(long *out) override {
        RN_CHECK(out, RN_E_ARG, "rn_get_counters: null output");
        out[0] = optBatches; out[1] = exactBatches; out[2] = fallbacks; out[3] = optHold;
        return RN_OK;
    }
    int hist_parts(int first, int n, double *out) override {
        RN_CHECK(first >= 0 && n >= 0 && first + n <= h_it, RN_E_ARG, "rn_get_history_parts: range outside the iterations run");
        RN_HIP(hipStreamSynchronize(stream));
        RN_HIP(hipMemcpy(out, d_histParts + (size_t)4 * first, (size_t)4 * n * sizeof(double), hipMemcpyDeviceToHost));
        return RN_OK;
    }
    int control_action(const double *x0, const double *up, const double *dp, const double *dhat, const double *ahat, int maxIt,
                       int project, double *u0) override {
        RN_CHECK(u0, RN_E_ARG, "rn_control_action: null output");
        if (injectBytes) {   // rn_debug_inject_allocation: a deliberate leak inside this control step (test of the callers' leak check)
            char *leak = nullptr;
            if (int rc = dalloc(&leak, injectBytes)) return rc;
            injectBytes = 0;
        }
        if (int rc = update_state_control(x0, up, dp)) return rc;
        if (int rc = eliminate(dhat, ahat)) return rc;
        if (warmStart && h_it > 0 && !poisoned) { if (int rc = apg_restart_keep_duals()) return rc; }   // y, y+ kept; theta = {1,1}
        else if (int rc = apg_reset()) return rc;
        if (int rc = apg_run(maxIt, nullptr)) return rc;
        T *src = d_u;
        if (project) {  // SmpcController.cu:1647-1650: clamp with the (scaled) bounds of the root node
            RN_HIP(hipMemcpyAsync(d_tmp, d_u, d.nu * sizeof(T), hipMemcpyDeviceToDevice, stream));
            hipLaunchKernelGGL(k_clamp_vec<>, dim3(1), dim3(128), 0, stream, (void *)d_tmp, (const void *)(d_lo + 2 * d.nx), (const void *)(d_hi + 2 * d.nx), d.nu, sizeof(T) == 8 ? 1 : 0);
            src = d_tmp;
        }
        return download(u0, src, d.nu);
    }

    // ---- step-wise API -----------------------------------------------------------------------------------
    // w = y+ + lambda (y+ - y), y = y+ (k_extrapolate<0>, k_dual.hpp): lambda rounded to T here, as the typed kernels took it
    void launch_extrapolate(double lambda) {
        hipLaunchKernelGGL(k_extrapolate<>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, (void *)p_acc, (void *)p_xi, (const void *)p_upd, (double)(T)lambda,
                           (long long)ntot(), sizeof(T) == 8 ? 1 : 0);
    }
    int extrapolate(double lambda) override {
        RN_HIP(hipSetDevice(device));
        launch_extrapolate(lambda);
        RN_HIP(hipGetLastError());
        p_acc_view = p_acc; acc_ready = true;
        return RN_OK;
    }
    int solve_step() override {
        RN_CHECK(factored && affine_ready, RN_E_STATE, "rn_solve_step before the factor step / affine terms");
        RN_HIP(hipSetDevice(device));
        p_acc_view = p_acc;
        return launch_sweep(nullptr);
    }
    int prox() override {
        RN_CHECK(factored, RN_E_STATE, "rn_proximal_fun_g before the factor step");
        RN_HIP(hipSetDevice(device));
        DualArgs<T> a = dual_args();
        a.w = p_acc_view;
        hipLaunchKernelGGL(k_prox_clamp<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, a);
        hipLaunchKernelGGL(k_decide<>, dim3(1), dim3(ELT_THREADS), 0, stream, d_partials, eltBlocks, d_state, a.thrX, a.thrS);
        hipLaunchKernelGGL(k_prox_soft<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, a);
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    int residual() override {
        RN_HIP(hipSetDevice(device));
        hipLaunchKernelGGL(k_axpby<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_res, d_hx, d_z, (T)1, (T)-1, ntot());
        RN_HIP(hipGetLastError());
        return RN_OK;
    }
    int dual_update() override {
        RN_HIP(hipSetDevice(device));
        if (algorithm != RN_ALG_APG) return fbe_dual_update();   // SmpcController.cu:866-880
        hipLaunchKernelGGL(k_axpby<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, p_upd, p_acc_view, d_res, (T)1, (T)stepSize, ntot());
        RN_HIP(hipGetLastError());
        acc_ready = false;
        return RN_OK;
    }
    int primal_infeasibility(double *value) override {
        RN_CHECK(value, RN_E_ARG, "rn_update_primal_infeasibility: null output");
        RN_HIP(hipSetDevice(device));
        hipLaunchKernelGGL(k_absmax<T>, dim3(eltBlocks), dim3(ELT_THREADS), 0, stream, d_res, ntot(), d.nx, ny, d_partials);
        RN_HIP(hipGetLastError());
        std::vector<Partial> hp(eltBlocks);
        RN_HIP(hipMemcpyAsync(hp.data(), d_partials, eltBlocks * sizeof(Partial), hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        double aX = -1, vX = 0, aP = -1, vP = 0; long long iX = 0x7fffffffffffffffLL, iP = iX;
        for (auto &p : hp) {
            if (p.absXi > aX || (p.absXi == aX && p.idxXi < iX)) { aX = p.absXi; vX = p.valXi; iX = p.idxXi; }
            if (p.absPsi > aP || (p.absPsi == aP && p.idxPsi < iP)) { aP = p.absPsi; vP = p.valPsi; iP = p.idxPsi; }
        }
        if (cutStage > 0 && has_comm() && d_scal) {
            // sharded quasi-Newton loops: the tree-global arg-max from the ranks' local ones.  A max all-reduce of (v, -v) per
            // part gives the largest magnitude and its sign (equal magnitudes of opposite sign on two ranks: the positive one)
            double h[4] = {vX, -vX, vP, -vP};
            RN_HIP(hipMemcpyAsync(d_scal + 32, h, sizeof h, hipMemcpyHostToDevice, stream));
            if (int rc = all_reduce(d_scal + 32, 4, true, "ncclAllReduce(primal infeasibility)", 2 /* ncclMax */)) return rc;
            RN_HIP(hipMemcpyAsync(h, d_scal + 32, sizeof h, hipMemcpyDeviceToHost, stream));
            RN_HIP(hipStreamSynchronize(stream));
            vX = h[0] >= h[1] ? h[0] : -h[1];
            vP = h[2] >= h[3] ? h[2] : -h[3];
        }
        *value = vX > vP ? vX : vP;
        return RN_OK;
    }
    int prox_distances(double *dx, double *ds) override {
        IterState st;
        RN_HIP(hipSetDevice(device));
        RN_HIP(hipMemcpyAsync(&st, d_state, sizeof st, hipMemcpyDeviceToHost, stream));
        RN_HIP(hipStreamSynchronize(stream));
        if (dx) *dx = st.distX;
        if (ds) *ds = st.distS;
        return RN_OK;
    }

    // ---- caller data into and out of the context: raw access, operator blocks, tree data, bounds -----------
#include "caller_data.inc"

    // ---- what the plan at hand costs and where it violates its bounds, per stage and per scenario ------------
#include "plan_report.inc"

    // ---- what the plan at hand looks like across the tree: quantiles per stage, rows along every leaf's path --
#include "plan_bands.inc"

    // ---- the warm start shifted one stage toward the root of the scenario tree --------------------------------
#include "shift_warm_start.inc"
#include "lipschitz.inc"

    // ---- the solve certificate: dual bound and optimality gap of the multiplier at hand -----------------------
#include "certificate.inc"

    // ---- multi-GPU ---------------------------------------------------------------------------------------
    // The communicator of this context.  ncclCommInitRank blocks until every rank of the id has arrived -- for ever if one never does.
    // It therefore runs on a HELPER THREAD and the caller waits for it against the wall clock: after `timeoutSeconds` (< 0:
    // $RAPIDNET_COMM_TIMEOUT_S, default 120) the call returns RN_E_COMM and the context stays usable, without a communicator (the
    // reference would exit(), Configuration.h:38-81; this must neither exit nor hang).  The abandoned helper stays blocked inside RCCL
    // for as long as RCCL waits (it holds only its own copies of the arguments); should it ever come back with a communicator, it
    // destroys it.  (First form, round 5: ncclCommInitRankConfig with blocking = 0, polled with ncclCommGetAsyncError and aborted on
    // time-out -- on the one-GPU box a rank of a two-rank id never came back from that sequence, tests/test_gpu_comm_timeout.py; the
    // blocking call is also the one every earlier multi-process rehearsal used.)
    double commTimeoutS = 120.0;
    struct CommJob { std::mutex m; std::condition_variable cv; bool done = false, abandoned = false; int rc = -1; void *comm = nullptr; };
    std::shared_ptr<CommJob> commJob;     // a set-up whose helper thread has not come back
    int comm_init(int rk, int nr, const void *id, double timeoutSeconds = -1.0) override {
        RN_CHECK(nr >= 1 && rk >= 0 && rk < nr, RN_E_ARG, "rn_comm_init: bad rank");
        if (id == nullptr) {               // id == NULL: bookkeeping only (tests emulate the exchange); allowed at any time
            rank = rk; nranks = nr; optHold = 0;
            return RN_OK;
        }
        RN_CHECK(comm == nullptr, RN_E_STATE, "rn_comm_init: the context already has a communicator");
        RN_CHECK(g_nccl.load(), RN_E_COMM, "rn_comm_init: cannot load librccl.so");
        RN_HIP(hipSetDevice(device));
        if (timeoutSeconds < 0) { timeoutSeconds = 120.0; if (const char *e = std::getenv("RAPIDNET_COMM_TIMEOUT_S")) { const double v = std::atof(e); if (v > 0) timeoutSeconds = v; } }
        commTimeoutS = timeoutSeconds;
        UniqueId128 u; std::memcpy(u.b, id, 128);
        auto job = std::make_shared<CommJob>();
        commJob = job;                     // kept: rn_destroy tells a helper that is still inside RCCL that nobody waits for it any more
        const int dev = device;
        std::thread([job, u, nr, rk, dev] {
            void *c = nullptr;
            int rc = hipSetDevice(dev) == hipSuccess ? g_nccl.InitRank(&c, nr, u, rk) : -2;
            std::unique_lock<std::mutex> lk(job->m);
            job->rc = rc; job->comm = rc == 0 ? c : nullptr; job->done = true;
            const bool orphan = job->abandoned;
            lk.unlock();
            job->cv.notify_all();
            if (orphan && rc == 0 && c) { if (g_nccl.CommAbort) (void)g_nccl.CommAbort(c); else if (g_nccl.CommDestroy) (void)g_nccl.CommDestroy(c); }
        }).detach();
        {
            std::unique_lock<std::mutex> lk(job->m);
            if (!job->cv.wait_for(lk, std::chrono::duration<double>(timeoutSeconds), [&] { return job->done; })) {
                job->abandoned = true;
                char b[256];
                snprintf(b, sizeof b, "ncclCommInitRank failed: rank %d of %d waited %.1f s for its peers (time-out; the context has no communicator)", rk, nr, timeoutSeconds);
                err = b;
                return RN_E_COMM;
            }
        }
        RN_CHECK(job->rc == 0 && job->comm, RN_E_COMM, std::string("ncclCommInitRank failed: ") + (job->rc == -2 ? "hipSetDevice on the helper thread" : (g_nccl.GetErrorString ? g_nccl.GetErrorString(job->rc) : "?")));
        commJob.reset();
        // The outcome must be the SAME on every rank.  A peer may have given up (its time-out) a moment before this rank's
        // ncclCommInitRank completed: this rank then holds a communicator whose peer is gone, and its first collective would wait for
        // ever.  So before the communicator is published every rank runs one tiny all-reduce with a BOUNDED wait (an event polled against
        // the same time-out, with ncclCommGetAsyncError): a rank whose handshake does not finish aborts its communicator and returns
        // RN_E_COMM like the peer that gave up.
        {
            void *c = job->comm;
            bool ok = true; std::string why;
            hipEvent_t ev = nullptr;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ok = false; why = "hipEventCreate"; }
            if (ok && hipMemsetAsync(d_tune, 0, sizeof(double), stream) != hipSuccess) { ok = false; why = "hipMemsetAsync"; }
            if (ok) {
                const int rc = g_nccl.AllReduce(d_tune, d_tune, 1, 8 /* ncclFloat64 */, 0 /* ncclSum */, c, stream);
                if (rc != 0) { ok = false; why = std::string("ncclAllReduce: ") + (g_nccl.GetErrorString ? g_nccl.GetErrorString(rc) : "?"); }
            }
            if (ok && hipEventRecord(ev, stream) != hipSuccess) { ok = false; why = "hipEventRecord"; }
            if (ok) {
                const auto t0 = std::chrono::steady_clock::now();
                for (;;) {
                    const hipError_t q = hipEventQuery(ev);
                    if (q == hipSuccess) break;
                    if (q != hipErrorNotReady) { ok = false; why = std::string("hipEventQuery: ") + hipGetErrorString(q); break; }
                    int st = 0;
                    if (g_nccl.GetAsyncError && g_nccl.GetAsyncError(c, &st) == 0 && st != 0 && st != NCCL_IN_PROGRESS) { ok = false; why = std::string("RCCL: ") + (g_nccl.GetErrorString ? g_nccl.GetErrorString(st) : "?"); break; }
                    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeoutSeconds) { ok = false; why = "a peer left between ncclCommInitRank and the first collective (time-out)"; break; }
                    std::this_thread::sleep_for(std::chrono::microseconds(200));
                }
            }
            (void)hipGetLastError();
            if (ev) (void)hipEventDestroy(ev);
            if (!ok) {
                if (g_nccl.CommAbort) (void)g_nccl.CommAbort(c); else if (g_nccl.CommDestroy) (void)g_nccl.CommDestroy(c);
                err = "rn_comm_init: the communicator's handshake failed (" + why + "); the context has no communicator";
                return RN_E_COMM;
            }
        }
        comm = job->comm;
        rank = rk; nranks = nr;
        optHold = 0;                       // every rank starts its batches aligned (the back-off counter decides which path a batch takes)
        // the one-shot transport, set up by the library itself where the cut is already known (rn_create_sharded does it after the cut stage otherwise)
        if (cutStage > 0 && transportReq != RN_EXCHANGE_COLLECTIVE) return exchange_prepare();
        return RN_OK;
    }
    // asynchronous errors of the communicator (a peer that died, a link that went down): asked once per batch, never inside one
    int comm_check() override {
        if (!comm || !g_nccl.GetAsyncError) return RN_OK;
        int st = 0;
        const int q = g_nccl.GetAsyncError(comm, &st);
        RN_CHECK(q == 0 && (st == 0 || st == NCCL_IN_PROGRESS), RN_E_COMM,
                 std::string("RCCL reports an asynchronous error on the communicator: ") + (g_nccl.GetErrorString ? g_nccl.GetErrorString(q != 0 ? q : st) : "?"));
        return RN_OK;
    }
    int set_allreduce(rn_allreduce_fn fn, void *user) override { arHook = fn; arUser = user; optHold = 0; return RN_OK; }
    int shard_info(int *info) override {
        RN_CHECK(info, RN_E_ARG, "rn_shard_info: null output");
        info[0] = rank; info[1] = nranks; info[2] = cutStage;
        info[3] = cutStage > 0 ? h_stageCum[cutStage] - h_stageCum[cutStage - 1] : 0;
        int cnt = 0;
        if (comm && g_nccl.CommCount) { if (g_nccl.CommCount(comm, &cnt) != 0) cnt = -1; }
        info[4] = cnt; info[5] = d.nodes; info[6] = fullNodes > 0 ? fullNodes : d.nodes;
        return RN_OK;
    }
    int shard_global_nodes(int *out, size_t n) override {
        RN_CHECK(out && n == (size_t)d.nodes, RN_E_ARG, "rn_shard_global_nodes: one entry per local node expected");
        for (int i = 0; i < d.nodes; i++) out[i] = globalNode.empty() ? i : globalNode[i];
        return RN_OK;
    }
    void set_global_nodes(const int *g, int n, int full) override { globalNode.assign(g, g + n); fullNodes = full; }
    int device_ordinal() const override { return device; }
    int join_local_group(LocalGroup *g, int rk) override {
        RN_CHECK(g && rk >= 0 && rk < g->n, RN_E_ARG, "rn_debug_local_group_join: bad rank");
        RN_CHECK(comm == nullptr, RN_E_STATE, "rn_debug_local_group_join: the context already has an RCCL communicator");
        if (!localMember) localMember = new LocalMember();
        localMember->g = g; localMember->rank = rk;
        rank = rk; nranks = g->n;
        return set_allreduce(local_allreduce, localMember);
    }
    int sweep_phase(int phase) override {
        RN_CHECK(factored && affine_ready, RN_E_STATE, "rn_debug_sweep_phase before the factor step / affine terms");
        RN_CHECK(phase == 1 || phase == 2, RN_E_ARG, "rn_debug_sweep_phase: phase must be 1 or 2");
        RN_HIP(hipSetDevice(device));
        p_acc_view = p_acc;
        return launch_sweep(nullptr, phase);
    }
    int cut_buffer(int write, double *host, size_t n) override {
        RN_CHECK(cutStage > 0, RN_E_STATE, "rn_debug_cut_buffer: no cut stage set");
        const size_t cnt = (size_t)(h_stageCum[cutStage] - h_stageCum[cutStage - 1]) * (d.nv + 2 * d.nx);
        RN_CHECK(host && n == cnt, RN_E_ARG, "rn_debug_cut_buffer: size mismatch");
        RN_HIP(hipSetDevice(device));
        return write ? upload(d_cut, host, n) : download(host, d_cut, n);
    }
    // streaming ceilings of this box: flat read-only and copy, `bytes` per pass (temporary buffers), best of `reps`
    int measure_hbm(size_t bytes, int reps, double *readGBs, double *copyGBs) override {
        RN_CHECK(bytes >= (1u << 20) && reps >= 1 && readGBs && copyGBs, RN_E_ARG, "rn_measure_hbm: bytes >= 1 MiB, reps >= 1");
        RN_HIP(hipSetDevice(device));
        void *a = nullptr, *b = nullptr; double *sink = nullptr;
        RN_HIP(hipMalloc(&a, bytes));
        if (hipMalloc(&b, bytes) != hipSuccess) { (void)hipFree(a); err = "rn_measure_hbm: out of memory"; return RN_E_HIP; }
        if (hipMalloc((void **)&sink, 65536 * sizeof(double)) != hipSuccess) { (void)hipFree(a); (void)hipFree(b); err = "rn_measure_hbm: out of memory"; return RN_E_HIP; }
        (void)hipMemsetAsync(a, 0, bytes, stream); (void)hipMemsetAsync(b, 0, bytes, stream);
        const long long n = (long long)(bytes / 16);
        const int blocks = 256 * 16;
        hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        double bestR = 0, bestC = 0;
        for (int r = 0; r < reps + 1; r++) {   // first pass = warm-up
            float ms = 0;
            (void)hipEventRecord(e0, stream);
            hipLaunchKernelGGL(k_bw_probe<>, dim3(blocks), dim3(256), 0, stream, (const nat_d2 *)a, (nat_d2 *)nullptr, n, sink);
            (void)hipEventRecord(e1, stream); (void)hipEventSynchronize(e1); (void)hipEventElapsedTime(&ms, e0, e1);
            if (r > 0 && ms > 0) bestR = std::max(bestR, (double)bytes / (ms * 1e-3) / 1e9);
            (void)hipEventRecord(e0, stream);
            // copy: 4 workgroups per CU measured best for a read + write stream (tools/probes/probe_stream.hip: 6.2 TB/s with
            // 1 024 workgroups, 5.2-5.4 with 4 096 or 8 192 on a 1 GiB vector)
            hipLaunchKernelGGL(k_bw_probe<>, dim3(numCUs * 4), dim3(256), 0, stream, (const nat_d2 *)a, (nat_d2 *)b, n, sink);
            (void)hipEventRecord(e1, stream); (void)hipEventSynchronize(e1); (void)hipEventElapsedTime(&ms, e0, e1);
            if (r > 0 && ms > 0) bestC = std::max(bestC, 2.0 * (double)bytes / (ms * 1e-3) / 1e9);
        }
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        (void)hipFree(a); (void)hipFree(b); (void)hipFree(sink);
        RN_HIP(hipGetLastError());
        *readGBs = bestR; *copyGBs = bestC;
        return RN_OK;
    }
    int set_operator_mode(int mode) override {
        RN_CHECK(mode == RN_OPS_DENSE || mode == RN_OPS_STRUCTURED || mode == RN_OPS_AUTO, RN_E_ARG, "rn_set_operator_mode: RN_OPS_DENSE, RN_OPS_STRUCTURED or RN_OPS_AUTO");
        const int want = mode == RN_OPS_DENSE ? 0 : 1;
        RN_CHECK(!factored || want == structured, RN_E_STATE, "rn_set_operator_mode must precede rn_factor_step");
        opsMode = mode; structured = want;
        return RN_OK;
    }
    int get_operator_mode(int *requested, int *active) override {
        if (requested) *requested = opsMode;
        if (active) *active = structured ? RN_OPS_STRUCTURED : RN_OPS_DENSE;
        return RN_OK;
    }
    int set_operator_storage(int storage) override {
        RN_CHECK(storage == RN_STORE_NATIVE || storage == RN_STORE_F32, RN_E_ARG, "rn_set_operator_storage: RN_STORE_NATIVE or RN_STORE_F32");
        RN_CHECK(!factored, RN_E_STATE, "rn_set_operator_storage must precede rn_factor_step");
        storeReq = storage;
        block_layout();
        lip_invalidate();
        return RN_OK;
    }
    int set_sweep_pairing(int mode) override {
        RN_CHECK(mode == RN_PAIR_OFF || mode == RN_PAIR_ON || mode == RN_PAIR_AUTO, RN_E_ARG, "rn_set_sweep_pairing: RN_PAIR_OFF, RN_PAIR_ON or RN_PAIR_AUTO");
        pairReq = mode;
        if (algorithm == RN_ALG_NAMA) { RN_HIP(hipSetDevice(device)); return ensure_pair_buffers(); }
        return RN_OK;
    }
    int get_sweep_pairing(int *requested, int *active) override {
        if (requested) *requested = pairReq;
        if (active) *active = (algorithm == RN_ALG_NAMA && pair_active()) ? 1 : 0;
        return RN_OK;
    }
    int get_operator_storage(int *requested, int *active) override {
        if (requested) *requested = storeReq;
        if (active) *active = (!structured && (d_A32 != nullptr || (sizeof(T) == 4 && d_A != nullptr))) ? RN_STORE_F32 : RN_STORE_NATIVE;
        return RN_OK;
    }
    // RN_OPS_AUTO, a caller hands in a block of its own: from here on the context runs on dense per-node blocks -- the factor step once
    // more on the saved inputs, this time expanding every block (Engine.cu:721-745) into d_A
    int materialise_dense() {
        RN_CHECK(factored && structured && opsMode == RN_OPS_AUTO && !h_sys.B.empty(), RN_E_STATE, "materialise_dense: not an RN_OPS_AUTO context after its factor step");
        if (int rc = v_flush()) return rc;       // (a pending v belongs to the structured form's last sweep)
        RN_HIP(hipStreamSynchronize(stream));
        structured = 0; splitFirst = -1;      // (the streaming kernel's launch shape is decided by the factor step)
        rn_system sy{h_sys.B.data(), h_sys.Gd.data(), h_sys.L.data(), h_sys.Lhat.data(), h_sys.W.data(), h_sys.diag.data(), h_sys.xmin.data(), h_sys.xmax.data(),
                     h_sys.xsafe.data(), h_sys.umin.data(), h_sys.umax.data(), h_sys.alpha1.data()};
        keepBounds = true;
        const int rcf = factor_step(&sy);
        keepBounds = false;
        if (rcf) { structured = 1; return rcf; }
        if (algorithm == RN_ALG_NAMA) return set_algorithm(algorithm, lbfgsSize);   // (its paired sweep needs buffers of its own in dense mode)
        return RN_OK;
    }
    // rn_create_sharded, after the moments: what k_tree_data needs to recompute them (and the full-tree row of every local node)
    int set_cut_children(const int *c0, const int *nc, int nPar, bool contiguous, int cutFirst, int nCutNodes, const double *fullP, const double *fullE) override {
        RN_CHECK(c0 && nc && fullP && nPar > 0 && nCutNodes > 0 && !globalNode.empty(), RN_E_ARG, "set_cut_children: bad input");
        RN_HIP(hipSetDevice(device));
        if (int rc = dalloc(&d_gmap, (size_t)d.nodes)) return rc;
        if (int rc = dalloc(&d_cutC0, (size_t)nPar)) return rc;
        if (int rc = dalloc(&d_cutNc, (size_t)nPar)) return rc;
        if (int rc = dalloc(&d_fullP, (size_t)nCutNodes)) return rc;
        if (int rc = dalloc(&d_fullE, (size_t)nCutNodes * d.nd)) return rc;
        RN_HIP(hipMemcpy(d_gmap, globalNode.data(), (size_t)d.nodes * sizeof(int), hipMemcpyHostToDevice));
        RN_HIP(hipMemcpy(d_cutC0, c0, (size_t)nPar * sizeof(int), hipMemcpyHostToDevice));
        RN_HIP(hipMemcpy(d_cutNc, nc, (size_t)nPar * sizeof(int), hipMemcpyHostToDevice));
        RN_HIP(hipMemcpy(d_fullP, fullP, (size_t)nCutNodes * sizeof(double), hipMemcpyHostToDevice));
        if (fullE) RN_HIP(hipMemcpy(d_fullE, fullE, (size_t)nCutNodes * d.nd * sizeof(double), hipMemcpyHostToDevice));
        else RN_HIP(hipMemset(d_fullE, 0, (size_t)nCutNodes * d.nd * sizeof(double)));
        nCutPar = nPar; cutFirstFull = cutFirst; cutContiguous = contiguous;
        return RN_OK;
    }
    int cut_moments(double *E, double *P, size_t nParents) override {
        RN_CHECK(cutStage > 0 && moments_set && d_momE, RN_E_STATE, "rn_debug_cut_moments: no children moments are set");
        RN_CHECK(E && P && nParents == (size_t)(h_stageCum[cutStage] - h_stageCum[cutStage - 1]), RN_E_ARG, "rn_debug_cut_moments: one row per cut parent expected");
        RN_HIP(hipSetDevice(device));
        if (int rc = download(E, d_momE, nParents * d.nd)) return rc;
        return download(P, d_momP, nParents);
    }
    int set_cut_moments(const double *E, const double *P, size_t nParents) override {
        RN_CHECK(cutStage > 0, RN_E_STATE, "rn_set_cut_children_moments: set the cut stage first");
        RN_CHECK(E && P && nParents == (size_t)(h_stageCum[cutStage] - h_stageCum[cutStage - 1]), RN_E_ARG, "rn_set_cut_children_moments: one row per cut parent expected");
        RN_HIP(hipSetDevice(device));
        if (!d_momE) { if (int rc = dalloc(&d_momE, nParents * d.nd)) return rc; if (int rc = dalloc(&d_momP, nParents)) return rc; }
        if (int rc = upload(d_momE, E, nParents * d.nd)) return rc;
        if (int rc = upload(d_momP, P, nParents)) return rc;
        moments_set = true;
        return RN_OK;
    }
    int set_cut_stage(int c) override {
        RN_CHECK(c == -1 || (c >= 1 && c < d.N), RN_E_ARG, "rn_set_cut_stage: stage out of range");
        cutStage = c; moments_set = false;
        return RN_OK;
    }

#include "fbe_methods.inc"
};

}  // namespace rn

struct rn_ctx { rn::CtxBase *impl; };
static thread_local std::string g_create_error;   // rn_create failure message of this thread (rn_last_error(NULL))

#define RN_GUARD(ctx) if (!(ctx) || !(ctx)->impl) return RN_E_ARG

extern "C" {

int rn_create(const rn_dims *dims, const rn_tree *tree, int precision, int device, rn_ctx **out) {
    if (!dims || !tree || !out) return RN_E_ARG;
    if (!tree->stages || !tree->nodesPerStage || !tree->nodesPerStageCumul || !tree->ancestor || !tree->probNode) return RN_E_ARG;
    *out = nullptr;
    int rc;
    rn::CtxBase *impl;
    if (precision == RN_F64) { auto *c = new rn::Ctx<double>(); impl = c; rc = c->init(dims, tree, device); }
    else if (precision == RN_F32) { auto *c = new rn::Ctx<float>(); impl = c; rc = c->init(dims, tree, device); }
    else return RN_E_ARG;
    if (rc != RN_OK) { g_create_error = impl->err; delete impl; return rc; }
    *out = new rn_ctx{impl};
    return RN_OK;
}
int rn_destroy(rn_ctx *ctx) { RN_GUARD(ctx); delete ctx->impl; delete ctx; return RN_OK; }
const char *rn_last_error(const rn_ctx *ctx) { return (ctx && ctx->impl) ? ctx->impl->err.c_str() : g_create_error.c_str(); }
int rn_synchronize(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->synchronize(); }
int rn_factor_step(rn_ctx *ctx, const rn_system *sys) { RN_GUARD(ctx); return ctx->impl->factor_step(sys); }
int rn_set_tree_errors(rn_ctx *ctx, const double *ed, const double *ep) { RN_GUARD(ctx); return ctx->impl->set_tree_errors(ed, ep); }
int rn_set_tree_data(rn_ctx *ctx, size_t nodes, const double *p, const double *ed, const double *ep) { RN_GUARD(ctx); return ctx->impl->set_tree_data(nodes, RN_F64, false, p, ed, ep); }
int rn_set_tree_data_device(rn_ctx *ctx, size_t nodes, int precision, const void *p, const void *ed, const void *ep) { RN_GUARD(ctx); return ctx->impl->set_tree_data(nodes, precision, true, p, ed, ep); }
int rn_get_tree_data(rn_ctx *ctx, size_t nodes, double *p, double *ed, double *ep) { RN_GUARD(ctx); return ctx->impl->get_tree_data(nodes, p, ed, ep); }
int rn_set_bounds(rn_ctx *ctx, int g, size_t rows, const double *xmin, const double *xmax, const double *xsafe, const double *umin, const double *umax) {
    RN_GUARD(ctx);
    const void *b[5] = {xmin, xmax, xsafe, umin, umax};
    return ctx->impl->set_bounds(g, rows, RN_F64, false, b);
}
int rn_set_bounds_device(rn_ctx *ctx, int g, size_t rows, int precision, const void *xmin, const void *xmax, const void *xsafe, const void *umin, const void *umax) {
    RN_GUARD(ctx);
    const void *b[5] = {xmin, xmax, xsafe, umin, umax};
    return ctx->impl->set_bounds(g, rows, precision, true, b);
}
int rn_get_bounds_layout(rn_ctx *ctx, int *g, size_t *rows) { RN_GUARD(ctx); return ctx->impl->get_bounds_layout(g, rows); }
int rn_get_bounds(rn_ctx *ctx, size_t rows, double *xmin, double *xmax, double *xsafe, double *umin, double *umax) {
    RN_GUARD(ctx);
    double *b[5] = {xmin, xmax, xsafe, umin, umax};
    return ctx->impl->get_bounds(rows, b);
}
int rn_debug_cut_moments(rn_ctx *ctx, double *E, double *P, size_t n) { RN_GUARD(ctx); return ctx->impl->cut_moments(E, P, n); }
int rn_plan_report(rn_ctx *ctx, size_t stages, double *perStage) { RN_GUARD(ctx); return ctx->impl->plan_report(stages, perStage); }
int rn_plan_report_scenarios(rn_ctx *ctx, size_t leaves, double *perLeaf, int *leafNode) { RN_GUARD(ctx); return ctx->impl->plan_report_scenarios(leaves, perLeaf, leafNode); }
int rn_plan_report_device(rn_ctx *ctx, void **perStage, void **perLeaf, size_t *leaves) { RN_GUARD(ctx); return ctx->impl->plan_report_device(perStage, perLeaf, leaves); }
int rn_plan_quantiles(rn_ctx *ctx, int which, size_t nq, const double *q, size_t stages, double *out) { RN_GUARD(ctx); return ctx->impl->plan_quantiles(which, nq, q, stages, out); }
int rn_plan_quantiles_device(rn_ctx *ctx, int which, size_t nq, const double *q, void **out) { RN_GUARD(ctx); return ctx->impl->plan_quantiles_device(which, nq, q, out); }
int rn_plan_paths(rn_ctx *ctx, int which, size_t leaves, double *out, int *leafNode) { RN_GUARD(ctx); return ctx->impl->plan_paths(which, leaves, out, leafNode); }
int rn_shift_warm_start(rn_ctx *ctx, int rootChild) { RN_GUARD(ctx); return ctx->impl->shift_warm_start(rootChild); }
int rn_set_shift_map(rn_ctx *ctx, size_t nodes, const int *map) { RN_GUARD(ctx); return ctx->impl->set_shift_map(nodes, map); }
int rn_get_shift_map(rn_ctx *ctx, int rootChild, size_t nodes, int *map) { RN_GUARD(ctx); return ctx->impl->get_shift_map(rootChild, nodes, map); }
int rn_estimate_lipschitz(rn_ctx *ctx, int maxIterations, double tol, int checkEvery, const double *startXi, const double *startPsi, unsigned long long seed, double *out, double *history) {
    RN_GUARD(ctx); return ctx->impl->estimate_lipschitz(maxIterations, tol, checkEvery, startXi, startPsi, seed, out, history);
}
int rn_get_lipschitz(rn_ctx *ctx, double *out, int *stale) { RN_GUARD(ctx); return ctx->impl->get_lipschitz(out, stale); }
int rn_set_step_rule(rn_ctx *ctx, int rule, double margin, int iterations) { RN_GUARD(ctx); return ctx->impl->set_step_rule(rule, margin, iterations); }
int rn_get_step_rule(rn_ctx *ctx, int *rule, double *margin, int *iterations, double *inForce) { RN_GUARD(ctx); return ctx->impl->get_step_rule(rule, margin, iterations, inForce); }
int rn_solve_certificate(rn_ctx *ctx, double *out) { RN_GUARD(ctx); return ctx->impl->solve_certificate(out); }
int rn_solve_certificate_device(rn_ctx *ctx, void **record) { RN_GUARD(ctx); return ctx->impl->solve_certificate_device(record); }
int rn_debug_certificate_hz(rn_ctx *ctx, double *hzXi, double *hzPsi) { RN_GUARD(ctx); return ctx->impl->certificate_hz(hzXi, hzPsi); }
int rn_set_uncertainty(rn_ctx *ctx, int dflag, int pflag, double w) { RN_GUARD(ctx); return ctx->impl->set_uncertainty(dflag, pflag, w); }
int rn_update_state_control(rn_ctx *ctx, const double *x, const double *u, const double *dm) { RN_GUARD(ctx); return ctx->impl->update_state_control(x, u, dm); }
int rn_eliminate_input_disturbance_coupling(rn_ctx *ctx, const double *dh, const double *ah) { RN_GUARD(ctx); return ctx->impl->eliminate(dh, ah); }
int rn_set_parameters(rn_ctx *ctx, double s, double px, double pxs) { RN_GUARD(ctx); return ctx->impl->set_parameters(s, px, pxs); }
int rn_apg_reset(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->apg_reset(); }
int rn_apg_iterate(rn_ctx *ctx, int n, double *h) { RN_GUARD(ctx); return ctx->impl->apg_iterate(n, h); }
int rn_algorithm_apg(rn_ctx *ctx, int n, double *h) { RN_GUARD(ctx); if (int rc = ctx->impl->apg_reset()) return rc; return ctx->impl->apg_run(n, h); }
int rn_apg_solve(rn_ctx *ctx, int maxIt, double tol, int every, int *run, double *h) { RN_GUARD(ctx); return ctx->impl->apg_solve(maxIt, tol, every, run, h); }
int rn_set_stop_tolerance(rn_ctx *ctx, double tol, int every) { RN_GUARD(ctx); return ctx->impl->set_stop_tolerance(tol, every); }
int rn_get_stop_tolerance(rn_ctx *ctx, double *tol, int *every) { RN_GUARD(ctx); return ctx->impl->get_stop_tolerance(tol, every); }
int rn_get_last_solve(rn_ctx *ctx, long out[4]) { RN_GUARD(ctx); return ctx->impl->last_solve(out); }
int rn_set_restart(rn_ctx *ctx, int mode) { RN_GUARD(ctx); return ctx->impl->set_restart(mode); }
int rn_get_restart(rn_ctx *ctx, int *mode) { RN_GUARD(ctx); return ctx->impl->get_restart(mode); }
int rn_get_restart_info(rn_ctx *ctx, long counts[4], double last[3]) { RN_GUARD(ctx); return ctx->impl->restart_info(counts, last); }
int rn_control_action(rn_ctx *ctx, const double *x, const double *u, const double *dm, const double *dh, const double *ah, int maxIt,
                      int project, double *u0) { RN_GUARD(ctx); return ctx->impl->control_action(x, u, dm, dh, ah, maxIt, project, u0); }
int rn_dual_extrapolation_step(rn_ctx *ctx, double l) { RN_GUARD(ctx); return ctx->impl->extrapolate(l); }
int rn_solve_step(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->solve_step(); }
int rn_proximal_fun_g(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->prox(); }
int rn_compute_fixed_point_residual(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->residual(); }
int rn_dual_update(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->dual_update(); }
int rn_update_primal_infeasibility(rn_ctx *ctx, double *v) { RN_GUARD(ctx); return ctx->impl->primal_infeasibility(v); }
int rn_get_prox_distances(rn_ctx *ctx, double *a, double *b) { RN_GUARD(ctx); return ctx->impl->prox_distances(a, b); }
size_t rn_buffer_size(const rn_ctx *ctx, int id) { return (ctx && ctx->impl) ? ctx->impl->buffer_size(id) : 0; }
int rn_get(rn_ctx *ctx, int id, double *h, size_t n) { RN_GUARD(ctx); return ctx->impl->get(id, h, n); }
int rn_set(rn_ctx *ctx, int id, const double *h, size_t n) { RN_GUARD(ctx); return ctx->impl->set(id, h, n); }
int rn_get_range(rn_ctx *ctx, int id, size_t first, size_t n, double *h) { RN_GUARD(ctx); return ctx->impl->get_range(id, first, n, h); }
int rn_set_range(rn_ctx *ctx, int id, size_t first, size_t n, const double *h) { RN_GUARD(ctx); return ctx->impl->set_range(id, first, n, h); }
int rn_get_operator(rn_ctx *ctx, int op, int node, double *h, size_t n) { RN_GUARD(ctx); return ctx->impl->get_operator(op, node, h, n); }
int rn_device_pointer(rn_ctx *ctx, int id, void **p, size_t *n, int *prec) { RN_GUARD(ctx); return ctx->impl->device_pointer(id, p, n, prec); }
int rn_profile_enable(rn_ctx *ctx, int on) { RN_GUARD(ctx); return ctx->impl->profile_enable(on); }
int rn_profile_reset(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->profile_reset(); }
int rn_profile_read(rn_ctx *ctx, double ms[4], long n[4]) { RN_GUARD(ctx); return ctx->impl->profile_read(ms, n); }
int rn_algorithmic_bytes(const rn_ctx *ctx, double *b, double *dl) { RN_GUARD(ctx); return ctx->impl->algorithmic_bytes(b, dl); }
void *rn_stream(rn_ctx *ctx) { return (ctx && ctx->impl) ? ctx->impl->stream_handle() : nullptr; }
int rn_comm_unique_id(void *id128) {
    if (!id128) return RN_E_ARG;
    if (!rn::g_nccl.load()) return RN_E_COMM;
    return rn::g_nccl.GetUniqueId(id128) == 0 ? RN_OK : RN_E_COMM;
}
int rn_comm_init(rn_ctx *ctx, int rank, int nranks, const void *id128) { RN_GUARD(ctx); return ctx->impl->comm_init(rank, nranks, id128); }
int rn_comm_init_timeout(rn_ctx *ctx, int rank, int nranks, const void *id128, double timeoutSeconds) { RN_GUARD(ctx); return ctx->impl->comm_init(rank, nranks, id128, timeoutSeconds); }
int rn_comm_check(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->comm_check(); }
int rn_comm_library(char *buf, size_t n) {
    if (!buf || n == 0) return RN_E_ARG;
    if (!rn::g_nccl.load()) { buf[0] = 0; return RN_E_COMM; }
    snprintf(buf, n, "%s", rn::g_nccl.path.c_str());
    return RN_OK;
}
int rn_set_cut_stage(rn_ctx *ctx, int stage) { RN_GUARD(ctx); return ctx->impl->set_cut_stage(stage); }
int rn_get_history_parts(rn_ctx *ctx, int first, int n, double *out) { RN_GUARD(ctx); return ctx->impl->hist_parts(first, n, out); }
int rn_get_kernel_info(rn_ctx *ctx, int info[8]) { RN_GUARD(ctx); return ctx->impl->kernel_info(info); }
int rn_get_counters(rn_ctx *ctx, long out[4]) { RN_GUARD(ctx); return ctx->impl->counters(out); }
int rn_set_cut_children_moments(rn_ctx *ctx, const double *E, const double *P, size_t n) { RN_GUARD(ctx); return ctx->impl->set_cut_moments(E, P, n); }
int rn_set_operator_mode(rn_ctx *ctx, int mode) { RN_GUARD(ctx); return ctx->impl->set_operator_mode(mode); }
int rn_get_operator_mode(rn_ctx *ctx, int *requested, int *active) { RN_GUARD(ctx); return ctx->impl->get_operator_mode(requested, active); }
int rn_set_operator_storage(rn_ctx *ctx, int storage) { RN_GUARD(ctx); return ctx->impl->set_operator_storage(storage); }
int rn_get_operator_storage(rn_ctx *ctx, int *requested, int *active) { RN_GUARD(ctx); return ctx->impl->get_operator_storage(requested, active); }
int rn_set_sweep_pairing(rn_ctx *ctx, int mode) { RN_GUARD(ctx); return ctx->impl->set_sweep_pairing(mode); }
int rn_get_sweep_pairing(rn_ctx *ctx, int *requested, int *active) { RN_GUARD(ctx); return ctx->impl->get_sweep_pairing(requested, active); }
int rn_set_operator(rn_ctx *ctx, int op, int node, const double *h, size_t n) { RN_GUARD(ctx); return ctx->impl->set_operator(op, node, h, n); }
int rn_set_operators(rn_ctx *ctx, size_t nodes, const double *phi, const double *psi, const double *D, const double *F) {
    RN_GUARD(ctx); const void *op[4] = {phi, psi, D, F}; return ctx->impl->set_operators(nodes, RN_F64, false, op);
}
int rn_get_operators(rn_ctx *ctx, size_t nodes, double *phi, double *psi, double *D, double *F) {
    RN_GUARD(ctx); void *op[4] = {phi, psi, D, F}; return ctx->impl->get_operators(nodes, RN_F64, false, op);
}
int rn_set_operators_device(rn_ctx *ctx, size_t nodes, int precision, const void *phi, const void *psi, const void *D, const void *F) {
    RN_GUARD(ctx); const void *op[4] = {phi, psi, D, F}; return ctx->impl->set_operators(nodes, precision, true, op);
}
int rn_get_operators_device(rn_ctx *ctx, size_t nodes, int precision, void *phi, void *psi, void *D, void *F) {
    RN_GUARD(ctx); void *op[4] = {phi, psi, D, F}; return ctx->impl->get_operators(nodes, precision, true, op);
}
int rn_set_warm_start(rn_ctx *ctx, int on) { RN_GUARD(ctx); return ctx->impl->set_warm_start(on); }
int rn_set_exchange_mode(rn_ctx *ctx, int mode) { RN_GUARD(ctx); return ctx->impl->set_exchange_mode(mode); }
int rn_measure_hbm(rn_ctx *ctx, size_t bytes, int reps, double *r, double *c) { RN_GUARD(ctx); return ctx->impl->measure_hbm(bytes, reps, r, c); }
int rn_set_algorithm(rn_ctx *ctx, int alg, int m) { RN_GUARD(ctx); return ctx->impl->set_algorithm(alg, m); }
int rn_fbe_reset(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->fbe_reset(); }
int rn_compute_hessian_oracle(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->hessian_oracle(); }
int rn_compute_gradient_fbe(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->gradient_fbe(); }
int rn_update_fixed_point_residual_nama(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->nama_residual(); }
int rn_compute_lbfgs_direction(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->lbfgs_direction(); }
int rn_update_lbfgs_buffer(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->lbfgs_update_buffer(); }
int rn_two_loop_recursion_lbfgs(rn_ctx *ctx) { RN_GUARD(ctx); return ctx->impl->lbfgs_two_loop(); }
int rn_compute_value_fbe(rn_ctx *ctx, double *v) { RN_GUARD(ctx); return ctx->impl->value_fbe(v); }
int rn_line_search_lbfgs_update(rn_ctx *ctx, double vy, double *tau) { RN_GUARD(ctx); return ctx->impl->line_search_fbe(vy, tau); }
int rn_line_search_ame_lbfgs_update(rn_ctx *ctx, double vy, double *tau) { RN_GUARD(ctx); return ctx->impl->line_search_ame(vy, tau); }
int rn_algorithm_fbe_nama(rn_ctx *ctx, int n, double *h, double *v, double *t) { RN_GUARD(ctx); return ctx->impl->algorithm_fbe_nama(n, h, v, t); }
int rn_lbfgs_state(rn_ctx *ctx, int set, int *col, int *mem, double *H, double *rho) { RN_GUARD(ctx); return ctx->impl->lbfgs_state(set, col, mem, H, rho); }
int rn_lbfgs_column(rn_ctx *ctx, int set, int which, int col, double *h, size_t n) { RN_GUARD(ctx); return ctx->impl->lbfgs_column(set, which, col, h, n); }
int rn_debug_sweep_phase(rn_ctx *ctx, int phase) { RN_GUARD(ctx); return ctx->impl->sweep_phase(phase); }
int rn_debug_cut_buffer(rn_ctx *ctx, int write, double *host, size_t n) { RN_GUARD(ctx); return ctx->impl->cut_buffer(write, host, n); }

// ---- multi-GPU through the boundary ------------------------------------------------------------------------------------
int rn_default_cut_stage(const rn_dims *dims, const rn_tree *tree) { return rn::default_cut_stage(dims, tree); }
int rn_partition_create(const rn_dims *dims, const rn_tree *tree, const double *errD, const double *errP, int rank, int nranks, int cutStage,
                        rn_partition *out) {
    return rn::build_partition(dims, tree, errD, errP, rank, nranks, cutStage, out, g_create_error);
}
void rn_partition_destroy(rn_partition *p) {
    if (!p || !p->owner) return;
    delete static_cast<rn::PartitionData *>(p->owner);
    std::memset(p, 0, sizeof *p);
}
int rn_create_sharded(const rn_dims *dims, const rn_tree *tree, const double *errD, const double *errP, int precision, int device, int rank,
                      int nranks, int cutStage, const void *id128, rn_ctx **out) {
    if (!dims || !tree || !out) return RN_E_ARG;
    *out = nullptr;
    if (nranks == 1) {   // a plain unsharded context
        if (rank != 0) { g_create_error = "rn_create_sharded: bad rank"; return RN_E_ARG; }
        if (int rc = rn_create(dims, tree, precision, device, out)) return rc;
        if (errD && errP) {
            const int rc = (*out)->impl->set_tree_errors(errD, errP);
            if (rc != RN_OK) { g_create_error = (*out)->impl->err; rn_destroy(*out); *out = nullptr; return rc; }
        }
        return RN_OK;
    }
    rn_partition part;
    if (int rc = rn::build_partition(dims, tree, errD, errP, rank, nranks, cutStage, &part, g_create_error)) return rc;
    rn_ctx *ctx = nullptr;
    int rc = rn_create(&part.dims, &part.tree, precision, device, &ctx);
    if (rc == RN_OK) {
        rn::CtxBase *c = ctx->impl;
        c->set_global_nodes(part.globalNode, part.dims.nodes, dims->nodes);
        c->set_full_tree(tree->nodesPerStageCumul, tree->ancestor, dims->N, dims->nodes);      // (rn_plan_quantiles / rn_plan_paths cover the whole tree)
        if (part.errorDemandNode && part.errorPriceNode) rc = c->set_tree_errors(part.errorDemandNode, part.errorPriceNode);
        if (rc == RN_OK) rc = c->comm_init(rank, nranks, id128);
        if (rc == RN_OK) rc = c->set_cut_stage(part.cutStage);
        if (rc == RN_OK) {
            std::vector<double> zeros;
            const double *E = part.momE;
            if (!E) { zeros.assign((size_t)part.nCutParents * dims->nd, 0.0); E = zeros.data(); }
            rc = c->set_cut_moments(E, part.momP, (size_t)part.nCutParents);
        }
        if (rc == RN_OK) {   // what rn_set_tree_data needs to recompute the moments: every cut parent's child range, the cut stage's full-tree p and errorDemand
            const rn::PartitionData *pd = static_cast<const rn::PartitionData *>(part.owner);
            const int c0 = tree->nodesPerStageCumul[part.cutStage], c1 = tree->nodesPerStageCumul[part.cutStage + 1];
            rc = c->set_cut_children(pd->cutChildStart.data(), pd->cutChildCount.data(), part.nCutParents, pd->cutContiguous, c0, c1 - c0,
                                     tree->probNode + c0, errD ? errD + (size_t)c0 * dims->nd : nullptr);
        }
        if (rc == RN_OK && id128) rc = c->exchange_prepare_api();    // AUTO / one-shot: this rank's inbox, the peers' mapped (collective; falls back by agreement)
        if (rc != RN_OK) { g_create_error = c->err; rn_destroy(ctx); ctx = nullptr; }
    }
    rn_partition_destroy(&part);
    *out = ctx;
    return rc;
}
int rn_shard_info(rn_ctx *ctx, int info[7]) { RN_GUARD(ctx); return ctx->impl->shard_info(info); }
int rn_shard_global_nodes(rn_ctx *ctx, int *g, size_t n) { RN_GUARD(ctx); return ctx->impl->shard_global_nodes(g, n); }
int rn_debug_set_allreduce(rn_ctx *ctx, rn_allreduce_fn fn, void *user) { RN_GUARD(ctx); return ctx->impl->set_allreduce(fn, user); }
int rn_debug_local_group_create(int nranks, void **group) {
    if (!group || nranks < 1 || nranks > rn::LOCAL_GROUP_MAX) return RN_E_ARG;
    rn::LocalGroup *g = new rn::LocalGroup();
    g->n = nranks; g->bufs.assign(nranks, nullptr); g->counts.assign(nranks, 0); g->f64.assign(nranks, 0);
    if (const char *e = std::getenv("RAPIDNET_GROUP_TIMEOUT_S")) { const int t = std::atoi(e); if (t > 0) g->timeoutSeconds = t; }
    *group = g;
    return RN_OK;
}
int rn_debug_local_group_join(rn_ctx *ctx, void *group, int rank) { RN_GUARD(ctx); return ctx->impl->join_local_group(static_cast<rn::LocalGroup *>(group), rank); }
int rn_debug_local_group_destroy(void *group) { if (!group) return RN_E_ARG; delete static_cast<rn::LocalGroup *>(group); return RN_OK; }
int rn_debug_inject_allocation(rn_ctx *ctx, size_t bytes) { RN_GUARD(ctx); return ctx->impl->inject_allocation(bytes); }
int rn_debug_guard_poke(rn_ctx *ctx, int nbytes) { RN_GUARD(ctx); return ctx->impl->guard_poke(nbytes); }
int rn_debug_set_knob(rn_ctx *ctx, int knob, int value) { RN_GUARD(ctx); return ctx->impl->set_knob(knob, value); }
int rn_debug_stream_info(rn_ctx *ctx, int info[4]) { RN_GUARD(ctx); return ctx->impl->stream_info(info); }
int rn_debug_stream_live(rn_ctx *ctx, long long out[4]) { RN_GUARD(ctx); return ctx->impl->stream_live(out); }
int rn_debug_stream_units(rn_ctx *ctx, long long out[3]) { RN_GUARD(ctx); return ctx->impl->stream_units(out); }
int rn_debug_stream_product(rn_ctx *ctx, int pair, double *my, double *my2, double *myB) { RN_GUARD(ctx); return ctx->impl->stream_product(pair, my, my2, myB); }
int rn_debug_slab_product(rn_ctx *ctx, const rn_slab_product_args *args, int *info) { RN_GUARD(ctx); return ctx->impl->slab_product(args, info); }
int rn_debug_dual_update(rn_ctx *ctx, const rn_dual_update_args *args, double info[RN_DUAL_INFO_COUNT]) { RN_GUARD(ctx); return ctx->impl->dual_update_alone(args, info); }
int rn_debug_restart_test(rn_ctx *ctx, double out[3]) { RN_GUARD(ctx); return ctx->impl->debug_restart_test(out); }
int rn_debug_peer_seq(rn_ctx *ctx, unsigned int seq) { RN_GUARD(ctx); return ctx->impl->debug_peer_seq(seq); }
int rn_guard_report(long out[2]) { if (!out) return RN_E_ARG; out[0] = rn::g_guardContexts.load(); out[1] = rn::g_guardBadBytes.load(); return RN_OK; }
int rn_peer_inbox_create(rn_ctx *ctx, void *ipcHandle64) { RN_GUARD(ctx); return ctx->impl->peer_inbox_create(ipcHandle64); }
int rn_peer_inbox_connect(rn_ctx *ctx, const void *ipcHandles, int nranks) { RN_GUARD(ctx); return ctx->impl->peer_inbox_connect(ipcHandles, nranks); }
int rn_debug_peer_inbox_connect_local(rn_ctx **ctxs, int nranks) {
    if (!ctxs || nranks < 2 || nranks > rn::PEER_MAX) return RN_E_ARG;
    std::vector<rn::CtxBase *> impls(nranks);
    for (int r = 0; r < nranks; r++) { if (!ctxs[r] || !ctxs[r]->impl) return RN_E_ARG; impls[r] = ctxs[r]->impl; }
    for (int r = 0; r < nranks; r++) if (int rc = impls[r]->peer_inbox_connect_local(impls.data(), nranks)) return rc;
    return RN_OK;
}
int rn_set_exchange_transport(rn_ctx *ctx, int transport) { RN_GUARD(ctx); return ctx->impl->set_exchange_transport(transport); }
int rn_exchange_autotune(rn_ctx *ctx, int iterations, double info[8]) { RN_GUARD(ctx); return ctx->impl->exchange_autotune_api(iterations, info); }
int rn_set_fused_walk_dual(rn_ctx *ctx, int on) { RN_GUARD(ctx); return ctx->impl->set_fused_walk_dual(on); }
int rn_fbe_counters(rn_ctx *ctx, long out[4]) { RN_GUARD(ctx); return ctx->impl->fbe_counters(out); }
int rn_guard_check(rn_ctx *ctx, long *badBytes) { RN_GUARD(ctx); return ctx->impl->guard_check(badBytes); }
int rn_device_memory_info(rn_ctx *ctx, size_t info[4]) { RN_GUARD(ctx); return ctx->impl->memory_info(info); }
int rn_reserve_iterations(rn_ctx *ctx, int maxIterations) { RN_GUARD(ctx); return ctx->impl->reserve_iterations(maxIterations); }
int rn_profile_read_collective(rn_ctx *ctx, double *ms, long *launches) { RN_GUARD(ctx); return ctx->impl->profile_read_collective(ms, launches); }

}  // extern "C"

#ifdef RN_KTIMING
// debug builds only (not part of include/rapidnet.h): phase stamps of the instrumented kernels, 8 workgroups x 16 slots
extern "C" int rn_debug_ktiming(unsigned long long *out128) {
    return hipMemcpyFromSymbol(out128, HIP_SYMBOL(rn::g_ktiming), sizeof(unsigned long long) * 128) == hipSuccess ? 0 : 1;
}
#endif
