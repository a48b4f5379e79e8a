// k_misc.hpp -- streaming probes, the factor step and the affine terms on the device, small utility kernels
// (part of the kernel sources of librapidnet_hip.so; kernels.hpp includes every family header, the translation units k_*.hip instantiate them)
#pragma once
#include "common.hpp"
#include "k_plan.hpp"   // the plan report's kernel: instantiated in k_misc.hip with this family

namespace rn {

// ------------------------------------------------------------------------------------------------------
// HBM ceiling probes for bench.py (rn_measure_hbm): what kernels that do nothing but stream reach on THIS box -- the practical
// denominator next to the 8 TB/s spec.  16 B per lane per load, non-temporal, flat: the whole grid sweeps one region, thread-interleaved.
// (The probes in the solver's access shapes -- chunk per workgroup, lockstep pieces -- live in tools/probes/probe_stream.hip.)
// One kernel, two loops: dst == nullptr is the read-only probe, otherwise the copy (the branch is outside the loops and uniform over the grid).
template <int PLAIN = 0>   // (a template so that one translation unit owns its code: instantiations/*.inc)
__global__ void __launch_bounds__(256) k_bw_probe(const nat_d2 *src, nat_d2 *dst, long long n, double *sink) {
    if (dst) {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
            __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);   // non-temporal both ways: the fastest copy variant of probe_stream.hip
        return;
    }
    double acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const nat_d2 v = __builtin_nontemporal_load(src + i);
        acc += v[0] + v[1];
    }
    if (acc == 1.2345e-300) sink[blockIdx.x & 65535] = acc;   // keeps the loads alive without a store stream
}

// ------------------------------------------------------------------------------------------------------
// Factor step on the device (Engine::factorStep Engine.cu:671-774 + preconditioning Utilities.cu:33-58,
// 360-405): expands the per-node blocks from the shared factors computed on the host in fp64,
//   Phi_i(:,c) = -T1(:,j) d_c / (2 sqrt p_i),  D_i(:,c)    = Bbt(:,j) sqrt(p_i) d_c     c = xi column of tank j
//   Psi_i(:,c) = -T2(:,j) d_c / (2 sqrt p_i),  Ftil_i(:,c) = Lt(:,j)  sqrt(p_i) d_c     c = psi column of input j
// with T1 = Rinv Bbt, T2 = Rinv L'.  One workgroup per (node, column); pure streaming store.
// S: the element type the blocks are stored in (fp32 under fp64 iterates, rn_set_operator_storage: the formulas are evaluated in T and every
// entry is rounded once, to nearest, on its way out; a.LD and a.strideA count entries of S)
template <typename T, typename S = T>
struct ExpandArgs {
    TreeDev<T> tr;
    int nx, nu, nv, ny, LD, nodes;
    size_t strideA;
    const T *T1, *T2, *Bbt, *Lt;
    S *A;
    // scaled bounds in y order
    int skipBlocks;       // structured operator mode: only the scaled bounds are produced
    const T *blo, *bhi;   // [rows][ny] unscaled: xmin|xsafe|umin and xmax|+BIG|umax
    int bStrideStage, bStrideNode;   // the row of a node (rn_set_bounds): stage * bStrideStage + node * bStrideNode, in elements
    T *lo, *hi;           // [node][ny]
};
template <typename T, typename S = T>
__global__ void k_expand_operators(ExpandArgs<T, S> a) {
    const int node = blockIdx.x;
    const int stage = a.tr.stageOf[node];
    const T sp = a.tr.sqrtp[node];
    const T *dy = a.tr.dy + (size_t)stage * a.ny;
    for (int c = blockIdx.y; c < a.ny; c += gridDim.y) {
        const T d = dy[c];
        const T s1 = (T)(-0.5) * d / sp, s2 = sp * d;
        const T *m1, *m2;
        if (c < 2 * a.nx) { const int j = c % a.nx; m1 = a.T1 + (size_t)j * a.nv; m2 = a.Bbt + (size_t)j * a.nv; }
        else { const int j = c - 2 * a.nx; m1 = a.T2 + (size_t)j * a.nv; m2 = a.Lt + (size_t)j * a.nv; }
        if (!a.skipBlocks) {
            S *col = a.A + (size_t)node * a.strideA + (size_t)c * a.LD;
            for (int r = threadIdx.x; r < a.LD; r += blockDim.x)
                col[r] = (S)(r < a.nv ? s1 * m1[r] : (r < 2 * a.nv ? s2 * m2[r - a.nv] : (T)0));
        }
        if (threadIdx.x == 0) {
            // bound scaling: preconditionConstraintX/U.  "+BIG" stays +BIG (no upper bound on the safety half)
            const T k = sp * d;
            const int bc = stage * a.bStrideStage + node * a.bStrideNode + c;
            a.lo[(size_t)node * a.ny + c] = k * a.blo[bc];
            const bool safety = (c >= a.nx && c < 2 * a.nx);
            a.hi[(size_t)node * a.ny + c] = safety ? a.bhi[bc] : k * a.bhi[bc];
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// All per-node blocks at once, to or from the caller's four arrays in the reference's layout (rn_set_operators / rn_get_operators and their
// _device forms; Engine.cuh getMatPhi() ... getMatF(): Phi, D [node][2nx columns][nv], Psi, F [node][nu columns][nv], dense, ld = nv).  The
// block layout is k_expand_operators' above: column c of a node at A + node * strideA + c * LD, rows [0, nv) Phi | Psi, [nv, 2nv) D | Ftil,
// [2nv, LD) padding.
// TO_BLOCKS: a lane owns one 16-byte slot of a block column (2 doubles or 4 floats; LD is whole slots), gathers its entries from the one or
// two arrays they come from -- a slot straddles the Phi / D boundary or reaches into the padding whenever nv is no multiple of the slot
// width --, converts each with a plain cast (the only rounding: fp64 -> fp32 to nearest, what Ctx::upload_block does on the host) and stores
// the slot once.  Where a slot holds entries that are not the caller's -- padding rows, rows of an array that was not given (nullptr) -- the
// lane reads the slot first and replaces only the given ones; a slot with none is not touched.  Every slot has one owner: no races, and
// neither the padding rows nor the tail of strideA change.  The other direction reads slots and scatters entry by entry.
// Consecutive lanes own consecutive slots of a node's block (columns are adjacent), so the block side is one flat 16-B-per-lane stream and
// the caller's side is contiguous per array; it is read 16 B wide where a slot's entries lie in one array at a 16-byte boundary, entry by
// entry otherwise (still coalesced).  Non-temporal both ways, as the copy loop of k_bw_probe.  Launch: blockIdx.x strides the slots of one node, blockIdx.y
// the nodes -- numCUs * 4 workgroups in all, the shape rn_measure_hbm found best for a read + write stream.
// The element types and the direction arrive as flags and not as template parameters: the four (caller, stored) pairs in two directions
// would be eight kernels; the branches are uniform over the grid.
struct PackOpsArgs {
    void *A;              // the blocks, doubles or floats (storedF64), first node of the range
    size_t strideA;       // in stored entries
    void *op[4];          // caller's phi, psi, D, F: doubles or floats (callerF64), first node of the range; nullptr: not given
    int LD, nv, nx2, nu, nodes;
    int callerF64, storedF64;
    int toBlocks;         // 1: caller's arrays -> blocks (set), 0: blocks -> caller's arrays (get)
};
constexpr int PACK_THREADS = 256;
typedef float nat_f2 __attribute__((ext_vector_type(2)));
// the N entries of a slot that lie behind one another at p, which is aligned to min(16, N * sizeof(C)) bytes
__device__ __forceinline__ nat_d2 pack_load_run(const double *p, nat_d2) { return __builtin_nontemporal_load(reinterpret_cast<const nat_d2 *>(p)); }
__device__ __forceinline__ nat_f4 pack_load_run(const float *p, nat_f4) { return __builtin_nontemporal_load(reinterpret_cast<const nat_f4 *>(p)); }
__device__ __forceinline__ nat_f4 pack_load_run(const double *p, nat_f4) {
    const nat_d2 a = __builtin_nontemporal_load(reinterpret_cast<const nat_d2 *>(p)), b = __builtin_nontemporal_load(reinterpret_cast<const nat_d2 *>(p) + 1);
    nat_f4 v; v[0] = (float)a[0]; v[1] = (float)a[1]; v[2] = (float)b[0]; v[3] = (float)b[1];
    return v;
}
__device__ __forceinline__ nat_d2 pack_load_run(const float *p, nat_d2) {
    const nat_f2 a = __builtin_nontemporal_load(reinterpret_cast<const nat_f2 *>(p));
    nat_d2 v; v[0] = (double)a[0]; v[1] = (double)a[1];
    return v;
}
template <typename C, typename S, bool TO_BLOCKS>
__device__ __forceinline__ void pack_operators_body(const PackOpsArgs &a) {
    typedef typename Slot<S>::type slot_t;
    constexpr int VPS = Slot<S>::N;
    constexpr unsigned RUN_ALIGN = VPS * sizeof(C) < 16 ? VPS * sizeof(C) : 16;
    const int nv = a.nv, spc = a.LD / VPS, perNode = (a.nx2 + a.nu) * spc;
    C *const phi = static_cast<C *>(a.op[0]), *const psi = static_cast<C *>(a.op[1]), *const D = static_cast<C *>(a.op[2]), *const F = static_cast<C *>(a.op[3]);
    for (int node = blockIdx.y; node < a.nodes; node += gridDim.y) {
        S *const blk = static_cast<S *>(a.A) + (size_t)node * a.strideA;
        for (int j = blockIdx.x * PACK_THREADS + threadIdx.x; j < perNode; j += gridDim.x * PACK_THREADS) {
            const int c = j / spc, r0 = (j - c * spc) * VPS;
            const bool xi = c < a.nx2;
            C *const top = xi ? phi : psi, *const bot = xi ? D : F;
            if (!top && !bot) continue;
            const size_t off = ((size_t)node * (xi ? a.nx2 : a.nu) + (xi ? c : c - a.nx2)) * nv;   // this column in either array
            slot_t *const slot = reinterpret_cast<slot_t *>(blk + (size_t)c * a.LD + r0);
            if (TO_BLOCKS) {
                bool all = true, any = false;
#pragma unroll
                for (int k = 0; k < VPS; k++) {
                    const int r = r0 + k;
                    const bool given = r < nv ? top != nullptr : (r < 2 * nv && bot != nullptr);
                    all = all && given; any = any || given;
                }
                if (!any) continue;
                const C *run = nullptr;   // the slot's entries lie in one array
                if (r0 + VPS <= nv) run = top + off + r0;
                else if (r0 >= nv && r0 + VPS <= 2 * nv) run = bot + off + (r0 - nv);
                slot_t v;
                if (run && (reinterpret_cast<uintptr_t>(run) & (RUN_ALIGN - 1)) == 0) v = pack_load_run(run, slot_t());
                else {
                    if (!all) v = __builtin_nontemporal_load(slot);
#pragma unroll
                    for (int k = 0; k < VPS; k++) {
                        const int r = r0 + k;
                        if (r < nv) { if (top) v[k] = (S)__builtin_nontemporal_load(top + off + r); }
                        else if (r < 2 * nv) { if (bot) v[k] = (S)__builtin_nontemporal_load(bot + off + (r - nv)); }
                    }
                }
                __builtin_nontemporal_store(v, slot);
            } else {
                if (r0 >= 2 * nv) continue;
                const slot_t v = __builtin_nontemporal_load(slot);
#pragma unroll
                for (int k = 0; k < VPS; k++) {
                    const int r = r0 + k;
                    if (r < nv) { if (top) __builtin_nontemporal_store((C)v[k], top + off + r); }
                    else if (r < 2 * nv) { if (bot) __builtin_nontemporal_store((C)v[k], bot + off + (r - nv)); }
                }
            }
        }
    }
}
template <typename C, typename S>
__device__ __forceinline__ void pack_operators_dir(const PackOpsArgs &a) {
    if (a.toBlocks) pack_operators_body<C, S, true>(a); else pack_operators_body<C, S, false>(a);
}
template <int PLAIN = 0>   // (a template so that one translation unit owns its code: instantiations/*.inc)
__global__ void __launch_bounds__(PACK_THREADS) k_pack_operators(PackOpsArgs a) {
    if (a.callerF64) { if (a.storedF64) pack_operators_dir<double, double>(a); else pack_operators_dir<double, float>(a); }
    else { if (a.storedF64) pack_operators_dir<float, double>(a); else pack_operators_dir<float, float>(a); }
}

// ------------------------------------------------------------------------------------------------------
// Scenario probabilities and tree errors replaced in place (rn_set_tree_data / rn_set_tree_data_device; ScenarioTree.cuh:92-154, devTreeProb
// Engine.cu:263-286, the errors of Engine.cu:1205,1228).  The caller's arrays hold elements of type Src (float or double: the host form stages
// doubles) and, on a context made by rn_create_sharded, the rows of the FULL tree: a local node reads row gmap[node].  Written in the context's
// type: prob, sqrt(prob) -- the square root taken in double, correctly rounded, then rounded to T: the bits rn_create uploads --, errD, errP;
// a pointer that is null leaves its array alone.  Probabilities that are not positive and finite are counted, one plain store per workgroup
// into bad[blockIdx.x] (the host adds the words behind a synchronisation it makes anyway); the words are only written when prob is given.
// On a multi-rank shard the children moments of the cut parents (rn_set_cut_children_moments) follow from the same arrays: one thread per
// (parent, component), children in ascending order, in double, product and sum rounded separately -- the bits of partition.hpp's host loop --
// then converted to T.  The array that was not given comes from the full-tree values of the cut stage the context retains (fullP, fullE),
// which a given array replaces.  A thread of component t < nd reads fullP only when prob is absent and the thread of component nd writes it
// only when prob is present; fullE[.., t] belongs to the thread of component t: no races.
// The element types arrive as flags and not as template parameters, as in k_pack_operators: the four (context, caller) pairs would be four
// kernels; the branch is uniform over the grid.
struct TreeDataArgs {
    const void *prob, *errD, *errP;   // [rows], [rows][nd], [rows][nu] of Src (callerF64); nullptr: not given
    const int *gmap;                  // [nodes] row of every local node; nullptr: identity
    int nodes, nd, nu;
    int ctxF64, callerF64;            // T, Src: doubles (1) or floats (0)
    void *dprob, *dsqrtp, *derrD, *derrP;   // of T
    double *prob64;                   // fp32 contexts: the probabilities once more as doubles (rn_get_tree_data, the host copy); else nullptr
    int *bad;                         // [gridDim.x]
    int nPar, cutFirst;               // cut parents (0: no moments); full-tree index of the first node of the cut stage
    const int *cutC0, *cutNc;         // [nPar] full-tree index of a cut parent's first child, its number of children
    double *fullP, *fullE;            // [cut-stage nodes], [cut-stage nodes][nd]
    void *momE, *momP;                // of T: [nPar][nd], [nPar]
    // Box and safety bounds replaced in place (rn_set_bounds / rn_set_bounds_device; Engine.cuh:294-314 getSysXmin() ... getSysUmax(), Engine.cu
    // preconditionConstraintX/U): the caller's physical values, [bRows][nx] (xmin, xmax, xsafe) and [bRows][nu] (umin, umax) of Src, nullptr: not
    // given.  A node reads row stage * bRowStage + node * bRowNode ((0,0) shared, (1,0) per stage, (0,1) per node; local nodes: no gmap).  Written
    // in T: the unscaled tables blo / bhi [bRows][ny] in y order (xmin|xsafe|umin, xmax|+BIG|umax; the +BIG columns are always written), the
    // scaled lo / hi [nodes][ny] of every node -- (sqrt(p_i) d_c) v, k_expand_operators' expression and rounding, straight from the caller's value
    // and not through the table, which other workgroups are still writing -- and, where they exist, the node-major copies rn_device_pointer hands
    // out.  An array that was not given leaves its columns of every output alone.  bRows == 0: no bounds in this launch.
    const void *bnd[5];               // xmin, xmax, xsafe, umin, umax
    int bRows, bRowStage, bRowNode, nx, ny;
    const int *stageOf;               // [nodes]
    const void *sqrtpIn, *dy;         // of T: [nodes], [N][ny]
    void *blo, *bhi, *lo, *hi;        // of T
    void *bndCopy[5];                 // of T: [nodes][nx | nu] in the order of bnd, or all nullptr
};
constexpr int TREE_THREADS = 256, TREE_MAX_BLOCKS = 64, BOUNDS_MAX_BLOCKS = 1024;
__device__ __forceinline__ void bounds_big(double &v) { v = __longlong_as_double(0x7F7F7F7F7F7F7F7FLL); }   // bytes 0x7F (Engine.cu:454-455)
__device__ __forceinline__ void bounds_big(float &v) { v = __int_as_float(0x7F7F7F7F); }
// column c of the y order: the caller's arrays that hold its lower / upper bound (hi == nullptr in the safety half: +BIG, or not given), the
// node-major copies they go to, the index inside a row and the row length (branches, not indexed pointer arrays: those would live in scratch)
template <typename T, typename Src>
struct BoundsCol { const Src *lo, *hi; T *copyLo, *copyHi; int t, dim; bool safety; };
template <typename T, typename Src>
__device__ __forceinline__ BoundsCol<T, Src> bounds_column(const TreeDataArgs &a, int c) {
    BoundsCol<T, Src> k;
    if (c < a.nx) {
        k.lo = static_cast<const Src *>(a.bnd[0]); k.hi = static_cast<const Src *>(a.bnd[1]);
        k.copyLo = static_cast<T *>(a.bndCopy[0]); k.copyHi = static_cast<T *>(a.bndCopy[1]); k.t = c; k.dim = a.nx; k.safety = false;
    } else if (c < 2 * a.nx) {
        k.lo = static_cast<const Src *>(a.bnd[2]); k.hi = nullptr;
        k.copyLo = static_cast<T *>(a.bndCopy[2]); k.copyHi = nullptr; k.t = c - a.nx; k.dim = a.nx; k.safety = true;
    } else {
        k.lo = static_cast<const Src *>(a.bnd[3]); k.hi = static_cast<const Src *>(a.bnd[4]);
        k.copyLo = static_cast<T *>(a.bndCopy[3]); k.copyHi = static_cast<T *>(a.bndCopy[4]); k.t = c - 2 * a.nx; k.dim = a.nu; k.safety = false;
    }
    return k;
}
template <typename T, typename Src>
__device__ __forceinline__ void bounds_body(const TreeDataArgs &a) {
    T *const blo = static_cast<T *>(a.blo), *const bhi = static_cast<T *>(a.bhi), *const lo = static_cast<T *>(a.lo), *const hi = static_cast<T *>(a.hi);
    const T *const sqrtp = static_cast<const T *>(a.sqrtpIn), *const dy = static_cast<const T *>(a.dy);
    const int ny = a.ny;
    const long long stride = (long long)gridDim.x * TREE_THREADS, gid = (long long)blockIdx.x * TREE_THREADS + threadIdx.x;
    T big; bounds_big(big);
    for (long long i = gid; i < (long long)a.bRows * ny; i += stride) {      // the unscaled tables
        const int row = (int)(i / ny), c = (int)(i - (long long)row * ny);
        const BoundsCol<T, Src> k = bounds_column<T, Src>(a, c);
        if (k.lo) blo[i] = (T)k.lo[(size_t)row * k.dim + k.t];
        if (k.safety) bhi[i] = big;
        else if (k.hi) bhi[i] = (T)k.hi[(size_t)row * k.dim + k.t];
    }
    for (long long i = gid; i < (long long)a.nodes * ny; i += stride) {      // the scaled bounds of every node
        const int node = (int)(i / ny), c = (int)(i - (long long)node * ny);
        const int stage = a.stageOf[node];
        const size_t row = (size_t)stage * a.bRowStage + (size_t)node * a.bRowNode;
        const BoundsCol<T, Src> k = bounds_column<T, Src>(a, c);
        const T f = sqrtp[node] * dy[(size_t)stage * ny + c];
        if (k.lo) {
            const T v = f * (T)k.lo[row * k.dim + k.t];
            lo[i] = v;
            if (k.copyLo) k.copyLo[(size_t)node * k.dim + k.t] = v;
        }
        if (k.hi) {
            const T v = f * (T)k.hi[row * k.dim + k.t];
            hi[i] = v;
            if (k.copyHi) k.copyHi[(size_t)node * k.dim + k.t] = v;
        }
    }
}
template <typename T, typename Src>
__device__ __forceinline__ void tree_data_body(const TreeDataArgs &a) {
    T *const dprob = static_cast<T *>(a.dprob), *const dsqrtp = static_cast<T *>(a.dsqrtp), *const derrD = static_cast<T *>(a.derrD), *const derrP = static_cast<T *>(a.derrP);
    T *const momE = static_cast<T *>(a.momE), *const momP = static_cast<T *>(a.momP);
    const Src *const prob = static_cast<const Src *>(a.prob), *const errD = static_cast<const Src *>(a.errD), *const errP = static_cast<const Src *>(a.errP);
    const int W = max(max(a.nd, a.nu), 1);
    const long long total = (long long)a.nodes * W;
    if (a.bRows > 0) bounds_body<T, Src>(a);
    if (!prob && !errD && !errP) return;      // (a launch of rn_set_bounds)
    int bad = 0;
    for (long long base = (long long)blockIdx.x * TREE_THREADS; base < total; base += (long long)gridDim.x * TREE_THREADS) {   // (uniform trip count: the barrier below)
        const long long i = base + threadIdx.x;
        bool isBad = false;
        if (i < total) {
            const int node = (int)(i / W), t = (int)(i - (long long)node * W);
            const size_t row = a.gmap ? (size_t)a.gmap[node] : (size_t)node;
            if (t == 0 && prob) {
                const double p = (double)prob[row];
                isBad = !(p > 0.0 && p < __builtin_huge_val());
                dprob[node] = (T)p;
                dsqrtp[node] = (T)__dsqrt_rn(p);
                if (a.prob64) a.prob64[node] = p;
            }
            if (errD && t < a.nd) derrD[(size_t)node * a.nd + t] = (T)errD[row * a.nd + t];
            if (errP && t < a.nu) derrP[(size_t)node * a.nu + t] = (T)errP[row * a.nu + t];
        }
        bad += __syncthreads_count(isBad);
    }
    if (prob && threadIdx.x == 0) a.bad[blockIdx.x] = bad;
    if (a.nPar <= 0 || (!prob && !errD)) return;
    const int C = a.nd + 1;
    for (int i = blockIdx.x * TREE_THREADS + threadIdx.x; i < a.nPar * C; i += gridDim.x * TREE_THREADS) {
        const int j = i / C, t = i - j * C, c0 = a.cutC0[j], nc = a.cutNc[j];
        double s = 0.0;
        for (int c = c0; c < c0 + nc; c++) {
#pragma clang fp contract(off)
            const size_t k = (size_t)(c - a.cutFirst);
            const double pc = prob ? (double)prob[c] : a.fullP[k];
            if (t < a.nd) {
                const double e = errD ? (double)errD[(size_t)c * a.nd + t] : a.fullE[k * a.nd + t];
                const double pe = pc * e;
                s = s + pe;
                if (errD) a.fullE[k * a.nd + t] = e;
            } else {
                s = s + pc;
                if (prob) a.fullP[k] = pc;
            }
        }
        if (t < a.nd) momE[(size_t)j * a.nd + t] = (T)s; else momP[j] = (T)s;
    }
}
template <int PLAIN = 0>   // (a template so that one translation unit owns its code: instantiations/*.inc)
__global__ void __launch_bounds__(TREE_THREADS) k_tree_data(TreeDataArgs a) {
    if (a.ctxF64) { if (a.callerF64) tree_data_body<double, double>(a); else tree_data_body<double, float>(a); }
    else { if (a.callerF64) tree_data_body<float, double>(a); else tree_data_body<float, float>(a); }
}

// ------------------------------------------------------------------------------------------------------
// Per-control-step affine terms (Engine::eliminateInputDistubanceCoupling Engine.cu:1147-1298), two kernels,
// one workgroup per node:
//   k_affine_demand: d_i = errD_i + dhat[stage]; e_i = Gd d_i; uhat_i = Lhat d_i;
//                    alpha_i = w_e (errP_i + ahat[stage] + alpha1)
//   k_affine_beta:   zeta_i = p_i (uhat_i - uhat_anc) - sum_c p_c (uhat_c - uhat_i)   (Utilities.cu:69-131)
//                    beta_i = 2 (W L)' zeta_i + p_i L' alpha_i
template <typename T>
struct AffineArgs {
    TreeDev<T> tr;
    int nx, nu, nv, nd;
    const T *Gd, *Lhat, *WLt, *Lt;      // WLt = (W L)' (nv x nu), Lt = L' (nv x nu)
    const T *errD, *errP, *dhat, *ahat, *alpha1, *prevUhat;
    T wEco; int useErrD, useErrP;
    T *e, *uhat, *alpha, *beta;
    // multi-GPU: children moments of the cut parents (whole tree): momE [parents][nd] = sum_c p_c errD_c, momP = sum_c p_c
    const T *momE, *momP; int cutStage;
};
constexpr int AFF_THREADS = 128;
template <typename T>
__global__ void __launch_bounds__(AFF_THREADS) k_affine_demand(AffineArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *sh_d = reinterpret_cast<T *>(smem_raw);                 // nd
    T *sh_o = sh_d + ((a.nd + 3) & ~3);                        // max(nx, nu)
    T *sh_scr = sh_o + ((max(a.nx, a.nu) + 3) & ~3);
    const int node = blockIdx.x, tid = threadIdx.x;
    const int stage = a.tr.stageOf[node];
    for (int t = tid; t < a.nd; t += AFF_THREADS)
        sh_d[t] = (a.useErrD ? a.errD[(size_t)node * a.nd + t] : (T)0) + a.dhat[(size_t)stage * a.nd + t];
    __syncthreads();
    block_gemv_shared<T>(a.Gd, a.nx, a.nd, sh_d, sh_o, sh_scr, AFF_THREADS);
    for (int t = tid; t < a.nx; t += AFF_THREADS) a.e[(size_t)node * a.nx + t] = sh_o[t];
    __syncthreads();
    block_gemv_shared<T>(a.Lhat, a.nu, a.nd, sh_d, sh_o, sh_scr, AFF_THREADS);
    for (int t = tid; t < a.nu; t += AFF_THREADS) {
        a.uhat[(size_t)node * a.nu + t] = sh_o[t];
        const T ep = a.useErrP ? a.errP[(size_t)node * a.nu + t] : (T)0;
        a.alpha[(size_t)node * a.nu + t] = a.wEco * (ep + (a.ahat[(size_t)stage * a.nu + t] + a.alpha1[t]));
    }
}
template <typename T>
__global__ void __launch_bounds__(AFF_THREADS) k_affine_beta(AffineArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T *sh_z = reinterpret_cast<T *>(smem_raw);                 // nu  zeta
    T *sh_a = sh_z + ((a.nu + 3) & ~3);                        // nu  alpha
    T *sh_o = sh_a + ((a.nu + 3) & ~3);                        // max(nv, nu)
    T *sh_o2 = sh_o + ((max(a.nv, a.nu) + 3) & ~3);            // nv
    T *sh_d = sh_o2 + ((a.nv + 3) & ~3);                       // nd
    T *sh_scr = sh_d + ((a.nd + 3) & ~3);
    const int node = blockIdx.x, tid = threadIdx.x, nu = a.nu;
    const int par = a.tr.parent[node];
    const int c0 = a.tr.childStart[node], nc = a.tr.childCount[node];
    const T p = a.tr.prob[node];
    const int stage = a.tr.stageOf[node];
    const bool presummed = a.momE != nullptr && stage == a.cutStage - 1;
    if (presummed) {   // sum_c p_c uhat_c = Lhat (E_i + P_i dhat[stage+1]) over ALL children, local or not
        const int pos = node - a.tr.stageCum[stage];
        const T P = a.momP[pos];
        for (int t = tid; t < a.nd; t += AFF_THREADS)
            sh_d[t] = (a.useErrD ? a.momE[(size_t)pos * a.nd + t] : (T)0) + P * a.dhat[(size_t)(stage + 1) * a.nd + t];
        __syncthreads();
        block_gemv_shared<T>(a.Lhat, nu, a.nd, sh_d, sh_o, sh_scr, AFF_THREADS);
    }
    for (int t = tid; t < nu; t += AFF_THREADS) {
        const T ui = a.uhat[(size_t)node * nu + t];
        const T ua = par < 0 ? a.prevUhat[t] : a.uhat[(size_t)par * nu + t];
        T z = p * (ui - ua);
        if (presummed) z -= sh_o[t] - a.momP[node - a.tr.stageCum[stage]] * ui;
        else for (int c = 0; c < nc; c++) z -= a.tr.prob[c0 + c] * (a.uhat[(size_t)(c0 + c) * nu + t] - ui);
        sh_z[t] = z;
        sh_a[t] = a.alpha[(size_t)node * nu + t];
    }
    __syncthreads();
    block_gemv_shared<T>(a.WLt, a.nv, nu, sh_z, sh_o, sh_scr, AFF_THREADS);
    block_gemv_shared<T>(a.Lt, a.nv, nu, sh_a, sh_o2, sh_scr, AFF_THREADS);
    for (int t = tid; t < a.nv; t += AFF_THREADS) a.beta[(size_t)node * a.nv + t] = (T)2 * sh_o[t] + p * sh_o2[t];
}

// small utilities ------------------------------------------------------------------------------------
// (one workgroup each, once per control step; the columns are requested eight at a time -- one at a time the loop was a chain of
//  `cols` dependent round trips, 35-50 us for a 63 x 114 matrix -- and added in the same order as before)
// k_bw0: the element type arrives as a flag and not as a template parameter (one kernel instead of two, as k_clamp_vec below: one workgroup once
// per control step); the products and the order of the sums are the typed ones, bit for bit
template <typename T>
__device__ __forceinline__ void bw0_body(const void *B_, int nx, int nu, const void *prevU_, const void *prevUhat_, void *bw0_) {   // bw0 = B (prevU - prevUhat)
    const T *__restrict__ B = static_cast<const T *>(B_), *__restrict__ prevU = static_cast<const T *>(prevU_), *__restrict__ prevUhat = static_cast<const T *>(prevUhat_);
    T *__restrict__ bw0 = static_cast<T *>(bw0_);
    for (int r = threadIdx.x; r < nx; r += blockDim.x) {
        T s = 0;
        for (int j0 = 0; j0 < nu; j0 += 8) {
            T m[8], d[8];
#pragma unroll
            for (int i = 0; i < 8; i++) { const int j = j0 + i < nu ? j0 + i : nu - 1; m[i] = B[r + (size_t)j * nx]; d[i] = prevU[j] - prevUhat[j]; }
#pragma unroll
            for (int i = 0; i < 8; i++) if (j0 + i < nu) s += m[i] * d[i];
        }
        bw0[r] = s;
    }
}
template <int PLAIN = 0>   // (a template so that one translation unit owns its code: instantiations/*.inc)
__global__ void k_bw0(const void *B, int nx, int nu, const void *prevU, const void *prevUhat, void *bw0, int f64) {
    if (f64) bw0_body<double>(B, nx, nu, prevU, prevUhat, bw0); else bw0_body<float>(B, nx, nu, prevU, prevUhat, bw0);
}
template <typename T>
__global__ void k_gemv_small(const T *__restrict__ M, int rows, int cols, const T *__restrict__ x, T *__restrict__ y) {   // y = M x, one block
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        T s = 0;
        for (int j0 = 0; j0 < cols; j0 += 8) {
            T m[8], v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) { const int j = j0 + i < cols ? j0 + i : cols - 1; m[i] = M[r + (size_t)j * rows]; v[i] = x[j]; }
#pragma unroll
            for (int i = 0; i < 8; i++) if (j0 + i < cols) s += m[i] * v[i];
        }
        y[r] = s;
    }
}
// y-layout <-> reference layout ([node][2nx] xi arrays and [node][nu] psi arrays)
template <typename T>
__global__ void k_pack(T *y, T *part, int ny, int off, int dim, long long nodes, int toY) {
    const long long n = nodes * dim;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long node = i / dim; const int t = (int)(i % dim);
        if (toY) y[node * ny + off + t] = part[i]; else part[i] = y[node * ny + off + t];
    }
}
// projectionBox<<<1,nu>>> SmpcController.cu:1649.  The element type arrives as a flag and not as a template parameter (one kernel instead of
// two, as k_tree_data); the comparisons and the stored value are the typed ones, bit for bit
template <typename T>
__device__ __forceinline__ void clamp_vec_body(void *u_, const void *lo_, const void *hi_, int n) {
    T *u = static_cast<T *>(u_);
    const T *lo = static_cast<const T *>(lo_), *hi = static_cast<const T *>(hi_);
    for (int i = threadIdx.x; i < n; i += blockDim.x) { const T v = u[i]; u[i] = v < lo[i] ? lo[i] : (v > hi[i] ? hi[i] : v); }
}
template <int PLAIN = 0>   // (a template so that one translation unit owns its code: instantiations/*.inc)
__global__ void k_clamp_vec(void *u, const void *lo, const void *hi, int n, int f64) {
    if (f64) clamp_vec_body<double>(u, lo, hi, n); else clamp_vec_body<float>(u, lo, hi, n);
}


// Structured mode, composite operator (k_gemm_comp): the forward walk's affine terms join the product's constant operand, so that the walk's running
// sums of [L v_i ; B L v_i] are u_i and x_i - x_anc themselves and the walk requests neither uhat nor eb (SweepArgs::lin bit 2):
//   lvconst_i[0 .. nu) += uhat_i - uhat_anc   (root: - prevUhat) ;   lvconst_i[nu .. nu + nx) += eb_i - eb_anc   (root: eb_0)
// The element type arrives as a flag and not as a template parameter (one kernel instead of two, as k_clamp_vec: the launch is once per
// control step); the arithmetic is the typed one, bit for bit
template <typename T>
__device__ __forceinline__ void fold_affine_body(void *lvconst_, const void *uhat_, const void *eb_, const void *prevUhat_, const int *parent, int nodes, int nu, int nx) {
    T *lvconst = static_cast<T *>(lvconst_);
    const T *uhat = static_cast<const T *>(uhat_), *eb = static_cast<const T *>(eb_), *prevUhat = static_cast<const T *>(prevUhat_);
    const int w = nu + nx;
    const long long n = (long long)nodes * w;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int node = (int)(i / w), t = (int)(i % w), par = parent[node];
        T add;
        if (t < nu) add = uhat[(size_t)node * nu + t] - (par < 0 ? prevUhat[t] : uhat[(size_t)par * nu + t]);
        else { const int j = t - nu; add = eb[(size_t)node * nx + j] - (par < 0 ? (T)0 : eb[(size_t)par * nx + j]); }
        lvconst[i] += add;
    }
}
template <int PLAIN = 0>   // (a template so that one translation unit owns its code: instantiations/*.inc)
__global__ void k_fold_affine(void *lvconst, const void *uhat, const void *eb, const void *prevUhat, const int *parent, int nodes, int nu, int nx, int f64) {
    if (f64) fold_affine_body<double>(lvconst, uhat, eb, prevUhat, parent, nodes, nu, nx);
    else fold_affine_body<float>(lvconst, uhat, eb, prevUhat, parent, nodes, nu, nx);
}

}  // namespace rn
