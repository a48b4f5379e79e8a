/* rapidnet_debug.h -- TEST HOOKS of librapidnet_hip.so.  Not part of the drop-in boundary (include/rapidnet.h): nothing here replaces a
 * member of the reference; the parity tests use these entry points the way the reference's own tests reach into protected members
 * (TestSmpcController.cu:134-159).  A production caller has no use for them. */
#ifndef RAPIDNET_DEBUG_H_
#define RAPIDNET_DEBUG_H_

#include "rapidnet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* test hook for a caller's leak check (SmpcController.cu:1612-1623): the NEXT rn_control_action allocates `bytes` of device memory
 * that stay with the context */
int rn_debug_inject_allocation(rn_ctx *ctx, size_t bytes);

/* Test hooks for the sharded sweep: run rn_solve_step in two halves around the exchange -- phase 1 stops after the
 * cut parents' LOCAL children sums (solveSumChildren, Utilities.cu:168-201) are in the exchange buffer, phase 2 resumes from a
 * buffer the caller has summed over the shards (rn_debug_cut_buffer reads / writes it: cutParents * (nv + 2 nx) reals). */
int rn_debug_sweep_phase(rn_ctx *ctx, int phase);
int rn_debug_cut_buffer(rn_ctx *ctx, int write, double *host, size_t n);

/* An in-process stand-in for the communicator, so that the device-resident sharded path (checkpoint, dist^2 tail, verdict vote,
 * replay) can run with several ranks on a box where RCCL cannot (one GPU: "Duplicate GPU detected").
 * rn_debug_set_allreduce installs a callback that is called wherever the library would call ncclAllReduce(in place):
 * devBuf / count / isF64 / op describe the payload and the reduction, stream is the context's hipStream_t; it must return 0 after the
 * reduced values are (or are stream-ordered to be) in devBuf.  rn_debug_local_group_* is such a callback inside the library for
 * `nranks` contexts of ONE process, each driven by its own host thread: stream sync, barrier, every rank sums the payloads
 * in rank order (bitwise the same on all ranks), barrier.  A rank that does not arrive within 120 s
 * ($RAPIDNET_GROUP_TIMEOUT_S when the group is created) fails the others with RN_E_COMM instead of hanging them. */
typedef int (*rn_allreduce_fn)(void *user, void *devBuf, size_t count, int isF64, int op /* 0 = sum, 2 = max (ncclRedOp_t) */, void *stream);
int rn_debug_set_allreduce(rn_ctx *ctx, rn_allreduce_fn fn, void *user);
int rn_debug_local_group_create(int nranks, void **group);
int rn_debug_local_group_join(rn_ctx *ctx, void *group, int rank);
int rn_debug_local_group_destroy(void *group);

/* one-shot exchange: wires the inboxes (rn_peer_inbox_create) of `nranks` contexts of ONE process -- same address space, no IPC
 * handle needed -- contexts in rank order */
int rn_debug_peer_inbox_connect_local(rn_ctx **ctxs, int nranks);

/* one-shot exchange: sets the sequence number of the context's LAST exchange (the next one carries seq + 1; every rank must be given the
 * same value) -- lets a test walk the 32-bit tag across its wrap, where two values are skipped so that the parity which selects the
 * inbox buffer keeps alternating */
int rn_debug_peer_seq(rn_ctx *ctx, unsigned int seq);

/* test of the guard-mode detector itself (rn_guard_check): overwrites `nbytes` (1 .. 256) right behind the payload of the context's
 * first buffer */
int rn_debug_guard_poke(rn_ctx *ctx, int nbytes);

/* Launch-shape choices the library makes by problem size, forced from outside: the parity tests run the kernels that only large
 * trees take (three slabs per workgroup, double-buffered dual update, ...) on small ones, and the A/B tools time a shipped choice against
 * its alternative.  value = -1 gives the choice back to the library.  Before the factor step only: RN_E_STATE afterwards.  Every knob
 * selects between forms with IDENTICAL results (bitwise where the test of the knob says so); none changes what is computed. */
enum {
    RN_KNOB_DUAL_TRIPS = 0,        /* k_dual_stage: 16-byte vectors per thread (1 .. 64) */
    RN_KNOB_DUAL_PIPE = 1,         /* k_dual_stage: 1 = one vector at a time, 2 = double-buffered */
    RN_KNOB_VLV_WIDE = 2,          /* v / Lv products: slabs per workgroup of k_gemm_vlv_wide (2, 3; 0 / 1 = k_gemm_vlv) */
    RN_KNOB_SLAB_PIPE = 3,         /* slab products: 1 = the software-pipelined MFMA loop, 0 = the lean one */
    RN_KNOB_SLAB_FRAG = 4,         /* slab products: 0 = A operands from the column-major operators instead of the fragment-ordered copies */
    RN_KNOB_UNSCALED_WALK = 5,     /* 0 = the forward walk always applies the preconditioner itself (k_down_chain / k_dual_stage pair) */
    RN_KNOB_STREAM_TWO_PER_CU = 6, /* k_stream_gemv: 1 = the instantiation that leaves room for two workgroups per CU, 0 = the other */
    RN_KNOB_STREAM_SPLIT = 7,      /* k_stream_gemv: 0 = the last partial round is not split by columns */
    RN_KNOB_NAMA_PAIR = 8,         /* NAMA: 0 = its two Hessian sweeps one after the other instead of one pass over the operator blocks */
    RN_KNOB_LS_SEQUENTIAL = 9,     /* global FBE / NAMA: 1 = trial-by-trial line search instead of the batched candidates */
    RN_KNOB_VALUE_MFMA = 10,       /* global FBE / NAMA: 0 = the value's primal terms on the vector ALUs */
    RN_KNOB_TUNE_BIAS_US = 11,     /* rn_exchange_autotune, test of the selection: microseconds per iteration added to THIS rank's measured one-shot time */
    RN_KNOB_STRUCT_LINEAR = 12,    /* structured mode: 0 = the first product k_gemm_prep_m2 in front of the chain walks instead of the linear form (k_up_chain_lin); 2 = the linear form without the chain walk riding in the fused walk + dual update; 3 = the linear form with the subtree sums of beta walked and multiplied in every iteration instead of once per control step; 4 = that constant, but v_i and [L v_i; B L v_i] as two products instead of one with the composite operator; 5 = the composite operator without the forward walk's affine terms in its constant operand */
    RN_KNOB_FUSE_SPLIT = 13,       /* fused forward walk + dual update: workgroups per chain (1 .. chain length); 0 = one per chain and only where the chains fill 3/4 of the CUs (round 6's first rule) */
    RN_KNOB_STREAM_SKIP = 14,      /* k_stream_gemv: 0 = every span of every operator block is walked; 1 = only the spans that meet a nonzero entry of the dual vector, whole spans; -1 (default) = the library's choice: that skip, by half-spans where RN_KNOB_STREAM_HALF admits them (bitwise the same results in every form) */
    RN_KNOB_STREAM_HALF = 15,      /* k_stream_gemv with two slots per thread and an even span, RN_KNOB_STREAM_SKIP at the library's choice: 0 = a span's two halves are walked or skipped together; 1 (default) = each half by itself where half a span is a whole number of 64-byte half lines (bitwise the same results) */
    RN_KNOB_COUNT = 16
};
int rn_debug_set_knob(rn_ctx *ctx, int knob, int value);

/* What the launches of k_stream_gemv look like, for the tests of its split last round: info = {splitFirst, splitSpanHalf, twoPerCU, numCUs}.
 * splitFirst: the first node whose block two workgroups share by columns (the second one's partials go to a buffer of their own); = nodes
 * when the launch is not split, -1 before the factor step has decided (a re-factor by rn_set_operator decides again).  splitSpanHalf: the
 * span at which the second workgroup starts (0 without a split).  twoPerCU: 1 = the instantiation that leaves room for two workgroups
 * per CU.  numCUs: the device's compute units, valid from rn_create on.  Reads only: nothing that is computed changes. */
int rn_debug_stream_info(rn_ctx *ctx, int info[4]);

/* What the context's most recent launch of k_stream_gemv walked: out = {live spans, spans, live columns, columns}, summed over the blocks of the
 * context.  A span (G consecutive operator columns, rn_get_kernel_info) is live when one of its entries of the dual vector the sweep is evaluated at
 * has any bit but the sign set (-0.0 is zero, a denormal is live; a pair of sweeps in one pass: in either vector); a live column likewise.  With
 * RN_KNOB_STREAM_SKIP = 0 every span is walked and counted.  Synchronises the context's stream, copies one record per workgroup and sums on the host.
 * RN_E_STATE before the first sweep and in the structured mode (no blocks).
 * Where the launch skips half-spans by themselves (rn_debug_stream_units) the live spans are an UPPER BOUND on what it requested: a live span
 * with one dead half is counted whole here.  rn_algorithmic_bytes counts what was requested: the live units of rn_debug_stream_units. */
int rn_debug_stream_live(rn_ctx *ctx, long long out[4]);

/* The same launch in the units its skip walks: out = {live units, units, columns per unit}, summed over the blocks.  A unit is half a span
 * (G / 2 columns; a ragged last span has one or two, ceil(ny / (G / 2)) per block in all) where the launch skips halves by themselves: the skip
 * at the library's choice (RN_KNOB_STREAM_SKIP = -1), RN_KNOB_STREAM_HALF != 0, two slots per thread, G even and half a span a whole number of
 * 64-byte half lines.  Everywhere else a unit is a
 * span and the figures are rn_debug_stream_live's first two with G.  Same synchronisation, same errors. */
int rn_debug_stream_units(rn_ctx *ctx, long long out[3]);

/* The product of k_stream_gemv alone, for a test that holds it to a GEMV: runs ONLY the streaming launch, with the arguments rn_solve_step would
 * give it on this context at the accelerated dual as it stands (what RN_BUF_ACC_* shows) -- the same instantiation, split, skip and half-span
 * choices as a sweep -- synchronises and copies out, widened to double: my [nodes][2 nv] = [m1_i; m2_i] = A_i w_i (for the blocks of a split last
 * round: the partial of the first workgroup, columns [0, splitSpanHalf * G)); my2 [nodes - splitFirst][2 nv], the second workgroups' partials
 * (NULL: not wanted; RN_E_ARG when given for a launch that is not split).  pair = 1: one launch with TWO right-hand sides as NAMA pairs its Hessian
 * sweeps -- the second is y (RN_BUF_XI / RN_BUF_PSI), its product goes to myB [nodes][2 nv]; the launch runs unsplit, as a paired sweep does.
 * RN_E_STATE unless rn_get_sweep_pairing reports the pair active.  pair = 0 ignores myB.  RN_E_STATE in the structured mode (no blocks) and before
 * the factor step.  Changes no iterate (the products and a_i are scratch that every sweep overwrites) and launches nothing but that kernel;
 * rn_debug_stream_live / _units report this launch afterwards. */
int rn_debug_stream_product(rn_ctx *ctx, int pair, double *my, double *my2, double *myB);

/* The products with the SHARED operators on the matrix cores alone (k_slab.hpp: k_gemm_vlv, k_gemm_vlv_wide, k_gemm_comp, k_gemm_prep_m2, k_gemm_slab,
 * k_gemm_shared), for a test that holds them to a plain GEMM: the caller's operators (column-major doubles, logical m x k) go through the context's own
 * padded and fragment-ordered uploads into scratch buffers of the hook's, the caller's inputs, auxiliary rows and probabilities into scratch rows with
 * the strides and offsets of the sweep's own buffers; ONE launch step runs -- the launching code a sweep of this context runs, with the sweep's own
 * choice of kernel, waves, loop, operand copy and slabs per workgroup, RN_KNOB_SLAB_PIPE / _SLAB_FRAG / _VLV_WIDE / _STRUCT_LINEAR acting as on a sweep --
 * and the outputs come back widened to double.
 *   launch = RN_SLABP_PAIR   v_i = aux_i (+ aux2_i) - MA in_i / (2 p_i) and [L v_i; B L v_i] = MB v_i as launch_v_lv runs them (foldRoot = 0).
 *            MA: nv x kA; MB: (nu + nx) x nv.  Dense context: kA = nv + nx, aux = m1 [nodes][2 nv] (the m1 half is read) and, on a context whose
 *            streaming launch has a split last round, aux2 [nodes - splitFirst][2 nv].  Structured context, RN_KNOB_STRUCT_LINEAR 0: kA = nv + nx,
 *            no aux; 3: kA = nv + nx + nu, no aux; 4: kA = nx + nu (read at offset nv of rows of nv + nx + nu), aux = c_i [nodes][nv] or NULL (a
 *            Hessian sweep's form).  storeV = 0: v lives only in LDS (outA is then not written).  outA = v [outNodes][nv], outB [outNodes][nu + nx].
 *            RN_E_ARG on a context whose sweep runs the composite product instead.
 *   launch = RN_SLABP_COMP   k_gemm_comp as the default linear form of a structured context launches it: MA (nu + nx) x (nx + nu), in as under knob 4,
 *            aux = lvconst [nodes][nu + nx] or NULL; outB [outNodes][nu + nx]; MB, aux2 and outA must be NULL.
 *   launch = RN_SLABP_PREP_M2  k_gemm_prep_m2 (structured contexts): only MA (nv x (nx + nu)) is the caller's, the slab [a_i; b_i] is built by the kernel
 *            from the accelerated dual as it stands (RN_BUF_ACC_*), sqrt(p) and the preconditioner rows of the context.  outA [outNodes][2 nv] (m2 in
 *            the second half of each row, as in the sweep's buffer), outB = qa [outNodes][nx].  in, aux, aux2, prob, MB must be NULL.
 *   launch = RN_SLABP_SINGLE  one launch_gemm for an operator `role`: 0 = [Rinv | Rinv Bbt] (EPI_V: nv x (nv + nx), aux = m1 [nodes][2 nv], aux2 as above;
 *            dense contexts), 1 = [L; B L] (EPI_LV: (nu + nx) x nv), 2 = B (EPI_Z: nx x nu, aux = e [nodes][nx]), 3 = [T1 | T2] (EPI_V: nv x (nx + nu),
 *            read at offset nv of rows of nv + nx + nu, aux = c_i [nodes][nv] or NULL).  outA [outNodes][m].
 * in is compact, [nodes][k]; the hook fills the columns of a scratch row the launch must not read with 7777.  prob [nodes] where the launch scales by
 * -1 / (2 p_i) (PAIR, COMP, roles 0 and 3), NULL elsewhere.  outNodes = (ceil(nodes / 48) + 1) * 48: the output buffers are uploaded before the launch and
 * read back whole afterwards, so the caller's fill shows every element that was not written.  nOutA / nOutB: the doubles behind outA / outB.
 * info[RN_SLAB_INFO_COUNT]: [0] [1] the kernel of the first / second launch (1 k_gemm_vlv, 2 k_gemm_vlv_wide, 3 k_gemm_comp, 4 k_gemm_prep_m2,
 * 5 k_gemm_slab, 6 k_gemm_shared; 0 none), [2] waves per workgroup, [3] 1 = the software-pipelined loop, [4] 1 = fragment-ordered A operands, [5] CT,
 * [6] grid, [7] LDS bytes, [8 .. 11] m, k, kp, ldin of the first product, [12 .. 15] of the second (0: none), [16 .. 18] waves, grid, LDS bytes of
 * the second launch, [19] auxSplit of the first product (nodes: none), [20] the device's CUs, [21] 7 = k_struct_prep ran in front (the first product
 * does not fit the slab), [22] outNodes, [23] the input's column offset in its rows.
 * RN_E_STATE before the factor step; RN_E_ARG for an operand the chosen launch does not read or lacks, and for a launch this context's sweep would not
 * run.  Changes no iterate and no operator of the context; allocates its scratch on first use; launches nothing but the product (PREP_M2 on a network
 * too wide for the slab: k_struct_prep in front, as in the sweep). */
enum { RN_SLABP_PAIR = 0, RN_SLABP_COMP = 1, RN_SLABP_PREP_M2 = 2, RN_SLABP_SINGLE = 3 };
enum { RN_SLAB_INFO_COUNT = 24 };
typedef struct {
    int launch, role, storeV;
    const double *MA, *MB, *in, *aux, *aux2, *prob;
    double *outA, *outB;
    size_t nOutA, nOutB;
} rn_slab_product_args;
int rn_debug_slab_product(rn_ctx *ctx, const rn_slab_product_args *args, int info[RN_SLAB_INFO_COUNT]);

/* The gradient restart test (rn_set_restart, rapidnet.h) alone: runs k_restart_test on the context's current w (the last sweep's input, what
 * RN_BUF_ACC_* shows), y+ and y and returns out = {g, na2, nb2} -- the kernel can be checked without running a solve.  Allocates the kernel's
 * partials on first use; changes no iterate.  On a sharded context every rank calls it (it contains the ranks' all-reduce). */
int rn_debug_restart_test(rn_ctx *ctx, double out[3]);

/* The children moments of the cut parents as the context holds them (rn_set_cut_children_moments, or recomputed by rn_set_tree_data on a
 * context made by rn_create_sharded): E [nParents][nd], P [nParents], widened from the context's type.  RN_E_STATE while none are set. */
int rn_debug_cut_moments(rn_ctx *ctx, double *E, double *P, size_t nParents);

/* Hz(y) = (F x(y), G u(y)) as the sweep of the last rn_solve_certificate left it and as k_certificate read it: hzXi [nodes][2 nx], hzPsi
 * [nodes][nu], widened from the context's type -- so that a test can hand the kernel's own inputs to a restatement of the record.
 * RN_E_STATE before the first certificate.  Changes nothing. */
int rn_debug_certificate_hz(rn_ctx *ctx, double *hzXi, double *hzPsi);

/* The dual update of ONE iteration alone (k_dual.hpp: k_dual_stage, k_dual_fused, its fix-up pass and the bookkeeping kernels), for a test that
 * holds it to an exactly rounded restatement.  Inputs are the context's buffers as they stand: Hx = what RN_BUF_PRIMAL_* shows, w = RN_BUF_ACC_*,
 * y = RN_BUF_UPD_* (the yprev of the batch loop's arguments); bounds, sqrt(p) and the preconditioner rows are the context's own.  The launching code is
 * the batch loop's (sweep.inc: dual_main_args / run_dual_main, run_close_optimistic, run_close_exact_sharded, exact_fixup_args / run_exact_fixup);
 * outputs, partials, iteration state and the history slot are scratch of the hook's own, allocated on first use: no iterate, no history entry and no
 * iteration state of the context changes.  The launches are enqueued back to back; the hook synchronises behind the last one.
 *   form = RN_DUALP_MAIN             the main pass only, as launch_dual_main chooses it: k_dual_stage with the context's trips and pipe (RN_KNOB_DUAL_TRIPS /
 *                                    _PIPE act as in a batch) or the flat k_dual_fused; flat = 1 forces the flat kernel, as an exact sharded batch does.
 *                                    unscaled = 1: Hx holds the primal values an unscaled walk leaves (k_dual_stage SCALE; flat: k_hx_scale in front, on a copy).
 *          RN_DUALP_EXACT            the main pass, then the single-GPU fix-up launch (decideHere, finalizedEarly, min(eltBlocks, RN_FIXUP_BLOCKS) workgroups)
 *          RN_DUALP_EXACT_SHARDED    the flat main pass, k_reduce_dist, the context's all-reduce where it has a communicator, k_decide_from, the fix-up
 *                                    launch, k_finalize
 *          RN_DUALP_OPTIMISTIC_CLOSE the main pass and k_finalize_optimistic (which sets the verdict flag)
 *          RN_DUALP_INFO             launches nothing: fills the record's launch cells only
 *          RN_DUALP_NEXT_W           launches nothing: wnext receives the buffer the next sweep would read as w
 *   materialize: 1 = z and res are written too (the last iteration of a batch).  iteration = t: the extrapolation parameter is entry t + 1 of the context's
 *   lambda table.  A combination the library never launches is RN_E_ARG: unscaled with materialize on a stage-tiled shape, unscaled in the exact forms.
 * ynew, wnext, z, res [nodes][ny] (the context's interleaved rows: 2 nx xi columns, nu psi columns): uploaded before the launches and read back whole, so the
 * caller's fill shows every element that was not written.  lo, hi [nodes][ny]: the materialised scaled bounds.  sqrtp [nodes], dy [N][ny], blo / bhi
 * [bRows][ny], stageOf [nodes]: the tables the kernels rebuild the bounds from (any of these NULL: skipped).  partials [nPartials][8]: the raw partials of
 * the main pass {d2x, d2s, absXi, valXi, absPsi, valPsi, idxXi, idxPsi} (an index that was never set reads -1); RN_E_ARG when the launch has more.
 * info[RN_DUAL_INFO_COUNT]: [0] lambda, [1] 1 / lambda, [2] the extrapolation parameter, each as the kernel's type holds it; [3] [4] thrX, thrS; [5] [6] d2x,
 * d2s: the fold of the main pass's partials (k_reduce_dist's, i.e. fold_partials'); [7] [8] distX, distS, [9] tripped, [10] [11] scaleX, scaleS, [12]
 * violated, from the scratch iteration state; [13 .. 15] |.|, signed value and element index of the xi arg-max, [16 .. 18] of the psi one: value and |.| from the
 * history parts the device wrote (MAIN: NaN), the index folded on the host from the partials of the pass that decided them; [19] the history entry (MAIN:
 * NaN); [20] kernel: 1 k_dual_stage, 0 k_dual_fused; [21] grid; [22] trips; [23] pipe; [24] crownBlocks; [25] bps; [26] vpn; [27] cs; [28] K; [29] node0;
 * [30] eltBlocks; [31] fix-up workgroups; [32] crownElems; [33] countCrown; [34] 1 = the SCALE instantiation ran; [35] [36] the bounds tables' strides per
 * stage / per node; [37] rows of the bounds tables; [38] 1 = k_hx_scale ran in front; [39] the iteration counter of the scratch state afterwards.
 * RN_E_STATE before the factor step and under global FBE / NAMA. */
enum { RN_DUALP_MAIN = 0, RN_DUALP_EXACT = 1, RN_DUALP_EXACT_SHARDED = 2, RN_DUALP_OPTIMISTIC_CLOSE = 3, RN_DUALP_INFO = 4, RN_DUALP_NEXT_W = 5 };
enum { RN_DUAL_INFO_COUNT = 40 };
typedef struct {
    int form, materialize, flat, unscaled, iteration;
    double *ynew, *wnext, *z, *res;
    double *lo, *hi;
    double *sqrtp, *dy, *blo, *bhi;
    int *stageOf;
    double *partials;
    size_t nPartials;
} rn_dual_update_args;
int rn_debug_dual_update(rn_ctx *ctx, const rn_dual_update_args *args, double info[RN_DUAL_INFO_COUNT]);

#ifdef __cplusplus
}
#endif
#endif /* RAPIDNET_DEBUG_H_ */
