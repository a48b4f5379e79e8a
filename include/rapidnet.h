/*
 * rapidnet.h -- C ABI of the MI355X-native APG solve path (librapidnet_hip.so).
 *
 * The reference (GPUEngineering/RapidNet) has no FFI layer: its seam is the C++ class surface
 * Engine / SmpcController and raw device pointers.  This header is the boundary a
 * maintainer binds instead: every entry point names the reference member function it replaces
 * (file:line relative to /root/reference/src).  The C++ classes in rapidnet_amd/csrc/host/ (same names and
 * signatures as the reference's) are a thin layer over exactly these functions.
 *
 * Conventions
 *   - plain pointers and sizes only; every HOST array is `double` whatever the device precision;
 *   - matrices are column-major, per-node vectors node-major `[node][dim]`, tree indices as in the
 *     reference's JSON (1-based `ancestor`, root = 0; `nodesPerStage` N+1 entries, `...Cumul` N+2);
 *   - every function returns 0 on success or a negative RN_E_* code and never calls exit();
 *     rn_last_error() returns a message for the last failure on that context;
 *   - one host thread per context, one HIP stream per context; contexts are independent.
 */
#ifndef RAPIDNET_H_
#define RAPIDNET_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rn_ctx rn_ctx;

enum { RN_F32 = 0, RN_F64 = 1 };

enum {
    RN_OK = 0,
    RN_E_ARG = -1,      /* bad argument / dimension mismatch */
    RN_E_HIP = -2,      /* HIP runtime error (message in rn_last_error) */
    RN_E_STATE = -3,    /* call order violated (e.g. iterate before factor step) */
    RN_E_SINGULAR = -4, /* L'WL singular: Engine::inverseBatchMat, Engine.cu:1334-1353 */
    RN_E_COMM = -5      /* RCCL error */
};

/* problem dimensions: DwnNetwork.cuh:67-87, SmpcConfiguration.cuh:60-75, ScenarioTree.cuh:64-84 */
typedef struct {
    int nx, nu, nv, nd; /* tanks, controls, reduced inputs (nu - ne), demands */
    int N, K;           /* prediction horizon, scenarios */
    int nodes, nNonLeafNodes;
} rn_dims;

/* scenario tree exactly as ScenarioTree's getters return it (ScenarioTree.cuh:92-154) */
typedef struct {
    const int *stages;             /* [nodes]   0-based stage of each node              */
    const int *nodesPerStage;      /* [N+1]                                             */
    const int *nodesPerStageCumul; /* [N+2]                                             */
    const int *ancestor;           /* [nodes]   1-based parent, root = 0                */
    const int *nChildren;          /* [nNonLeafNodes]                                   */
    const int *nChildrenCumul;     /* [nodes]                                           */
    const double *probNode;        /* [nodes]                                           */
} rn_tree;

/* inputs of the factor step: what Engine::initialiseSystemDevice (Engine.cu:382-463) reads from DwnNetwork
 * and SmpcConfiguration */
typedef struct {
    const double *matB;          /* nx x nu */
    const double *matGd;         /* nx x nd */
    const double *matL;          /* nu x nv  null-space basis of E (config "matL")      */
    const double *matLhat;       /* nu x nd  -pinv(E) Ed          (config "matLhat")   */
    const double *costW;         /* nu x nu */
    const double *matDiagPrecnd; /* [N][nu | nx | nx] dual preconditioner diagonal      */
    const double *vecXmin, *vecXmax, *vecXsafe; /* nx */
    const double *vecUmin, *vecUmax;            /* nu */
    const double *costAlpha1;                   /* nu */
} rn_system;

/* buffer ids for rn_get / rn_set: the protected device vectors of SmpcController (SmpcController.cuh:336-462)
 * and the affine-term arrays of Engine (Engine.cuh:426-648), in the reference's node-major layout */
enum {
    RN_BUF_X = 0,      /* devVecX            nodes*nx   */
    RN_BUF_U,          /* devVecU            nodes*nu   */
    RN_BUF_V,          /* devVecV            nodes*nv   */
    RN_BUF_XI,         /* devVecXi           nodes*2nx  (y)        */
    RN_BUF_PSI,        /* devVecPsi          nodes*nu              */
    RN_BUF_ACC_XI,     /* devVecAcceleratedXi   (w)                */
    RN_BUF_ACC_PSI,    /* devVecAcceleratedPsi                     */
    RN_BUF_UPD_XI,     /* devVecUpdateXi        (y+)               */
    RN_BUF_UPD_PSI,    /* devVecUpdatePsi                          */
    RN_BUF_PRIMAL_XI,  /* devVecPrimalXi        (Hx)               */
    RN_BUF_PRIMAL_PSI, /* devVecPrimalPsi                          */
    RN_BUF_DUAL_XI,    /* devVecDualXi          (z)                */
    RN_BUF_DUAL_PSI,   /* devVecDualPsi                            */
    RN_BUF_RES_XI,     /* devVecFixedPointResidualXi               */
    RN_BUF_RES_PSI,    /* devVecFixedPointResidualPsi              */
    RN_BUF_UHAT,       /* Engine devVecUhat  nodes*nu   */
    RN_BUF_E,          /* Engine devVecE     nodes*nx   */
    RN_BUF_BETA,       /* Engine devVecBeta  nodes*nv   */
    RN_BUF_ALPHA,      /* Engine devVecAlpha nodes*nu (getPriceAlpha) */
    RN_BUF_XMIN, RN_BUF_XMAX, RN_BUF_XS, /* scaled bounds, nodes*nx */
    RN_BUF_UMIN, RN_BUF_UMAX,            /* nodes*nu */
    /* global FBE / NAMA (valid after rn_set_algorithm selected one of them) */
    RN_BUF_PREV_XI, RN_BUF_PREV_PSI,                       /* devVecPrevXi / devVecPrevPsi                              */
    RN_BUF_LBFGS_CUR_YVEC_XI, RN_BUF_LBFGS_CUR_YVEC_PSI,   /* ptrLbfgsCurrentYvec*: devVecGradientFbe* (FBE) or
                                                              devVecCurrentFixedPointResidual* (NAMA), SmpcController.cu:513-524 */
    RN_BUF_LBFGS_PREV_YVEC_XI, RN_BUF_LBFGS_PREV_YVEC_PSI, /* ptrLbfgsPreviousYvec*                                     */
    RN_BUF_LBFGS_DIR_XI, RN_BUF_LBFGS_DIR_PSI,             /* devVecLbfgsDirXi / Psi                                    */
    RN_BUF_PRIMAL_XI_DIR, RN_BUF_PRIMAL_PSI_DIR,           /* devVecPrimalXiDir / PsiDir                                */
    RN_BUF_XDIR, RN_BUF_UDIR,                              /* devVecXdir nodes*nx, devVecUdir nodes*nu                  */
    /* Extension (rn_solve_certificate): x(y), u(y) of the last certificate, nodes*nx and nodes*nu; size 0 before the first; read-only */
    RN_BUF_CERT_X, RN_BUF_CERT_U,
    RN_BUF_COUNT
};

/* per-node operator blocks of Engine::factorStep for rn_get_operator (Engine.cuh getMatPhi() ...) */
enum { RN_OP_PHI = 0 /* nv x 2nx */, RN_OP_PSI /* nv x nu */, RN_OP_D /* nv x 2nx */, RN_OP_F /* nv x nu */,
       RN_OP_OMEGA /* nv x nv */, RN_OP_THETA /* nv x nx */, RN_OP_G /* nv x nx */ };

/* ---- lifetime ------------------------------------------------------------------------------------ */
/* Engine::Engine + allocate*Device (Engine.cu:126-380) and SmpcController::allocateSmpcController /
 * allocateApgAlgorithm (SmpcController.cu:117-232).  `device` is the HIP device ordinal. */
int rn_create(const rn_dims *dims, const rn_tree *tree, int precision, int device, rn_ctx **out);
int rn_destroy(rn_ctx *ctx);
const char *rn_last_error(const rn_ctx *ctx);
int rn_synchronize(rn_ctx *ctx);

/* Operator storage, to be chosen BEFORE rn_factor_step.
 *   RN_OPS_DENSE: the reference's storage model -- dense per-node blocks Phi_i, Psi_i, D_i, Ftil_i
 *     (Engine.cu:166-189), streamed from HBM once per iteration (4.09 GB for the 493-scenario Barcelona tree).
 *   RN_OPS_STRUCTURED: the blocks are never materialised; the factor step's own formulas (block = shared matrix x
 *     stage diagonal x power of p_i, Engine.cu:721-745) are applied as shared-operator GEMMs.  Same iterates (the parity
 *     suite runs both), 6-7 x the iteration rate on the 493-scenario tree.
 *   RN_OPS_AUTO (the default of a new context): structured for as long as every block is the factor step's own -- which is
 *     always, unless the caller hands in a block through rn_set_operator; the first such call materialises the dense blocks
 *     (one more factor step on the inputs of the last one) and the context runs dense from then on.
 * rn_get_operator_mode: *requested = what was asked for, *active = RN_OPS_DENSE or RN_OPS_STRUCTURED, what the context runs. */
enum { RN_OPS_DENSE = 0, RN_OPS_STRUCTURED = 1, RN_OPS_AUTO = 2 };
int rn_set_operator_mode(rn_ctx *ctx, int mode);
int rn_get_operator_mode(rn_ctx *ctx, int *requested, int *active);
/* Element type of the DENSE per-node blocks, to be chosen BEFORE rn_factor_step (afterwards: RN_E_STATE; an unknown value: RN_E_ARG).
 *   RN_STORE_NATIVE (the default): the blocks are stored in the context's precision.
 *   RN_STORE_F32: an RN_F64 context stores them in fp32 -- the reference's own element type (Configuration.h:31) and half the bytes the
 *     dominant kernel streams -- while every vector stays fp64 and every sum over a block is accumulated in fp64: the iterates are the fp64
 *     solution of the problem WITH THE ROUNDED BLOCKS (to 1e-9 against an fp64 oracle given the same blocks), and the problem itself is
 *     perturbed by at most 2^-24 relative (6e-8) per block entry.  rn_get_operator returns the stored values (fp32-representable doubles);
 *     rn_set_operator rounds the caller's block to nearest fp32 on upload.  On an RN_F32 context the value is accepted and changes nothing.
 *     The quasi-Newton loops run their two Hessian sweeps one after the other in this mode unless rn_set_sweep_pairing(RN_PAIR_ON) asks for
 *     the shared pass over the blocks (below).
 * The setting concerns the dense blocks only: under RN_OPS_STRUCTURED it is remembered and has no effect, under RN_OPS_AUTO it takes effect
 * when the first rn_set_operator materialises the blocks.
 * rn_get_operator_storage: *requested = what was asked for, *active = RN_STORE_F32 only while dense blocks exist in fp32. */
enum { RN_STORE_NATIVE = 0, RN_STORE_F32 = 1 };
int rn_set_operator_storage(rn_ctx *ctx, int storage);
int rn_get_operator_storage(rn_ctx *ctx, int *requested, int *active);
/* NAMA's two Hessian oracles of a line search (SmpcController.cu:1331 on the residual, :1341-1345 on the corrected direction) do not feed each
 * other, so one pass over the DENSE per-node blocks can serve both (two right-hand sides in the streaming kernel): a NAMA iteration then
 * streams the blocks twice instead of three times.  Bitwise the results of the two sweeps run one after the other.
 *   RN_PAIR_AUTO (the default of a new context): blocks in the context's own type pair whenever the streaming launch has no split last round
 *     and both right-hand sides' LDS sets fit 64 KB; RN_STORE_F32 blocks under fp64 iterates do not pair.
 *   RN_PAIR_ON: AUTO plus RN_STORE_F32 blocks, a context whose streaming launch has a split last round included (the pair sweep alone runs
 *     unsplit; every other sweep keeps its split); their two LDS sets (doubles) may take the CU's 160 KB.  Opt-in because its gain has not been measured on an MI355X yet.
 *   RN_PAIR_OFF: the two sweeps always run one after the other.
 * Valid at any time (an unknown value: RN_E_ARG).  The pair needs buffers of its own: allocated by this call when RN_ALG_NAMA is already
 * selected, by the next rn_set_algorithm(RN_ALG_NAMA) otherwise.  Sharded contexts (rn_set_cut_stage, a communicator) never pair.
 * rn_get_sweep_pairing: *requested = what was asked for; *active = 1 when the context as it stands would pair its next NAMA line search
 * (RN_ALG_NAMA selected, dense blocks, the pair buffers present, both LDS sets fit, not sharded), else 0.  rn_fbe_counters out[3] counts the pairs. */
enum { RN_PAIR_OFF = 0, RN_PAIR_ON = 1, RN_PAIR_AUTO = 2 };
int rn_set_sweep_pairing(rn_ctx *ctx, int mode);
int rn_get_sweep_pairing(rn_ctx *ctx, int *requested, int *active);

/* ---- Engine -------------------------------------------------------------------------------------- */
/* Engine::factorStep (Engine.cu:671-774) incl. initialiseSystemDevice / preconditioning kernels. */
int rn_factor_step(rn_ctx *ctx, const rn_system *sys);
/* tree errors uploaded once (the reference re-uploads them every control step, Engine.cu:1205,1228) */
int rn_set_tree_errors(rn_ctx *ctx, const double *errorDemandNode /* nodes*nd */, const double *errorPriceNode /* nodes*nu */);
/* Scenario probabilities and tree errors replaced in place, for a forecaster that re-weights a tree of FIXED topology between two control
 * steps (ScenarioTree.cuh:92-154 getProbArray / getErrorDemandArray / getErrorPriceArray; the reference uploads devTreeProb once,
 * Engine.cu:263-286, and the errors with every control step, Engine.cu:1205,1228; calculateZeta, Engine.cu:1251, is what reads them).
 * Layouts as in rn_tree and rn_set_tree_errors: probNode [nodes], errorDemandNode [nodes][nd], errorPriceNode [nodes][nu].  Any pointer may be
 * NULL: on a set that array keeps its bits, on a get it is skipped; all three NULL: RN_E_ARG.
 * nodes: the context's node count; on a context made by rn_create_sharded with nranks > 1 a SET takes the FULL tree's count (rn_shard_info
 *   info[6]) and the full-tree arrays -- every rank makes the same call, as rn_create_sharded takes the full tree, and the context picks its rows
 *   by its global-node map -- while a GET takes the local count and returns local rows in the order of rn_shard_global_nodes.  Any other count:
 *   RN_E_ARG.
 * Values: probNode entries must be positive and finite (rn_create's rule).  The host form checks first and returns RN_E_ARG with nothing
 *   changed.  The device form cannot without a synchronisation: its kernel counts the offending entries on the device and the library reads the
 *   count behind the synchronisation of the rn_eliminate_input_disturbance_coupling that has to follow (rn_control_action included): that call
 *   returns RN_E_ARG, its message names rn_set_tree_data_device and the count, and the context refuses to iterate (RN_E_STATE) until a valid
 *   set and an elimination have been made.  The errors are not validated (rn_set_tree_errors does not either).
 * State: before rn_factor_step the arrays are replaced and the factor step uses them.  On a factored context a call that gives probNode
 *   re-runs, on the context's stream, what of the factor step depends on p -- p, sqrt(p), the scaled bounds and, where the context holds dense
 *   blocks, their expansion (Engine.cu:721-745) in the storage type in force; no host factorisation, no upload of a shared matrix -- and the
 *   context stays factored.  As after rn_factor_step, blocks handed in by the caller are recomputed from the factor step's formulas; an
 *   RN_OPS_AUTO context that was never handed a block stays structured.  With probNode given the affine terms and every control-step constant
 *   derived from them are invalid: iterating before the next rn_eliminate_input_disturbance_coupling is RN_E_STATE (rn_control_action
 *   recomputes them itself).  Errors alone behave as rn_set_tree_errors: they take effect at the next elimination.  Duals, warm start,
 *   algorithm, L-BFGS memory, stop tolerance, operator mode, operator storage and sweep pairing are untouched.
 * Sharded: a context made by rn_create_sharded recomputes the children moments of its cut parents (rn_set_cut_children_moments) whenever
 *   probNode or errorDemandNode is given, over ALL children in ascending order, from the arrays of the call and -- for the one that is
 *   missing -- the full-tree values of the cut stage it retains.  A context sharded by hand (rn_create on a local tree, rn_set_cut_stage) takes
 *   local rows and its moments become unset: rn_set_cut_children_moments has to follow before the affine terms.
 * rn_set_tree_data / rn_get_tree_data: host arrays of doubles; they synchronise, as rn_set does, and their staging is allocated and freed inside
 *   the call (rn_device_memory_info info[2] is the same before and after).
 * rn_set_tree_data_device: arrays in device memory, elements of type `precision` (RN_F32 / RN_F64 whatever the context's own type; any other
 *   value: RN_E_ARG); launches on the context's stream only -- no allocation, no host synchronisation; the caller orders its producer against
 *   rn_stream as rn_device_pointer describes.  Every non-NULL pointer is checked as rn_set_operators_device checks its arrays (device of the
 *   context, alignment, length where the runtime knows it) before anything is launched: otherwise RN_E_ARG. */
int rn_set_tree_data(rn_ctx *ctx, size_t nodes, const double *probNode, const double *errorDemandNode, const double *errorPriceNode);
int rn_set_tree_data_device(rn_ctx *ctx, size_t nodes, int precision, const void *probNode, const void *errorDemandNode, const void *errorPriceNode);
int rn_get_tree_data(rn_ctx *ctx, size_t nodes, double *probNode, double *errorDemandNode, double *errorPriceNode);
/* Box and safety bounds per stage or per node, replaced in place (the reference keeps devSysXmin ... devSysUmax as per-node arrays and hands
 * out their device pointers, Engine.cuh:294-314 getSysXmin() ... getSysUmax(), so its callers can give any node its own bounds; the scaling is
 * Engine.cu preconditionConstraintX / preconditionConstraintU): a safety volume that follows the demand forecast, a pump out of service for
 * the next hours, a tank taken down in one scenario only -- without another rn_factor_step.
 * granularity / rows: RN_BOUNDS_SHARED, rows = 1: one row for the whole tree (what rn_factor_step sets from rn_system); RN_BOUNDS_PER_STAGE,
 *   rows = dims.N: a node at stage s uses row s, the row index of matDiagPrecnd; RN_BOUNDS_PER_NODE, rows = the context's node count: node i
 *   uses row i -- on a sharded context the LOCAL rows in the order of rn_shard_global_nodes, as rn_set_operators takes them (the caller gives
 *   replicated crown nodes the same values on every rank).  Any other pair: RN_E_ARG.
 * Values: xmin, xmax, xsafe [rows][nx], umin, umax [rows][nu], physical (unscaled), the units of rn_system.  The library applies
 *   sqrt(p_i) d_c exactly as the factor step does (the same expression, the same single rounding); the upper bound of the safety half stays
 *   the internal +BIG.
 * NULL: a NULL array keeps its values while the granularity stays what it is; a call that changes the granularity needs all five (RN_E_ARG
 *   otherwise); all five NULL: RN_E_ARG.
 * State: RN_E_STATE before rn_factor_step.  A later rn_factor_step returns the context to RN_BOUNDS_SHARED with its own vectors (as it
 *   recomputes handed-in operator blocks); a later rn_set_tree_data[_device] that gives probNode keeps granularity and physical values and
 *   rescales them with the new sqrt(p).  Duals, warm start, algorithm, L-BFGS memory, stop tolerance, operator mode and storage, sweep pairing
 *   and the affine terms are untouched (bounds do not enter rn_eliminate_input_disturbance_coupling); an RN_OPS_AUTO context stays structured.
 *   rn_control_action(..., projectOnBounds) clamps with the root's row.
 * rn_set_bounds: host arrays of doubles.  It validates first -- every value finite, xmin <= xmax, umin <= umax (an array that is not given is
 *   compared as the context holds it) -- and returns RN_E_ARG with nothing changed otherwise; its staging is allocated and freed inside the
 *   call (rn_device_memory_info info[2] is the same before and after at a granularity already in force) and it synchronises, as rn_set does.
 * rn_set_bounds_device: arrays in device memory, elements of type `precision` (RN_F32 / RN_F64 whatever the context's own type); launches on
 *   the context's stream only, no host synchronisation.  Pointers are checked as rn_set_operators_device checks its arrays.  The VALUES ARE NOT
 *   VALIDATED: a NaN or a lower bound above its upper bound goes into the solver as given.  The first call at a new granularity (either
 *   form) allocates that table ([rows][ny] x 2 in the context's type) and may synchronise; later calls allocate nothing.
 * rn_get_bounds: the physical values as the context holds them (in its own type: an fp32 context returns the floats it keeps), rows as
 *   rn_get_bounds_layout reports; a NULL array is skipped, all five NULL: RN_E_ARG.
 * Cost: RN_BOUNDS_SHARED and RN_BOUNDS_PER_STAGE tables stay in cache; in RN_BOUNDS_PER_NODE the fused dual update reads two more streams
 *   (rn_algorithmic_bytes counts 7 n_y instead of 5 n_y reals per node in that mode): the caller's choice. */
enum { RN_BOUNDS_SHARED = 0, RN_BOUNDS_PER_STAGE = 1, RN_BOUNDS_PER_NODE = 2 };
int rn_set_bounds(rn_ctx *ctx, int granularity, size_t rows, const double *xmin, const double *xmax, const double *xsafe /* [rows][nx] */,
                  const double *umin, const double *umax /* [rows][nu] */);
int rn_set_bounds_device(rn_ctx *ctx, int granularity, size_t rows, int precision, const void *xmin, const void *xmax, const void *xsafe,
                         const void *umin, const void *umax);
int rn_get_bounds_layout(rn_ctx *ctx, int *granularity, size_t *rows);
int rn_get_bounds(rn_ctx *ctx, size_t rows, double *xmin, double *xmax, double *xsafe, double *umin, double *umax);
/* Plan report: what the plan the context holds costs and where it violates its bounds, per stage and per scenario.  The reference's KPIs
 * (SmpcController::updateKpi and the read-outs getEconomicKpi, getSmoothKpi, getSafeKpi, getNetworkKpi, SmpcController.cu:1819-1859) are
 * closed-loop sums over ONE realised trajectory; these entry points give the predictive counterpart over the scenario tree, from the x and u
 * that rn_get(RN_BUF_X / RN_BUF_U) would return at that moment, without a read-back and without the tree bookkeeping on the host.
 * Per-node terms, all physical: du_i = u_i - u_parent(i) (the root against prevU), alpha_i the context's RN_BUF_ALPHA, the bounds the
 *   unscaled table in force (rn_set_bounds, any granularity):
 *     RN_PLAN_ECON      p_i alpha_i' u_i                     RN_PLAN_SMOOTH    p_i du_i' W du_i          RN_PLAN_STORED   p_i sum_j x_ij
 *     RN_PLAN_SHORT_EXP p_i sum_j max(xs_j - x_ij, 0)        RN_PLAN_XBOX_EXP  p_i sum_j [max(xmin_j - x_ij, 0) + max(x_ij - xmax_j, 0)]
 *     RN_PLAN_UBOX_EXP  the same for u                       RN_PLAN_*_MAX     the largest single entry of the same three violations, not weighted
 * rn_plan_report: perStage [stages][RN_PLAN_COLS], stages = dims.N: the sum columns summed over the nodes of the stage, the maxima taken
 *   over the same nodes.  On a sharded context the call is collective and every rank receives the whole tree's table, the same bits.
 * rn_plan_report_scenarios: perLeaf [leaves][RN_PLAN_COLS], leaves = the context's (local) node count at the last stage: the terms NOT
 *   weighted, summed (maxima: taken) along the path from the leaf to the root; RN_PLAN_STORED holds the leaf's own sum_j x.  leafNode (may be
 *   NULL) receives the node index of every row (local on a shard: map it through rn_shard_global_nodes).  With probNode of the leaves the
 *   caller has the cost distribution, hence a CVaR.  Rows stay local on a sharded context (the crown is replicated: every path is complete),
 *   but the call is collective there as well.
 * rn_plan_report_device: the same two tables, doubles in device memory, valid until the next report on this context; launches on the
 *   context's stream, no host synchronisation.  *perStage is COLUMN-major, [RN_PLAN_COLS][dims.N] (the sum columns and the maxima are each
 *   one contiguous block); *perLeaf is [*leaves][RN_PLAN_COLS]; row l is local node (nodes - *leaves + l).
 * Arithmetic: fp64 on fp32 contexts too (every stored value converted first); every sum in an order fixed by the tree and the launch shape,
 *   no floating-point atomics: two calls on an unchanged context return the same bits.  There are no thresholded counts ("probability of
 *   shortfall"): APG drives active constraints to exactly x = xs, such a column would be noise.
 * State: RN_E_STATE before rn_factor_step, before the affine terms, or before the first sweep of a solve.  stages / leaves wrong or a NULL
 *   output: RN_E_ARG.  Memory: the first report allocates a [nodes][RN_PLAN_COLS] table and the result tables and keeps them; later reports
 *   allocate nothing (rn_device_memory_info info[2]); a context that never asks allocates and launches nothing. */
enum { RN_PLAN_ECON = 0, RN_PLAN_SMOOTH, RN_PLAN_STORED, RN_PLAN_SHORT_EXP, RN_PLAN_XBOX_EXP, RN_PLAN_UBOX_EXP,   /* sums   */
       RN_PLAN_SHORT_MAX, RN_PLAN_XBOX_MAX, RN_PLAN_UBOX_MAX, RN_PLAN_COLS };                                     /* maxima */
int rn_plan_report(rn_ctx *ctx, size_t stages, double *perStage /* [stages][RN_PLAN_COLS] */);
int rn_plan_report_scenarios(rn_ctx *ctx, size_t leaves, double *perLeaf /* [leaves][RN_PLAN_COLS] */, int *leafNode /* may be NULL */);
int rn_plan_report_device(rn_ctx *ctx, void **perStage, void **perLeaf, size_t *leaves);
/* Plan bands: what the plan the context holds looks like across the scenario tree -- per stage the band of every tank level (RN_BAND_X) or
 * pump flow (RN_BAND_U) over the scenarios, and the trajectories themselves: a fan chart's 5 % / median / 95 % with scenario paths drawn over
 * it, the companion of the plan report's cost distribution.  The reference has no counterpart (its read-outs, SmpcController.cu:1819-1859,
 * follow ONE realised trajectory).  Values are the physical x and u that rn_get(RN_BUF_X / RN_BUF_U) would return at that moment; results
 * are doubles whatever the context's precision (an fp32 value is widened exactly).
 * Quantile of stage k, component c, level q in [0, 1], under the probabilities in force (rn_set_tree_data): the nodes i of the stage with
 *   p_i > 0, ordered by (value ascending, node index ascending); their p added in that order in fp64, one after the other,
 *   c_1 = p_(1), c_j = c_(j-1) + p_(j); the result is the value of the first j with c_j >= q * c_m (c_m the last sum, q * c_m one product).
 *   It is always one of the inputs (no interpolation); q = 0 is the minimum and q = 1 the maximum over the nodes that can occur; a stage of
 *   one node returns that node's value for every q.  The summation order is part of the definition: two calls, and every rank of a sharded
 *   context, return the same bits.
 * rn_plan_quantiles: out [stages][dim][nq], stages = dims.N, dim = nx or nu, level l at the caller's position l (q in any order, nq <=
 *   RN_BAND_MAX_LEVELS).
 * rn_plan_quantiles_device: the same table, doubles in device memory, valid until the next rn_plan_quantiles* call on this context; launches
 *   on the context's stream, no host synchronisation (the levels travel in the kernel's arguments).  A (stage, component) that holds a
 *   value that is not finite reads NaN at every level there; the host form returns RN_E_STATE instead.
 * rn_plan_paths: out [leaves][dims.N][dim]: row (l, k) is the row of the ancestor at stage k of leaf l, the l-th node of the last stage;
 *   leafNode (may be NULL) receives that node's index.
 * Sharded contexts (rn_create_sharded): every rank calls; each packs its rows and probabilities into a table of the whole tree, the table
 *   is summed on the context's communicator (exact: one rank at most holds a nonzero value at each entry; a zero's sign may change), and
 *   every rank then holds the WHOLE tree's results, the same bits: stages and node indices are the full tree's, `leaves` its last stage's.
 * Errors: RN_E_ARG for a wrong `which`, nq = 0 or nq > RN_BAND_MAX_LEVELS, a level outside [0, 1] or NaN, stages / leaves not the tree's, a
 *   NULL levels or output pointer; RN_E_STATE before the first sweep of a solve, after a batch that failed half-way (until rn_apg_reset), when
 *   the plan holds a value that is not finite, when a stage holds more than 4096 nodes (the sort's keys of one stage stay in LDS), or on a
 *   context sharded by hand.  Memory: the first call allocates the result tables (sized for the larger of nx and nu; on a shard the whole
 *   tree's table as well) and keeps them; later calls allocate nothing (rn_device_memory_info info[2]); a context that never asks
 *   allocates and launches nothing. */
enum { RN_BAND_X = 0, RN_BAND_U = 1 };
enum { RN_BAND_MAX_LEVELS = 16 };
int rn_plan_quantiles(rn_ctx *ctx, int which, size_t nq, const double *q, size_t stages, double *out /* [stages][dim][nq] */);
int rn_plan_quantiles_device(rn_ctx *ctx, int which, size_t nq, const double *q, void **out /* device, fp64, same layout */);
int rn_plan_paths(rn_ctx *ctx, int which, size_t leaves, double *out /* [leaves][N][dim] */, int *leafNode /* may be NULL */);
/* Engine::setDemandUncertaintyFlag / setPriceUncertaintyFlag / SmpcConfiguration::getWeightEconomical */
int rn_set_uncertainty(rn_ctx *ctx, int demandUncertainty, int priceUncertainty, double weightEconomical);
/* Engine::updateStateControl (Engine.cu:1300-1316) */
int rn_update_state_control(rn_ctx *ctx, const double *currentX, const double *prevU, const double *prevDemand);
/* Engine::eliminateInputDistubanceCoupling (Engine.cu:1147-1298): nominalDemand [N][nd], nominalPrices [N][nu] */
int rn_eliminate_input_disturbance_coupling(rn_ctx *ctx, const double *nominalDemand, const double *nominalPrices);

/* ---- SmpcController: algorithm parameters -------------------------------------------------------- */
/* stepSize, penaltyStateX, penaltySafetyX (SmpcConfiguration.cuh:120-135) */
int rn_set_parameters(rn_ctx *ctx, double stepSize, double penaltyStateX, double penaltySafetyX);

/* ---- SmpcController: the APG loop ---------------------------------------------------------------- */
/* SmpcController::initialiseAlgorithm (SmpcController.cu:420-450): zero the duals, theta = {1,1} */
int rn_apg_reset(rn_ctx *ctx);
/* `n` iterations of the loop body of SmpcController::algorithmApg (SmpcController.cu:1512-1522), device
 * resident, no host synchronisation.  primalInfs (may be NULL) receives vecPrimalInfs[] for these n
 * iterations (this copy synchronises). */
int rn_apg_iterate(rn_ctx *ctx, int n, double *primalInfs);
/* SmpcController::algorithmApg (SmpcController.cu:1500-1525) = rn_apg_reset + rn_apg_iterate(maxIterations) */
int rn_algorithm_apg(rn_ctx *ctx, int maxIterations, double *primalInfs);
/* Extension: SmpcController::algorithmApg runs maxIterations whatever the residual (SmpcController.cu:1500-1525), although it records the
 * primal infeasibility of every iteration (updatePrimalInfeasibity, :1480-1496, into vecPrimalInfs, :1521).  rn_apg_solve = rn_apg_reset, then
 * batches of checkEvery iterations (the last one shorter when maxIterations is no multiple) exactly as rn_apg_iterate(checkEvery) runs them;
 * after each batch the solve ends if the residual of that batch's LAST iteration -- the entry rn_apg_iterate returns in primalInfs -- is <= tol.
 * The iterates are therefore bit for bit those of rn_apg_reset followed by the same sequence of rn_apg_iterate calls; a batch that was replayed
 * through the exact path is judged on the replay.  The decision is the host's, taken behind the synchronisation that closes a batch; the
 * launch that closes the batch publishes what it needs.  On a sharded context every rank calls it and every rank stops at the same count.
 * maxIterations as rn_algorithm_apg; tol >= 0 (0: never stops early); checkEvery <= 0: the library's default (20); values below 16 run the
 * exact path, as rn_apg_iterate with that n does.  *iterationsRun (required) = iterations run; primalInfs (may be NULL, maxIterations entries)
 * receives the first *iterationsRun entries of vecPrimalInfs.  tol negative, NaN or infinite, maxIterations < 0, iterationsRun NULL: RN_E_ARG;
 * before the factor step or the affine terms: RN_E_STATE.  Within rn_reserve_iterations no device memory is allocated. */
int rn_apg_solve(rn_ctx *ctx, int maxIterations, double tol, int checkEvery, int *iterationsRun, double *primalInfs);
/* Extension (SmpcController.cu:1500-1525, :1480-1496 as above): what rn_control_action and rn_algorithm_apg then do -- with tol > 0 they run the
 * loop of rn_apg_solve in place of their one batch of maxIterations (rn_control_action after its own reset or warm start, rn_set_warm_start).
 * The default, tol = 0, is the fixed iteration count of the reference, bit for bit.  checkEvery <= 0: the library's default (20).  The
 * quasi-Newton loops (rn_algorithm_fbe_nama) ignore the setting. */
int rn_set_stop_tolerance(rn_ctx *ctx, double tol, int checkEvery);
/* the setting of rn_set_stop_tolerance (SmpcController.cu:1500-1525, :1480-1496); either pointer may be NULL */
int rn_get_stop_tolerance(rn_ctx *ctx, double *tol, int *checkEvery);
/* Of the last rn_apg_solve / rn_algorithm_apg / rn_control_action (the count the reference fixes in advance, SmpcController.cu:1500-1525; the
 * residuals of :1480-1496): out = {iterations it ran, 1 if it stopped on the tolerance, first iteration (0-based, within that solve) whose
 * residual was <= tol or -1 (also -1 when no tolerance was set), batches run}. */
int rn_get_last_solve(rn_ctx *ctx, long out[4]);
/* Extension: adaptive restart of the momentum (O'Donoghue & Candes, gradient scheme).  The reference's theta recursion runs on for the whole
 * solve (SmpcController.cu:1500-1525; the extrapolation it feeds: :535-557).  With RN_RESTART_GRADIENT, rn_apg_solve, rn_algorithm_apg and
 * rn_control_action run their iterations in batches of checkEvery (rn_apg_solve's argument; rn_set_stop_tolerance's for the other two,
 * default 20 -- a tolerance of 0 is allowed: restart without an early stop) and, at every batch end, behind the tolerance check (a solve that
 * stops does not restart), one kernel evaluates g = <w_k - y_{k+1}, y_{k+1} - y_k> over the whole tree, summed in fp64 in a fixed order.
 * g > 0: y := y_{k+1}, the next extrapolation starts the theta sequence again at {1, 1}; the iteration count, the residual history,
 * rn_get_last_solve and the batch counters carry on.  A batch replayed through the exact path is judged on the replay; on a sharded
 * context every rank holds the same bits of g and takes the same decision.  RN_RESTART_OFF (the default): nothing is launched or allocated,
 * every solve is the reference's, bit for bit.  rn_algorithm_fbe_nama ignores the setting.  Any other mode: RN_E_ARG. */
enum { RN_RESTART_OFF = 0, RN_RESTART_GRADIENT = 1 };
int rn_set_restart(rn_ctx *ctx, int mode);
/* the setting of rn_set_restart (SmpcController.cu:1500-1525, :535-557); mode NULL: RN_E_ARG */
int rn_get_restart(rn_ctx *ctx, int *mode);
/* Of the last rn_apg_solve / rn_algorithm_apg / rn_control_action under RN_RESTART_GRADIENT (the loop of SmpcController.cu:1500-1525, the
 * extrapolation of :535-557): counts = {restarts, iteration count at the last restart or -1, batch ends tested, 0}; last = {g, na2, nb2} of
 * the last test, na2 = |w_k - y_{k+1}|^2, nb2 = |y_{k+1} - y_k|^2 (g / sqrt(na2 nb2) is the cosine: how marginal the decision was).  With the
 * mode off: {0, -1, 0, 0} and zeros.  Either pointer NULL: RN_E_ARG. */
int rn_get_restart_info(rn_ctx *ctx, long counts[4], double last[3]);
/* SmpcController::controlAction(real_t*) (SmpcController.cu:1607-1625): update state, eliminate, APG, copy u of the root node
 * (nu reals) to the host.  The reference's leak check around these calls (cudaMemGetInfo before and after, :1612-1623) is the
 * caller's, with rn_device_memory_info below -- the host class SmpcController::controlAction does exactly that. */
int rn_control_action(rn_ctx *ctx, const double *currentX, const double *prevU, const double *prevDemand,
                      const double *nominalDemand, const double *nominalPrices, int maxIterations,
                      int projectOnBounds, double *u0);

/* cudaMemGetInfo of the reference's leak check (SmpcController.cu:1612, :1619, :1641, :1657): info = {free bytes of the context's
 * device, total bytes, bytes THIS context holds, live contexts of this process}.  The device-wide figure moves with every other
 * context and process on the device; the context's own does not. */
int rn_device_memory_info(rn_ctx *ctx, size_t info[4]);
/* SmpcController::allocateApgAlgorithm sizes the per-iteration storage by maxIterations once (SmpcController.cu:124-151): reserves
 * the iteration tables and the checkpoint buffers for batches of up to maxIterations iterations, so that no later
 * rn_apg_iterate / rn_control_action allocates device memory.  (1 022 iterations are reserved by rn_create.) */
int rn_reserve_iterations(rn_ctx *ctx, int maxIterations);

/* Extension (the reference always cold-starts, SmpcController.cu:1509): when on,
 * rn_control_action keeps the duals of the previous control step and only restarts the momentum. */
int rn_set_warm_start(rn_ctx *ctx, int on);
/* Extension (the other half; the reference always cold-starts, SmpcController.cu:1509): the warm start
 * SHIFTED one stage toward the root.  In a receding horizon what was stage k + 1 is stage k of the next control step, so every node starts
 * from the multiplier of the node that stood one stage below it on the branch that was taken, per unit of probability.
 * The correspondence m (purely topological, built on the host): m(root) = child number rootChild of the root, 0-based in child order (a root
 *   that is a leaf, N = 1: m(root) = root); for the r-th child j of i: child number min(r, nc - 1) of m(i) when m(i) has nc > 0 children,
 *   else m(j) = m(i) -- the last stage repeats.
 * The values: with y+ the updated dual of the last solve (RN_BUF_UPD_XI / RN_BUF_UPD_PSI; rows [node][2 nx + nu] in the context), d the stage
 *   diagonal of the factor step in the same column order, p the probabilities in force (rn_set_tree_data), for node i, component c, m = m(i):
 *     f = sqrt(p_i / p_m) * (d[stage(m)][c] / d[stage(i)][c])      in fp64, in this order (a quotient, a root, a quotient, a product)
 *     y_new[i][c] = (T)( f * (double) y+[m][c] )                    one more product, rounded once to the context's type
 *     f = 0 where p_i == 0, p_m == 0 or d[stage(i)][c] == 0
 *   i.e. the multiplier per unit of probability is carried over: F_i' xi_i / p_i = F_m' xi_m / p_m with F_i = sqrt(p_i) diag(d_stage(i)).  A
 *   zero of y+ enters as +0 (so that a shard, whose rows pass through a sum, holds the bits of one GPU).  fp64 arithmetic on fp32 contexts
 *   too, with the probabilities as given.  The result is written to BOTH y (RN_BUF_XI / _PSI) and y+; the accelerated dual is marked not
 *   current, as rn_set_warm_start's restart leaves it, and the next solve starts its momentum at theta = {1, 1}.  No atomics: two calls from
 *   the same state give the same bits.
 * rn_shift_warm_start: rootChild in [0, children of the root), or -1 for the root's child with the largest probability in force, ties to the
 *   lowest index -- the one form that reads values back and so waits for the stream; otherwise one kernel and one copy on the context's
 *   stream, no host synchronisation (the first call, and a call with another rootChild, also upload the correspondence).  It does NOT switch
 *   the warm start on: with rn_set_warm_start off the next rn_control_action cold-starts as ever.  Call it between two control steps, before
 *   the rn_control_action that is to start from the shifted duals.
 * rn_set_shift_map: a forecaster's own correspondence in place of the rule: `nodes` entries for the nodes of the WHOLE tree (also on a
 *   shard), each in [0, nodes) or -1 for "start this node from zero"; map == NULL returns to the rule.  With a caller's map in force
 *   rootChild is ignored.  rn_get_shift_map: the map in force, or the rule's for that rootChild (on a shard -1 is refused: name the child).
 * Sharded contexts (rn_create_sharded): every rank calls; each packs its rows of y+ and its probabilities into a zeroed table of the whole
 *   tree, one sum all-reduce follows (exact: one rank at most holds a nonzero value at each entry), and each rank gathers its rows from the
 *   table: one collective per control step.  The replicated crown gets the same bits on every rank.
 * Errors: RN_E_STATE before a first solve, after a batch that failed half-way (until rn_apg_reset), on a context sharded by hand or without a
 *   communicator, and while the algorithm is global FBE or NAMA (their L-BFGS memory belongs to the unshifted duals); RN_E_ARG for a rootChild
 *   out of range, a map of another size or with an entry outside [-1, nodes).  Memory: the first shift allocates two ints per local node (on a
 *   shard the whole tree's table, (2 nx + nu + 1) doubles per node, as well) and keeps them; a context that never shifts allocates nothing. */
int rn_shift_warm_start(rn_ctx *ctx, int rootChild);
int rn_set_shift_map(rn_ctx *ctx, size_t nodes, const int *map /* [nodes] or NULL */);
int rn_get_shift_map(rn_ctx *ctx, int rootChild, size_t nodes, int *map /* [nodes] */);

/* ---- the dual Lipschitz constant, estimated on the device ---------------------------------------------------------------------------
 * APG's step size must be margin / L with L = lambda_max(M), M = K H^-1 K' the dual Hessian of the operators the context holds.  The
 * reference has no counterpart: its stepSize is a figure computed offline (MATLAB) and written into the configuration file.  Here the
 * context estimates L of what it HOLDS -- caller-owned blocks, re-weighted probabilities and fp32-stored blocks included -- by power
 * iteration over its Hessian sweep (the linear map of rn_compute_hessian_oracle).  With w_0 = the start vector, for k = 1 .. maxIterations:
 *     s = <w, w> ;  t = <v, w> (k >= 2) ;  v = w / sqrt(s) ;  w = M v
 * and record j (j = 1 .. iterations run), formed from the w of application j: NORM = sqrt(s) (<= lambda_max), RAYLEIGH = |t| (<= NORM),
 * RESIDUAL = sqrt(max(s - t^2, 0)) / sqrt(s) = |w - rho v| / |w| for the unit v.  `out` is the last record plus the number of
 * applications run; `history` (may be NULL) receives all records.  The estimate is a LOWER bound of L -- hence the margin of the step
 * rule -- and RESIDUAL says how far the iteration is from an eigenvector; a tree with single-child stages can make 40 iterations undershoot.
 * Start vector: startXi / startPsi in the layout of rn_set(RN_BUF_XI / RN_BUF_PSI), or both NULL for the library's own: the element in
 *   column c (c < 2 nx: xi; 2 nx + j: psi) of the node with index g in the WHOLE tree is, with i = g (2 nx + nu) + c in unsigned 64-bit
 *   arithmetic,  x = seed + (i + 1) 0x9E3779B97F4A7C15;  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;
 *   x ^= x >> 31;  value = (double)(x >> 11) 2^-52 - 1,  rounded to the context's type: a shard starts from the one-GPU context's vector.
 * Arithmetic: sums in fp64 (fp32 contexts too), fixed order, no atomics: two calls return the same bits.  No host synchronisation between
 *   iterations: tol == 0 runs exactly maxIterations applications with one synchronisation at the end; tol > 0 reads the latest record every
 *   checkEvery iterations (<= 0: 20) and stops when RESIDUAL <= tol.  s - t^2 is formed in fp64, so RESIDUAL has a cancellation floor near
 *   sqrt(n 2^-53): a tolerance below about 1e-6 cannot be met.
 * State: a call between any two entry points leaves every RN_BUF_* buffer, the L-BFGS memory, the history and the batch state untouched;
 *   it needs rn_factor_step only (not the affine terms), under every algorithm, operator mode and storage type.  The first call allocates
 *   buffers of its own (about 2 (2 nx + nu) + nx + nu + nv reals per node, rn_device_memory_info) and keeps them; a context that never asks
 *   allocates and launches nothing.  Sharded contexts (rn_create_sharded): every rank calls; all ranks hold the same bits.
 * Errors: RN_E_STATE before rn_factor_step, after a batch that failed half-way (until rn_apg_reset), on a shard of several ranks without a
 *   communicator; RN_E_ARG for maxIterations < 1, a negative or NaN tol, exactly one start pointer, a NULL out, or a start vector whose
 *   norm is 0 or not finite (seen in the first record).
 * rn_get_lipschitz: the record held and whether it is stale: rn_factor_step, rn_set_operator, rn_set_operators[_device],
 *   rn_set_operator_storage and rn_set_tree_data[_device] with probabilities mark it stale (bounds, tree errors alone, forecasts and the
 *   state do not enter M).  RN_E_STATE if none was ever computed. */
enum { RN_LIP_NORM = 0, RN_LIP_RAYLEIGH, RN_LIP_RESIDUAL, RN_LIP_ITERATIONS, RN_LIP_COLS };
int rn_estimate_lipschitz(rn_ctx *ctx, int maxIterations, double tol, int checkEvery,
                          const double *startXi /* nodes*2nx or NULL */, const double *startPsi /* nodes*nu or NULL */,
                          unsigned long long seed, double out[RN_LIP_COLS], double *history /* [maxIterations][3] or NULL */);
int rn_get_lipschitz(rn_ctx *ctx, double out[RN_LIP_COLS], int *stale);
/* The step size from the estimate (opt-in).  RN_STEP_FIXED (default): stepSize is rn_set_parameters', nothing is launched.
 * RN_STEP_LIPSCHITZ: rn_control_action, rn_algorithm_apg, rn_apg_solve and rn_algorithm_global_fbe / rn_algorithm_nama estimate on entry
 * when no estimate is held or the held one is stale (`iterations` applications, <= 0: 40; the library's start, seed 0) and run with
 * stepSize = margin / NORM, margin in (0, 1]; the penalties are rn_set_parameters'.  rn_set_parameters' own step size is kept and returns
 * with RN_STEP_FIXED.  rn_get_step_rule: any pointer may be NULL; stepSizeInForce is what the next iteration would use. */
enum { RN_STEP_FIXED = 0, RN_STEP_LIPSCHITZ = 1 };
int rn_set_step_rule(rn_ctx *ctx, int rule, double margin /* (0,1] */, int iterations /* <=0: 40 */);
int rn_get_step_rule(rn_ctx *ctx, int *rule, double *margin, int *iterations, double *stepSizeInForce);

/* ---- the solve certificate: dual bound and optimality gap of the multiplier at hand ---------------------------------------------------
 * Extension.  Built on the reference's solveStep (SmpcController.cu:563-755: the minimiser of the Lagrangian), proximalFunG (:759-835: the
 * sets and penalties of g) and computeValueFbe (:1066-1146: the primal terms sum_i p_i (du' W du + alpha' u)); the reference itself reports
 * no bound.  In the scaled space of the sweep and the prox (DESIGN.md "the solve certificate"): f(z) = sum_i p_i (du_i' W du_i + alpha_i' u_i) on
 * the dynamics, Hz = (F_i x_i, G_i u_i), g = gamma_x dist(., [xmin, xmax]) + gamma_s dist(., {>= xs}) + indicator of [umin, umax], both
 * distances tree-global.  y = (xi_b, xi_s, psi) is the multiplier the context would warm-start from: what rn_get(RN_BUF_UPD_XI / _UPD_PSI)
 * shows.  z(y) is the minimiser of the Lagrangian at y: one sweep at y, on the context's stream, in the operator form in force.
 *   COST    f(z(y))                                  INNER   <xi, F x> + <psi, G u>
 *   SUPPORT sum max(xi_b xmin, xi_b xmax) + sum xi_s xs + sum max(psi umin, psi umax)
 *   DUAL    COST + INNER - SUPPORT: a lower bound of the optimal value when VALID = 1
 *   NORM_X  |xi_b|_2   NORM_S  |xi_s|_2   XIS_POS  max(xi_s, 0) over all entries
 *   VALID   1 when NORM_X <= gamma_x (1 + 4 2^-53 sqrt(n)), the same for NORM_S with gamma_s, and XIS_POS <= 2^-53 NORM_S (n: entries of one
 *           half over the whole tree); else 0 -- y is outside the domain of g* -- and DUAL is still the number above, never -inf
 *   DIST_X, DIST_S  distances of Hz(y) from the two x sets    PRIMAL  COST + gamma_x DIST_X + gamma_s DIST_S
 *   U_EXCESS  largest violation of the u box by u(y), physical units, on the bounds table in force (rn_set_bounds)
 *   GAP     PRIMAL - DUAL: an upper bound of the suboptimality of z(y) ONLY when U_EXCESS = 0 (and VALID = 1)
 *   ABS_TERMS  sum of the absolute values of the terms of COST (per node: p_i |alpha_i' u_i| + p_i |du_i' W du_i|), INNER and SUPPORT (per
 *           entry): the scale on which DUAL, PRIMAL and GAP are judged
 * The scaled bounds are formed as the dual update forms them (sqrt(p_i) d_c times the row of the table in force, in the context's type);
 * gamma_x, gamma_s are rn_set_parameters' penalties.  After rn_apg_reset, before any iteration, y = 0: DUAL is the unconstrained minimum.
 * Arithmetic: every product and sum in fp64 whatever the context's precision, one fixed order (k_certificate, k_plan.hpp; COST: a node's
 *   terms as rn_plan_report's node phase sums them, then the nodes), no floating-point atomics: two calls give the same bits.
 * State: the call leaves every other RN_BUF_*, the batch state, the history and the checkpoints bit for bit; the next rn_apg_iterate continues
 *   as if it had not happened.  It does change what rn_algorithmic_bytes / rn_debug_stream_live report as "the most recent launch" (the
 *   sweep at y is one).  The first call allocates buffers of the certificate's own (about 2 nx + 2 nu + nv + 9 reals per node) and keeps them;
 *   later calls allocate nothing, a context that never asks allocates and launches nothing.  RN_BUF_CERT_X / RN_BUF_CERT_U hold x(y), u(y) afterwards.
 * rn_solve_certificate synchronises once; rn_solve_certificate_device leaves the record (RN_CERT_COLS doubles, device memory, valid until
 *   the next certificate on this context) and does not synchronise.
 * Sharded contexts: every rank calls; the sums are all-reduced with the replicated crown counted on one rank, U_EXCESS and XIS_POS by MAX;
 *   every rank holds the same bits.
 * Errors: RN_E_STATE before the affine terms of a control step exist or before rn_apg_reset, after a batch that failed half-way, on a cut
 *   context of several ranks without a communicator, and while the algorithm is global FBE or NAMA (their multiplier is another buffer). */
enum { RN_CERT_DUAL = 0, RN_CERT_PRIMAL, RN_CERT_GAP, RN_CERT_COST, RN_CERT_INNER, RN_CERT_SUPPORT, RN_CERT_DIST_X, RN_CERT_DIST_S,
       RN_CERT_U_EXCESS, RN_CERT_NORM_X, RN_CERT_NORM_S, RN_CERT_XIS_POS, RN_CERT_ABS_TERMS, RN_CERT_VALID, RN_CERT_COLS = 16 };
int rn_solve_certificate(rn_ctx *ctx, double out[RN_CERT_COLS]);
int rn_solve_certificate_device(rn_ctx *ctx, void **record);

/* step-wise entry points mirroring the protected methods the reference's known-answer tests call */
int rn_dual_extrapolation_step(rn_ctx *ctx, double lambda); /* SmpcController.cu:535-557  */
int rn_solve_step(rn_ctx *ctx);                             /* SmpcController.cu:563-755  */
int rn_proximal_fun_g(rn_ctx *ctx);                         /* SmpcController.cu:759-835  */
int rn_compute_fixed_point_residual(rn_ctx *ctx);           /* SmpcController.cu:839-850  */
int rn_dual_update(rn_ctx *ctx);                            /* SmpcController.cu:854-864  */
int rn_update_primal_infeasibility(rn_ctx *ctx, double *value); /* SmpcController.cu:1480-1496 */
/* tree-global distances computed by the last prox (SmpcController.cu:792,810) */
int rn_get_prox_distances(rn_ctx *ctx, double *distanceXcst, double *distanceXs);

/* ---- SmpcController: the global-FBE and NAMA loops --------------------- */
/* Engine's algorithm flags (Engine.cu:151-163, "algorithmName" of the controller configuration).  Selecting FBE or
 * NAMA allocates their vectors and the L-BFGS buffers (SmpcController::allocateGlobalFbeAlgorithm /
 * allocateNamaAlgorithm / allocateLbfgsBuffer, SmpcController.cu:234-330) and runs rn_fbe_reset.  On a sharded context
 * (rn_create_sharded) every dot product, value term and prox distance of the loops is all-reduced over the ranks (the
 * replicated crown counted once), so all ranks take the same skip / line-search decisions. */
enum { RN_ALG_APG = 0, RN_ALG_GLOBAL_FBE = 1, RN_ALG_NAMA = 2 };
int rn_set_algorithm(rn_ctx *ctx, int algorithm, int lbfgsBufferSize);
/* SmpcController::initialiseAlgorithm (FBE / NAMA part, :436-449) + initaliseLbfgBuffer (:453-468) */
int rn_fbe_reset(rn_ctx *ctx);
/* SmpcController::algorithmGlobalFbe (:1529-1555) or algorithmNama (:1559-1586), whichever is selected.
 * primalInfs[maxIterations] = vecPrimalInfs, valueFbe / tau [maxIterations-1] = vecValueFbe / vecTau (may be NULL). */
int rn_algorithm_fbe_nama(rn_ctx *ctx, int maxIterations, double *primalInfs, double *valueFbe, double *tau);
/* step-wise entry points (the reference's known-answer tests call these protected methods);
 * rn_dual_update takes the FBE / NAMA branch (SmpcController.cu:866-880) once one of them is selected */
int rn_compute_hessian_oracle(rn_ctx *ctx);                 /* computeHessianOracalGlobalFbe          :884-1055  */
int rn_compute_gradient_fbe(rn_ctx *ctx);                   /* computeGradientFbe                     :1077-1097 */
int rn_update_fixed_point_residual_nama(rn_ctx *ctx);       /* updateFixedPointResidualNamaAlgorithm  :1060-1072 */
int rn_compute_lbfgs_direction(rn_ctx *ctx);                /* computeLbfgsDirection                  :1103-1237 */
int rn_update_lbfgs_buffer(rn_ctx *ctx);                    /*   its first half:  updateLbfgsBuffer   :1103-1169 */
int rn_two_loop_recursion_lbfgs(rn_ctx *ctx);               /*   its second half: twoLoopRecursionLbfgs :1175-1229 */
int rn_compute_value_fbe(rn_ctx *ctx, double *value);       /* computeValueFbe                        :1416-1476 */
int rn_line_search_lbfgs_update(rn_ctx *ctx, double valueFbeY, double *tau);     /* computeLineSearchLbfgsUpdate    :1242-1305 */
int rn_line_search_ame_lbfgs_update(rn_ctx *ctx, double valueAmeY, double *tau); /* computeLineSearchAmeLbfgsUpdate :1311-1414 */
/* How the line searches ran (both loops evaluate the trials tau = 1, 1/2, 1/4 ... of SmpcController.cu:1272-1300 in batches of six
 * candidates -- two passes and one read-back per batch instead of eight launches and two read-backs per trial; identical tau):
 * out = {line searches, candidate batches evaluated, searches that ran trial by trial (a candidate's prox tripped the
 * soft-constraint branch, or the batch kernel's LDS tile does not fit), NAMA iterations whose two Hessian oracles (:1331, :1341-1345)
 * shared one pass over the operator blocks} */
int rn_fbe_counters(rn_ctx *ctx, long out[4]);
/* lbfgsBufferCol / lbfgsBufferMemory / lbfgsBufferHessian and lbfgsBufferRho (lbfgsBufferSize + 1 entries, the
 * reference addresses entries 1..lbfgsBufferSize; rho may be NULL): get (set = 0) or set (set = 1) */
int rn_lbfgs_state(rn_ctx *ctx, int set, int *col, int *mem, double *H, double *rho);
/* one column (0..lbfgsBufferSize) of devLbfgsBufferMatS (which = 0) / MatY (which = 1), nodes*(2nx+nu) reals in the
 * reference's order (all xi, then all psi) */
int rn_lbfgs_column(rn_ctx *ctx, int set, int which, int col, double *host, size_t n);

/* ---- raw access (tests, closed loop) ------------------------------------------------------------- */
size_t rn_buffer_size(const rn_ctx *ctx, int buffer_id); /* element count, 0 for a bad id */
int rn_get(rn_ctx *ctx, int buffer_id, double *host, size_t n);
int rn_set(rn_ctx *ctx, int buffer_id, const double *host, size_t n);
/* elements [first, first + n) only (e.g. the nx reals of node 0: first = 0, n = nx); dual-shaped buffers (RN_BUF_XI ...
 * RN_BUF_UMAX and the FBE vectors) are addressed in whole nodes (first and n multiples of the per-node dimension) */
int rn_get_range(rn_ctx *ctx, int buffer_id, size_t first, size_t n, double *host);
int rn_set_range(rn_ctx *ctx, int buffer_id, size_t first, size_t n, const double *host);
/* one node's operator block, reference layout (col-major, ld = nv): the values as stored (RN_STORE_F32: fp32-representable doubles) */
int rn_get_operator(rn_ctx *ctx, int op_id, int node, double *host, size_t n);
/* ... and its counterpart: a block handed in by the caller (the reference's Engine returns the device pointers of these arrays,
 * Engine.cuh:170-230 getMatPhi() ... getPtrMatF(), so its callers may overwrite any block).  RN_OP_PHI, _PSI, _D, _F of one node -- the
 * blocks solveStep multiplies with (SmpcController.cu:617-638); the next sweep uses them.  After rn_factor_step; a later rn_factor_step
 * recomputes every block, and so does a later rn_set_tree_data / rn_set_tree_data_device that gives probNode.  RN_OPS_AUTO contexts switch to dense storage on the first call; RN_OPS_STRUCTURED contexts (no per-node
 * blocks by request): RN_E_STATE.  Omega_i, Theta_i, G_i are shared matrices scaled by p_i here (K identical copies in the reference,
 * Engine.cu:306-308): RN_E_ARG.  A context with RN_STORE_F32 blocks rounds the caller's values to the nearest fp32 on upload.
 * Block entries must be finite.  The sweep does not read the operator columns whose entry of the dual vector is zero -- in spans of G columns
 * (rn_get_kernel_info), and only spans in which every entry is +-0: for finite blocks that changes no bit of any result; an Inf / NaN entry in
 * such a column, which used to turn the node's products into NaN (Inf * 0), is not seen and the sums stay finite. */
int rn_set_operator(rn_ctx *ctx, int op_id, int node, const double *host, size_t n);
/* ALL per-node blocks in one call, as the reference's four arrays (Engine.cuh getMatPhi(), getMatPsi(), getMatD(), getMatF(): devMatPhi
 * and devMatD are [node][2nx columns][nv], devMatPsi and devMatF [node][nu columns][nv], col-major, ld = nv, Engine.cu:166-205) -- for
 * a caller whose blocks change with every control step: rn_set_operator costs two blocking copies of a whole block per call, these
 * one kernel (k_pack_operators) that re-strides the arrays into (or out of) the interleaved block layout with the storage type's rounding
 * (RN_STORE_F32: to nearest fp32, the bits rn_set_operator stores).  Any of the four pointers may be NULL: on a set that operator's rows
 * keep their bits, on a get it is skipped; all four NULL: RN_E_ARG.  `nodes` must be the context's node count (the LOCAL one of a sharded
 * context, rows in the order of rn_shard_global_nodes): otherwise RN_E_ARG.  State rules are rn_set_operator's: before rn_factor_step
 * RN_E_STATE; a set on an RN_OPS_STRUCTURED context RN_E_STATE; an RN_OPS_AUTO context becomes dense on its first set (that one call
 * allocates the blocks and synchronises); a later rn_factor_step recomputes every block.  The get forms read stored blocks: a context
 * that runs the structured form has none -- RN_E_STATE, rn_get_operator evaluates one node's block there.
 *   rn_set_operators / rn_get_operators: host arrays of doubles.  The kernel runs behind a device staging buffer of at most 64 MiB (one
 *     node's arrays if they are larger), whole nodes per chunk, allocated and freed inside the call -- rn_device_memory_info's info[2] is
 *     the same before and after.  They synchronise, as rn_set / rn_get do.
 *   rn_set_operators_device / rn_get_operators_device (Engine.cuh getMatPhi() ... getMatF() written or read by a kernel of the caller's):
 *     arrays in device memory, elements of type `precision` (RN_F32 floats, RN_F64 doubles, whatever the context's own precision and
 *     storage are; any other value: RN_E_ARG).  One launch on the context's stream, no host synchronisation, no allocation: the next
 *     sweep on that stream uses the new blocks, and the caller orders its own producer (or consumer) against the stream exactly as
 *     rn_device_pointer describes (rn_stream).  Every non-NULL pointer is checked with hipPointerGetAttributes before anything is
 *     launched: memory of the context's device, aligned to its element type and, where the runtime knows the allocation, long enough --
 *     otherwise RN_E_ARG; a host pointer never reaches the kernel. */
int rn_set_operators(rn_ctx *ctx, size_t nodes, const double *phi, const double *psi, const double *D, const double *F);
int rn_get_operators(rn_ctx *ctx, size_t nodes, double *phi, double *psi, double *D, double *F);
int rn_set_operators_device(rn_ctx *ctx, size_t nodes, int precision, const void *phi, const void *psi, const void *D, const void *F);
int rn_get_operators_device(rn_ctx *ctx, size_t nodes, int precision, void *phi, void *psi, void *D, void *F);
/* The raw device pointer of a buffer that the library keeps in the reference's own layout -- the counterpart of the reference's raw
 * getters and protected device vectors for those arrays (Engine.cuh:108-318 getVecUhat / getVecBeta / getVecE / getPriceAlpha ...,
 * SmpcController.cuh:336-462 devVecX / devVecU / devVecV): RN_BUF_X, _U, _V, _UHAT, _E, _BETA, _ALPHA, _XDIR, _UDIR, node-major
 * [node][dim].  *precision = RN_F64 / RN_F32 (the element type is the context's), *n = element count.  The pointer stays valid until
 * rn_destroy; its contents are those of the last call that has COMPLETED on the context's stream (rn_synchronize, or order your own
 * work behind rn_stream).  x, u, v are stored by the last iteration of a batch and by every step-wise call.  (In the structured operator
 * mode v feeds nothing inside the solver and is normally computed when rn_get asks for it; asking for ITS raw pointer switches the context
 * to computing it with every such iteration, so the sentence before holds for the pointer's whole life.)
 * The scaled bounds RN_BUF_XMIN, _XMAX, _XS, _UMIN, _UMAX (Engine.cuh:294-314 getSysXmin ... getSysUmax) are kept interleaved in the dual
 * layout; the first request for one of them (after rn_factor_step) makes node-major copies of all five in the reference's layout
 * ((3 nx + 2 nu) reals per node: this call allocates), which every later rn_factor_step refreshes.  The dual iterates (RN_BUF_XI ...
 * RN_BUF_RES_PSI) and the operator blocks are kept in other layouts: RN_E_ARG, use rn_get / rn_get_operator. */
int rn_device_pointer(rn_ctx *ctx, int buffer_id, void **devPtr, size_t *n, int *precision);

/* ---- measurement --------------------------------------------------------------------------------- */
/* per-kernel-class device time accumulated by hipEvents when profiling is on (costs a little; off by default).
 * classes: 0 backward sweep, 1 forward sweep, 2 fused dual update, 3 bookkeeping. ms[] receives the totals,
 * launches[] the launch counts since the last rn_profile_reset. */
int rn_profile_enable(rn_ctx *ctx, int on);
int rn_profile_reset(rn_ctx *ctx);
int rn_profile_read(rn_ctx *ctx, double ms[4], long launches[4]);
/* sharded contexts: device time between hipEvents recorded on the solver's stream around every all-reduce (RCCL or an installed
 * stand-in) since the last rn_profile_reset -- wire latency plus the wait for the slowest peer; these intervals lie INSIDE
 * class 1 of rn_profile_read. */
int rn_profile_read_collective(rn_ctx *ctx, double *ms, long *launches);
/* algorithmic HBM bytes of ONE launch of the dominant kernels, as defined in DESIGN.md (RN_STORE_F32 blocks under fp64 iterates: the
 * block entries at 4 bytes, the vectors at 8).  backwardStageBytesTotal: the streaming sweep reads only the operator spans (G consecutive
 * columns, rn_get_kernel_info) that meet a nonzero entry of the dual vector, so its block bytes are a property of the data -- the figure is that of
 * the context's MOST RECENT streaming launch: live whole spans x G x LD x bytes per block entry (LD: the column's rows padded to 16 bytes), a live
 * ragged last span at its ny % G columns, plus the vectors (ny + 2 nv + nx reals per node).  Before the first sweep of a context the dense figure
 * (every column of every block).  Synchronises the context's stream and copies one small record per workgroup. */
int rn_algorithmic_bytes(const rn_ctx *ctx, double *backwardStageBytesTotal, double *dualUpdateBytes);
/* which kernels an iteration of this context launches: info = {1 if k_dual_stage is the main pass of the fused dual update
 * (0: the flat k_dual_fused), its workgroups, vectors per thread, pipeline depth, k_stream_gemv columns per span, slots per
 * thread and span, first chain stage c*, 1 if the v / Lv products run as the fused slab kernel k_gemm_vlv -- 2 or 3 once a sweep
 * has chosen k_gemm_vlv_wide with that many slabs per workgroup} */
int rn_get_kernel_info(rn_ctx *ctx, int info[8]);
/* streaming ceilings of THIS device measured with do-nothing kernels (16 B per lane per load, non-temporal): flat
 * grid-stride read-only GB/s and copy GB/s (read + written bytes), best of `reps` passes over `bytes`.
 * bench.py reports them beside the 8 TB/s spec peak as the practical denominator. */
int rn_measure_hbm(rn_ctx *ctx, size_t bytes, int reps, double *readGBs, double *copyGBs);
/* the context's stream as a hipStream_t (void* to keep HIP types out of this header) */
void *rn_stream(rn_ctx *ctx);

/* ---- multi-GPU: subtree sharding with one RCCL all-reduce at the cut per iteration ---------------- */
/* see DESIGN.md "multi-GPU"; ncclUniqueId bytes are produced by rn_comm_unique_id on rank 0 and
 * distributed by the caller (bench.py uses torch.distributed for that). */
int rn_comm_unique_id(void *id128 /* 128 bytes out */);
/* id128 == NULL records rank / nranks without creating a communicator (the exchange is then a test's job, rapidnet_debug.h).
 * ncclCommInitRank waits for every rank of the id; it runs on a helper thread and the caller waits against the wall clock: a rank
 * whose peers do not arrive within the time-out ($RAPIDNET_COMM_TIMEOUT_S, default 120 s; rn_comm_init_timeout: `timeoutSeconds`)
 * gets RN_E_COMM back -- never a hang (the reference exits on any failure, Configuration.h:38-81) -- and the context stays usable
 * without a communicator. */
int rn_comm_init(rn_ctx *ctx, int rank, int nranks, const void *id128);
int rn_comm_init_timeout(rn_ctx *ctx, int rank, int nranks, const void *id128, double timeoutSeconds);
/* asynchronous errors of the communicator (ncclCommGetAsyncError: a peer died, a link went down): RN_E_COMM if RCCL reports one.
 * The library asks once per batch of rn_apg_iterate by itself. */
int rn_comm_check(rn_ctx *ctx);
/* Path of the RCCL image the library bound (an image the process has already loaded -- e.g. the one PyTorch links --
 * is reused, never a second copy), written as a C string into buf; RN_E_COMM when RCCL cannot be loaded. */
int rn_comm_library(char *buf, size_t n);
/* stage c of the (rank-local) tree whose nodes are the roots of the sharded subtrees: the children sums of the
 * stage c-1 nodes (replicated on every rank) are all-reduced once per iteration; -1 switches sharding off. */
int rn_set_cut_stage(rn_ctx *ctx, int stage);
/* How the tree-global prox distances (SmpcController.cu:792,810) are obtained across ranks.
 *   1 (default) optimistic: the prox runs as a pure projection, every rank's dist^2 of iteration t rides in the tail of
 *     iteration t+1's cut all-reduce and is checked on the device -- ONE collective per iteration; if a threshold is
 *     ever exceeded the batch is replayed from a checkpoint with mode 0, so the result is exact either way;
 *   0 exact: a second 2-element all-reduce per iteration before the trip decision.
 * Single-GPU contexts use the same switch: with 1 (default) a batch of >= 16 iterations runs the prox as a pure projection,
 * the bookkeeping of iteration t (history entry, distance check) rides in a launch of iteration t+1 instead of a decision
 * launch of its own, and the batch is replayed from a checkpoint through the exact path if a distance ever exceeded its
 * threshold; with 0 every iteration decides before the next one starts.  Results are identical. */
int rn_set_exchange_mode(rn_ctx *ctx, int mode);
/* static tree data a shard cannot derive from its local children: for every cut parent i (stage-1 nodes of the cut, in
 * stage order) E_i = sum over ALL children c of p_c * errorDemand_c (nd reals) and P_i = sum_c p_c.  They replace the
 * children loop of calculateZeta (Utilities.cu:100-131) for those nodes: sum_c p_c uhat_c = Lhat (E_i + P_i dhat). */
int rn_set_cut_children_moments(rn_ctx *ctx, const double *E /* parents*nd */, const double *P /* parents */, size_t nParents);
/* per-iteration {max|res_xi|, signed entry, max|res_psi|, signed entry} over THIS RANK's nodes for iterations [first, first+n).
 * (The history rn_apg_iterate returns is tree-global on a sharded context with a communicator: one MAX all-reduce per batch
 * combines the ranks' parts into vecPrimalInfs, SmpcController.cu:1480-1496, :1521.  Without a communicator -- id128 == NULL,
 * the exchange emulated by a test -- it is rank-local and these parts are what the caller combines.) */
int rn_get_history_parts(rn_ctx *ctx, int first, int n, double *out /* 4*n */);
/* Batch bookkeeping of rn_apg_iterate: out = {optimistic batches, exact batches, optimistic batches that were replayed
 * through the exact path because a tree-global prox distance exceeded its threshold, exact batches still to run before the
 * optimistic path is tried again (back-off after a replay)}. */
int rn_get_counters(rn_ctx *ctx, long out[4]);

/* ---- multi-GPU through the boundary: partition + communicator + cut stage in one call --------------------------------
 * The reference is single-GPU: its seam for a whole solver is `Engine(SmpcConfiguration*)` / `SmpcController(string)`
 * (Engine.cuh:68, SmpcController.cuh:57-87).  A sharded solver is created the same way, one per process / GPU, from the
 * FULL scenario tree plus (rank, nranks): the library cuts the tree, keeps the rank's subtrees and
 * the replicated crown, creates the RCCL communicator and installs the static children moments -- the host classes pass
 * rank / nranks straight through (Engine(config, precision, device, rank, nranks, id128)). */

/* First stage at which the tree has all its K scenario chains (the most balanced cut: K subtrees dealt round-robin);
 * max(1, N-1) for a tree that branches until the end.  Negative RN_E_* on bad input. */
int rn_default_cut_stage(const rn_dims *dims, const rn_tree *tree);

/* The rank-local scenario tree of a subtree partition.  Nodes of stages < cutStage (the crown) are replicated on every
 * rank, the subtrees rooted at stage cutStage are dealt round-robin by position; local nodes keep their stage-by-stage
 * order, so a local tree is an ordinary scenario tree (ScenarioTree.cuh:92-154 conventions: 1-based ancestor, nChildren
 * lists the non-leaf nodes -- a cut parent without local children is a local leaf).  All arrays are owned by the
 * partition object and stay valid until rn_partition_destroy. */
typedef struct {
    rn_dims dims;                 /* local: nodes, K (local leaves), nNonLeafNodes; nx..N as given                    */
    rn_tree tree;                 /* local tree arrays                                                                 */
    const int *globalNode;        /* [dims.nodes] index of every local node in the full tree                          */
    const double *errorDemandNode, *errorPriceNode; /* local rows of the full tree's errors (NULL if none were given)  */
    int rank, nranks, cutStage, nCutParents;
    /* static children moments of the cut parents over ALL their children (rn_set_cut_children_moments): the replacement
     * of the children loop of calculateZeta (Utilities.cu:100-131) for nodes whose children live on other ranks */
    const double *momE;           /* [nCutParents][nd]  sum_c p_c errorDemand_c   (NULL if no errors were given)        */
    const double *momP;           /* [nCutParents]      sum_c p_c                                                      */
    void *owner;                  /* internal */
} rn_partition;
int rn_partition_create(const rn_dims *dims, const rn_tree *tree, const double *errorDemandNode /* nodes*nd or NULL */,
                        const double *errorPriceNode /* nodes*nu or NULL */, int rank, int nranks,
                        int cutStage /* <= 0: rn_default_cut_stage */, rn_partition *out);
void rn_partition_destroy(rn_partition *p);

/* rn_create for rank `rank` of `nranks`: partition (above) + rn_create on the local tree + rn_set_tree_errors (local rows)
 * + rn_comm_init + rn_set_cut_stage + rn_set_cut_children_moments.  id128 = the ncclUniqueId of rn_comm_unique_id (rank 0's,
 * distributed by the caller); NULL creates no RCCL communicator (rn_comm_init may follow -- a caller that wants to keep the context when
 * the communicator cannot be created within its time-out does it that way; here a failed set-up destroys the context).
 * nranks == 1 gives a plain unsharded context. */
int rn_create_sharded(const rn_dims *dims, const rn_tree *tree, const double *errorDemandNode, const double *errorPriceNode,
                      int precision, int device, int rank, int nranks, int cutStage, const void *id128, rn_ctx **out);
/* what a sharded context is: info = {rank, nranks, cut stage (-1: none), cut parents, ranks the RCCL communicator itself
 * reports (ncclCommCount; 0 without a communicator), local nodes, nodes of the full tree} */
int rn_shard_info(rn_ctx *ctx, int info[7]);
/* index in the FULL tree of every local node (rn_get returns local node-major arrays); identity for unsharded contexts */
int rn_shard_global_nodes(rn_ctx *ctx, int *globalNode, size_t n);

/* ---- transport of the per-iteration exchange at the cut ----------------------------------------------
 * The reference has no counterpart (single GPU).  What is exchanged is exactly what solveSumChildren computes at the cut
 * (Utilities.cu:168-201): the cut parents' children sums, once per iteration.  Two transports carry it:
 *   RN_EXCHANGE_COLLECTIVE  ncclAllReduce on the solver's stream (RCCL), one launch between the chain walks and the crown;
 *   RN_EXCHANGE_ONESHOT     the kernel that produces a rank's partial sums writes them straight into an inbox on every peer (xGMI peer
 *                           mappings) as self-validating {32 payload bits, 32-bit sequence tag} packets and the same workgroup adds the
 *                           n contributions for its cut parent in rank order (the same bits on every rank): no collective launch, no
 *                           launch boundary.  The per-BATCH collectives (dist^2 tail, verdict + history) stay with the communicator.
 *   RN_EXCHANGE_AUTO        (the default) the context times both on its OWN iterations and keeps the faster: rn_exchange_autotune.
 * Inboxes: with a communicator made by rn_comm_init / rn_create_sharded the library allocates this rank's inbox (uncached device
 * memory), gathers the hipIpcMemHandle_t of all ranks over the communicator and maps the peers' inboxes by itself, unless the
 * transport was fixed to RN_EXCHANGE_COLLECTIVE before; if any rank cannot, all ranks agree to do without (AUTO then has one
 * candidate).  rn_peer_inbox_create / rn_peer_inbox_connect do the same with handles the caller distributes.  A reader that waits
 * longer than 2 s ($RAPIDNET_ONESHOT_TIMEOUT_MS) for a peer's packets gives up: the batch returns RN_E_COMM (never a hang) on every
 * rank (the flag rides in the per-batch MAX all-reduce).  rn_peer_inbox_connect is once per context.  $RAPIDNET_EXCHANGE =
 * collective | oneshot | auto sets the default of contexts that were not told.  (Tests wire the inboxes of contexts of one process:
 * rapidnet_debug.h.) */
enum { RN_EXCHANGE_COLLECTIVE = 0, RN_EXCHANGE_ONESHOT = 1, RN_EXCHANGE_AUTO = 2 };
int rn_peer_inbox_create(rn_ctx *ctx, void *ipcHandle64 /* 64 bytes out */);
int rn_peer_inbox_connect(rn_ctx *ctx, const void *ipcHandles /* nranks x 64 bytes, rank order */, int nranks);
int rn_set_exchange_transport(rn_ctx *ctx, int transport);
/* The exchange chooses itself.  iterations > 0: every rank of the communicator calls this at the same point (after the factor step and
 * the affine terms); each candidate transport runs `iterations` device-resident APG iterations of the context (after a warm-up run of
 * half as many) from the current iterates, which are restored afterwards -- the dual iterates (y, y+, w), the iteration count and the
 * batch counters are what they were (the output buffers x, u, v, z, res hold the tuner's last iteration until the next batch writes
 * them); the ranks' times are combined by a MAX all-reduce, so every rank keeps the same transport.  A context whose transport is AUTO
 * does this by itself in its first device-resident batch (min(max(n, 20), 100) iterations).  iterations == 0: report only.
 * info = {transport in use (0 / 1), candidates timed (bit 0 collective, bit 1 one-shot), microseconds per iteration with the
 * collective (max over ranks), with the one-shot exchange (max over ranks; -1: it failed on a rank; 0: not a candidate), this rank's
 * own two figures, iterations per candidate, tunes run so far}. */
int rn_exchange_autotune(rn_ctx *ctx, int iterations, double info[8]);
/* The forward walk and the fused dual update of the nodes it has just walked in ONE launch (k_down_chain_dual: Hx stays in LDS between
 * the two; SmpcController.cu:676-747 + :759-864 per node) inside batches of >= 16 iterations; identical iterates (bitwise).
 * on = -1 (default): on, shaped by the context -- one workgroup per scenario chain where the (rank-local) tree has at least 3/4 as many chains as
 * the device has compute units (the 493-scenario tree: 2 % faster per iteration, 5.6 % in structured mode), up to four per chain -- each updating
 * the dual of its own slice of the chain's nodes -- on small trees and small shards (1-4 % faster; with one per chain those measured 3-4 % slower);
 * 0 / 1: off / on whenever the shape allows it.  $RAPIDNET_FUSE_DOWN_DUAL = 0 / 1 sets the default of contexts that were not told.  While
 * rn_profile_enable is on the dual update always runs as a launch of its own. */
int rn_set_fused_walk_dual(rn_ctx *ctx, int on);
/* Device-buffer guard mode ("race detection / sanitizers": no GPU address sanitizer exists on this pool).
 * With RAPIDNET_GUARD=1 in the environment when a context is created, every device buffer of the context gets a 128 KiB red
 * zone on both sides; red zones and payloads of floating-point buffers start as NaN (0xFF bytes), so an out-of-bounds or
 * uninitialised READ carries a NaN into the iterates, and an out-of-bounds WRITE changes a red zone: rn_guard_check counts the
 * red-zone bytes that no longer hold their pattern (0 outside guard mode); rn_destroy reports them on stderr. */
int rn_guard_check(rn_ctx *ctx, long *badBytes);
/* process-wide tally of the checks rn_destroy makes in guard mode: out = {contexts checked so far, red-zone bytes found overwritten} */
int rn_guard_report(long out[2]);

#ifdef __cplusplus
}
#endif
#endif /* RAPIDNET_H_ */
