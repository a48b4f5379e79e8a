// Engine.hpp -- the reference's Engine class surface (src/Engine.cuh:49-358) over the C-ABI of include/rapidnet.h.
// The reference's Engine owns ~60 raw device arrays and hands out device pointers; here the device state lives behind
// an opaque rn_ctx and the getters copy to the host on demand (node-major, the reference's layout):
//   reference getter returning a device pointer        here
//   getVecUhat() / getVecBeta() / getVecE() ...         getBuffer(RN_BUF_UHAT, host) ...  -- or, for the arrays the library keeps in the
//                                                       reference's own node-major layout, the raw device pointer under the
//                                                       reference's name: getVecUhat(), getVecBeta(), getVecE(), getPriceAlpha()
//                                                       (element type = the engine's precision: getDevicePrecision())
//   getMatPhi() / getPtrMatPhi()[node] ...              getOperator(RN_OP_PHI, node, host) ...  (the blocks are stored interleaved: DESIGN.md section 4)
//   getMatPhi() ... getMatF() as whole arrays           setOperators / getOperators (host arrays), setOperatorsDevice / getOperatorsDevice (device arrays)
#ifndef RAPIDNET_ENGINE_HPP_
#define RAPIDNET_ENGINE_HPP_

#include "../../../include/rapidnet.h"
#include "DataModel.hpp"

class Engine {
public:
    // reference: Engine(SmpcConfiguration*) news its own network and tree from the paths in the configuration
    // (Engine.cu:126-132).  precision: RN_F64 (default) or RN_F32; device: HIP device ordinal.
    // operatorMode: how the per-node operator blocks of the factor step (Engine.cu:166-189, :721-745) are kept.  RN_OPS_AUTO: never
    // materialised while they are the factor step's own -- block = shared matrix x stage diagonal x power of p_i, applied as shared-operator
    // products: identical iterates, 32 instead of 335 ms per 500-iteration control step on the 493-scenario tree -- and dense from the
    // first setOperator() on; RN_OPS_DENSE: the reference's storage (one dense block per node, streamed every iteration); RN_OPS_STRUCTURED:
    // never any block.  -1 (default): the configuration file's optional "operatorMode" key ("auto" | "dense" | "structured"; absent: auto).
    explicit Engine(SmpcConfiguration *smpcConfig, int precision = RN_F64, int device = 0, int operatorMode = -1);
    Engine(DwnNetwork *network, ScenarioTree *scenarioTree, SmpcConfiguration *smpcConfig, int precision = RN_F64, int device = 0, int operatorMode = -1);
    // Multi-GPU (new; the reference is single-GPU): rank `rank` of `nranks`, one process and one GPU per rank.  The engine is
    // given the FULL network / tree / configuration exactly as above; the library keeps this rank's subtrees plus the
    // replicated crown (rn_create_sharded: partition below `cutStage`, 0 = the most balanced cut), creates the RCCL
    // communicator from `ncclUniqueId128` (rn_comm_unique_id on rank 0, distributed by the caller; NULL: no communicator, the
    // exchange is a test's job) and all-reduces the cut parents' children sums once per APG iteration.  Everything else --
    // factorStep, updateStateControl, eliminateInputDistubanceCoupling, the controller -- is called as on one GPU; node-major
    // buffers are local (getNumLocalNodes() nodes; getGlobalNodes() maps them to nodes of the full tree).
    Engine(SmpcConfiguration *smpcConfig, int precision, int device, int rank, int nranks, const void *ncclUniqueId128, int cutStage = 0, int operatorMode = -1);
    Engine(DwnNetwork *network, ScenarioTree *scenarioTree, SmpcConfiguration *smpcConfig, int precision, int device, int rank, int nranks,
           const void *ncclUniqueId128, int cutStage = 0, int operatorMode = -1);
    void setOperatorMode(int mode);                  // RN_OPS_AUTO / _DENSE / _STRUCTURED; before factorStep()
    int getOperatorMode();                           // what the engine runs: RN_OPS_DENSE or RN_OPS_STRUCTURED
    // element type of the dense blocks (rapidnet.h, rn_set_operator_storage): RN_STORE_NATIVE or RN_STORE_F32 -- fp32 blocks under fp64 iterates,
    // half the bytes per iteration, every sum in fp64.  The constructors take it from the configuration file's optional "operatorStorage" key
    // ("native" | "f32"; absent: native).  Before factorStep().
    void setOperatorStorage(int storage);
    int getOperatorStorage();                        // RN_STORE_F32 while the engine holds dense blocks in fp32, else RN_STORE_NATIVE
    // NAMA's two Hessian sweeps in one pass over the dense blocks (rapidnet.h, rn_set_sweep_pairing): RN_PAIR_AUTO / _ON / _OFF; _ON adds fp32-stored
    // blocks to what _AUTO pairs.  The constructors take it from the configuration file's optional "sweepPairing" key ("auto" | "on" | "off";
    // absent: auto).  At any time.
    void setSweepPairing(int mode);
    // the APG solve of a control step ends once the primal infeasibility of the last iteration of a batch of `checkEvery` iterations is <= tol
    // (rapidnet.h, rn_set_stop_tolerance; the reference always runs maxIterations, SmpcController.cu:1500-1525).  tol = 0 (the default): off;
    // checkEvery <= 0: the library's default (20).  The constructors take both from the configuration file's optional "stopTolerance" /
    // "stopCheckEvery" keys (absent: off).  At any time; the quasi-Newton loops ignore it.
    void setStopTolerance(real_t tol, int checkEvery = 0);
    real_t getStopTolerance(int *checkEvery = nullptr);
    // adaptive restart of the APG momentum (rapidnet.h, rn_set_restart; the reference's theta recursion is never restarted,
    // SmpcController.cu:1500-1525, :535-557): RN_RESTART_OFF (the default) or RN_RESTART_GRADIENT -- the solve of a control step then runs in
    // batches of the stop tolerance's checkEvery iterations and the gradient test at every batch end decides.  The constructors take it from
    // the configuration file's optional "momentumRestart" key ("off" | "gradient"; absent: off).  At any time; the quasi-Newton loops ignore it.
    void setRestart(int mode);
    int getRestart();
    int getSweepPairing(int *active = nullptr);      // what was asked for; *active: 1 when the next NAMA line search would run the pair
    // a per-node block handed in by the caller (the reference: write through getMatPhi() / getPtrMatPhi()[node] ..., Engine.cuh:170-230);
    // RN_OP_PHI, _PSI, _D, _F, col-major nv x (2nx | nu); after factorStep()
    void setOperator(int opId, uint_t node, const real_t *host, size_t n);
    // ... and all of them at once, as the reference's whole arrays (getMatPhi(), getMatPsi(), getMatD(), getMatF(), Engine.cuh:170-230: [node][2nx | nu
    // columns][nv]; getNumLocalNodes() nodes): rapidnet.h, rn_set_operators.  A null pointer leaves that operator as it is (set) or out (get).
    // Host arrays (these synchronise) ...
    void setOperators(const real_t *phi, const real_t *psi, const real_t *D, const real_t *F);
    void getOperators(real_t *phi, real_t *psi, real_t *D, real_t *F);
    // ... or device arrays of RN_F32 / RN_F64 elements, filled or read by the caller's own kernels: one launch on the engine's stream
    // (rn_stream(getContext())), nothing is waited for
    void setOperatorsDevice(int precision, const void *phi, const void *psi, const void *D, const void *F);
    void getOperatorsDevice(int precision, void *phi, void *psi, void *D, void *F);
    // Scenario probabilities and tree errors replaced in place between two control steps (rapidnet.h, rn_set_tree_data; the reference uploads
    // devTreeProb once, Engine.cu:263-286, and the errors with every control step, Engine.cu:1205,1228): probNode [nodes], errorDemandNode
    // [nodes][nd], errorPriceNode [nodes][nu] of the FULL tree (a sharded engine picks its rows, as its constructor does); a null pointer
    // leaves that array as it is.  With prob given the next eliminateInputDistubanceCoupling (controlAction makes one) has to precede any iteration.
    void setTreeData(const real_t *prob, const real_t *errorDemand, const real_t *errorPrice);
    // ... device arrays of RN_F32 / RN_F64 elements: launches on the engine's stream (rn_stream(getContext())), nothing is waited for
    void setTreeDataDevice(int precision, const void *prob, const void *errorDemand, const void *errorPrice);
    // what the engine holds (getNumLocalNodes() rows, in the order of getGlobalNodes()); a null pointer skips that array
    void getTreeData(real_t *prob, real_t *errorDemand, real_t *errorPrice);
    // pushes the ScenarioTree's current arrays (ScenarioTree::setProbArray ... / reload)
    void updateScenarioTree();
    // Box and safety bounds per stage or per node, replaced in place after factorStep() (rapidnet.h, rn_set_bounds; the reference's callers write
    // through getSysXmin() ... getSysUmax(), Engine.cuh:294-314): physical values, xmin / xmax / xsafe [rows][nx], umin / umax [rows][nu];
    // granularity RN_BOUNDS_SHARED (rows 1), RN_BOUNDS_PER_STAGE (rows N) or RN_BOUNDS_PER_NODE (rows getNumLocalNodes(), in the order of
    // getGlobalNodes()).  A null pointer keeps that array while the granularity stays what it is; factorStep() returns to the network's vectors.
    void setBounds(int granularity, size_t rows, const real_t *xmin, const real_t *xmax, const real_t *xsafe, const real_t *umin, const real_t *umax);
    // ... device arrays of RN_F32 / RN_F64 elements: launches on the engine's stream (rn_stream(getContext())), nothing is waited for and
    // the values are not validated
    void setBoundsDevice(int granularity, size_t rows, int precision, const void *xmin, const void *xmax, const void *xsafe, const void *umin, const void *umax);
    // what the engine holds: the granularity in force (*rows: its row count), and the physical values (rows as getBoundsLayout reports; a null
    // pointer skips that array)
    int getBoundsLayout(size_t *rows = nullptr);
    void getBounds(size_t rows, real_t *xmin, real_t *xmax, real_t *xsafe, real_t *umin, real_t *umax);
    // What the plan the engine holds costs and where it violates its bounds (rapidnet.h, rn_plan_report / rn_plan_report_scenarios: the
    // predictive counterpart over the scenario tree of the reference's closed-loop KPIs, SmpcController.cu:1819-1859).  perStage
    // [stages][RN_PLAN_COLS], perScenario [scenarios][RN_PLAN_COLS], leafNode [scenarios]: the local node of every scenario row (map it
    // through getGlobalNodes() on a shard).  After a solve; on a sharded engine every rank calls it (the per-stage table is the whole tree's).
    struct PlanReport {
        size_t stages = 0, scenarios = 0;
        std::vector<real_t> perStage, perScenario;
        std::vector<int> leafNode;
        real_t stage(size_t k, int column) const { return perStage[k * RN_PLAN_COLS + column]; }
        real_t scenario(size_t l, int column) const { return perScenario[l * RN_PLAN_COLS + column]; }
    };
    size_t getNumLocalScenarios();                   // local nodes at the last stage: the rows of PlanReport::perScenario
    void evaluatePlan(PlanReport &report);
    // Dual bound and optimality gap of the multiplier the engine would warm-start from (rapidnet.h, rn_solve_certificate; the reference reports
    // none): out[RN_CERT_DUAL] is a lower bound of the optimal expected cost when out[RN_CERT_VALID] is 1, out[RN_CERT_GAP] bounds the
    // suboptimality of the plan one gradient step past the last iterate only when out[RN_CERT_U_EXCESS] is 0.  One sweep; the solve goes on as
    // if nobody had asked.  After a solve (APG only); on a sharded engine every rank calls it and all hold the same bits.
    void solveCertificate(real_t out[RN_CERT_COLS]);
    // What the plan looks like across the tree (rapidnet.h, rn_plan_quantiles / rn_plan_paths; the reference has no counterpart): weighted
    // quantiles of every component of x (RN_BAND_X) or u (RN_BAND_U) per stage at `levels`, out [stages][dim][levels]; and the rows along
    // every scenario's path, out [scenarios][stages][dim] with leafNode [scenarios], the node of the whole tree each path ends in.  After
    // a solve; on a sharded engine every rank calls them and receives the whole tree's tables.
    void planQuantiles(int which, const std::vector<real_t> &levels, std::vector<real_t> &out);
    void planPaths(int which, std::vector<real_t> &out, std::vector<int> &leafNode);
    int getRank() { return myRank; }
    int getNumRanks() { return numRanks; }
    uint_t getNumLocalNodes();                       // nodes this rank holds (= the tree's node count on one GPU)
    std::vector<int> getGlobalNodes();               // index in the full tree of every local node
    void eliminateInputDistubanceCoupling(real_t *nominalDemand, real_t *nominalPrices);  // Engine.cu:1147
    void updateStateControl(real_t *currentX, real_t *prevU, real_t *prevDemand);        // Engine.cu:1300
    void factorStep();                                                                    // Engine.cu:671
    // Engine::calculateMatLandMatLhat (Engine.cu:466-669): L = null(E), Lhat = -pinv(E) Ed from the network's E, Ed.
    // By default the factor step uses matL / matLhat of the controller configuration (they are already there,
    // SmpcConfiguration.cu:59-68); after this call it uses the computed ones.  Any orthonormal basis of null(E) gives
    // the same x, u and duals.
    void calculateMatLandMatLhat();
    real_t *getMatL() { return useComputedL ? computedL.data() : ptrMySmpcConfig->getMatL(); }
    real_t *getMatLhat() { return useComputedL ? computedLhat.data() : ptrMySmpcConfig->getMatLhat(); }
    void setWarmStart(bool on);
    // The warm start shifted one stage toward the root (rapidnet.h, rn_shift_warm_start; the reference has no counterpart): between two control
    // steps, the duals of the last solve move up the tree along child number rootChild of the root (-1: its most probable child), scaled to
    // the multiplier per unit of probability; with setWarmStart(true) the next control step starts from them.  The constructors switch the
    // warm start on for the configuration file's optional "warmStart" key "keep" or "shift" (absent or "off": the reference's cold start).
    // setShiftMap: a correspondence of one's own, an entry per node of the whole tree (a node, or -1 for "from zero"); empty: the rule again.
    // On a sharded engine every rank calls shiftWarmStart.
    void shiftWarmStart(int rootChild = -1);
    void setShiftMap(const std::vector<int> &map);
    void getShiftMap(int rootChild, std::vector<int> &map);
    // The dual Lipschitz constant of the operators the engine holds, by power sweeps on the device (rapidnet.h, rn_estimate_lipschitz; the reference
    // takes stepSize from an offline MATLAB figure in the configuration file).  The estimate is a LOWER bound of lambda_max -- hence the margin of
    // the step rule; residual says how far the iteration is from an eigenvector.  After factorStep(); caller-owned blocks, new probabilities and a
    // new factor step make the held estimate stale (getLipschitz).  start: empty for the library's own start vector of `seed`, or xi [nodes][2nx]
    // followed by psi [nodes][nu].  On a sharded engine every rank calls it.
    struct LipschitzEstimate {
        real_t norm = 0, rayleigh = 0, residual = 0;
        uint_t iterations = 0;
        bool stale = false;
        std::vector<real_t> history;      // [iterations][3] when asked for
    };
    LipschitzEstimate estimateLipschitz(int maxIterations = 40, real_t tol = 0, int checkEvery = 0, const std::vector<real_t> &start = std::vector<real_t>(),
                                        unsigned long long seed = 0, bool history = false);
    bool getLipschitz(LipschitzEstimate &held);      // false: none was computed yet
    // RN_STEP_FIXED: the configuration's stepSize; RN_STEP_LIPSCHITZ: margin / norm, estimated on entry of a solve when no estimate is held or it is
    // stale (rapidnet.h, rn_set_step_rule).  The constructors take the rule from the configuration file's optional "stepSizeRule" /
    // "stepSizeMargin" / "lipschitzIterations" keys (absent: fixed, the reference's behaviour).
    void setStepRule(int rule, real_t margin = 0.9, int iterations = 0);
    int getStepRule(real_t *margin = nullptr, int *iterations = nullptr, real_t *stepSizeInForce = nullptr);
    ScenarioTree *getScenarioTree() { return ptrMyScenarioTree; }
    DwnNetwork *getDwnNetwork() { return ptrMyNetwork; }
    SmpcConfiguration *getSmpcConfiguration() { return ptrMySmpcConfig; }
    bool getPriceUncertainty() { return priceUncertaintyFlag; }
    bool getDemandUncertantiy() { return demandUncertaintyFlag; }
    bool getApgFlag() { return apgFlag; }
    bool getGlobalFbeFlag() { return globalFbeFlag; }
    bool getNamaFlag() { return namaFlag; }
    void setPriceUncertaintyFlag(bool inputFlag);
    void setDemandUncertaintyFlag(bool inputFlag);
    // device state access (replaces the raw device-pointer getters)
    rn_ctx *getContext() { return ctx; }
    size_t getBufferSize(int bufferId);
    void getBuffer(int bufferId, real_t *host);
    void setBuffer(int bufferId, const real_t *host);
    void getBufferRange(int bufferId, size_t first, size_t n, real_t *host);         // elements [first, first + n) only
    void setBufferRange(int bufferId, size_t first, size_t n, const real_t *host);
    void getOperator(int opId, uint_t node, real_t *host, size_t n);
    // Raw device pointers under the reference's names (Engine.cuh:108-318) for the arrays whose device layout IS the reference's:
    // [node][dim], valid until the engine is destroyed, contents as of the last completed call (rn_synchronize / rn_stream).  The
    // element type is double for RN_F64 engines (the default) and float for RN_F32 ones -- the reference's real_t is float, this
    // host API's is double, so the pointers are untyped and getDevicePrecision() says which.
    int getDevicePrecision();                           // RN_F64 or RN_F32
    void *getDevicePointer(int bufferId, size_t *n = nullptr);      // RN_BUF_X, _U, _V, _UHAT, _E, _BETA, _ALPHA, _XMIN ... _UMAX (others: std::runtime_error)
    void *getVecUhat() { return getDevicePointer(RN_BUF_UHAT); }   // Engine.cuh: getVecUhat
    void *getVecBeta() { return getDevicePointer(RN_BUF_BETA); }   //             getVecBeta
    void *getVecE() { return getDevicePointer(RN_BUF_E); }         //             getVecE
    void *getPriceAlpha() { return getDevicePointer(RN_BUF_ALPHA); }   //         getPriceAlpha
    // the scaled bounds (Engine.cuh:294-314; after factorStep()): node-major copies in the reference's layout, made by the first call of any of the five
    void *getSysXmin() { return getDevicePointer(RN_BUF_XMIN); }   //             getSysXmin
    void *getSysXmax() { return getDevicePointer(RN_BUF_XMAX); }   //             getSysXmax
    void *getSysXs() { return getDevicePointer(RN_BUF_XS); }       //             getSysXs
    void *getSysUmin() { return getDevicePointer(RN_BUF_UMIN); }   //             getSysUmin
    void *getSysUmax() { return getDevicePointer(RN_BUF_UMAX); }   //             getSysUmax
    void *getVecX() { return getDevicePointer(RN_BUF_X); }         // SmpcController.cuh: devVecX (protected there; public here for GPU-side consumers)
    void *getVecU() { return getDevicePointer(RN_BUF_U); }         //                     devVecU
    void *getVecV() { return getDevicePointer(RN_BUF_V); }         //                     devVecV
    ~Engine();

private:
    void create(int precision, int device, int operatorMode, int rank = 0, int nranks = 1, const void *id128 = nullptr, int cutStage = 0);
    int myRank = 0, numRanks = 1;
    void check(int rc, const char *what);
    DwnNetwork *ptrMyNetwork;
    ScenarioTree *ptrMyScenarioTree;
    SmpcConfiguration *ptrMySmpcConfig;
    rn_ctx *ctx;
    bool priceUncertaintyFlag, demandUncertaintyFlag, apgFlag, globalFbeFlag, namaFlag;
    bool useComputedL = false;
    std::vector<real_t> computedL, computedLhat;
};

#endif
