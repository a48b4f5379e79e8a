// SmpcController.hpp -- the reference's SmpcController class surface (src/SmpcController.cuh:42-259) over the C-ABI.
// Public methods keep the reference's names, arguments and return values; the protected step methods (the seam the
// reference's known-answer tests subclass into, TestSmpcController.cuh:80) forward one-to-one to rn_* entry points.
// The reference's protected raw device vectors (devVecXi ...) are replaced by getVector / setVector with RN_BUF_* ids.
#ifndef RAPIDNET_SMPCCONTROLLER_HPP_
#define RAPIDNET_SMPCCONTROLLER_HPP_

#include "Engine.hpp"

class SmpcController {
public:
    SmpcController(Forecaster *myForecaster, Engine *myEngine, SmpcConfiguration *mySmpcConfig);
    // operatorMode: Engine.hpp (RN_OPS_AUTO / _DENSE / _STRUCTURED; -1 = the configuration file's optional "operatorMode" key, absent: auto)
    explicit SmpcController(string pathToConfigFile, int operatorMode = -1);
    // Multi-GPU (new): rank `rank` of `nranks`, see Engine's sharded constructor.  Same configuration file on every rank.
    SmpcController(string pathToConfigFile, int rank, int nranks, const void *ncclUniqueId128, int device = 0, int precision = RN_F64, int cutStage = 0,
                   int operatorMode = -1);
    void initialiseSmpcController();                        // SmpcController.cu:476-487
    void controllerSmpc();                                  // :1593-1599
    uint_t controlAction(real_t *u);                        // :1607-1625  (1 = ok)
    uint_t controlAction(std::fstream &controlOutputJson);  // :1633-1667
    DwnNetwork *getDwnNetwork() { return ptrMyEngine->getDwnNetwork(); }
    ScenarioTree *getScenarioTree() { return ptrMyEngine->getScenarioTree(); }
    SmpcConfiguration *getSmpcConfiguration() { return ptrMySmpcConfig; }
    Forecaster *getForecaster() { return ptrMyForecaster; }
    Engine *getEngine() { return ptrMyEngine; }
    // a re-weighted scenario tree between two controlAction calls: re-reads a scenarioTree.json of the SAME topology (ScenarioTree::reload; any
    // other throws std::invalid_argument and changes nothing) and hands its probabilities and errors to the device (Engine::updateScenarioTree,
    // rapidnet.h rn_set_tree_data) -- no new context, no factor step; the next controlAction recomputes the affine terms as it always does
    void updateScenarioTree(const std::string &pathToScenarioTreeJson) {
        ptrMyEngine->getScenarioTree()->reload(pathToScenarioTreeJson);
        ptrMyEngine->updateScenarioTree();
    }
    // bounds per stage or per node between two controlAction calls (Engine::setBounds, rapidnet.h rn_set_bounds): no new context, no factor
    // step beyond the first; a receding horizon shifts the rows every step, so the caller sets them each step
    void updateBounds(int granularity, size_t rows, const real_t *xmin, const real_t *xmax, const real_t *xsafe, const real_t *umin, const real_t *umax) {
        if (!factorStepFlag) { ptrMyEngine->factorStep(); factorStepFlag = true; }
        ptrMyEngine->setBounds(granularity, rows, xmin, xmax, xsafe, umin, umax);
    }
    // The shifted warm start (Engine::shiftWarmStart, rapidnet.h rn_shift_warm_start) between two control steps.  With the configuration's
    // "warmStart": "shift" both controlAction forms call it themselves before every step but the first -- in front of their leak check's
    // window, since the first shift allocates its index arrays and keeps them -- along the root's most probable child.
    void shiftWarmStart(int rootChild = -1) { ptrMyEngine->shiftWarmStart(rootChild); }
    // The step size the next iteration would use: the configuration's "stepSize", or -- "stepSizeRule": "lipschitz" -- stepSizeMargin over the
    // engine's estimate of the dual Lipschitz constant (Engine::setStepRule, rapidnet.h rn_set_step_rule).  With the rule both controlAction forms
    // make the FIRST estimate themselves, in front of their leak check's window (it allocates its vectors and keeps them); a stale estimate --
    // new probabilities, blocks of the caller's -- is renewed inside the control step, in the buffers it has.
    real_t getStepSizeInForce() { real_t s = 0; ptrMyEngine->getStepRule(nullptr, nullptr, &s); return s; }
    void moveForewardInTime();                              // :1679-1716
    // in-built simulator of moveForewardInTime: false (default) = the reference as written, x+ = x + B u (its disturbance
    // term lands in the x of node 0 instead of the state update, :1695); true = x+ = x + e_0 + B u (DwnNetwork.cuh:41-57)
    void setSimulatorDisturbance(bool on) { simulatorDisturbance = on; }
    void setSimulatorFlag(bool inBuilt) { simulatorFlag = inBuilt; }   // false: external simulator, the state is re-read from the configuration file
    real_t getEconomicKpi(uint_t simulationTime);           // :1808-1811
    real_t getSmoothKpi(uint_t simulationTime);             // :1817-1820
    real_t getNetworkKpi(uint_t simulationTime);            // :1826-1835
    real_t getSafetyKpi(uint_t simulationTime);             // :1841-1843
    void updateKpi(real_t *state, real_t *control);         // :1769-1802
    real_t *getPrimalInfeasibility() { return vecPrimalInfs.data(); }
    // iterations the last APG solve (controlAction, algorithmApg) ran: maxIterations unless Engine::setStopTolerance / the configuration's
    // "stopTolerance" ended it earlier (rapidnet.h, rn_get_last_solve)
    uint_t getIterationsRun();
    // momentum restarts of the last APG solve (controlAction, algorithmApg): 0 unless Engine::setRestart / the configuration's
    // "momentumRestart": "gradient" asked for the gradient test (rapidnet.h, rn_get_restart_info)
    uint_t getRestartsRun();
    // What the plan of the last control step costs and where it violates its bounds, per stage and per scenario (Engine::evaluatePlan,
    // rapidnet.h rn_plan_report: the predictive counterpart of the closed-loop read-outs above, :1819-1859).  To be called AFTER
    // controlAction, outside the window of its leak check: the first report allocates its tables on the device and keeps them.
    const Engine::PlanReport &getPlanReport();
    // ... written as one more entry of the control output: "planReport" : {"columns": [...], "perStage": [[...]], "leafNode": [...],
    // "perScenario": [[...]]}, a JSON object with 17 significant digits.  controlAction(fstream&)'s own output is unchanged.
    uint_t writePlanReport(std::fstream &controlOutputJson);
    // Dual bound and optimality gap of the solve at hand (Engine::solveCertificate): the record by column RN_CERT_*, and written as one more
    // entry of the control output: "solveCertificate" : {"dual": ..., "primal": ..., "gap": ..., ..., "valid": ...}.  AFTER controlAction.
    const std::vector<real_t> &getSolveCertificate();
    uint_t writeSolveCertificate(std::fstream &controlOutputJson);
    // What the plan of the last control step looks like across the tree (Engine::planQuantiles / planPaths, rapidnet.h rn_plan_quantiles):
    // the fan chart of every tank level and pump flow -- quantiles per stage at `levels` -- and every scenario's trajectory.  To be called
    // AFTER controlAction, like getPlanReport: the first call allocates its tables on the device and keeps them.
    struct PlanBands {
        size_t stages = 0, scenarios = 0, nx = 0, nu = 0;
        std::vector<real_t> levels;
        std::vector<real_t> xQuantiles, uQuantiles;      // [stages][nx | nu][levels]
        std::vector<real_t> xPaths, uPaths;              // [scenarios][stages][nx | nu]
        std::vector<int> leafNode;                       // [scenarios]
    };
    const PlanBands &getPlanBands(const std::vector<real_t> &levels);
    // ... written as one more entry of the control output: "planBands" : {"shape": [stages, scenarios, nx, nu, levels], "levels": [...],
    // "leafNode": [...], "xQuantiles": [...], "uQuantiles": [...], "xPaths": [...], "uPaths": [...]}, flat arrays in the layouts above, with
    // 17 significant digits, at the levels 0.05, 0.5, 0.95.  controlAction(fstream&)'s own output is unchanged.
    uint_t writePlanBands(std::fstream &controlOutputJson);
    real_t *getValueFbe() { return vecValueFbe.data(); }    // :1883
    real_t *getVecTau() { return vecTau.data(); }
    ~SmpcController();

protected:
    void initialiseAlgorithm();                             // :420-450  zero the iterates of the selected algorithm
    void initialiseAlgorithmSpecificData() {}               // :494-528  rebuilds device pointer tables: nothing to do here
    void initaliseLbfgBuffer();                             // :453-468
    void updateLbfgsBuffer();                               // :1103
    void twoLoopRecursionLbfgs();                           // :1175
    void dualExtrapolationStep(real_t lambda);              // :535
    void solveStep();                                       // :563
    void proximalFunG();                                    // :759
    void dualUpdate();                                      // :854
    uint_t algorithmApg();                                  // :1500
    void computeFixedPointResidual();                       // :839
    real_t updatePrimalInfeasibity();                       // :1480
    // global FBE / NAMA (selected by "algorithmName" of the controller configuration, Engine.cu:151-163)
    uint_t algorithmGlobalFbe();                            // :1529
    uint_t algorithmNama();                                 // :1559
    void computeHessianOracalGlobalFbe();                   // :884
    void updateFixedPointResidualNamaAlgorithm();           // :1060
    void computeGradientFbe();                              // :1077
    void computeLbfgsDirection();                           // :1234  (updateLbfgsBuffer :1103 + twoLoopRecursionLbfgs :1175)
    real_t computeLineSearchLbfgsUpdate(real_t valueFbeY);  // :1242
    real_t computeLineSearchAmeLbfgsUpdate(real_t valueFbeYvar);   // :1311
    real_t computeValueFbe();                               // :1416
    // lbfgsBufferCol / lbfgsBufferMemory / lbfgsBufferHessian / lbfgsBufferRho and the columns of devLbfgsBufferMatS / MatY
    void getLbfgsState(int &col, int &mem, real_t &H, real_t *rho) { check(rn_lbfgs_state(ptrMyEngine->getContext(), 0, &col, &mem, &H, rho), "rn_lbfgs_state"); }
    void setLbfgsState(int col, int mem, real_t H, real_t *rho) { check(rn_lbfgs_state(ptrMyEngine->getContext(), 1, &col, &mem, &H, rho), "rn_lbfgs_state"); }
    void getLbfgsColumn(int which, int col, real_t *host, size_t n) { check(rn_lbfgs_column(ptrMyEngine->getContext(), 0, which, col, host, n), "rn_lbfgs_column"); }
    void setLbfgsColumn(int which, int col, const real_t *host, size_t n) { check(rn_lbfgs_column(ptrMyEngine->getContext(), 1, which, col, const_cast<real_t *>(host), n), "rn_lbfgs_column"); }
    void getVector(int bufferId, real_t *host) { ptrMyEngine->getBuffer(bufferId, host); }
    void setVector(int bufferId, const real_t *host) { ptrMyEngine->setBuffer(bufferId, host); }
    void check(int rc, const char *what);
    bool deviceMemoryChanged(const size_t before[4]);       // the leak check of :1612-1623 (prints the reference's message)

    Engine *ptrMyEngine;
    Forecaster *ptrMyForecaster;
    SmpcConfiguration *ptrMySmpcConfig;
    real_t stepSize;
    bool factorStepFlag, simulatorFlag, ownsObjects, simulatorDisturbance = false;
    std::vector<real_t> vecPrimalInfs, vecValueFbe, vecTau, lastControl;
    real_t economicKpi, smoothKpi, safeKpi, networkKpi;
    Engine::PlanReport planReport;
    std::vector<real_t> solveCertificate;
    PlanBands planBands;
    uint_t controlSteps = 0;      // control steps solved so far ("warmStart": "shift" moves the duals before every one but the first)
    void shiftBeforeStep();
    void estimateBeforeStep();
};

#endif
