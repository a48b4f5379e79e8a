// Engine.cpp -- see Engine.hpp.
#include "Engine.hpp"

#include "NullSpace.hpp"

void Engine::check(int rc, const char *what) {
    if (rc != RN_OK) throw std::runtime_error(string(what) + ": " + rn_last_error(ctx));
}

Engine::Engine(SmpcConfiguration *smpcConfig, int precision, int device, int operatorMode) : ctx(nullptr) {
    ptrMySmpcConfig = smpcConfig;
    ptrMyNetwork = new DwnNetwork(smpcConfig->getPathToNetwork());          // never deleted by the reference either
    ptrMyScenarioTree = new ScenarioTree(smpcConfig->getPathToScenarioTree());
    create(precision, device, operatorMode);
}

Engine::Engine(DwnNetwork *network, ScenarioTree *scenarioTree, SmpcConfiguration *smpcConfig, int precision, int device, int operatorMode) : ctx(nullptr) {
    ptrMyNetwork = network; ptrMyScenarioTree = scenarioTree; ptrMySmpcConfig = smpcConfig;
    create(precision, device, operatorMode);
}

Engine::Engine(SmpcConfiguration *smpcConfig, int precision, int device, int rank, int nranks, const void *id128, int cutStage, int operatorMode) : ctx(nullptr) {
    ptrMySmpcConfig = smpcConfig;
    ptrMyNetwork = new DwnNetwork(smpcConfig->getPathToNetwork());
    ptrMyScenarioTree = new ScenarioTree(smpcConfig->getPathToScenarioTree());
    create(precision, device, operatorMode, rank, nranks, id128, cutStage);
}

Engine::Engine(DwnNetwork *network, ScenarioTree *scenarioTree, SmpcConfiguration *smpcConfig, int precision, int device, int rank, int nranks,
               const void *id128, int cutStage, int operatorMode) : ctx(nullptr) {
    ptrMyNetwork = network; ptrMyScenarioTree = scenarioTree; ptrMySmpcConfig = smpcConfig;
    create(precision, device, operatorMode, rank, nranks, id128, cutStage);
}

uint_t Engine::getNumLocalNodes() {
    int info[7];
    check(rn_shard_info(ctx, info), "rn_shard_info");
    return (uint_t)info[5];
}
std::vector<int> Engine::getGlobalNodes() {
    std::vector<int> g(getNumLocalNodes());
    check(rn_shard_global_nodes(ctx, g.data(), g.size()), "rn_shard_global_nodes");
    return g;
}

void Engine::setOperatorMode(int mode) { check(rn_set_operator_mode(ctx, mode), "rn_set_operator_mode"); }
int Engine::getOperatorMode() {
    int active = RN_OPS_DENSE;
    check(rn_get_operator_mode(ctx, nullptr, &active), "rn_get_operator_mode");
    return active;
}
void Engine::setOperatorStorage(int storage) { check(rn_set_operator_storage(ctx, storage), "rn_set_operator_storage"); }
int Engine::getOperatorStorage() {
    int active = RN_STORE_NATIVE;
    check(rn_get_operator_storage(ctx, nullptr, &active), "rn_get_operator_storage");
    return active;
}
void Engine::setStopTolerance(real_t tol, int checkEvery) { check(rn_set_stop_tolerance(ctx, tol, checkEvery), "rn_set_stop_tolerance"); }
real_t Engine::getStopTolerance(int *checkEvery) {
    double tol = 0;
    check(rn_get_stop_tolerance(ctx, &tol, checkEvery), "rn_get_stop_tolerance");
    return tol;
}
void Engine::setRestart(int mode) { check(rn_set_restart(ctx, mode), "rn_set_restart"); }
int Engine::getRestart() {
    int mode = RN_RESTART_OFF;
    check(rn_get_restart(ctx, &mode), "rn_get_restart");
    return mode;
}
void Engine::setSweepPairing(int mode) { check(rn_set_sweep_pairing(ctx, mode), "rn_set_sweep_pairing"); }
int Engine::getSweepPairing(int *active) {
    int requested = RN_PAIR_AUTO;
    check(rn_get_sweep_pairing(ctx, &requested, active), "rn_get_sweep_pairing");
    return requested;
}
void Engine::setOperator(int op, uint_t node, const real_t *host, size_t n) { check(rn_set_operator(ctx, op, node, host, n), "rn_set_operator"); }

void Engine::setOperators(const real_t *phi, const real_t *psi, const real_t *D, const real_t *F) {
    check(rn_set_operators(ctx, getNumLocalNodes(), phi, psi, D, F), "rn_set_operators");
}
void Engine::getOperators(real_t *phi, real_t *psi, real_t *D, real_t *F) { check(rn_get_operators(ctx, getNumLocalNodes(), phi, psi, D, F), "rn_get_operators"); }
void Engine::setOperatorsDevice(int precision, const void *phi, const void *psi, const void *D, const void *F) {
    check(rn_set_operators_device(ctx, getNumLocalNodes(), precision, phi, psi, D, F), "rn_set_operators_device");
}
void Engine::getOperatorsDevice(int precision, void *phi, void *psi, void *D, void *F) {
    check(rn_get_operators_device(ctx, getNumLocalNodes(), precision, phi, psi, D, F), "rn_get_operators_device");
}

void Engine::setTreeData(const real_t *prob, const real_t *errorDemand, const real_t *errorPrice) {
    check(rn_set_tree_data(ctx, ptrMyScenarioTree->getNumNodes(), prob, errorDemand, errorPrice), "rn_set_tree_data");
}
void Engine::setTreeDataDevice(int precision, const void *prob, const void *errorDemand, const void *errorPrice) {
    check(rn_set_tree_data_device(ctx, ptrMyScenarioTree->getNumNodes(), precision, prob, errorDemand, errorPrice), "rn_set_tree_data_device");
}
void Engine::getTreeData(real_t *prob, real_t *errorDemand, real_t *errorPrice) {
    check(rn_get_tree_data(ctx, getNumLocalNodes(), prob, errorDemand, errorPrice), "rn_get_tree_data");
}
void Engine::updateScenarioTree() {
    setTreeData(ptrMyScenarioTree->getProbArray(), ptrMyScenarioTree->getErrorDemandArray(), ptrMyScenarioTree->getErrorPriceArray());
}

void Engine::setBounds(int granularity, size_t rows, const real_t *xmin, const real_t *xmax, const real_t *xsafe, const real_t *umin, const real_t *umax) {
    check(rn_set_bounds(ctx, granularity, rows, xmin, xmax, xsafe, umin, umax), "rn_set_bounds");
}
void Engine::setBoundsDevice(int granularity, size_t rows, int precision, const void *xmin, const void *xmax, const void *xsafe, const void *umin, const void *umax) {
    check(rn_set_bounds_device(ctx, granularity, rows, precision, xmin, xmax, xsafe, umin, umax), "rn_set_bounds_device");
}
int Engine::getBoundsLayout(size_t *rows) {
    int granularity = RN_BOUNDS_SHARED;
    size_t r = 0;
    check(rn_get_bounds_layout(ctx, &granularity, &r), "rn_get_bounds_layout");
    if (rows) *rows = r;
    return granularity;
}
void Engine::getBounds(size_t rows, real_t *xmin, real_t *xmax, real_t *xsafe, real_t *umin, real_t *umax) {
    check(rn_get_bounds(ctx, rows, xmin, xmax, xsafe, umin, umax), "rn_get_bounds");
}
size_t Engine::getNumLocalScenarios() {
    const uint_t *stage = ptrMyScenarioTree->getStageNodes();
    const uint_t nodes = ptrMyScenarioTree->getNumNodes();
    uint_t last = 0;
    for (uint_t i = 0; i < nodes; i++) last = stage[i] > last ? stage[i] : last;
    size_t n = 0;
    for (int g : getGlobalNodes()) n += stage[g] == last;
    return n;
}
void Engine::evaluatePlan(PlanReport &r) {
    r.stages = ptrMyScenarioTree->getPredHorizon();
    r.scenarios = getNumLocalScenarios();
    r.perStage.assign(r.stages * RN_PLAN_COLS, 0.0);
    r.perScenario.assign(r.scenarios * RN_PLAN_COLS, 0.0);
    r.leafNode.assign(r.scenarios, 0);
    check(rn_plan_report(ctx, r.stages, r.perStage.data()), "rn_plan_report");
    check(rn_plan_report_scenarios(ctx, r.scenarios, r.perScenario.data(), r.leafNode.data()), "rn_plan_report_scenarios");
}
void Engine::solveCertificate(real_t out[RN_CERT_COLS]) { check(rn_solve_certificate(ctx, out), "rn_solve_certificate"); }
void Engine::planQuantiles(int which, const std::vector<real_t> &levels, std::vector<real_t> &out) {
    const size_t stages = ptrMyScenarioTree->getPredHorizon(), dim = which == RN_BAND_U ? ptrMySmpcConfig->getNU() : ptrMySmpcConfig->getNX();
    out.assign(stages * dim * levels.size(), 0.0);
    check(rn_plan_quantiles(ctx, which, levels.size(), levels.data(), stages, out.data()), "rn_plan_quantiles");
}
void Engine::planPaths(int which, std::vector<real_t> &out, std::vector<int> &leafNode) {
    const size_t stages = ptrMyScenarioTree->getPredHorizon(), dim = which == RN_BAND_U ? ptrMySmpcConfig->getNU() : ptrMySmpcConfig->getNX();
    const size_t scenarios = ptrMyScenarioTree->getNumScenarios();
    out.assign(scenarios * stages * dim, 0.0);
    leafNode.assign(scenarios, 0);
    check(rn_plan_paths(ctx, which, scenarios, out.data(), leafNode.data()), "rn_plan_paths");
}

void Engine::create(int precision, int device, int operatorMode, int rank, int nranks, const void *id128, int cutStage) {
    myRank = rank; numRanks = nranks;
    priceUncertaintyFlag = true; demandUncertaintyFlag = true;
    const string alg = ptrMySmpcConfig->getOptimisationAlgorithm();   // Engine.cu:151-163
    globalFbeFlag = (alg == "globalFbeAlgorithm");
    namaFlag = (alg == "namaAlgorithm");
    apgFlag = !globalFbeFlag && !namaFlag;
    _ASSERT(ptrMyNetwork->getNumTanks() == ptrMySmpcConfig->getNX() && ptrMyNetwork->getNumControls() == ptrMySmpcConfig->getNU());
    _ASSERT(ptrMyNetwork->getNumDemands() == ptrMySmpcConfig->getND());
    rn_dims d;
    d.nx = ptrMyNetwork->getNumTanks(); d.nu = ptrMyNetwork->getNumControls(); d.nv = ptrMySmpcConfig->getNV();
    d.nd = ptrMyNetwork->getNumDemands(); d.N = ptrMyScenarioTree->getPredHorizon(); d.K = ptrMyScenarioTree->getNumScenarios();
    d.nodes = ptrMyScenarioTree->getNumNodes(); d.nNonLeafNodes = ptrMyScenarioTree->getNumNonleafNodes();
    rn_tree t;
    t.stages = ptrMyScenarioTree->getStageNodes(); t.nodesPerStage = ptrMyScenarioTree->getNodesPerStage();
    t.nodesPerStageCumul = ptrMyScenarioTree->getNodesPerStageCumul(); t.ancestor = ptrMyScenarioTree->getAncestorArray();
    t.nChildren = ptrMyScenarioTree->getNumChildren(); t.nChildrenCumul = ptrMyScenarioTree->getNumChildrenCumul();
    t.probNode = ptrMyScenarioTree->getProbArray();
    // one entry point for both cases: nranks == 1 is a plain rn_create + rn_set_tree_errors
    const int rc = rn_create_sharded(&d, &t, ptrMyScenarioTree->getErrorDemandArray(), ptrMyScenarioTree->getErrorPriceArray(), precision, device,
                                     rank, nranks, cutStage, id128, &ctx);
    if (rc != RN_OK) throw std::runtime_error(string("rn_create_sharded: ") + rn_last_error(nullptr));
    check(rn_set_parameters(ctx, ptrMySmpcConfig->getStepSize(), ptrMySmpcConfig->getPenaltyState(), ptrMySmpcConfig->getPenaltySafety()),
          "rn_set_parameters");
    if (operatorMode < 0) {   // the configuration's optional key (absent: auto)
        const string m = ptrMySmpcConfig->getOperatorMode();
        operatorMode = m == "dense" ? RN_OPS_DENSE : (m == "structured" ? RN_OPS_STRUCTURED : RN_OPS_AUTO);
    }
    check(rn_set_operator_mode(ctx, operatorMode), "rn_set_operator_mode");
    if (ptrMySmpcConfig->getOperatorStorage() == "f32") check(rn_set_operator_storage(ctx, RN_STORE_F32), "rn_set_operator_storage");
    {
        const string m = ptrMySmpcConfig->getSweepPairing();
        if (m != "auto") check(rn_set_sweep_pairing(ctx, m == "on" ? RN_PAIR_ON : RN_PAIR_OFF), "rn_set_sweep_pairing");
    }
    if (ptrMySmpcConfig->getStopTolerance() > 0)   // (a file without the key makes exactly the calls it always made)
        check(rn_set_stop_tolerance(ctx, ptrMySmpcConfig->getStopTolerance(), (int)ptrMySmpcConfig->getStopCheckEvery()), "rn_set_stop_tolerance");
    if (ptrMySmpcConfig->getMomentumRestart() == "gradient") check(rn_set_restart(ctx, RN_RESTART_GRADIENT), "rn_set_restart");
    if (ptrMySmpcConfig->getWarmStart() != "off") check(rn_set_warm_start(ctx, 1), "rn_set_warm_start");      // "keep" | "shift"
    if (ptrMySmpcConfig->getStepSizeRule() == "lipschitz")   // (a file without the key makes exactly the calls it always made)
        check(rn_set_step_rule(ctx, RN_STEP_LIPSCHITZ, ptrMySmpcConfig->getStepSizeMargin(), (int)ptrMySmpcConfig->getLipschitzIterations()), "rn_set_step_rule");
    // SmpcController::allocateApgAlgorithm (SmpcController.cu:124-151): per-iteration storage for maxIterations, allocated once
    check(rn_reserve_iterations(ctx, (int)ptrMySmpcConfig->getMaxIterations()), "rn_reserve_iterations");
    if (!apgFlag)   // SmpcController::allocateGlobalFbeAlgorithm / allocateNamaAlgorithm / allocateLbfgsBuffer (SmpcController.cu:234-330)
        check(rn_set_algorithm(ctx, globalFbeFlag ? RN_ALG_GLOBAL_FBE : RN_ALG_NAMA, (int)ptrMySmpcConfig->getLbfgsBufferSize()), "rn_set_algorithm");
}

Engine::~Engine() { if (ctx) rn_destroy(ctx); }

void Engine::factorStep() {
    rn_system s;
    s.matB = ptrMyNetwork->getMatB(); s.matGd = ptrMyNetwork->getMatGd();
    s.matL = getMatL(); s.matLhat = getMatLhat();
    s.costW = ptrMySmpcConfig->getCostW(); s.matDiagPrecnd = ptrMySmpcConfig->getMatPrcndDiag();
    s.vecXmin = ptrMyNetwork->getXmin(); s.vecXmax = ptrMyNetwork->getXmax(); s.vecXsafe = ptrMyNetwork->getXsafe();
    s.vecUmin = ptrMyNetwork->getUmin(); s.vecUmax = ptrMyNetwork->getUmax(); s.costAlpha1 = ptrMyNetwork->getAlpha();
    check(rn_factor_step(ctx, &s), "rn_factor_step");
}
void Engine::updateStateControl(real_t *currentX, real_t *prevU, real_t *prevDemand) {
    check(rn_update_state_control(ctx, currentX, prevU, prevDemand), "rn_update_state_control");
}
void Engine::eliminateInputDistubanceCoupling(real_t *nominalDemand, real_t *nominalPrices) {
    check(rn_eliminate_input_disturbance_coupling(ctx, nominalDemand, nominalPrices), "rn_eliminate_input_disturbance_coupling");
}
void Engine::setPriceUncertaintyFlag(bool f) {
    priceUncertaintyFlag = f;
    check(rn_set_uncertainty(ctx, demandUncertaintyFlag, priceUncertaintyFlag, ptrMySmpcConfig->getWeightEconomical()), "rn_set_uncertainty");
}
void Engine::setDemandUncertaintyFlag(bool f) {
    demandUncertaintyFlag = f;
    check(rn_set_uncertainty(ctx, demandUncertaintyFlag, priceUncertaintyFlag, ptrMySmpcConfig->getWeightEconomical()), "rn_set_uncertainty");
}
size_t Engine::getBufferSize(int id) { return rn_buffer_size(ctx, id); }
void Engine::getBuffer(int id, real_t *host) { check(rn_get(ctx, id, host, rn_buffer_size(ctx, id)), "rn_get"); }
void Engine::setBuffer(int id, const real_t *host) { check(rn_set(ctx, id, host, rn_buffer_size(ctx, id)), "rn_set"); }
void Engine::getBufferRange(int id, size_t first, size_t n, real_t *host) { check(rn_get_range(ctx, id, first, n, host), "rn_get_range"); }
void Engine::setBufferRange(int id, size_t first, size_t n, const real_t *host) { check(rn_set_range(ctx, id, first, n, host), "rn_set_range"); }
void Engine::getOperator(int op, uint_t node, real_t *host, size_t n) { check(rn_get_operator(ctx, op, node, host, n), "rn_get_operator"); }
void *Engine::getDevicePointer(int bufferId, size_t *n) {
    void *p = nullptr;
    size_t cnt = 0;
    int prec = 0;
    check(rn_device_pointer(ctx, bufferId, &p, &cnt, &prec), "rn_device_pointer");
    if (n) *n = cnt;
    return p;
}
int Engine::getDevicePrecision() {
    void *p = nullptr;
    size_t cnt = 0;
    int prec = 0;
    check(rn_device_pointer(ctx, RN_BUF_UHAT, &p, &cnt, &prec), "rn_device_pointer");
    return prec;
}

void Engine::calculateMatLandMatLhat() {
    const int ne = ptrMyNetwork->getNumMixNodes(), nu = ptrMyNetwork->getNumControls(), nd = ptrMyNetwork->getNumDemands();
    const int rank = computeNullSpaceAndParticular(ptrMyNetwork->getMatE(), ptrMyNetwork->getMatEd(), ne, nu, nd, computedL, computedLhat);
    if (nu - rank != (int)ptrMySmpcConfig->getNV())
        throw std::logic_error("calculateMatLandMatLhat: null space of E has dimension " + std::to_string(nu - rank) + ", the configuration says nv = " +
                               std::to_string(ptrMySmpcConfig->getNV()));
    useComputedL = true;
}
Engine::LipschitzEstimate Engine::estimateLipschitz(int maxIterations, real_t tol, int checkEvery, const std::vector<real_t> &start, unsigned long long seed, bool history) {
    LipschitzEstimate e;
    const size_t nodes = getNumLocalNodes(), nxi = nodes * 2 * ptrMySmpcConfig->getNX(), npsi = nodes * ptrMySmpcConfig->getNU();
    if (!start.empty() && start.size() != nxi + npsi) throw std::invalid_argument("estimateLipschitz: the start vector holds xi [nodes][2nx] followed by psi [nodes][nu]");
    if (history) e.history.assign((size_t)(maxIterations > 0 ? maxIterations : 0) * 3, 0.0);
    double out[RN_LIP_COLS] = {0, 0, 0, 0};
    check(rn_estimate_lipschitz(ctx, maxIterations, tol, checkEvery, start.empty() ? nullptr : start.data(), start.empty() ? nullptr : start.data() + nxi, seed, out,
                                history ? e.history.data() : nullptr), "rn_estimate_lipschitz");
    e.norm = out[RN_LIP_NORM]; e.rayleigh = out[RN_LIP_RAYLEIGH]; e.residual = out[RN_LIP_RESIDUAL]; e.iterations = (uint_t)out[RN_LIP_ITERATIONS];
    if (history) e.history.resize((size_t)e.iterations * 3);
    return e;
}
bool Engine::getLipschitz(LipschitzEstimate &e) {
    double out[RN_LIP_COLS] = {0, 0, 0, 0};
    int stale = 0;
    const int rc = rn_get_lipschitz(ctx, out, &stale);
    if (rc == RN_E_STATE) return false;
    check(rc, "rn_get_lipschitz");
    e.norm = out[RN_LIP_NORM]; e.rayleigh = out[RN_LIP_RAYLEIGH]; e.residual = out[RN_LIP_RESIDUAL]; e.iterations = (uint_t)out[RN_LIP_ITERATIONS];
    e.stale = stale != 0;
    e.history.clear();
    return true;
}
void Engine::setStepRule(int rule, real_t margin, int iterations) { check(rn_set_step_rule(ctx, rule, margin, iterations), "rn_set_step_rule"); }
int Engine::getStepRule(real_t *margin, int *iterations, real_t *stepSizeInForce) {
    int rule = RN_STEP_FIXED;
    check(rn_get_step_rule(ctx, &rule, margin, iterations, stepSizeInForce), "rn_get_step_rule");
    return rule;
}
void Engine::setWarmStart(bool on) { check(rn_set_warm_start(ctx, on ? 1 : 0), "rn_set_warm_start"); }
void Engine::shiftWarmStart(int rootChild) { check(rn_shift_warm_start(ctx, rootChild), "rn_shift_warm_start"); }
void Engine::setShiftMap(const std::vector<int> &map) { check(rn_set_shift_map(ctx, map.size(), map.empty() ? nullptr : map.data()), "rn_set_shift_map"); }
void Engine::getShiftMap(int rootChild, std::vector<int> &map) {
    map.assign(ptrMyScenarioTree->getNumNodes(), 0);
    check(rn_get_shift_map(ctx, rootChild, map.size(), map.data()), "rn_get_shift_map");
}
