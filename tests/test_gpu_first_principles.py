"""The HIP kernels against the problem's definition (tests/first_principles.py), not against the oracle.

The oracle-pinned files need the oracle to be right to notice a mistake both sides share -- sqrt(p_i) in k_tree_data after a re-weighting, the
children moments of a cut parent, per-node bounds: features without a reference vector, whose oracle side was written by the same hand.  Here
a context's iterates are held to the mathematics: the dense minimiser of the Lagrangian on tiny / small / odd / ragged (argmin), feasibility +
stationarity at the accelerated dual plus the prox chain everywhere else (check_state).  RN_BUF_ACC_* hold the LAST sweep's input after a
batch (include/rapidnet_debug.h); a form that left w_next there would fail stationarity at once.

fp64: 1e-9 per stage, the project's figure; a dense case counts only with a refinement correction <= 1e-12 of |V| and fails otherwise.
fp32: e_gpu <= 4 e_cpu + 32 * 2^-24 per stage and quantity, e_cpu the fp32 oracle against the model, on tests/test_gpu_apg_f32.py's scales.
Fp32-stored blocks under fp64 iterates solve a different, rounded problem: out of scope.
When FIRST_PRINCIPLES_ERRORS names a file the measured figures are appended to it (profiles/first_principles_errors.txt)."""
import gc

import numpy as np
import pytest
import torch            # before librapidnet_hip.so is loaded (load order)

import first_principles as fp
import test_first_principles as cpu
import test_gpu_apg_f32 as a32
import test_gpu_stream_split as spl
from rapidnet_amd import capi, synth
from test_gpu_sharded_batched import Ranks

pytestmark = pytest.mark.gpu

TOL, CORRECTION = cpu.TOL, cpu.CORRECTION
DENSE = ["tiny", "small", "odd", "ragged"]
BID = a32.BID
LAMBDA = 0.618      # a fixed extrapolation weight for the solve step behind 9 iterations
# every operator form of the sweep: constructor arguments of capi.Solver
FORMS = {"dense": dict(operator_mode="dense"), "structured": dict(operator_mode="structured"),
         "lin0": dict(operator_mode="structured", knobs={"struct_linear": 0}), "lin2": dict(operator_mode="structured", knobs={"struct_linear": 2}),
         "lin3": dict(operator_mode="structured", knobs={"struct_linear": 3}), "lin4": dict(operator_mode="structured", knobs={"struct_linear": 4}),
         "lin5": dict(operator_mode="structured", knobs={"struct_linear": 5}), "auto": dict(operator_mode="auto"), "auto_set": dict(operator_mode="auto"),
         "vlv2": dict(operator_mode="dense", knobs={"vlv_wide": 2}), "vlv3": dict(operator_mode="dense", knobs={"vlv_wide": 3}),
         "lin0_vlv2": dict(operator_mode="structured", knobs={"struct_linear": 0, "vlv_wide": 2}),
         "frag0": dict(operator_mode="structured", knobs={"slab_frag": 0}), "unscaled0": dict(operator_mode="dense", knobs={"unscaled_walk": 0}),
         "unscaled0_structured": dict(operator_mode="structured", knobs={"unscaled_walk": 0})}


def getter(s):
    return lambda nm: s.get(BID[nm])


def gathered(rk):
    dim = a32.dims_of(rk.shards[0])
    return lambda nm: rk.gathered(BID[nm], dim(nm))


def model(p, fc, **kw):
    return fp.Model(p["network"], p["tree"], p["config"], fc, **kw)


def context(p, fc, form="dense", precision="f64", fuse=None, **kw):
    s = capi.Solver(p["network"], p["tree"], p["config"], precision=precision, **dict(FORMS[form], **kw))
    if fuse is not None:
        s.setFusedWalkDual(fuse)
    s.initialiseSmpcController(*fc)
    if form == "auto_set":          # one block of its own handed back: the auto context becomes dense, the factor step runs again
        node = s.nodes // 2
        s.setOperator(capi.OP_PHI, node, s.getOperator(capi.OP_PHI, node))
        assert s.operatorMode() == ("auto", "dense"), s.operatorMode()
        s.initialiseSmpcController(*fc)
    return s


def inject(s, wxi, wpsi):
    """y = y+ = w, then the extrapolation with weight 0: the route on which the library re-derives w itself (tests/test_gpu_apg_f32.py, form A)"""
    s.apgReset()
    for bid, v in ((capi.BUF_XI, wxi), (capi.BUF_UPD_XI, wxi), (capi.BUF_PSI, wpsi), (capi.BUF_UPD_PSI, wpsi)):
        s.set(bid, v)
    s.dualExtrapolationStep(0.0)


def set_duals(s, kind, seed=3):
    if kind == "random":
        rng = np.random.default_rng(seed)
        inject(s, rng.standard_normal(s.nodes * 2 * s.nx), rng.standard_normal(s.nodes * s.nu))
    else:
        s.apgReset()
        s.apgIterate(9)
        for bid in (capi.BUF_XI, capi.BUF_PSI, capi.BUF_UPD_XI, capi.BUF_UPD_PSI):      # (a `set` makes the library re-derive w from y and y+)
            s.set(bid, s.get(bid))
        s.dualExtrapolationStep(LAMBDA)


def step_chain(s):
    s.solveStep(); s.proximalFunG(); s.computeFixedPointResidual(); s.dualUpdate()


def assert_state(m, get, what, tol=TOL, prox=True):
    e = m.check_state(get, prox=prox)
    w = fp.worst(e)
    print("%s: worst %.1e in %s, stage %d; stationarity %.1e" % (what, w[0], w[1], w[2], e["stationarity"].max()))
    assert w[0] <= tol, (what,) + w
    return e


def assert_argmin(m, get, what):
    ref = m.argmin(get("accXi"), get("accPsi"))
    assert ref["correction"] <= CORRECTION, "%s: the model's refinement correction %.1e does not qualify the case" % (what, ref["correction"])
    w = fp.worst(fp.argmin_errors(m, get, ref))
    assert w[0] <= TOL, (what,) + w
    return w[0]


# ---- 1. rn_solve_step in every operator form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DENSE + ["medium"])
@pytest.mark.parametrize("form", list(FORMS))
def test_solve_step_in_every_operator_form(form, name):
    p, fc = cpu.problem(name)
    m, s = model(p, fc), context(p, fc, form)
    worst = 0.0
    for kind in cpu.DUALS:
        set_duals(s, kind)
        step_chain(s)
        what = "%s %s %s" % (name, form, kind)
        if name in DENSE:
            worst = max(worst, assert_argmin(m, getter(s), what))
        worst = max(worst, fp.worst(assert_state(m, getter(s), what))[0])
    cpu.record("gpu f64 solve step %-8s %-20s worst stage %.1e" % (name, form, worst))
    s.close()


# ---- 2. behind rn_apg_iterate(1) and rn_apg_iterate(16) ----------------------------------------------------------------------------------
BATCHES = [("medium", "dense", None, {}), ("medium", "structured", None, {}), ("medium", "dense", 0, {}), ("medium", "structured", 0, {}),
           ("medium", "dense", 1, {"fuse_split": 1}), ("medium", "dense", 1, {"fuse_split": 2}), ("medium", "structured", 1, {"fuse_split": 1000}),
           ("barcelona31", "dense", 1, {"fuse_split": 1}), ("barcelona31", "structured", 1, {"fuse_split": 2}), ("barcelona31", "dense", 1, {"fuse_split": 1000}),
           ("barcelona31", "dense", 0, {}), ("small", "dense", None, {}), ("small", "structured", None, {}), ("odd", "dense", None, {}), ("ragged", "structured", None, {})]


@pytest.mark.parametrize("name,form,fuse,knobs", BATCHES)
def test_state_behind_an_exact_and_an_optimistic_batch(name, form, fuse, knobs):
    """one exact iteration and one optimistic batch of 16 behind 9 iterations: the fused walk + dual update by shape, off, and on with 1, 2 and
    chain-length workgroups per chain; `small` (ny = 19) takes the flat k_dual_fused"""
    p, fc = cpu.problem(name)
    m = model(p, fc)
    s = context(p, fc, form, fuse=fuse, knobs=dict(FORMS[form].get("knobs", {}), **knobs))
    s.apgReset()
    s.apgIterate(9)
    c0 = s.counters()
    s.apgIterate(1)
    c1 = s.counters()
    assert c1["exact"] == c0["exact"] + 1, (c0, c1)
    e1 = assert_state(m, getter(s), "%s %s fuse %s %s, exact iteration" % (name, form, fuse, knobs))
    s.apgIterate(16)
    c2 = s.counters()
    assert c2["optimistic"] == c1["optimistic"] + 1 and c2["replayed"] == 0, (c1, c2)
    e2 = assert_state(m, getter(s), "%s %s fuse %s %s, optimistic batch" % (name, form, fuse, knobs))
    cpu.record("gpu f64 batches %-12s %-10s fuse %-4s %-22s exact %.1e optimistic %.1e" % (name, form, fuse, knobs, fp.worst(e1)[0], fp.worst(e2)[0]))
    s.close()


@pytest.mark.parametrize("form", ["dense", "structured"])
def test_state_behind_a_replayed_batch(form):
    """the soft-penalty problem (`medium`, penalties 2 / 1): both thresholds trip, the optimistic batch is replayed through the exact path"""
    p, fc = cpu.problem("medium", penalty_x=2.0, penalty_xs=1.0)
    m, s = model(p, fc), context(p, fc, form)
    s.apgReset()
    s.apgIterate(16)
    assert s.counters()["replayed"] == 1, s.counters()
    dx, ds = s.proxDistances()
    assert dx > m.gammaX / m.step and ds > m.gammaS / m.step, "both thresholds must trip"
    assert_state(m, getter(s), "medium soft %s" % form)
    want = m.prox(s.get(BID["primalXi"]), s.get(BID["primalPsi"]), s.get(BID["accXi"]), s.get(BID["accPsi"]))
    assert abs(want["distX"] - dx) <= TOL * dx and abs(want["distS"] - ds) <= TOL * ds
    s.close()


# ---- 3. the features without reference vectors ---------------------------------------------------------------------------------------------
def reweighted_model(p, fc, new, **kw):
    return model(p, fc, probNode=new["probNode"], errorDemandNode=new["errorDemandNode"], errorPriceNode=new["errorPriceNode"], **kw)


def rerun(s, fc, n=16):
    s.updateStateControl()
    s.eliminateInputDistubanceCoupling(*fc)
    s.apgReset()
    s.apgIterate(n)


def tree_data_on_device(s, new):
    t = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(new[j], float))).cuda()
         for k, j in (("prob", "probNode"), ("errorDemand", "errorDemandNode"), ("errorPrice", "errorPriceNode"))}
    torch.cuda.synchronize()            # the producer is done before the call (the context's stream does not wait for torch's)
    s.setTreeDataDevice("f64", **{k: v.data_ptr() for k, v in t.items()})
    s.synchronize()
    return t


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("form", ["dense", "structured"])
@pytest.mark.parametrize("name", ["ragged", "medium"])
def test_after_set_tree_data(name, form, route):
    p, fc = cpu.problem(name)
    new = cpu.reweighted(p, fc)
    s = context(p, fc, form)
    s.apgReset()
    s.apgIterate(5)
    keep = s.updateTree(new) if route == "host" else tree_data_on_device(s, new)
    m = reweighted_model(p, fc, new)
    rerun(s, fc)
    assert_state(m, getter(s), "%s %s re-weighted (%s), batch" % (name, form, route))
    set_duals(s, "random")
    step_chain(s)
    if name in DENSE:
        assert_argmin(m, getter(s), "%s %s re-weighted (%s)" % (name, form, route))
    assert_state(m, getter(s), "%s %s re-weighted (%s), step" % (name, form, route))
    assert fp.worst(model(p, fc).check_state(getter(s)))[0] >= cpu.REFUSED          # the old tree's model is refused: the data moved
    del keep
    s.close()


def set_bounds(s, rows, gran):
    s.setBounds(gran, **{k: rows[k] for k in ("xmin", "xmax", "xsafe", "umin", "umax")})


@pytest.mark.parametrize("gran", ["stage", "node"])
@pytest.mark.parametrize("form", ["dense", "structured"])
@pytest.mark.parametrize("name", ["small", "ragged", "medium"])
def test_after_set_bounds(name, form, gran):
    """per stage and per node, one u row with umin = umax (a pump out of service) and one xmin = xmax row"""
    p, fc = cpu.problem(name)
    rows = cpu.stage_rows(p, 11) if gran == "stage" else cpu.node_rows(p, 11)
    assert (rows["umax"][-1, 1] == rows["umin"][-1, 1]) and (rows["xmax"][-1, 0] == rows["xmin"][-1, 0])
    s = context(p, fc, form)
    set_bounds(s, rows, gran)
    m = model(p, fc, bounds=dict(rows, granularity=gran))
    s.apgReset()
    s.apgIterate(12)
    assert_state(m, getter(s), "%s %s %s bounds, exact batch" % (name, form, gran))
    s.apgIterate(16)
    assert_state(m, getter(s), "%s %s %s bounds, optimistic batch" % (name, form, gran))
    assert fp.worst(model(p, fc).check_state(getter(s)))[0] >= cpu.REFUSED, "the moved bounds must be active"
    s.close()


@pytest.mark.parametrize("form", ["dense", "structured"])
def test_after_set_tree_data_and_set_bounds_on_one_context(form):
    p, fc = cpu.problem("ragged")
    new, rows = cpu.reweighted(p, fc), cpu.node_rows(p, 11)
    s = context(p, fc, form)
    set_bounds(s, rows, "node")
    s.updateTree(new)
    m = reweighted_model(p, fc, new, bounds=dict(rows, granularity="node"))
    rerun(s, fc, 20)
    assert_state(m, getter(s), "ragged %s re-weighted with per-node bounds" % form)
    s.close()


@pytest.mark.parametrize("form", ["dense", "structured"])
@pytest.mark.parametrize("name", ["ragged", "medium"])
def test_second_control_action_warm_started(name, form):
    p, fc = cpu.problem(name)
    fc2 = synth.forecast_at(p["forecast"], 1)
    rng = np.random.default_rng(5)
    c = p["config"]
    x0 = np.asarray(c["currentX"], float) * (1 + 0.1 * rng.standard_normal(len(c["currentX"])))
    d0 = np.asarray(fc[0], float)[: len(c["prevDemand"])] * 1.1
    s = context(p, fc, form)
    s.setWarmStart(True)
    u0 = s.controlAction(*fc, maxIterations=32)
    s.controlAction(*fc2, currentX=x0, prevU=u0, prevDemand=d0, maxIterations=32)
    m = model(p, fc2, currentX=x0, prevU=u0, prevDemand=d0)
    assert_state(m, getter(s), "%s %s second control action" % (name, form))
    assert fp.worst(model(p, fc2).check_state(getter(s)))[0] >= cpu.REFUSED
    s.close()


@pytest.mark.parametrize("form", ["dense", "structured"])
def test_uncertainty_switches(form):
    p, fc = cpu.problem("ragged")
    s = context(p, fc, form)
    s.setUncertainty(demand=False, price=True, weightEconomical=0.35)
    rerun(s, fc)
    assert_state(model(p, fc, demandUncertainty=False, weightEconomical=0.35), getter(s), "ragged %s demand off" % form)
    s.setUncertainty(demand=True, price=False, weightEconomical=1.0)
    rerun(s, fc)
    assert_state(model(p, fc, priceUncertainty=False), getter(s), "ragged %s price off" % form)
    s.close()


@pytest.mark.parametrize("form", ["dense", "structured"])
def test_across_a_momentum_restart_that_fires(form):
    """`small`, batches of 20: the boundary at 180 fires (tests/test_gpu_restart.py); the state behind the next batch is a minimiser all the same"""
    p, fc = cpu.problem("small", feasible=True)
    s = context(p, fc, form, restart="gradient")
    run, _ = s.apg_solve(200, 0.0, 20)
    info = s.last_restarts()
    assert run == 200 and info["restarts"] == 1 and info["last_at"] == 180, info
    assert_state(model(p, fc), getter(s), "small %s behind the restart" % form)
    s.close()


# ---- 4. shards ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structured", [False, True])
@pytest.mark.parametrize("name,world,cut", [("medium", 2, 1), ("medium", 3, 2), ("medium", 3, 1), ("medium", 2, 2), ("ragged", 2, 1), ("ragged", 3, 2),
                                            ("ragged", 3, 1), ("ragged", 2, 2)])
def test_shards_gathered_in_global_node_order(name, world, cut, structured):
    """the stationarity sum of a cut parent spans the ranks: this is what checks the children moments"""
    p, fc = cpu.problem(name)
    m = model(p, fc)
    for optimistic in (True, False):
        rk = Ranks(p, world, cut, structured, optimistic=optimistic)
        try:
            def solve(s):
                s.initialiseSmpcController(*fc)
                s.apgReset()
                s.apgIterate(16)
                return s.counters()

            counters = rk.run(solve)
            assert all((c["optimistic"] >= 1) == optimistic for c in counters), counters
            get = gathered(rk)
            assert_state(m, get, "%s %d ranks cut %d %s %s" % (name, world, cut, "structured" if structured else "dense", "optimistic" if optimistic else "exact"))
        finally:
            rk.close()


@pytest.mark.parametrize("structured", [False, True])
def test_shards_after_set_tree_data(structured):
    p, fc = cpu.problem("medium")
    new = cpu.reweighted(p, fc)
    rk = Ranks(p, 3, 1, structured)
    try:
        def solve(s):
            s.initialiseSmpcController(*fc)
            s.apgReset()
            s.apgIterate(5)
            s.updateTree(new)
            rerun(s, fc)

        rk.run(solve)
        get = gathered(rk)
        assert_state(reweighted_model(p, fc, new), get, "medium 3 ranks re-weighted")
        assert fp.worst(model(p, fc).check_state(get))[0] >= cpu.REFUSED
    finally:
        rk.close()


# ---- 5. the split last round ---------------------------------------------------------------------------------------------------------------
def test_the_split_last_round():
    p, fc = spl.problem("b240", "r1")
    s = spl.solver(p, fc)
    spl.expect_split(s, spl.position("r1", spl.num_cus())[0])
    assert s.nodes == spl.num_cus() + 1
    m = model(p, fc)
    set_duals(s, "random")
    step_chain(s)
    assert_state(m, getter(s), "split round, one step")
    s.apgReset()
    s.apgIterate(16)
    assert_state(m, getter(s), "split round, batch")
    s.close()


# ---- 6. quasi-Newton entry points ----------------------------------------------------------------------------------------------------------
def direction_get(s):
    names = {"x": capi.BUF_XDIR, "u": capi.BUF_UDIR, "primalXi": capi.BUF_PRIMAL_XI_DIR, "primalPsi": capi.BUF_PRIMAL_PSI_DIR}
    return lambda nm: s.get(names[nm])


def direction_errors(m, got, ref):
    e = fp.argmin_errors(m, lambda nm: ref[nm] if nm == "v" else got(nm), ref)
    del e["v"]
    return e


@pytest.mark.parametrize("algorithm", ["globalFbeAlgorithm", "namaAlgorithm"])
@pytest.mark.parametrize("form", ["dense", "structured"])
@pytest.mark.parametrize("name", DENSE)
def test_hessian_oracle_is_the_linear_part_of_the_argmin_map(name, form, algorithm):
    p, fc = cpu.problem(name)
    m, s = model(p, fc), context(p, fc, form)
    s.setAlgorithm(algorithm, 5)
    s.fbeReset()
    rng = np.random.default_rng(9)
    dxi, dpsi = rng.standard_normal(s.nodes * 2 * s.nx), rng.standard_normal(s.nodes * s.nu)
    fbe = algorithm == "globalFbeAlgorithm"
    s.set(capi.BUF_LBFGS_CUR_YVEC_XI if fbe else capi.BUF_RES_XI, dxi)
    s.set(capi.BUF_LBFGS_CUR_YVEC_PSI if fbe else capi.BUF_RES_PSI, dpsi)
    s.computeHessianOracalGlobalFbe()
    ref = m.hessian_direction(dxi, dpsi)
    assert ref["correction"] <= CORRECTION
    w = fp.worst(direction_errors(m, direction_get(s), ref))
    assert w[0] <= TOL, w
    s.close()


@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("form", ["dense", "structured"])
@pytest.mark.parametrize("name", ["small", "ragged"])
def test_namas_paired_sweep(name, form, pair):
    """computeLineSearchAmeLbfgsUpdate with a direction of positive slope (nothing is searched): x, u and Hx have moved by lambda H(r), the
    direction buffers hold H(d - lambda r) -- one pass over the operator blocks (pair = 1) or two sweeps"""
    p, fc = cpu.problem(name)
    m = model(p, fc)
    s = context(p, fc, form, knobs=dict(FORMS[form].get("knobs", {}), nama_pair=pair))
    s.setAlgorithm("namaAlgorithm", 5)
    s.fbeReset()
    rng = np.random.default_rng(10)
    n_xi, n_psi = s.nodes * 2 * s.nx, s.nodes * s.nu
    rxi, rpsi, dxi, dpsi = rng.standard_normal(n_xi), rng.standard_normal(n_psi), rng.standard_normal(n_xi), rng.standard_normal(n_psi)
    if rxi @ dxi + rpsi @ dpsi > 0:      # valueDirection = -<r, d> must be positive
        dxi, dpsi = -dxi, -dpsi
    zero = lambda n: np.zeros(n)                         # x, u, Hx and w start at 0: what the first sweep adds is then read off without cancellation
    for bid, v in ((capi.BUF_RES_XI, rxi), (capi.BUF_RES_PSI, rpsi), (capi.BUF_LBFGS_DIR_XI, dxi), (capi.BUF_LBFGS_DIR_PSI, dpsi),
                   (capi.BUF_X, zero(s.nodes * s.nx)), (capi.BUF_U, zero(n_psi)), (capi.BUF_ACC_XI, zero(n_xi)), (capi.BUF_ACC_PSI, zero(n_psi)),
                   (capi.BUF_PRIMAL_XI, zero(n_xi)), (capi.BUF_PRIMAL_PSI, zero(n_psi))):
        s.set(bid, v)
    tau = s.computeLineSearchAmeLbfgsUpdate(0.0)
    assert tau == 1.0
    if form == "dense":
        assert (s.fbeCounters()["sweep_pairs"] >= 1) == bool(pair), s.fbeCounters()
    lam = m.step
    first, second = m.hessian_direction(rxi, rpsi), m.hessian_direction(dxi - lam * rxi, dpsi - lam * rpsi)
    assert max(first["correction"], second["correction"]) <= CORRECTION
    moved = {nm: s.get(bid) / lam for nm, bid in (("x", capi.BUF_X), ("u", capi.BUF_U), ("primalXi", capi.BUF_PRIMAL_XI), ("primalPsi", capi.BUF_PRIMAL_PSI))}
    assert np.abs(s.get(capi.BUF_ACC_XI) - lam * rxi).max() <= 1e-15 * lam * np.abs(rxi).max()
    w1 = fp.worst(direction_errors(m, moved.__getitem__, first))
    w2 = fp.worst(direction_errors(m, direction_get(s), second))
    assert w1[0] <= TOL and w2[0] <= TOL, (w1, w2)
    s.close()


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("form", ["dense", "structured"])
@pytest.mark.parametrize("name", ["small", "medium"])
def test_value_fbe_is_the_primal_value_plus_its_dual_terms(name, form, soft):
    p, fc = cpu.problem(name, **(dict(penalty_x=2.0, penalty_xs=1.0) if soft else {}))
    m, s = model(p, fc), context(p, fc, form)
    s.setAlgorithm("globalFbeAlgorithm", 5)
    s.fbeReset()
    rng = np.random.default_rng(4)
    scale = 1.0 if soft else 1e-3
    s.set(capi.BUF_ACC_XI, scale * rng.standard_normal(s.nodes * 2 * s.nx)); s.set(capi.BUF_ACC_PSI, scale * rng.standard_normal(s.nodes * s.nu))
    s.solveStep(); s.proximalFunG(); s.computeFixedPointResidual()
    got = s.computeValueFbe()
    get = getter(s)
    assert_state(m, get, "%s %s value" % (name, form), prox=False)
    w = np.concatenate([get("accXi"), get("accPsi")])
    pr = m.prox(get("primalXi"), get("primalPsi"), get("accXi"), get("accPsi"))
    r = np.concatenate([pr["resXi"], pr["resPsi"]])
    terms = [float(w @ r), 0.5 * m.step * float(r @ r), m.primal_value(get("u"))]
    for dist, gamma in ((pr["distX"], m.gammaX), (pr["distS"], m.gammaS)):
        if dist > gamma / m.step:
            terms.append(gamma * (dist - gamma / m.step))
    assert (len(terms) == 5) == soft
    assert abs(got - sum(terms)) <= TOL * sum(abs(t) for t in terms), (got, terms)
    s.close()


# ---- 7. fp32 contexts ----------------------------------------------------------------------------------------------------------------------
_E_CPU = {}


def e_cpu(name, form):
    if (name, form) not in _E_CPU:
        p, fc = cpu.problem(name)
        _E_CPU[(name, form)] = model(p, fc).check_state(cpu.f32_state(p, fc, form).get, scales="z")
    return _E_CPU[(name, form)]


@pytest.mark.parametrize("form", ["step", "batch"])
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name", ["medium", "barcelona31"])
def test_f32_context_against_the_model(name, mode, form):
    """e_gpu <= 4 e_cpu + 32 * 2^-24 per stage and quantity, both against the model at the state each side holds"""
    p, fc = cpu.problem(name)
    m, s = model(p, fc), context(p, fc, mode, precision="f32")
    if form == "step":
        set_duals(s, "random")
        step_chain(s)
    else:
        d = cpu.oracle(p, fc)
        d.apg(9)
        s.apgReset()
        for nm in ("xi", "psi", "updXi", "updPsi"):
            s.set(BID[nm], a32.round32(d.get(nm)))
        s.apgIterate(16)
        assert s.counters()["optimistic"] == 1, s.counters()
    eg, ec = m.check_state(getter(s), scales="z"), e_cpu(name, form)
    share = {nm: float((eg[nm] / (a32.FACTOR * ec[nm] + a32.FLOOR)).max()) for nm in eg}
    cpu.record("gpu f32 %-12s %-10s %-5s worst share of the bound: %s" % (name, mode, form, "  ".join("%s %.2f" % kv for kv in share.items())))
    bad = {nm: v for nm, v in share.items() if not v <= 1.0}
    assert not bad, bad
    s.close()


# ---- 8. random shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "structured"])
@pytest.mark.parametrize("seed", range(6))
def test_random_shapes(seed, form):
    p, fc = cpu.problem("random%d" % seed)
    m, s = model(p, fc), context(p, fc, form)
    for kind in cpu.DUALS:
        set_duals(s, kind)
        step_chain(s)
        assert_state(m, getter(s), "random shape %d %s %s" % (seed, form, kind))
    s.apgIterate(16)
    e = assert_state(m, getter(s), "random shape %d %s batch" % (seed, form))
    cpu.record("gpu f64 random shape %d %-10s batch worst %.1e" % (seed, form, fp.worst(e)[0]))
    s.close()


# ---- 9. under the buffer guard (tests/test_gpu_guard.py) -----------------------------------------------------------------------------------
def guard_body():
    """`small`, dense and structured: the solve step from random duals and the state behind a batch; returns the number of contexts"""
    for form in ("dense", "structured"):
        test_solve_step_in_every_operator_form(form, "small")
        test_state_behind_an_exact_and_an_optimistic_batch("small", form, None, {})
    gc.collect()
    return 4
