"""The CPU oracle against the problem's definition (tests/first_principles.py): no GPU.

Every parity test ends at the oracle; these tests check the oracle against the mathematics its sweep is supposed to implement -- the unique
minimiser of the Lagrangian built from the JSON data by a dense solve (argmin, small trees), or feasibility + stationarity, which by strict
convexity mean the same (residuals, any size) -- and give the model teeth: seven deliberate mistakes in the model must each be refused.

fp64 bound: 1e-9 per stage, the project's figure -- not measured against the code under test.  The model's own error is its refinement
correction, which must be <= 1e-12 of |V| for a dense case to count (a case that does not meet it FAILS).  The normalised stationarity
residual of the oracle itself must stay below 1e-11 on every problem, or its scale is wrong.
When FIRST_PRINCIPLES_ERRORS names a file the measured figures are appended to it: profiles/first_principles_errors.txt is such a file."""
import copy
import os

import numpy as np
import pytest

import first_principles as fp
from conftest import GOLDEN
from oracle.oracle import Oracle, forecast_at, load_json
from rapidnet_amd import synth
from test_gpu_random_shapes import random_config

TOL = 1e-9
CORRECTION = 1e-12
ORACLE_STATIONARITY = 1e-11
REFUSED = 1e-6
EPS32 = 2.0 ** -24
DENSE = ["tiny", "small", "odd", "ragged", "reference_fixture"]
LARGE = ["medium", "barcelona31", "reference_barcelona30", "medium_lazy"] + ["random%d" % s for s in range(6)]
DUALS = ["random", "apg9"]
_PROBLEMS = {}


def record(line):
    print(line)
    path = os.environ.get("FIRST_PRINCIPLES_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def problem(name, **kw):
    """(problem dicts, (dhat, ahat)) of a named problem; built once"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _PROBLEMS:
        if name.startswith("reference_"):
            d = os.path.join(GOLDEN, name)
            p = {k: load_json(os.path.join(d, f)) for k, f in (("network", "network.json"), ("tree", "scenarioTree.json"),
                                                                ("config", "controllerConfig.json"), ("forecast", "forecastor.json"))}
            fc = forecast_at(p["forecast"], 1 if name == "reference_fixture" else 0)
        elif name.startswith("random"):
            tag = "_random_%s" % name[6:]
            synth.CONFIGS[tag] = random_config(int(name[6:]))
            try:
                p = synth.make_problem(tag, **kw)
            finally:
                del synth.CONFIGS[tag]
            fc = synth.forecast_at(p["forecast"], 0)
        else:
            p = synth.make_problem(name, **kw)
            fc = synth.forecast_at(p["forecast"], 0)
        _PROBLEMS[key] = (p, fc)
    return _PROBLEMS[key]


def oracle(p, fc, precision="f64", lazy=False, tree=None):
    o = Oracle(p["network"], p["tree"] if tree is None else tree, p["config"], precision=precision, lazy_operators=lazy)
    o.initialise(*fc)
    return o


def random_duals(o, seed, scale=1.0):
    """random normal duals in the accelerated dual, the sweep's input"""
    rng = np.random.default_rng(seed)
    o.apg_reset()
    o.set("accXi", scale * rng.standard_normal(o.nodes * 2 * o.nx))
    o.set("accPsi", scale * rng.standard_normal(o.nodes * o.nu))


def set_duals(o, kind, seed=3):
    """random: random normal w.  apg9: the oracle's own accelerated dual after 9 APG iterations and one more extrapolation at the theta the
    tenth iteration would use.  Either way the sweep has NOT run on that w yet."""
    if kind == "random":
        random_duals(o, seed)
    else:
        o.apg_reset()
        th = o.apg_continue(9, [1.0, 1.0])
        o.extrapolate(th[1] * (1.0 / th[0] - 1.0))


def reweighted(p, fc, seed=7):
    """the same topology with new probabilities (every non-leaf node deals its own among its children by weights from [0.2, 1]) and new errors"""
    tree = p["tree"]
    rng = np.random.default_rng(seed)
    nodes, N = int(tree["nodes"][0]), int(tree["N"][0])
    nd, nu = int(tree["dimDemand"][0]), int(tree["dimPrice"][0])
    anc, stages = np.asarray(tree["ancestor"], int) - 1, np.asarray(tree["stages"], int)
    kids = [[] for _ in range(nodes)]
    for c in range(1, nodes):
        kids[anc[c]].append(c)
    prob = np.ones(nodes)
    for i in range(nodes):
        if kids[i]:
            w = rng.uniform(0.2, 1.0, len(kids[i]))
            prob[kids[i]] = prob[i] * w / w.sum()
    dh, ah = np.asarray(fc[0], float).reshape(N, nd), np.asarray(fc[1], float).reshape(N, nu)
    err_d, err_a = 0.05 * rng.standard_normal((nodes, nd)) * dh[stages], 0.05 * rng.standard_normal((nodes, nu)) * ah[stages]
    err_d[0], err_a[0] = 0.0, 0.0
    new = copy.deepcopy(tree)
    new["probNode"], new["errorDemandNode"], new["errorPriceNode"] = prob.tolist(), err_d.ravel().tolist(), err_a.ravel().tolist()
    return new


def assert_argmin(m, o, what):
    """the oracle's (x, u, v, Hx) against the dense minimiser at the oracle's w; returns the worst per-stage error"""
    ref = m.argmin(o.get("accXi"), o.get("accPsi"))
    assert ref["correction"] <= CORRECTION, "%s: the model's refinement correction %.1e does not qualify the case" % (what, ref["correction"])
    e = fp.argmin_errors(m, o.get, ref)
    w = fp.worst(e)
    assert w[0] <= TOL, (what,) + w
    return w[0], ref["correction"]


def assert_state(m, o, what, prox=True, tol=TOL):
    e = m.check_state(o.get, prox=prox)
    w = fp.worst(e)
    assert w[0] <= tol, (what,) + w
    return e


# ---- 1. solve_step is the argmin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", DUALS)
@pytest.mark.parametrize("name", DENSE)
def test_solve_step_is_the_dense_minimiser(name, kind):
    p, fc = problem(name)
    o, m = oracle(p, fc), fp.Model(p["network"], p["tree"], p["config"], fc)
    assert o.nodes * o.nv <= 616, "no dense case larger than `ragged`"
    set_duals(o, kind)
    o.solve_step()
    worst, corr = assert_argmin(m, o, "%s %s" % (name, kind))
    e = assert_state(m, o, "%s %s" % (name, kind), prox=False)
    record("oracle f64 argmin %-18s %-6s worst stage %.1e  correction %.1e  stationarity %.1e" % (name, kind, worst, corr, e["stationarity"].max()))
    assert e["stationarity"].max() <= ORACLE_STATIONARITY


@pytest.mark.parametrize("kind", DUALS)
@pytest.mark.parametrize("name", LARGE)
def test_solve_step_is_feasible_and_stationary(name, kind):
    p, fc = problem("medium" if name == "medium_lazy" else name)
    o, m = oracle(p, fc, lazy=name == "medium_lazy"), fp.Model(p["network"], p["tree"], p["config"], fc)
    set_duals(o, kind)
    o.solve_step()
    e = assert_state(m, o, "%s %s" % (name, kind), prox=False)
    record("oracle f64 residuals %-22s %-6s feasibility %.1e  stationarity %.1e" % (name, kind, max(e["feas_u"].max(), e["feas_x"].max()), e["stationarity"].max()))
    assert e["stationarity"].max() <= ORACLE_STATIONARITY, "the oracle's own stationarity figure says the scale is wrong"


def test_the_dense_solve_refuses_large_problems():
    p, fc = problem("medium")
    m = fp.Model(p["network"], p["tree"], p["config"], fc)
    with pytest.raises(ValueError):
        m.argmin(np.zeros(m.nodes * 2 * m.nx), np.zeros(m.nodes * m.nu))


def test_the_model_refuses_a_network_whose_A_is_not_the_identity():
    p, fc = problem("tiny")
    net = dict(p["network"])
    a = np.asarray(net["matA"], float).copy()
    a[0] = 0.99
    net["matA"] = a.tolist()
    with pytest.raises(AssertionError):
        fp.Model(net, p["tree"], p["config"], fc)


# ---- 2. every knob of the model against the same knob of the oracle --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "ragged"])
def test_a_second_control_step_from_another_state(name):
    p, fc = problem(name)
    fc2 = synth.forecast_at(p["forecast"], 1)
    rng = np.random.default_rng(5)
    x0 = np.asarray(p["config"]["currentX"], float) * (1 + 0.1 * rng.standard_normal(len(p["config"]["currentX"])))
    u0 = np.asarray(p["config"]["prevU"], float) * (1 + 0.2 * rng.standard_normal(len(p["config"]["prevU"])))
    d0 = np.asarray(fc[0], float)[: len(p["config"]["prevDemand"])] * 1.1
    o = oracle(p, fc)
    o.apg(5)
    o.update_state_control(x0, u0, d0)
    o.eliminate(*fc2)
    m = fp.Model(p["network"], p["tree"], p["config"], fc2, currentX=x0, prevU=u0, prevDemand=d0)
    for kind in DUALS:
        set_duals(o, kind)
        o.solve_step()
        assert_argmin(m, o, "%s step 2 %s" % (name, kind))
    stale = fp.Model(p["network"], p["tree"], p["config"], fc2)             # the model at the first step's state must be refused
    assert fp.worst(stale.check_state(o.get, prox=False))[0] >= REFUSED


@pytest.mark.parametrize("knob", [dict(weight_economical=0.35), dict(demand_uncertainty=False), dict(price_uncertainty=False),
                                  dict(weight_economical=2.5, demand_uncertainty=False, price_uncertainty=False)], ids=lambda k: "-".join(k))
@pytest.mark.parametrize("name", ["odd", "ragged"])
def test_uncertainty_switches_and_the_economic_weight(name, knob):
    """demand uncertainty off zeroes ALL demand errors in the oracle where the reference zeroes a prefix: the model
    follows the oracle"""
    p, fc = problem(name)
    o = oracle(p, fc)
    o.eliminate(*fc, **knob)
    m = fp.Model(p["network"], p["tree"], p["config"], fc, weightEconomical=knob.get("weight_economical", 1.0),
                 demandUncertainty=knob.get("demand_uncertainty", True), priceUncertainty=knob.get("price_uncertainty", True))
    for kind in DUALS:
        set_duals(o, kind)
        o.solve_step()
        assert_argmin(m, o, "%s %s %s" % (name, knob, kind))
    default = fp.Model(p["network"], p["tree"], p["config"], fc)            # the knob matters on these data
    assert fp.worst(default.check_state(o.get, prox=False))[0] >= REFUSED


@pytest.mark.parametrize("name", ["tiny", "ragged", "medium"])
def test_reweighted_probabilities_and_errors(name):
    p, fc = problem(name)
    new = reweighted(p, fc)
    o = oracle(p, fc, tree=new)
    m = fp.Model(p["network"], p["tree"], p["config"], fc, probNode=new["probNode"], errorDemandNode=new["errorDemandNode"],
                 errorPriceNode=new["errorPriceNode"])
    for kind in DUALS:
        set_duals(o, kind)
        o.solve_step()
        if m.nodes * m.nv <= fp.DENSE_LIMIT:
            assert_argmin(m, o, "%s re-weighted %s" % (name, kind))
        o.prox(); o.residual(); o.dual_update()
        assert_state(m, o, "%s re-weighted %s" % (name, kind))
    old = fp.Model(p["network"], p["tree"], p["config"], fc)
    assert fp.worst(old.check_state(o.get))[0] >= REFUSED


def stage_rows(p, seed):
    """physical bounds per stage: the network's, each row moved by its own factors; u row 1 is a pump out of service (umin = umax) from
    stage 2 on, x row 0 is held (xmin = xmax) at the last stage"""
    rng = np.random.default_rng(seed)
    n, N = p["network"], int(p["tree"]["N"][0])
    b = {k: np.repeat(np.asarray(n[j], float)[None, :], N, axis=0) for k, j in (("xmin", "vecXmin"), ("xmax", "vecXmax"), ("xsafe", "vecXsafe"),
                                                                               ("umin", "vecUmin"), ("umax", "vecUmax"))}
    b["xmax"] *= rng.uniform(0.7, 1.0, b["xmax"].shape)
    b["xsafe"] *= rng.uniform(1.0, 1.5, b["xsafe"].shape)
    b["umax"] *= rng.uniform(0.5, 1.0, b["umax"].shape)
    b["umax"][2:, 1] = b["umin"][2:, 1]
    b["xmax"][-1, 0] = b["xmin"][-1, 0]
    return b


def node_rows(p, seed):
    st = np.asarray(p["tree"]["stages"], int)[: int(p["tree"]["nodes"][0])]
    rng = np.random.default_rng(seed + 1)
    b = {k: v[st].copy() for k, v in stage_rows(p, seed).items()}
    b["xsafe"] *= rng.uniform(1.0, 1.25, b["xsafe"].shape)
    b["umax"][::3] *= 0.9
    return b


def oracle_bounds(o, rows, gran, p):
    """the oracle holds scaled per-node bounds: bound x (its own scaled bound / the network's), so that the scaling stays the factor step's"""
    st = np.asarray(p["tree"]["stages"], int)[: o.nodes]
    scale = {}
    for fam, name, net, dim in (("x", "xmax", "vecXmax", o.nx), ("xs", "xs", "vecXsafe", o.nx), ("u", "umax", "vecUmax", o.nu)):
        base = np.asarray(p["network"][net], float)
        assert (base != 0).all()
        scale[fam] = o.get(name).reshape(o.nodes, dim) / base
    for key, name, fam in (("xmin", "xmin", "x"), ("xmax", "xmax", "x"), ("xsafe", "xs", "xs"), ("umin", "umin", "u"), ("umax", "umax", "u")):
        o.set(name, scale[fam] * (rows[key][st] if gran == "stage" else rows[key]))


@pytest.mark.parametrize("gran", ["stage", "node"])
@pytest.mark.parametrize("name", ["small", "ragged"])
def test_bounds_per_stage_and_per_node_through_the_prox(name, gran):
    p, fc = problem(name)
    rows = stage_rows(p, 11) if gran == "stage" else node_rows(p, 11)
    o = oracle(p, fc)
    oracle_bounds(o, rows, gran, p)
    m = fp.Model(p["network"], p["tree"], p["config"], fc, bounds=dict(rows, granularity=gran))
    o.apg_reset()
    th = [1.0, 1.0]
    for it in range(12):
        th = o.apg_continue(1, th)
        if it in (0, 5, 11):
            assert_state(m, o, "%s %s bounds, iteration %d" % (name, gran, it + 1))
    shared = fp.Model(p["network"], p["tree"], p["config"], fc)
    assert fp.worst(shared.check_state(o.get))[0] >= REFUSED, "the moved bounds must be active"


@pytest.mark.parametrize("which,px,ps", [("both", 32.0, 2.5), ("box only", 32.0, 1e12), ("safety only", 1e12, 2.5)])
def test_soft_penalties_trip(which, px, ps):
    """`medium` with penalties 32 / 2.5 (tests/test_gpu_receding_horizon.py): both thresholds trip, each half with its own distance -- the
    documented divergence from the reference's both-thresholds branch -- and one threshold only"""
    p, fc = problem("medium", penalty_x=px, penalty_xs=ps)
    o = oracle(p, fc)
    m = fp.Model(p["network"], p["tree"], p["config"], fc)
    lam = m.step
    tripped = set()
    random_duals(o, 8)                                  # y = y+ = random normal duals: large enough for both distances at the first iteration
    for nm in ("xi", "updXi"):
        o.set(nm, o.get("accXi"))
    for nm in ("psi", "updPsi"):
        o.set(nm, o.get("accPsi"))
    th = [1.0, 1.0]
    for it in range(10):
        th = o.apg_continue(1, th)
        dx, ds = o.dist()
        tripped.add((dx > px / lam, ds > ps / lam))
        assert_state(m, o, "medium penalties %s, iteration %d" % (which, it + 1))
        want = m.prox(o.get("primalXi"), o.get("primalPsi"), o.get("accXi"), o.get("accPsi"))
        assert abs(want["distX"] - dx) <= TOL * dx and abs(want["distS"] - ds) <= TOL * ds
    expect = {"both": (True, True), "box only": (True, False), "safety only": (False, True)}[which]
    assert expect in tripped, (which, tripped)
    # the model's penalties are knobs of their own: handed in, not read from the config
    m2 = fp.Model(p["network"], p["tree"], dict(p["config"], penaltyStateX=[1.0], penaltySafetyX=[1.0]), fc, penaltyStateX=px, penaltySafetyX=ps)
    assert fp.worst(m2.check_state(o.get))[0] <= TOL


def test_the_step_size_is_a_knob():
    p, fc = problem("small")
    o = oracle(p, fc)
    lam = 0.5 * float(p["config"]["stepSize"][0])
    o.lib.oracle_set_params(o.h, lam, float(p["config"]["penaltyStateX"][0]), float(p["config"]["penaltySafetyX"][0]))
    o.apg(10)
    assert_state(fp.Model(p["network"], p["tree"], p["config"], fc, stepSize=lam), o, "small, half the step size")
    assert fp.worst(fp.Model(p["network"], p["tree"], p["config"], fc).check_state(o.get))[0] >= REFUSED


def test_across_a_momentum_restart_that_fires():
    """`small`, batches of 20 (tests/restart_oracle.py): the boundary at 180 fires; the state behind the next batch is a minimiser all the same"""
    import restart_oracle as ro

    p, fc = problem("small", feasible=True)
    o = oracle(p, fc)
    assert ro.restart_loop(o, 200, 20, restart=True, tol=0.0)["fires"] == [180]
    assert_state(fp.Model(p["network"], p["tree"], p["config"], fc), o, "small behind the restart")


# ---- 3. the other step entry points --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ["globalFbeAlgorithm", "namaAlgorithm"])
@pytest.mark.parametrize("name", DENSE + ["medium"])
def test_hessian_oracle_is_the_linear_part_of_the_argmin_map(name, algorithm):
    p, fc = problem(name)
    o = Oracle(p["network"], p["tree"], p["config"])
    o.set_algorithm(algorithm, 5)
    o.initialise(*fc)
    o.fbe_reset()
    m = fp.Model(p["network"], p["tree"], p["config"], fc)
    rng = np.random.default_rng(9)
    dxi, dpsi = rng.standard_normal(o.nodes * 2 * o.nx), rng.standard_normal(o.nodes * o.nu)
    src = ("gradXi", "gradPsi") if algorithm == "globalFbeAlgorithm" else ("resXi", "resPsi")
    o.set(src[0], dxi); o.set(src[1], dpsi)
    o.hessian_oracle()
    got = {"x": o.get("xdir"), "u": o.get("udir"), "v": o.get("v"), "primalXi": o.get("primalXiDir"), "primalPsi": o.get("primalPsiDir")}
    e = m.residuals(dxi, dpsi, got["x"], got["u"], got["v"], homogeneous=True)
    assert fp.worst(e)[0] <= TOL, fp.worst(e)
    if m.nodes * m.nv <= fp.DENSE_LIMIT:
        ref = m.hessian_direction(dxi, dpsi)
        assert ref["correction"] <= CORRECTION
        w = fp.worst(fp.argmin_errors(m, got, ref))
        assert w[0] <= TOL, w
        # the linear part: argmin(w + d) - argmin(w), the affine data cancelled
        w0 = rng.standard_normal(dxi.size), rng.standard_normal(dpsi.size)
        a, b = m.argmin(w0[0] + dxi, w0[1] + dpsi), m.argmin(*w0)
        for nm in ("x", "u", "v"):
            assert np.abs((a[nm] - b[nm]) - ref[nm]).max() <= 1e-12 * max(np.abs(a[nm]).max(), np.abs(ref[nm]).max()), nm
    record("oracle f64 hessian  %-18s %-18s worst %.1e" % (name, algorithm, fp.worst(e)[0]))


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("name", ["small", "ragged", "medium"])
def test_value_fbe_is_the_primal_value_plus_its_dual_terms(name, soft):
    """computeValueFbe = <w, r> + lambda / 2 |r|^2 + g(z) + sum_i p_i (du_i' W du_i + alpha_i' u_i), r = Hx - z; g(z) = gamma dist(z, C) per
    xi half where its threshold trips"""
    kw = dict(penalty_x=2.0, penalty_xs=1.0) if soft else {}      # (tests/test_gpu_apg_f32.py's pair: trips on the small trees too)
    p, fc = problem(name, **kw)
    o = Oracle(p["network"], p["tree"], p["config"])
    o.set_algorithm("globalFbeAlgorithm", 5)
    o.initialise(*fc)
    o.fbe_reset()
    m = fp.Model(p["network"], p["tree"], p["config"], fc)
    random_duals(o, 4, scale=1.0 if soft else 1e-3)
    o.solve_step(); o.prox(); o.residual()
    got = o.value_fbe()
    w = np.concatenate([o.get("accXi"), o.get("accPsi")])
    pr = m.prox(o.get("primalXi"), o.get("primalPsi"), o.get("accXi"), o.get("accPsi"))
    r = np.concatenate([pr["resXi"], pr["resPsi"]])
    terms = [float(w @ r), 0.5 * m.step * float(r @ r), m.primal_value(o.get("u"))]
    for dist, gamma in ((pr["distX"], m.gammaX), (pr["distS"], m.gammaS)):
        if dist > gamma / m.step:
            terms.append(gamma * (dist - gamma / m.step))
    assert (len(terms) == 5) == soft, "the soft case trips both thresholds, the other none"
    assert abs(got - sum(terms)) <= TOL * sum(abs(t) for t in terms), (got, terms)


# ---- 4. the fp32 oracle: the yardstick of the GPU bound -----------------------------------------------------------------------------------
def f32_state(p, fc, form, precision="f32"):
    """the fp32 oracle after solve_step + prox chain at fp32-representable random duals (form "step") or after one batch of 16 iterations from
    the fp32-rounded duals of 9 fp64 iterations (form "batch")"""
    o = oracle(p, fc, precision=precision)
    if form == "step":
        random_duals(o, 3)
        o.solve_step(); o.prox(); o.residual(); o.dual_update()
    else:
        d = oracle(p, fc)
        d.apg(9)
        o.apg_reset()
        for nm in ("xi", "psi", "updXi", "updPsi"):
            o.set(nm, np.asarray(d.get(nm), np.float32))
        o.apg_continue(16, [1.0, 1.0])
    return o


@pytest.mark.parametrize("form", ["step", "batch"])
@pytest.mark.parametrize("name", ["medium", "barcelona31"])
def test_f32_oracle_against_the_model(name, form):
    """e_cpu per stage: recorded as the yardstick of the GPU bound e_gpu <= 4 e_cpu + 32 * 2^-24 (tests/test_gpu_first_principles.py).  Here: finite,
    and rounding-sized on every quantity but the stationarity residual, which carries the conditioning of p_i L'WL at the leaves"""
    p, fc = problem(name)
    m = fp.Model(p["network"], p["tree"], p["config"], fc)
    e = m.check_state(f32_state(p, fc, form).get, scales="z")
    for nm, v in e.items():
        assert np.isfinite(v).all(), nm
        if nm != "stationarity":      # test_gpu_apg_f32.CAP: the derived bound must say more than the suite's FP32_TOL does
            assert 4 * v.max() + 32 * EPS32 <= 2e-4 / 4, (nm, v.max())
    record("oracle f32 e_cpu %-12s %-5s %s" % (name, form, "  ".join("%s %.1e" % (nm, v.max()) for nm, v in e.items())))


# ---- 5. negative controls: a mistake in the MODEL must be refused by the oracle -------------------------------------------------------------
@pytest.mark.parametrize("mistake", fp.PERTURBATIONS)
@pytest.mark.parametrize("name", ["ragged", "medium"])
def test_a_model_with_a_mistake_is_refused(name, mistake):
    """p_i for sqrt(p_i) in F / in G, d_x and d_xs swapped, the child term of du dropped at one branching node, Gd d_i dropped at one node,
    prevU - Lhat prevDemand dropped at the root, alpha per stage without errPrice, one distance shared by both xi halves.
    A control that is not refused means the data do not exercise that datum."""
    soft = dict(penalty_x=2.0, penalty_xs=1.0) if mistake == "shared_distance" else {}
    p, fc = problem(name, **soft)
    o = oracle(p, fc)
    good, bad = fp.Model(p["network"], p["tree"], p["config"], fc), fp.Model(p["network"], p["tree"], p["config"], fc, perturb=(mistake,))
    random_duals(o, 6)
    o.solve_step(); o.prox(); o.residual(); o.dual_update()
    if mistake == "shared_distance":
        dx, ds = o.dist()
        assert dx > good.gammaX / good.step and ds > good.gammaS / good.step, "both thresholds must trip for this control"
    assert fp.worst(good.check_state(o.get))[0] <= TOL
    e = bad.check_state(o.get)
    w = fp.worst(e)
    if bad.nodes * bad.nv <= fp.DENSE_LIMIT and mistake not in ("drop_child_term", "shared_distance"):
        wa = fp.worst(fp.argmin_errors(bad, o.get, bad.argmin(o.get("accXi"), o.get("accPsi"))))
        assert wa[0] >= REFUSED, (mistake,) + wa
    record("control %-24s %-7s refused at %.1e in %s, stage %d: %.0e x the bound" % (mistake, name, w[0], w[1], w[2], w[0] / TOL))
    assert w[0] >= REFUSED, (mistake,) + w
