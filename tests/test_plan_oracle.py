"""The numpy restatement of the plan report (tests/plan_oracle.py) checked by hand and shown to have teeth, without a GPU.

1. A three-node tree whose table was computed by hand.
2. Negative controls on `tiny`, `ragged` and `barcelona31` with the CPU oracle's x and u after 5 iterations: six ways of getting the
   bookkeeping wrong, each of which must move its column by more than 1e-6 of that column's sum of absolute terms -- a fixture on which a
   mistake does not show would prove nothing about the kernel that is compared with the restatement (tests/test_gpu_plan_report.py).
3. The cases of the GPU test meet its condition on the CPU oracle alone: every column is nonzero in at least half of the stages.

The helpers below (tightened bounds, the oracle run under them, the restatement of a run) are shared with the GPU test.  The fixtures'
own bounds leave columns dead (after one iteration from cold no input leaves its box; xmin is 0 everywhere), so every case runs under
tightened per-stage rows: umax_t = umin + f_t (umax - umin), f_t in (0.5, 0.35, 0.2) by stage mod 3; xmax_t = xmin + (0.7 - 0.3 t)(xmax -
xmin); xsafe_t = xmin + (1.0 + 0.2 t)(xmax - xmin), t = stage / (N - 1): the safety volume lies above the tightened xmax, so a tank is
short of it wherever the plan respects xmax and above xmax wherever it does not."""
import numpy as np
import pytest

import plan_oracle as po
from oracle.oracle import Oracle
from rapidnet_amd import synth

KEYS = ("xmin", "xmax", "xsafe", "umin", "umax")
NET = {"xmin": "vecXmin", "xmax": "vecXmax", "xsafe": "vecXsafe", "umin": "vecUmin", "umax": "vecUmax"}
ORACLE_BUF = {"xmin": "xmin", "xmax": "xmax", "xsafe": "xs", "umin": "umin", "umax": "umax"}

_PROBLEMS, _RUNS = {}, {}


def problem(name):
    if name not in _PROBLEMS:
        p = synth.make_problem(name)
        _PROBLEMS[name] = (p, synth.forecast_at(p["forecast"], 0))
    return _PROBLEMS[name]


def tree_arrays(tree):
    """(parent [nodes], -1 for the root; stage [nodes])"""
    return np.asarray(tree["ancestor"], int) - 1, np.asarray(tree["stages"], int)


def tight_rows(p):
    """the tightened per-stage rows of the module docstring: {key: [N][dim]}"""
    N = int(p["tree"]["N"][0])
    own = {k: np.asarray(p["network"][NET[k]], float)[None, :] for k in KEYS}
    s = np.arange(N)
    t = (s / (N - 1))[:, None]
    fu = np.array([0.5, 0.35, 0.2])[s % 3][:, None]
    rx, ru = own["xmax"] - own["xmin"], own["umax"] - own["umin"]
    return {"xmin": np.repeat(own["xmin"], N, 0), "xmax": own["xmin"] + (0.7 - 0.3 * t) * rx, "xsafe": own["xmin"] + (1.0 + 0.2 * t) * rx,
            "umin": np.repeat(own["umin"], N, 0), "umax": own["umin"] + fu * ru}


def node_rows(rows, tree):
    """per-node rows: a node takes its stage's row; every second node of the last stage gets a lower safety volume and a wider umax"""
    _, stage = tree_arrays(tree)
    out = {k: v[stage].copy() for k, v in rows.items()}
    sel = np.flatnonzero(stage == stage.max())[::2]
    out["xsafe"][sel] *= 0.9
    out["umax"][sel] += 0.1 * (out["umax"][sel] - out["umin"][sel])
    return out


def table_for(p, gran, tree=None):
    """(the bounds rows the context is given, the row of every node)"""
    tree = p["tree"] if tree is None else tree
    _, stage = tree_arrays(tree)
    rows = tight_rows(p)
    if gran == "stage":
        return rows, stage
    return node_rows(rows, tree), np.arange(len(stage))


def scaled_bounds(p, tree, rows, brow):
    """the oracle's scaled per-node bounds for physical rows: sqrt(p_i) d_c v (Engine.cu preconditionConstraintX / U)"""
    _, stage = tree_arrays(tree)
    nx, nu = int(np.ravel(p["network"]["nx"])[0]), int(np.ravel(p["network"]["nu"])[0])
    diag = np.asarray(p["config"]["matDiagPrecnd"], float).reshape(-1, nu + 2 * nx)[stage]      # [N][d_u | d_x | d_xs] by stage
    sp = np.sqrt(np.asarray(tree["probNode"], float))[:, None]
    d = {"xmin": diag[:, nu:nu + nx], "xmax": diag[:, nu:nu + nx], "xsafe": diag[:, nu + nx:], "umin": diag[:, :nu], "umax": diag[:, :nu]}
    return {k: sp * d[k] * rows[k][brow] for k in KEYS}


def oracle_run(name, iters, gran="stage", tree=None, tag=None, nama=False):
    """x, u, alpha of the CPU oracle under the tightened bounds after `iters` iterations from cold; computed once per case and not changed"""
    key = (name, iters, gran, tag, nama)
    if key not in _RUNS:
        p, fc = problem(name)
        tree = p["tree"] if tree is None else tree
        o = Oracle(p["network"], tree, p["config"])
        if nama:
            o.set_algorithm("namaAlgorithm", 5)
        o.factor_step()
        rows, brow = table_for(p, gran, tree)
        for k, v in scaled_bounds(p, tree, rows, brow).items():
            o.set(ORACLE_BUF[k], v)
        o.update_state_control()
        o.eliminate(*fc)
        if nama:
            o.fbe_reset()
            o.fbe_nama(iters)
        else:
            o.apg(iters)
        _RUNS[key] = {k: o.get(k).copy() for k in ("x", "u", "alpha")}
    return _RUNS[key]


def restate(p, tree, xua, rows, brow, prob=None, prevU=None, W=None, **kw):
    parent, stage = tree_arrays(tree)
    nx, nu = int(np.ravel(p["network"]["nx"])[0]), int(np.ravel(p["network"]["nu"])[0])
    return po.evaluate(np.asarray(xua["x"]).reshape(-1, nx), np.asarray(xua["u"]).reshape(-1, nu), np.asarray(xua["alpha"]).reshape(-1, nu),
                       np.asarray(p["config"]["prevU"], float).ravel() if prevU is None else prevU,
                       np.asarray(tree["probNode"], float) if prob is None else prob, np.asarray(p["config"]["costW"], float) if W is None else W,
                       kw.pop("parent", parent), stage, rows["xmin"], rows["xmax"], rows["xsafe"], rows["umin"], rows["umax"], brow, **kw)


def assert_alive(r, what):
    frac = po.alive(r["stage"])
    assert (frac >= 0.5).all(), "%s: columns %s are nonzero in fewer than half of the stages (%s)" % (
        what, [po.COLUMNS[i] for i in np.flatnonzero(frac < 0.5)], np.round(frac, 2))


# ---- 1. by hand ----------------------------------------------------------------------------------------------------------------------------
def test_three_node_tree_by_hand():
    x = np.array([[5.0, 1.0], [3.0, 8.0], [0.5, 2.0]])
    u = np.array([[1.0, 2.0], [2.0, 0.0], [-1.0, 3.0]])
    alpha = np.array([[1.0, 0.5], [2.0, 1.0], [0.5, -1.0]])
    W = np.array([[2.0, 0.5], [0.5, 1.0]])
    b = dict(xmin=np.array([[1.0, 1.5]]), xmax=np.array([[4.0, 6.0]]), xs=np.array([[2.0, 3.0]]), umin=np.array([[0.0, 0.5]]), umax=np.array([[1.5, 2.5]]))
    r = po.evaluate(x, u, alpha, [0.0, 1.0], [1.0, 0.25, 0.75], W, [-1, 0, 0], [0, 1, 1], brow=[0, 0, 0], **b)
    # node terms, not weighted: ECON, SMOOTH, STORED, SHORT, XBOX, UBOX | the three maxima
    #   node 0: du = (1, 1):    2,    4,  6,    2,   1.5, 0   | 2,   1,   0
    #   node 1: du = (1, -2):   4,    4,  11,   0,   2,   1   | 0,   2,   0.5
    #   node 2: du = (-2, 1):  -3.5,  7,  2.5,  2.5, 0.5, 1.5 | 1.5, 0.5, 1
    want_stage = np.array([[2.0, 4.0, 6.0, 2.0, 1.5, 0.0, 2.0, 1.0, 0.0],
                           [-1.625, 6.25, 4.625, 1.875, 0.875, 1.375, 1.5, 2.0, 1.0]])
    want_leaf = np.array([[6.0, 8.0, 11.0, 2.0, 3.5, 1.0, 2.0, 2.0, 0.5],
                          [-1.5, 11.0, 2.5, 4.5, 2.0, 1.5, 2.0, 1.0, 1.0]])
    assert np.array_equal(r["stage"], want_stage), r["stage"]
    assert np.array_equal(r["leaf"], want_leaf), r["leaf"]
    assert np.array_equal(r["leafNode"], [1, 2])
    assert np.array_equal(r["stage_m"][1], 2 * np.array([2, 4, 2, 2, 4, 4]))
    assert np.array_equal(r["leaf_m"][0], [4, 8, 2, 4, 8, 8])
    assert r["stage_abs"][1, po.ECON] == 0.25 * 4.0 + 0.75 * 3.5 and r["stage_abs"][1, po.SMOOTH] == 0.25 * 8.0 + 0.75 * 11.0
    # the cost distribution adds up: sum_leaf p_leaf ECON_leaf = sum_stage ECON_stage
    assert 0.25 * 6.0 + 0.75 * -1.5 == want_stage[:, 0].sum()


# ---- 2. negative controls ------------------------------------------------------------------------------------------------------------------
CONTROL_TREES = ("tiny", "ragged", "barcelona31")


def controls(p, tree, rows):
    parent, stage = tree_arrays(tree)
    crown = np.where(stage < 2, 2.0, 1.0)          # two ranks, cut at stage 2: the crown counted on both
    return [("p dropped from SMOOTH", po.SMOOTH, dict(variant="smooth_unweighted")),
            ("the root's du taken against 0", po.SMOOTH, dict(prevU=np.zeros_like(np.asarray(p["config"]["prevU"], float).ravel()))),
            ("xs read from the xmin column", po.SHORT_EXP, dict(rows=dict(rows, xsafe=rows["xmin"]))),
            ("the crown counted on every rank", po.ECON, dict(mult=crown)),
            ("the parent taken as i - 1", po.SMOOTH, dict(parent=np.arange(len(parent)) - 1)),
            ("SHORT_MAX weighted by p", po.SHORT_MAX, dict(variant="short_max_weighted"))]


@pytest.mark.parametrize("name", CONTROL_TREES)
def test_negative_controls_move_their_column(name):
    p, _ = problem(name)
    rows, brow = table_for(p, "stage")
    xua = oracle_run(name, 5)
    good = restate(p, p["tree"], xua, rows, brow)
    assert_alive(good, name)
    for what, col, kw in controls(p, p["tree"], rows):
        kw = dict(kw)
        bad = restate(p, p["tree"], xua, kw.pop("rows", rows), brow, **kw)
        moved = np.abs(bad["stage"][:, col] - good["stage"][:, col]).sum()
        scale = good["stage_abs"][:, col].sum() if col < po.SUMS else good["stage"][:, col].max()
        print("%s: %s moves %s by %.2e of its scale" % (name, what, po.COLUMNS[col], moved / scale))
        assert moved > 1e-6 * scale, (name, what)


# ---- 3. the GPU test's cases keep every column alive on the oracle alone ------------------------------------------------------------------------
@pytest.mark.parametrize("name,iters,gran", [("tiny", 1, "stage"), ("tiny", 5, "stage"), ("tiny", 40, "stage"), ("odd", 5, "stage"), ("odd", 40, "node"),
                                             ("ragged", 1, "stage"), ("ragged", 40, "node"), ("barcelona31", 5, "stage"), ("medium", 24, "stage"), ("odd", -8, "stage")])
def test_every_column_is_alive_in_the_cases_of_the_gpu_test(name, iters, gran):
    """(a negative count: that many NAMA iterations)"""
    p, _ = problem(name)
    rows, brow = table_for(p, gran)
    assert_alive(restate(p, p["tree"], oracle_run(name, abs(iters), gran, nama=iters < 0), rows, brow), "%s after %d iterations, %s rows" % (name, iters, gran))
