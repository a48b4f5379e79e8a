"""rn_plan_report, rn_plan_report_scenarios, rn_plan_report_device (k_plan_report, k_plan.hpp): what a plan costs and where it violates its
bounds, per stage and per scenario, against the numpy restatement tests/plan_oracle.py.

A  the kernel alone.  The restatement is fed what the context itself holds, and every getter used here returns doubles:
     rn_get(RN_BUF_X / _U / _ALPHA)   the context's own values (an fp32 context: its floats, converted exactly);
     rn_get_bounds                    the physical rows as the context keeps them, in its own type (fp32: floats, converted exactly);
     rn_get_tree_data                 probNode AS GIVEN, in doubles, on fp32 contexts too -- the kernel reads the context's fp32 copy there, so
                                      the test rounds what this getter returns to fp32 for an fp32 context;
     costW and prevU have no getter: the test takes what it handed in, rounded to fp32 for an fp32 context (rn_factor_step and
                                      rn_update_state_control upload with one rounding to nearest).
   Both sides then sum the same exact fp64 terms in different orders: a sum column must satisfy |gpu - numpy| <= 2 (m + 2) 2^-53 sum|terms|
   (m terms: (m - 1) roundings of either summation and at most three of a term's own products), a maximum column must be equal bit for bit.
B  end to end, fp64 contexts with fp64 blocks: the same tables against the restatement on the CPU ORACLE's x, u and alpha, at the project's
   parity level: 1e-9 of the row's sum|terms| (2e-9 for the quadratic column), maxima 1e-9 of the stage's max |x| or |u|.
Every case runs under the tightened bounds of tests/test_plan_oracle.py and must have every column nonzero in at least half of the stages
according to the restatement, or it FAILS: a table of zeros proves nothing.

When PLAN_REPORT_ERRORS names a file, the worst ratios of every case are appended to it (profiles/plan_report_errors.txt is such a file)."""
import gc
import os

import numpy as np
import pytest

import plan_oracle as po
from rapidnet_amd import capi
from test_gpu_device_pointer import _d2h
from test_gpu_sharded_batched import Ranks
from test_gpu_tree_data import make, reweighted
from test_plan_oracle import KEYS, assert_alive, oracle_run, problem, restate, table_for, tree_arrays

pytestmark = pytest.mark.gpu

RN_E_ARG, RN_E_STATE = -1, -3
U = 2.0 ** -53


def record(line):
    print(line)
    path = os.environ.get("PLAN_REPORT_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def tables(s):
    """(stage [N][9], leaf [leaves][9], leafNode) through the Python layer"""
    r = s.planReport()
    return (np.stack([r["stage"][k] for k in capi.PLAN_COLUMNS], 1), np.stack([r["scenario"][k] for k in capi.PLAN_COLUMNS], 1), r["leafNode"])


def f32_if(kind, a):
    a = np.asarray(a, float)
    return a.astype(np.float32).astype(np.float64) if kind == "f32" else a


def held(s, p, tree, kind, prevU=None):
    """the restatement on what the context holds (A)"""
    nx, nu = s.nx, s.nu
    xua = {"x": s.get(capi.BUF_X), "u": s.get(capi.BUF_U), "alpha": s.get(capi.BUF_ALPHA)}
    b = s.getBounds()
    _, stage = tree_arrays(tree)
    brow = {capi.BOUNDS_SHARED: np.zeros(len(stage), int), capi.BOUNDS_PER_STAGE: stage, capi.BOUNDS_PER_NODE: np.arange(len(stage))}[b["granularity"]]
    rows = {k: b[k] for k in KEYS}
    return restate(p, tree, xua, rows, brow, prob=f32_if(kind, s.getTreeData()["prob"]), W=f32_if(kind, p["config"]["costW"]),
                   prevU=f32_if(kind, np.ravel(p["config"]["prevU"]) if prevU is None else prevU))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_a(what, stage, leaf, leaf_node, r):
    """the kernel against the restatement of its own inputs; returns the worst share of the bound used"""
    assert_alive(r, what)
    worst = 0.0
    for got, want, ab, m, rows in ((stage, r["stage"], r["stage_abs"], r["stage_m"], "stage"), (leaf, r["leaf"], r["leaf_abs"], r["leaf_m"], "leaf")):
        assert np.isfinite(got).all(), (what, rows)
        bound = 2.0 * (m + 2.0) * U * ab
        err = np.abs(got[:, :po.SUMS] - want[:, :po.SUMS])
        assert (err <= bound).all(), (what, rows, "sum columns", [po.COLUMNS[c] for c in np.flatnonzero((err > bound).any(0))], float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert np.array_equal(bits(got[:, po.SUMS:]), bits(want[:, po.SUMS:])), (what, rows, "maxima", got[:, po.SUMS:] - want[:, po.SUMS:])
    assert np.array_equal(leaf_node, r["leafNode"]), what
    return worst


def check_b(what, stage, leaf, r):
    """the tables against the restatement on the oracle's iterates; returns the worst ratios (sums, maxima) to their tolerances"""
    assert_alive(r, what + " (oracle)")
    tol = np.full(po.SUMS, 1e-9)
    tol[po.SMOOTH] = 2e-9
    ws = wm = 0.0
    for got, want, ab, rows in ((stage, r["stage"], r["stage_abs"], "stage"), (leaf, r["leaf"], r["leaf_abs"], "leaf")):
        err = np.abs(got[:, :po.SUMS] - want[:, :po.SUMS])
        ratio = np.divide(err, tol * ab, out=np.zeros_like(err), where=ab > 0)
        ws = max(ws, float(ratio.max()))
        print("%s, %s rows: worst error / (tol * sum|terms|) by column %s" % (what, rows, np.array2string(ratio.max(0), precision=2)))
        assert (err <= tol * ab).all(), (what, rows, [po.COLUMNS[c] for c in np.flatnonzero((err > tol * ab).any(0))], ws)
    scale = np.stack([r["stage_absmax_x"], r["stage_absmax_x"], r["stage_absmax_u"]], 1)
    errm = np.abs(stage[:, po.SUMS:] - r["stage"][:, po.SUMS:])
    wm = float((errm / (1e-9 * scale)).max())
    assert (errm <= 1e-9 * scale).all(), (what, "maxima", wm)
    lscale = np.array([r["stage_absmax_x"].max(), r["stage_absmax_x"].max(), r["stage_absmax_u"].max()])
    assert (np.abs(leaf[:, po.SUMS:] - r["leaf"][:, po.SUMS:]) <= 1e-9 * lscale).all(), (what, "maxima of the leaf rows")
    return ws, wm


def context(name, mode, kind, gran, tree=None, **kw):
    p, fc = problem(name)
    s = make(p, p["tree"] if tree is None else tree, mode, kind, **kw)
    s.initialiseSmpcController(*fc)
    rows, _ = table_for(p, gran, tree)
    s.setBounds(gran, **rows)
    return s


def both(what, s, p, tree, kind, oracle=None, prevU=None):
    stage, leaf, leaf_node = tables(s)
    wa = check_a(what, stage, leaf, leaf_node, held(s, p, tree, kind, prevU))
    line = "%s: A %.3f of the bound" % (what, wa)
    if oracle is not None:
        rows, brow = oracle["table"]
        ws, wm = check_b(what, stage, leaf, restate(p, tree, oracle["xua"], rows, brow, prevU=prevU))
        line += "; B sums %.2e, maxima %.2e of their tolerances" % (ws, wm)
    record(line)
    return stage, leaf


# ---- 1. cold APG solves: 1, 5 and 40 iterations; dense, structured and fp32-stored blocks; fp32 contexts; per-stage and per-node rows ------------
CASES = [("tiny", "dense", "f64", 1, "stage"), ("tiny", "dense", "f64", 5, "stage"), ("tiny", "structured", "f64", 40, "stage"),
         ("odd", "dense", "f64_store32", 5, "stage"), ("odd", "structured", "f32", 40, "node"), ("odd", "dense", "f64", 40, "node"),
         ("ragged", "dense", "f32", 1, "stage"), ("ragged", "structured", "f64", 1, "stage"), ("ragged", "dense", "f64", 40, "node"),
         ("barcelona31", "dense", "f64", 5, "stage"), ("barcelona31", "structured", "f32", 5, "stage")]


@pytest.mark.parametrize("name,mode,kind,iters,gran", CASES)
def test_tables_after_a_cold_solve(name, mode, kind, iters, gran):
    p, fc = problem(name)
    s = context(name, mode, kind, gran)
    s.apgReset()
    s.apgIterate(iters)
    oracle = {"xua": oracle_run(name, iters, gran), "table": table_for(p, gran)} if kind == "f64" else None
    stage, leaf = both("%s %s %s, %d iterations, %s rows" % (name, mode, kind, iters, gran), s, p, p["tree"], kind, oracle)
    # the cost distribution over the scenarios adds up to the expected cost: sum_leaf p_leaf ECON_leaf = sum_i (sum of the leaves' p below i)
    # alpha_i' u_i, which is the per-stage total wherever p_i is the sum of its leaves' -- up to the defect of the fixture's p in that
    prob = np.asarray(p["tree"]["probNode"], float)
    parent, st = tree_arrays(p["tree"])
    r = held(s, p, p["tree"], kind)
    below = np.zeros(len(prob))
    for lf in np.flatnonzero(st == st.max()):
        i = lf
        while i >= 0:
            below[i] += prob[lf]
            i = parent[i]
    pl = prob[r["leafNode"]]
    m = r["stage_m"][:, po.ECON].sum() + len(pl)
    bound = 2.0 * (m + 2.0) * U * (pl * r["leaf_abs"][:, po.ECON]).sum() + (np.abs(below - f32_if(kind, prob)) * r["node_abs"][:, po.ECON]).sum()
    assert abs((pl * leaf[:, po.ECON]).sum() - stage[:, po.ECON].sum()) <= bound
    s.close()


# ---- 2. after rn_set_tree_data, after a warm second rn_control_action, after a NAMA run ---------------------------------------------------------
@pytest.mark.parametrize("mode,kind", [("dense", "f64"), ("structured", "f32")])
def test_tables_after_a_reweighting(mode, kind):
    name = "ragged"
    p, fc = problem(name)
    new = reweighted(p["tree"], fc, 7)
    s = context(name, mode, kind, "stage")
    s.apgReset()
    s.apgIterate(3)
    s.updateTree(new)
    assert s.lib.rn_plan_report(s.h, s.N, np.zeros((s.N, 9)).ctypes.data) == RN_E_STATE      # the affine terms are the old tree's
    s.updateStateControl()
    s.eliminateInputDistubanceCoupling(*fc)
    s.apgReset()
    s.apgIterate(5)
    oracle = {"xua": oracle_run(name, 5, "stage", tree=new, tag="reweighted"), "table": table_for(p, "stage", new)} if kind == "f64" else None
    both("%s %s %s after rn_set_tree_data" % (name, mode, kind), s, p, new, kind, oracle)
    s.close()


def warm_oracle(name, n0, n1, x1):
    """the two-step recipe of tests/test_gpu_receding_horizon.py under the tightened bounds; returns (the first step's u0, x / u / alpha after
    the second step)"""
    from oracle.oracle import Oracle
    from test_plan_oracle import ORACLE_BUF, scaled_bounds

    p, fc = problem(name)
    o = Oracle(p["network"], p["tree"], p["config"])
    o.factor_step()
    rows, brow = table_for(p, "stage")
    for k, v in scaled_bounds(p, p["tree"], rows, brow).items():
        o.set(ORACLE_BUF[k], v)
    o.update_state_control()
    o.eliminate(*fc)
    o.apg(n0)
    u0 = o.get("u")[: o.nu].copy()
    o.set("xi", o.get("updXi")); o.set("psi", o.get("updPsi"))
    o.update_state_control(x1, u0, np.ravel(p["config"]["prevDemand"]))
    o.eliminate(*fc)
    o.apg_continue(n1, [1.0, 1.0])
    return u0, {k: o.get(k).copy() for k in ("x", "u", "alpha")}


@pytest.mark.parametrize("mode,kind", [("dense", "f64"), ("dense", "f32")])
def test_tables_after_a_warm_second_control_action(mode, kind):
    name = "tiny"
    p, fc = problem(name)
    x1 = 0.97 * np.asarray(p["config"]["currentX"], float).ravel()
    u0, xua = warm_oracle(name, 20, 20, x1)
    s = context(name, mode, kind, "stage")
    s.setWarmStart(True)
    s.controlAction(*fc, maxIterations=20)
    s.controlAction(*fc, currentX=x1, prevU=u0, maxIterations=20)      # (the oracle's u0: both sides start the second step from the same numbers)
    oracle = {"xua": xua, "table": table_for(p, "stage")} if kind == "f64" else None
    both("%s %s %s after a warm second control action" % (name, mode, kind), s, p, p["tree"], kind, oracle, prevU=u0)
    s.close()


def test_tables_after_a_nama_run():
    name = "odd"
    p, fc = problem(name)
    s = context(name, "dense", "f64", "stage")
    s.setAlgorithm("namaAlgorithm", 5)
    s.algorithmNama(8)
    oracle = {"xua": oracle_run(name, 8, "stage", nama=True), "table": table_for(p, "stage")}
    both("%s dense f64 after 8 NAMA iterations" % name, s, p, p["tree"], "f64", oracle)
    s.close()


# ---- 3. the same bits twice; host and device forms; memory ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("odd", "f64"), ("barcelona31", "f32")])
def test_two_calls_give_the_same_bits_allocate_once_and_the_device_form_holds_the_host_forms_bits(name, kind):
    s = context(name, "dense", kind, "node")
    m_never = s.deviceMemoryInfo()["context_bytes"]
    s.apgReset()
    s.apgIterate(5)
    assert s.deviceMemoryInfo()["context_bytes"] == m_never            # nothing is allocated for a context that has not asked
    a = tables(s)
    m1 = s.deviceMemoryInfo()["context_bytes"]
    leaves = s.planLeaves()
    assert m1 - m_never == 8 * 9 * (s.nodes + s.N + leaves) + 4 * leaves
    b = tables(s)
    ps, pl, n = s.planReportDevice()
    s.synchronize()
    assert s.deviceMemoryInfo()["context_bytes"] == m1                  # later calls allocate nothing
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y)
    assert n == leaves
    assert np.array_equal(bits(_d2h(ps, 9 * s.N, "f64").reshape(9, s.N).T), bits(a[0]))      # column-major on the device
    assert np.array_equal(bits(_d2h(pl, 9 * leaves, "f64").reshape(leaves, 9)), bits(a[1]))
    s.close()


# ---- 4. sharded: every rank the same bits, the one-GPU table within bound A ---------------------------------------------------------------------
@pytest.mark.parametrize("world,structured", [(2, False), (3, True)])
def test_shards_hold_the_whole_trees_table(world, structured):
    name = "medium"
    p, fc = problem(name)
    rows, _ = table_for(p, "stage")
    one = context(name, "structured" if structured else "dense", "f64", "stage")
    one.apgReset()
    one.apgIterate(24)
    want_stage, want_leaf, want_nodes = tables(one)
    r = held(one, p, p["tree"], "f64")
    assert_alive(r, "medium, 24 iterations")
    src = {bid: one.get(bid) for bid in (capi.BUF_X, capi.BUF_U, capi.BUF_ALPHA)}
    one.close()
    rk = Ranks(p, world, 0, structured)
    try:
        def solve(s):
            s.initialiseSmpcController(*fc)
            s.setBounds("stage", **rows)
            s.apgReset()
            s.apgIterate(24)
            g = np.asarray(s.global_nodes, int)
            for bid, dim in ((capi.BUF_X, s.nx), (capi.BUF_U, s.nu), (capi.BUF_ALPHA, s.nu)):      # the one-GPU run's plan, so that both tables
                s.set(bid, src[bid].reshape(-1, dim)[g])                                            # sum the same terms
            return tables(s)

        out = rk.run(solve)
        bound = 2.0 * (r["stage_m"] + 2.0) * U * r["stage_abs"]
        for rank, (stage, leaf, leaf_node) in enumerate(out):
            assert np.array_equal(bits(stage), bits(out[0][0])), rank                                # every rank holds the same bits
            assert (np.abs(stage[:, :po.SUMS] - want_stage[:, :po.SUMS]) <= bound).all(), rank
            assert np.array_equal(bits(stage[:, po.SUMS:]), bits(want_stage[:, po.SUMS:])), rank
            g = np.asarray(rk.shards[rank].global_nodes, int)[leaf_node]                             # local rows: the crown is replicated,
            sel = np.searchsorted(want_nodes, g)                                                     # every path is complete on its rank
            assert np.array_equal(want_nodes[sel], g)
            lb = 2.0 * (r["leaf_m"][sel] + 2.0) * U * r["leaf_abs"][sel]
            assert (np.abs(leaf[:, :po.SUMS] - want_leaf[sel, :po.SUMS]) <= lb).all(), rank
            assert np.array_equal(bits(leaf[:, po.SUMS:]), bits(want_leaf[sel, po.SUMS:])), rank
        assert sorted(np.concatenate([np.asarray(rk.shards[k].global_nodes, int)[out[k][2]] for k in range(world)]).tolist()) == want_nodes.tolist()
        record("medium on %d shards (%s): every rank the same bits, worst %.3f of bound A against the one-GPU table" % (
            world, "structured" if structured else "dense", float((np.abs(out[0][0][:, :po.SUMS] - want_stage[:, :po.SUMS])[bound > 0] / bound[bound > 0]).max())))
    finally:
        rk.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_state():
    name = "odd"
    p, fc = problem(name)
    s = make(p, p["tree"], "dense", "f64")
    lib, C = s.lib, capi.C
    N, leaves = s.N, s.planLeaves()
    st, lf, ln = np.zeros((N, 9)), np.zeros((leaves, 9)), np.zeros(leaves, np.int32)
    a, b, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)

    def all_three():
        return (lib.rn_plan_report(s.h, N, st.ctypes.data), lib.rn_plan_report_scenarios(s.h, leaves, lf.ctypes.data, ln.ctypes.data),
                lib.rn_plan_report_device(s.h, C.byref(a), C.byref(b), C.byref(n)))

    assert all_three() == (RN_E_STATE,) * 3                                                 # before the factor step
    s.factorStep()
    s.updateStateControl()
    assert all_three() == (RN_E_STATE,) * 3                                                 # before the affine terms
    s.eliminateInputDistubanceCoupling(*fc)
    assert all_three() == (RN_E_STATE,) * 3                                                 # before the first sweep
    assert "first sweep" in lib.rn_last_error(s.h).decode()
    m0 = s.deviceMemoryInfo()["context_bytes"]
    s.apgReset()
    s.apgIterate(2)
    for cnt in (N - 1, N + 1, 0):
        assert lib.rn_plan_report(s.h, cnt, st.ctypes.data) == RN_E_ARG
    for cnt in (leaves - 1, leaves + 1, s.nodes):
        assert lib.rn_plan_report_scenarios(s.h, cnt, lf.ctypes.data, ln.ctypes.data) == RN_E_ARG
    assert lib.rn_plan_report(s.h, N, None) == RN_E_ARG
    assert lib.rn_plan_report_scenarios(s.h, leaves, None, ln.ctypes.data) == RN_E_ARG
    assert lib.rn_plan_report_device(s.h, None, C.byref(b), C.byref(n)) == RN_E_ARG
    assert lib.rn_plan_report_device(s.h, C.byref(a), None, C.byref(n)) == RN_E_ARG
    assert lib.rn_plan_report_device(s.h, C.byref(a), C.byref(b), None) == RN_E_ARG
    assert s.deviceMemoryInfo()["context_bytes"] == m0                                      # none of the refused calls allocated anything
    assert all_three() == (0, 0, 0)
    assert lib.rn_plan_report_scenarios(s.h, leaves, lf.ctypes.data, None) == 0             # leafNode may be NULL
    assert np.isfinite(st).all() and np.isfinite(lf).all() and a.value and b.value and n.value == leaves
    s.close()


# ---- 6. guard mode -----------------------------------------------------------------------------------------------------------------------------
def test_under_the_buffer_guard(monkeypatch):
    """RAPIDNET_GUARD=1 (read when a context is created): every buffer between red zones and NaN until written.  A row read outside the
    tables would bring a NaN into the report (check_a asserts finiteness), a write outside a buffer changes a red zone."""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    for name, mode, kind, gran in (("odd", "dense", "f64", "node"), ("ragged", "structured", "f32", "stage")):
        p, fc = problem(name)
        s = context(name, mode, kind, gran)
        s.apgReset()
        s.apgIterate(5)
        both("guard: %s %s %s" % (name, mode, kind), s, p, p["tree"], kind)
        assert s.guardCheck() == 0
        s.close()
    after = capi.guard_report()
    assert after[0] - before[0] == 2 and after[1] == before[1]      # both contexts were checked once more when they went away: 0 bytes
