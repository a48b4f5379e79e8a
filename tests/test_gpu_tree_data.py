"""Scenario probabilities and tree errors replaced in place (rn_set_tree_data, rn_set_tree_data_device, rn_get_tree_data; k_tree_data).

The contract: a context that is handed a re-weighted tree of the same topology is, after the elimination that has to follow, bit for bit a
context freshly created on that tree -- through the host and the device form, in every operator mode and storage type, unsharded and sharded --
and agrees with the CPU oracle of the new tree at the suite's tolerances.

The fresh context's results are computed once per (tree, mode, kind) and shared (fresh())."""
import copy
import gc

import numpy as np
import pytest
import torch

from oracle.oracle import Oracle
from rapidnet_amd import capi, partition, synth
from test_gpu_parity import FP32_TOL, PAIRS, REL_TOL, compare_all, relmax
from test_gpu_sharded_batched import Ranks

pytestmark = pytest.mark.gpu

TREES = ["tiny", "odd", "ragged", "small"]
MODES = ["dense", "structured", "auto"]
KINDS = ["f64", "f32", "f64_store32"]       # the context's precision, and fp32-stored blocks under fp64 iterates
RN_E_ARG, RN_E_STATE = -1, -3
BEFORE, AFTER = 20, 40
ALL_BUFS = PAIRS + [(capi.BUF_UHAT, "uhat"), (capi.BUF_E, "e"), (capi.BUF_BETA, "beta"), (capi.BUF_ALPHA, "alpha"), (capi.BUF_XMIN, "xmin"),
                    (capi.BUF_XMAX, "xmax"), (capi.BUF_XS, "xs"), (capi.BUF_UMIN, "umin"), (capi.BUF_UMAX, "umax")]
ALL_OPS = (capi.OP_PHI, capi.OP_PSI, capi.OP_D, capi.OP_F, capi.OP_OMEGA, capi.OP_THETA, capi.OP_G)

_PROBLEMS, _FRESH = {}, {}


def problem(name):
    """(problem, (nominal demand, nominal prices), re-weighted tree)"""
    if name not in _PROBLEMS:
        p = synth.make_problem(name)
        fc = synth.forecast_at(p["forecast"], 0)
        _PROBLEMS[name] = (p, fc, reweighted(p["tree"], fc, 7))
    return _PROBLEMS[name]


def reweighted(tree, fc, seed, float32=False):
    """the same topology with new probabilities -- every non-leaf node deals its own among its children by weights drawn from [0.2, 1] --
    and new errors at synth.make_tree's scale.  float32: every value representable in fp32 (children products rounded)."""
    rng = np.random.default_rng(seed)
    nodes, N = int(tree["nodes"][0]), int(tree["N"][0])
    nd, nu = int(tree["dimDemand"][0]), int(tree["dimPrice"][0])
    anc = np.asarray(tree["ancestor"], int) - 1
    stages = np.asarray(tree["stages"], int)
    old = np.asarray(tree["probNode"], float)
    kids = [[] for _ in range(nodes)]
    for c in range(1, nodes):
        kids[anc[c]].append(c)
    prob = np.ones(nodes)
    for i in range(nodes):              # stage by stage: the parent's probability is final
        if kids[i]:
            w = rng.uniform(0.2, 1.0, len(kids[i]))
            w = w / w.sum()
            for c, wc in zip(kids[i], w):
                prob[c] = prob[i] * wc
                if float32:
                    prob[c] = float(np.float32(prob[c]))
    dh, ah = np.asarray(fc[0], float).reshape(N, nd), np.asarray(fc[1], float).reshape(N, nu)
    err_d = 0.05 * rng.standard_normal((nodes, nd)) * dh[stages]
    err_a = 0.05 * rng.standard_normal((nodes, nu)) * ah[stages]
    err_d[0] = 0.0
    err_a[0] = 0.0
    if float32:
        err_d, err_a = err_d.astype(np.float32).astype(np.float64), err_a.astype(np.float32).astype(np.float64)
    assert (prob > 0).all() and np.isfinite(prob).all()
    assert (np.abs(prob - old) > 0.1 * old).mean() >= 0.5, "the re-weighting must move at least half of the nodes by more than 10 %"
    new = copy.deepcopy(tree)
    new["probNode"] = prob.tolist()
    new["errorDemandNode"] = err_d.ravel().tolist()
    new["errorPriceNode"] = err_a.ravel().tolist()
    return new


def make(p, tree, mode, kind, **kw):
    return capi.Solver(p["network"], tree, p["config"], precision="f32" if kind == "f32" else "f64", operator_mode=mode,
                       operator_storage="f32" if kind == "f64_store32" else "native", **kw)


def last_four(s, fc, iters=AFTER):
    s.updateStateControl()
    s.eliminateInputDistubanceCoupling(*fc)
    s.apgReset()
    return s.apgIterate(iters)


def op_nodes(s):
    return sorted({0, s.nodes // 2, s.nodes - 1})


def snapshot(s, hist):
    out = {"history": np.array(hist)}
    for bid, nm in ALL_BUFS:
        out[nm] = s.get(bid)
    for k, v in s.getTreeData().items():
        out["tree." + k] = v
    for op in ALL_OPS:
        for node in op_nodes(s):
            out["op%d.%d" % (op, node)] = s.getOperator(op, node)
    return out


def same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in b:
        assert np.isfinite(a[k]).all(), (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max()))


def fresh(name, mode, kind):
    """context B: created on the NEW tree, initialised, then the last four calls -- computed once, never changed"""
    key = (name, mode, kind)
    if key not in _FRESH:
        p, fc, new = problem(name)
        b = make(p, new, mode, kind)
        b.initialiseSmpcController(*fc)
        _FRESH[key] = snapshot(b, last_four(b, fc))
        b.close()
    return _FRESH[key]


def reweighted_context(name, mode, kind):
    """context A: created on the OLD tree, initialised, 20 iterations"""
    p, fc, _ = problem(name)
    a = make(p, p["tree"], mode, kind)
    a.initialiseSmpcController(*fc)
    a.apgReset()
    a.apgIterate(BEFORE)
    return a


def check_bitwise(name, mode, kind, guard=False):
    p, fc, new = problem(name)
    want = fresh(name, mode, kind)
    a = reweighted_context(name, mode, kind)
    a.updateTree(new)
    same(snapshot(a, last_four(a, fc)), want, "%s %s %s: re-weighted after the factor step" % (name, mode, kind))
    a2 = make(p, p["tree"], mode, kind)            # A': re-weighted BEFORE its first factor step
    a2.updateTree(new)
    a2.initialiseSmpcController(*fc)
    same(snapshot(a2, last_four(a2, fc)), want, "%s %s %s: re-weighted before the factor step" % (name, mode, kind))
    for s in (a, a2):
        if guard:
            assert s.guardCheck() == 0
        s.close()


# ---- 1. bitwise against a fresh context ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", TREES)
def test_reweighted_context_is_bitwise_a_fresh_one(name, mode, kind):
    check_bitwise(name, mode, kind)


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,tol", [("f64", REL_TOL), ("f32", FP32_TOL)])
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name", TREES)
def test_reweighted_context_matches_the_oracle_of_the_new_tree(name, mode, precision, tol):
    p, fc, new = problem(name)
    o = Oracle(p["network"], new, p["config"], precision=precision)
    o.initialise(*fc)
    ohist = o.apg(25)
    a = reweighted_context(name, mode, precision)
    a.updateTree(new)
    hist = last_four(a, fc, 25)
    w = compare_all(a, o, tol, "%s %s %s after re-weighting" % (name, mode, precision))
    print("\n%s %s %s: worst %.1e, history %.1e" % (name, mode, precision, max(w.values()), np.abs(hist - ohist).max() / np.abs(ohist).max()))
    assert np.abs(hist - ohist).max() <= tol * np.abs(ohist).max()
    for bid, nm in ((capi.BUF_UHAT, "uhat"), (capi.BUF_E, "e"), (capi.BUF_BETA, "beta"), (capi.BUF_ALPHA, "alpha")):
        assert relmax(a.get(bid), o.get(nm)) <= tol, nm
    a.close()


# ---- 3. device form ------------------------------------------------------------------------------------------------------------------------
def on_device(tree, dtype):
    t = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(tree[j], float).astype(dtype))).cuda()
         for k, j in (("prob", "probNode"), ("errorDemand", "errorDemandNode"), ("errorPrice", "errorPriceNode"))}
    torch.cuda.synchronize()            # the producer is done before the call (the context's stream does not wait for torch's)
    return t


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name", ["odd", "ragged"])
def test_device_form_is_bitwise_the_host_form(name, mode, kind, dtype):
    p, fc, new = problem(name)
    if dtype == np.float32:            # values an fp32 array can hold, so that both routes are given the same numbers
        new = reweighted(p["tree"], fc, 11, float32=True)
    h = reweighted_context(name, mode, kind)
    h.updateTree(new)
    want = snapshot(h, last_four(h, fc))
    h.close()
    if dtype == np.float64:
        same(want, fresh(name, mode, kind), "host form")
    d = reweighted_context(name, mode, kind)
    t = on_device(new, dtype)
    d.setTreeDataDevice("f64" if dtype == np.float64 else "f32", **{k: v.data_ptr() for k, v in t.items()})
    got = snapshot(d, last_four(d, fc))          # no synchronize in between: everything is ordered on the context's stream
    same(got, want, "%s %s %s: device form (%s)" % (name, mode, kind, dtype.__name__))
    td = d.getTreeData()
    assert np.array_equal(td["prob"], np.asarray(new["probNode"]))             # a get round-trips (fp32 contexts keep the doubles as given)
    stored = (lambda v: v.astype(np.float32).astype(np.float64)) if kind == "f32" else (lambda v: v)
    assert np.array_equal(td["errorDemand"].ravel(), stored(np.asarray(new["errorDemandNode"])))
    assert np.array_equal(td["errorPrice"].ravel(), stored(np.asarray(new["errorPriceNode"])))
    d.close()
    del t


# ---- 4. partial sets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "structured"])
def test_partial_sets(mode):
    name = "odd"
    p, fc, new = problem(name)
    s = reweighted_context(name, mode, "f64")
    own = s.getTreeData()
    newp, newd, newa = np.asarray(new["probNode"]), np.asarray(new["errorDemandNode"]).reshape(s.nodes, s.nd), np.asarray(new["errorPriceNode"]).reshape(s.nodes, s.nu)
    # errors alone: iterable at once, and the bits of rn_set_tree_errors
    s.setTreeData(errorDemand=newd)
    td = s.getTreeData()
    assert np.array_equal(td["prob"], own["prob"]) and np.array_equal(td["errorPrice"], own["errorPrice"]) and np.array_equal(td["errorDemand"], newd)
    s.apgIterate(1)
    s.setTreeData(errorPrice=newa)
    td = s.getTreeData()
    assert np.array_equal(td["prob"], own["prob"]) and np.array_equal(td["errorPrice"], newa) and np.array_equal(td["errorDemand"], newd)
    s.apgIterate(1)
    r = reweighted_context(name, mode, "f64")
    r._check(r.lib.rn_set_tree_errors(r.h, np.ascontiguousarray(newd).ctypes.data, np.ascontiguousarray(newa).ctypes.data))
    hs, hr = last_four(s, fc), last_four(r, fc)
    assert np.array_equal(hs, hr)
    for bid, nm in ALL_BUFS:
        assert np.array_equal(s.get(bid), r.get(bid)), nm
    # probabilities alone: the affine terms are the old tree's
    s.setTreeData(prob=newp)
    td = s.getTreeData()
    assert np.array_equal(td["prob"], newp) and np.array_equal(td["errorPrice"], newa) and np.array_equal(td["errorDemand"], newd)
    assert s.lib.rn_apg_iterate(s.h, 1, None) == RN_E_STATE
    assert s.lib.rn_solve_step(s.h) == RN_E_STATE
    same(snapshot(s, last_four(s, fc)), fresh(name, mode, "f64"), "the three arrays one after the other")
    s.close(); r.close()


# ---- 5. the caller's blocks are recomputed ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64", "f64_store32"])
def test_callers_blocks_are_recomputed(kind):
    name = "odd"
    p, fc, new = problem(name)
    b = make(p, new, "dense", kind)
    b.initialiseSmpcController(*fc)
    want = b.getOperators()
    b.close()
    for mode in ("dense", "auto"):
        a = reweighted_context(name, mode, kind)
        if mode == "auto":
            assert a.operatorMode() == ("auto", "structured")
            a.setOperators(phi=np.zeros((a.nodes, a.nv * 2 * a.nx)))          # becomes dense
        own = a.getOperators()
        rng = np.random.default_rng(3)
        a.setOperators(**{k: own[nm] * (1.0 + 0.3 * rng.standard_normal(own[nm].shape)) for k, nm in (("phi", "Phi"), ("psi", "Psi"), ("D", "D"), ("F", "Ftil"))})
        assert not np.array_equal(a.getOperators()["Psi"], own["Psi"])
        a.setTreeData(prob=new["probNode"])
        got = a.getOperators()
        for nm in want:
            assert np.array_equal(got[nm], want[nm]), (mode, nm)
        assert a.operatorMode()[1] == "dense"
        a.close()


def test_auto_context_stays_structured():
    p, fc, new = problem("odd")
    a = reweighted_context("odd", "auto", "f64")
    a.updateTree(new)
    assert a.operatorMode() == ("auto", "structured")
    last_four(a, fc, 5)
    assert a.operatorMode() == ("auto", "structured")
    a.close()


# ---- 6. NAMA and FBE -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("alg", ["globalFbeAlgorithm", "namaAlgorithm"])
def test_quasi_newton_loops_after_reweighting(alg, mode):
    name = "odd"
    p, fc, new = problem(name)

    def run(s):
        s.updateStateControl()
        s.eliminateInputDistubanceCoupling(*fc)
        s.fbeReset()
        out = s._algorithmFbeNama(8)
        return out, {nm: s.get(bid) for bid, nm in ALL_BUFS}

    b = make(p, new, mode, "f64")
    b.setAlgorithm(alg)
    b.initialiseSmpcController(*fc)
    (hb, vb, tb), bufs_b = run(b)
    a = make(p, p["tree"], mode, "f64")
    a.setAlgorithm(alg)
    a.initialiseSmpcController(*fc)
    a.fbeReset()
    a._algorithmFbeNama(4)
    a.updateTree(new)
    (ha, va, ta), bufs_a = run(a)
    assert np.array_equal(ta, tb), (ta, tb)
    assert np.isfinite(va).all() and np.array_equal(va, vb) and np.array_equal(ha, hb)
    for nm in bufs_b:
        assert np.array_equal(bufs_a[nm], bufs_b[nm]), nm
    a.close(); b.close()


# ---- 7. warm start -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "structured"])
def test_warm_start_keeps_the_duals(mode):
    name = "small"
    p, fc, new = problem(name)
    a = make(p, p["tree"], mode, "f64")
    a.factorStep()
    a.setWarmStart(True)
    a.controlAction(*fc, maxIterations=30)
    duals = {bid: a.get(bid) for bid in (capi.BUF_XI, capi.BUF_PSI, capi.BUF_UPD_XI, capi.BUF_UPD_PSI)}
    a.updateTree(new)
    for bid, v in duals.items():
        assert np.array_equal(a.get(bid), v)                  # untouched by the re-weighting
    ua = a.controlAction(*fc, maxIterations=30)
    assert np.isfinite(ua).all()
    c = make(p, new, mode, "f64")                             # C: a fresh context on the new tree given the same duals
    c.factorStep()
    c.setWarmStart(True)
    c.controlAction(*fc, maxIterations=1)                     # (a context that has never iterated cold-starts)
    for bid, v in duals.items():
        c.set(bid, v)
    uc = c.controlAction(*fc, maxIterations=30)
    assert np.array_equal(ua, uc)
    for bid, nm in PAIRS:
        assert np.array_equal(a.get(bid), c.get(bid)), nm
    a.close(); c.close()


# ---- 8. shards -----------------------------------------------------------------------------------------------------------------------------
def shards_run(p, tree_at_creation, world, fc, update=None, structured=False):
    pp = dict(p, tree=tree_at_creation)
    rk = Ranks(pp, world, 0, structured)
    try:
        def solve(s):
            s.initialiseSmpcController(*fc)
            s.apgReset()
            s.apgIterate(BEFORE)
            if update is not None:
                s.updateTree(update)
            return last_four(s, fc, 24)

        hists = rk.run(solve)
        d = {"nx": rk.shards[0].nx, "nu": rk.shards[0].nu, "nv": rk.shards[0].nv, "2nx": 2 * rk.shards[0].nx}
        vecs = ((capi.BUF_X, "x", "nx"), (capi.BUF_U, "u", "nu"), (capi.BUF_V, "v", "nv"), (capi.BUF_UPD_XI, "updXi", "2nx"), (capi.BUF_UPD_PSI, "updPsi", "nu"),
                (capi.BUF_BETA, "beta", "nv"))
        out = {"hist": hists, "local": [{nm: s.get(bid) for bid, nm in ALL_BUFS} for s in rk.shards], "tree": [s.getTreeData() for s in rk.shards],
               "moments": [s.debugCutMoments() for s in rk.shards], "cut": rk.shards[0].shardInfo()["cut_stage"],
               "global": {nm: rk.gathered(bid, d[dm]) for bid, nm, dm in vecs}, "guard": [s.guardCheck() for s in rk.shards]}
        return out
    finally:
        rk.close()


def check_shards(world, structured=False):
    p, fc, new = problem("medium")
    got = shards_run(p, p["tree"], world, fc, update=new, structured=structured)
    want = shards_run(p, new, world, fc, structured=structured)
    o = Oracle(p["network"], new, p["config"])
    o.initialise(*fc)
    ohist = o.apg(24)
    E, P = partition.cut_children_moments(new, got["cut"])
    for r in range(world):
        assert np.array_equal(got["hist"][r], want["hist"][r]) and np.array_equal(got["hist"][r], got["hist"][0])
        assert np.abs(got["hist"][r] - ohist).max() <= 1e-9 * np.abs(ohist).max()
        for nm in want["local"][r]:
            assert np.isfinite(got["local"][r][nm]).all(), nm
            assert np.array_equal(got["local"][r][nm], want["local"][r][nm]), (r, nm)
        for k in want["tree"][r]:
            assert np.array_equal(got["tree"][r][k], want["tree"][r][k]), (r, k)
        assert np.array_equal(got["moments"][r][0], E) and np.array_equal(got["moments"][r][1], P), r
        assert np.array_equal(want["moments"][r][0], E) and np.array_equal(want["moments"][r][1], P), r
    for nm, v in got["global"].items():
        assert relmax(v, o.get(nm)) < 1e-9, nm
    return got


@pytest.mark.parametrize("world,structured", [(2, False), (3, False), (3, True)])
def test_shards_reweighted_in_place(world, structured):
    check_shards(world, structured)


def test_partial_sets_on_shards_use_the_retained_full_tree_values():
    """probabilities alone, then the demand errors alone: the moments need both, the missing one is the context's own copy"""
    p, fc, new = problem("medium")
    rk = Ranks(p, 2, 0, False)
    try:
        cut = rk.shards[0].shardInfo()["cut_stage"]
        mixed = dict(p["tree"], probNode=new["probNode"])
        for s in rk.shards:
            s.setTreeData(prob=new["probNode"])
            E, P = s.debugCutMoments()
            wE, wP = partition.cut_children_moments(mixed, cut)
            assert np.array_equal(E, wE) and np.array_equal(P, wP)
            s.setTreeData(errorDemand=new["errorDemandNode"])
            E, P = s.debugCutMoments()
            wE, wP = partition.cut_children_moments(new, cut)
            assert np.array_equal(E, wE) and np.array_equal(P, wP)
            assert s.lib.rn_set_tree_data(s.h, s.nodes, np.ones(s.nodes).ctypes.data, None, None) == RN_E_ARG        # the local count
            rows = np.asarray(s.global_nodes, int)
            assert np.array_equal(s.getTreeData()["prob"], np.asarray(new["probNode"])[rows])
    finally:
        rk.close()


def test_hand_sharded_context_wants_its_moments_again():
    p, fc, new = problem("medium")
    cut = partition.default_cut_stage(p["tree"])
    lt, gids = partition.local_tree(p["tree"], 0, 2, cut)
    lnew, _ = partition.local_tree(new, 0, 2, cut)
    s = capi.Solver(p["network"], lt, p["config"])
    s.commInit(0, 2, None)
    s.setCutStage(cut, partition.cut_children_moments(p["tree"], cut))
    s.initialiseSmpcController(*fc)
    s.updateTree(lnew)                                         # local rows
    dh, ah = (np.ascontiguousarray(v, dtype=np.float64) for v in fc)
    assert s.lib.rn_eliminate_input_disturbance_coupling(s.h, dh.ctypes.data, ah.ctypes.data) == RN_E_STATE
    assert "rn_set_cut_children_moments" in s.lib.rn_last_error(s.h).decode()
    s.setCutStage(cut, partition.cut_children_moments(new, cut))
    s.eliminateInputDistubanceCoupling(*fc)
    o = Oracle(p["network"], new, p["config"])
    o.initialise(*fc)
    crown = p["tree"]["nodesPerStageCumul"][cut]
    assert relmax(s.get(capi.BUF_BETA)[: crown * o.nv], o.get("beta")[: crown * o.nv]) < 1e-12
    s.close()


# ---- 9. arguments and state ----------------------------------------------------------------------------------------------------------------
def test_arguments_and_state():
    name = "odd"
    p, fc, new = problem(name)
    s = reweighted_context(name, "dense", "f64")
    lib, n = s.lib, s.nodes
    own = s.getTreeData()
    newp = np.asarray(new["probNode"])
    t = on_device(new, np.float64)
    dp = t["prob"].data_ptr()
    assert lib.rn_set_tree_data(s.h, n + 1, newp.ctypes.data, None, None) == RN_E_ARG
    assert lib.rn_set_tree_data(s.h, n - 1, newp.ctypes.data, None, None) == RN_E_ARG
    assert lib.rn_set_tree_data_device(s.h, n + 1, capi.RN_F64, dp, None, None) == RN_E_ARG
    assert lib.rn_get_tree_data(s.h, n + 1, newp.copy().ctypes.data, None, None) == RN_E_ARG
    assert lib.rn_set_tree_data(s.h, n, None, None, None) == RN_E_ARG
    assert lib.rn_set_tree_data_device(s.h, n, capi.RN_F64, None, None, None) == RN_E_ARG
    assert lib.rn_get_tree_data(s.h, n, None, None, None) == RN_E_ARG
    for prec in (7, -1, 2):
        assert lib.rn_set_tree_data_device(s.h, n, prec, dp, None, None) == RN_E_ARG
    assert lib.rn_set_tree_data_device(s.h, n, capi.RN_F64, newp.ctypes.data, None, None) == RN_E_ARG          # a host pointer
    assert "device memory" in lib.rn_last_error(s.h).decode()
    assert lib.rn_set_tree_data_device(s.h, n, capi.RN_F64, dp + 4, None, None) == RN_E_ARG                    # misaligned
    for bad in (0.0, -0.25, float("nan"), float("inf")):
        q = newp.copy()
        q[n // 2] = bad
        assert lib.rn_set_tree_data(s.h, n, q.ctypes.data, None, None) == RN_E_ARG, bad
    with pytest.raises(ValueError):
        s.setTreeData(prob=np.ones(3))
    other = copy.deepcopy(new)
    other["ancestor"][-1] -= 1
    with pytest.raises(ValueError):
        s.updateTree(other)
    td = s.getTreeData()
    for k in own:
        assert np.array_equal(td[k], own[k]), k                 # none of the refused calls changed anything
    s.apgIterate(1)                                             # ... nor the state
    # the device form cannot look: the elimination that follows reports
    q = newp.copy()
    q[3], q[n - 1] = -1.0, 0.0
    tq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    s.setTreeDataDevice("f64", prob=tq.data_ptr())
    dh, ah = (np.ascontiguousarray(v, dtype=np.float64) for v in fc)
    assert lib.rn_eliminate_input_disturbance_coupling(s.h, dh.ctypes.data, ah.ctypes.data) == RN_E_ARG
    msg = lib.rn_last_error(s.h).decode()
    assert "rn_set_tree_data_device" in msg and " 2 " in msg, msg
    assert lib.rn_apg_iterate(s.h, 1, None) == RN_E_STATE
    assert lib.rn_eliminate_input_disturbance_coupling(s.h, dh.ctypes.data, ah.ctypes.data) == RN_E_ARG           # still
    s.setTreeDataDevice("f64", **{k: v.data_ptr() for k, v in t.items()})
    same(snapshot(s, last_four(s, fc)), fresh(name, "dense", "f64"), "usable again after a valid set")
    s.close()
    del t, tq


def test_memory():
    p, fc, new = problem("small")
    s = reweighted_context("small", "dense", "f64")
    s.getTreeData()
    m0 = s.deviceMemoryInfo()["context_bytes"]
    s.updateTree(new)
    m1 = s.deviceMemoryInfo()["context_bytes"]
    s.getTreeData()
    m2 = s.deviceMemoryInfo()["context_bytes"]
    t = on_device(p["tree"], np.float32)
    s.setTreeDataDevice("f32", **{k: v.data_ptr() for k, v in t.items()})
    m3 = s.deviceMemoryInfo()["context_bytes"]
    last_four(s, fc, 5)
    m4 = s.deviceMemoryInfo()["context_bytes"]
    assert m0 == m1 == m2 == m3 == m4 and m0 > 0, (m0, m1, m2, m3, m4)
    s.close()
    del t


# ---- 10. guard mode ------------------------------------------------------------------------------------------------------------------------
def test_under_the_buffer_guard(monkeypatch):
    """RAPIDNET_GUARD=1: every buffer of the context between red zones and NaN until written: a row read outside the caller's arrays or the
    context's would bring a NaN into what is compared (same() asserts finiteness), a write outside a buffer changes a red zone"""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    saved = dict(_FRESH)
    _FRESH.clear()                       # (the fresh contexts are made under the guard too)
    try:
        check_bitwise("ragged", "dense", "f64", guard=True)
        check_bitwise("odd", "structured", "f32", guard=True)
        got = check_shards(3)
        assert got["guard"] == [0, 0, 0]
    finally:
        _FRESH.clear()
        _FRESH.update(saved)
    gc.collect()
    after = capi.guard_report()
    assert after[0] > before[0] and after[1] == before[1], (before, after)
