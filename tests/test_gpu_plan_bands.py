"""rn_plan_quantiles, rn_plan_quantiles_device, rn_plan_paths (k_plan_bands, k_plan.hpp): per-stage weighted quantiles of x and u and the rows
along every leaf's path, against the numpy restatement tests/bands_oracle.py.

a  bit for bit against the restatement fed with what the context holds -- rn_get of x and u (an fp32 context: its floats, widened exactly) and
   the probabilities of rn_get_tree_data (rounded to fp32 for an fp32 context, whose kernel reads the fp32 copy).  Nothing is excluded: the
   definition fixes the order of the additions, so there is no rounding to allow for.
b  against the CPU oracle's iterates (fp64 contexts, fp64 blocks): the weighted quantile is 1-Lipschitz in the infinity norm of the values
   for fixed weights, so every quantile of a stage differs from the oracle's by no more than that stage's worst entry difference of x (or u);
   the iterates themselves meet the project's 1e-9 per-stage bound.
When PLAN_BANDS_ERRORS names a file, the worst ratio of (b) of every case is appended to it (profiles/plan_bands_errors.txt is such a file)."""
import gc
import os

import numpy as np
import pytest

import bands_oracle as bo
from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from stagewise import stage_relmax
from test_gpu_device_pointer import _d2h
from test_gpu_sharded_batched import Ranks
from test_gpu_tree_data import make, reweighted

pytestmark = pytest.mark.gpu

RN_E_ARG, RN_E_STATE = -1, -3
LEVELS = (0.0, 0.05, 0.5, 0.95, 1.0)
UNSORTED = (0.95, 0.0, 1.0, 0.5, 0.05)
SINGLE = (0.3,)
ITERS = 25
WHICH = (("x", capi.BUF_X), ("u", capi.BUF_U))

_PROBLEMS, _ORACLE = {}, {}


def record(line):
    print(line)
    path = os.environ.get("PLAN_BANDS_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def problem(name):
    if name not in _PROBLEMS:
        p = synth.make_problem(name)
        _PROBLEMS[name] = (p, synth.forecast_at(p["forecast"], 0))
    return _PROBLEMS[name]


def oracle_run(name):
    """x and u of the CPU oracle after ITERS iterations from cold; computed once per problem and not changed"""
    if name not in _ORACLE:
        p, fc = problem(name)
        # (horizon1: the reference's aliasing of Omega / Theta by scenario position indexes before the first block there; its oracle runs with
        #  the aliasing off, as in tests/test_gpu_parity.py)
        o = Oracle(p["network"], p["tree"], p["config"], alias_operators=name != "horizon1")
        o.initialise(*fc)
        o.apg(ITERS)
        _ORACLE[name] = {"x": o.get("x").copy(), "u": o.get("u").copy()}
    return _ORACLE[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def f32_if(kind, a):
    a = np.asarray(a, float)
    return a.astype(np.float32).astype(np.float64) if kind == "f32" else a


def dim_of(s, which):
    return s.nx if which == "x" else s.nu


def solved(name, mode="dense", kind="f64", tree=None):
    p, fc = problem(name)
    s = make(p, p["tree"] if tree is None else tree, mode, kind)
    s.initialiseSmpcController(*fc)
    s.apgReset()
    s.apgIterate(ITERS)
    return s


def check_a(what, s, tree, kind, levels=(LEVELS, UNSORTED, SINGLE)):
    """(a): every entry of both tables, both arrays, bit for bit against the restatement of what the context holds"""
    parent, stage = bo.tree_arrays(tree)
    prob = f32_if(kind, s.getTreeData()["prob"])
    for which, bid in WHICH:
        vals = s.get(bid).reshape(-1, dim_of(s, which))
        assert np.isfinite(vals).all(), what
        for q in levels:
            got = s.planQuantiles(which, q)
            want = bo.quantiles(vals, prob, stage, q)
            assert got.shape == want.shape == (s.N, dim_of(s, which), len(q)), what
            assert np.array_equal(bits(got), bits(want)), (what, which, q, np.argwhere(bits(got) != bits(want))[:5])
        got, leaf = s.planPaths(which)
        want, want_leaf = bo.paths(vals, parent, stage)
        assert np.array_equal(bits(got), bits(want)), (what, which, "paths")
        assert np.array_equal(leaf, want_leaf), (what, which, "leafNode")


# ---- 1. cold solves: one-node stages, ragged trees, widths that are no power of two and cross a wave; (a) and (b) -------------------------------
@pytest.mark.parametrize("name", ["tiny", "horizon1", "toy", "ragged", "fan", "bigfan", "small", "medium"])
def test_bands_after_a_cold_solve(name):
    p, fc = problem(name)
    tree = p["tree"]
    s = solved(name)
    check_a(name, s, tree, "f64")
    _, stage = bo.tree_arrays(tree)
    prob = np.asarray(tree["probNode"], float)
    o = oracle_run(name)
    worst = 0.0
    for which, bid in WHICH:
        dim = dim_of(s, which)
        mine, ref = s.get(bid).reshape(-1, dim), o[which].reshape(-1, dim)
        rel = stage_relmax(mine, ref, tree, dim)
        assert rel.max() <= 1e-9, (name, which, rel)
        dist = np.zeros(s.N)
        np.maximum.at(dist, stage, np.abs(mine - ref).max(axis=1))      # the stage's worst entry difference
        got, want = s.planQuantiles(which, LEVELS), bo.quantiles(ref, prob, stage, LEVELS)
        err = np.abs(got - want).max(axis=(1, 2))
        print("%s %s: per stage |quantile - oracle's| %s, worst entry difference %s" % (name, which, err, dist))
        assert (err <= dist).all(), (name, which, err, dist)
        live = dist > 0
        if live.any():
            worst = max(worst, float((err[live] / dist[live]).max()))
    record("%s dense f64, %d iterations: worst |quantile - oracle's| / (the stage's worst entry difference) %.3f" % (name, ITERS, worst))
    s.close()


# ---- 2. forms and states ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,kind", [("ragged", "structured", "f64"), ("small", "dense", "f64_store32"), ("bigfan", "dense", "f32"),
                                            ("ragged", "structured", "f32"), ("fan", "structured", "f64")])
def test_bands_of_other_forms(name, mode, kind):
    s = solved(name, mode, kind)
    check_a("%s %s %s" % (name, mode, kind), s, problem(name)[0]["tree"], kind)
    s.close()


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_bands_after_a_reweighting_and_with_a_zero_probability(kind):
    import torch

    name = "ragged"
    p, fc = problem(name)
    new = reweighted(p["tree"], fc, 7)
    s = solved(name, "dense", kind)
    s.updateTree(new)
    s.updateStateControl()
    s.eliminateInputDistubanceCoupling(*fc)
    s.apgReset()
    s.apgIterate(5)
    check_a("%s %s after rn_set_tree_data" % (name, kind), s, new, kind)
    # One probability set to 0 (the device form takes it; the host form refuses it): the node that holds the last stage's minimum of x's
    # first component cannot occur any more, so q = 0 moves off it.  The quantiles read x, u and the probabilities in force, nothing else.
    _, stage = bo.tree_arrays(new)
    x = s.get(capi.BUF_X).reshape(-1, s.nx)
    last = np.flatnonzero(stage == stage.max())
    gone = last[np.argmin(x[last, 0])]
    before = s.planQuantiles("x", [0.0])[-1, 0, 0]
    assert before == x[gone, 0]
    prob = np.asarray(new["probNode"], float).copy()
    prob[gone] = 0.0
    t = torch.from_numpy(prob).cuda()
    torch.cuda.synchronize()
    s.setTreeDataDevice("f64", prob=t.data_ptr())
    s.synchronize()
    assert s.getTreeData()["prob"][gone] == 0.0
    check_a("%s %s with p = 0 at node %d" % (name, kind, gone), s, new, kind)
    after = s.planQuantiles("x", [0.0])[-1, 0, 0]
    assert after == np.delete(x[last, 0], np.argmin(x[last, 0])).min() and after > before
    s.close()
    del t


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_bands_after_a_warm_second_control_action(kind):
    name = "tiny"
    p, fc = problem(name)
    s = make(p, p["tree"], "dense", kind)
    s.initialiseSmpcController(*fc)
    s.setWarmStart(True)
    u0 = s.controlAction(*fc, maxIterations=20)
    x1 = 0.97 * np.asarray(p["config"]["currentX"], float).ravel()
    s.controlAction(*fc, currentX=x1, prevU=u0, maxIterations=20)
    check_a("%s %s after a warm second control action" % (name, kind), s, p["tree"], kind)
    s.close()


def test_bands_after_a_nama_run():
    name = "small"
    p, fc = problem(name)
    s = make(p, p["tree"], "dense", "f64")
    s.initialiseSmpcController(*fc)
    s.setAlgorithm("namaAlgorithm", 5)
    s.algorithmNama(8)
    check_a("%s after 8 NAMA iterations" % name, s, p["tree"], "f64")
    s.close()


@pytest.mark.parametrize("name,kind", [("bigfan", "f64"), ("medium", "f32")])
def test_two_calls_give_the_same_bits_allocate_once_and_the_device_form_holds_the_host_forms_bits(name, kind):
    p, fc = problem(name)
    s = make(p, p["tree"], "dense", kind)
    s.initialiseSmpcController(*fc)
    m_never = s.deviceMemoryInfo()["context_bytes"]
    s.apgReset()
    s.apgIterate(ITERS)
    assert s.deviceMemoryInfo()["context_bytes"] == m_never            # nothing is allocated for a context that has not asked
    a = {w: (s.planQuantiles(w, UNSORTED), s.planPaths(w)) for w, _ in WHICH}
    m1 = s.deviceMemoryInfo()["context_bytes"]
    leaves, dim = s.bandLeaves(), max(s.nx, s.nu)
    assert m1 - m_never == 8 * (s.N * dim * capi.BAND_MAX_LEVELS + leaves * s.N * dim) + 4 * leaves + 4
    for w, _ in WHICH:
        q2, (p2, l2) = s.planQuantiles(w, UNSORTED), s.planPaths(w)
        assert np.array_equal(bits(q2), bits(a[w][0])) and np.array_equal(bits(p2), bits(a[w][1][0])) and np.array_equal(l2, a[w][1][1])
        ptr = s.planQuantilesDevice(w, UNSORTED)
        s.synchronize()
        n = s.N * dim_of(s, w) * len(UNSORTED)
        assert ptr and np.array_equal(bits(_d2h(ptr, n, "f64").reshape(a[w][0].shape)), bits(a[w][0])), w
    assert s.deviceMemoryInfo()["context_bytes"] == m1                  # later calls allocate nothing
    s.close()


# ---- 3. sharded: every rank holds the whole tree's tables, the one-GPU values, the same bits ---------------------------------------------------
@pytest.mark.parametrize("world,structured", [(2, False), (3, True)])
def test_shards_hold_the_whole_trees_bands(world, structured):
    name = "medium"
    p, fc = problem(name)
    one = solved(name, "structured" if structured else "dense")
    src = {bid: one.get(bid) for _, bid in WHICH}
    want = {w: (one.planQuantiles(w, LEVELS), one.planQuantiles(w, SINGLE), one.planPaths(w)) for w, _ in WHICH}
    one.close()
    rk = Ranks(p, world, 0, structured)
    try:
        def solve(s):
            s.initialiseSmpcController(*fc)
            s.apgReset()
            s.apgIterate(ITERS)
            g = np.asarray(s.global_nodes, int)
            for (w, bid) in WHICH:                                   # the one-GPU run's plan, so that the tables can be compared as doubles
                s.set(bid, src[bid].reshape(-1, dim_of(s, w))[g])
            return {w: (s.planQuantiles(w, LEVELS), s.planQuantiles(w, SINGLE), s.planPaths(w)) for w, _ in WHICH}

        out = rk.run(solve)
        for rank, res in enumerate(out):
            for w, _ in WHICH:
                ql, qs, (pth, leaf) = res[w]
                wl, ws, (wp, wleaf) = want[w]
                assert np.array_equal(ql, wl) and np.array_equal(qs, ws) and np.array_equal(pth, wp), (rank, w)      # ==: a zero's sign may differ
                assert np.array_equal(leaf, wleaf), (rank, w)
                for x, y in ((ql, out[0][w][0]), (qs, out[0][w][1]), (pth, out[0][w][2][0])):
                    assert np.array_equal(bits(x), bits(y)), (rank, w)                                                # across ranks: the same bits
    finally:
        rk.close()


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_state():
    name = "small"
    p, fc = problem(name)
    s = make(p, p["tree"], "dense", "f64")
    lib, C = s.lib, capi.C
    N, leaves = s.N, s.bandLeaves()
    q = np.array(LEVELS)
    out, pth, ln = np.zeros((N, s.nu, 16)), np.zeros((leaves, N, s.nu)), np.zeros(leaves, np.int32)
    dev = C.c_void_p()

    def quant(which=capi.BAND_X, nq=len(LEVELS), qq=q, stages=N, o=out):
        return lib.rn_plan_quantiles(s.h, which, nq, None if qq is None else qq.ctypes.data, stages, None if o is None else o.ctypes.data)

    def quant_dev(which=capi.BAND_X, nq=len(LEVELS), qq=q, o=dev):
        return lib.rn_plan_quantiles_device(s.h, which, nq, None if qq is None else qq.ctypes.data, None if o is None else C.byref(o))

    def paths(which=capi.BAND_X, cnt=leaves, o=pth, leaf=ln):
        return lib.rn_plan_paths(s.h, which, cnt, None if o is None else o.ctypes.data, None if leaf is None else leaf.ctypes.data)

    assert (quant(), quant_dev(), paths()) == (RN_E_STATE,) * 3                               # before the factor step
    s.initialiseSmpcController(*fc)
    assert (quant(), quant_dev(), paths()) == (RN_E_STATE,) * 3                               # before the first sweep
    assert "first sweep" in lib.rn_last_error(s.h).decode()
    m0 = s.deviceMemoryInfo()["context_bytes"]
    s.apgReset()
    s.apgIterate(2)
    for which in (-1, 2):
        assert (quant(which=which), quant_dev(which=which), paths(which=which)) == (RN_E_ARG,) * 3
    for nq in (0, 17):
        assert quant(nq=nq, qq=np.linspace(0.0, 1.0, 17)) == RN_E_ARG and quant_dev(nq=nq, qq=np.linspace(0.0, 1.0, 17)) == RN_E_ARG
    for bad in (-1e-9, 1.0000001, np.nan, np.inf):
        qq = np.array([0.5, bad, 0.1])
        assert quant(nq=3, qq=qq) == RN_E_ARG and quant_dev(nq=3, qq=qq) == RN_E_ARG
    for stages in (N - 1, N + 1, 0):
        assert quant(stages=stages) == RN_E_ARG
    for cnt in (leaves - 1, leaves + 1, 0, s.nodes):
        assert paths(cnt=cnt) == RN_E_ARG
    assert quant(o=None) == RN_E_ARG and quant(qq=None) == RN_E_ARG and quant_dev(o=None) == RN_E_ARG and quant_dev(qq=None) == RN_E_ARG and paths(o=None) == RN_E_ARG
    assert lib.rn_plan_quantiles(None, 0, 1, q.ctypes.data, N, out.ctypes.data) == RN_E_ARG
    assert s.deviceMemoryInfo()["context_bytes"] == m0                                        # none of the refused calls allocated anything
    assert (quant(), quant_dev(), paths(), paths(leaf=None)) == (0, 0, 0, 0)                   # the context is usable; leafNode may be NULL
    assert quant(nq=16, qq=np.linspace(0.0, 1.0, 16)) == 0                                    # the cap itself is allowed
    s.synchronize()
    assert dev.value and np.isfinite(out).all() and np.isfinite(pth).all() and ln[0] == s.nodes - leaves
    # a value that is not finite: the host form says so, the device form reads NaN at that (stage, component) and nowhere else
    x = s.get(capi.BUF_X)
    broken = x.copy()
    broken[s.nx * (s.nodes - 1) + 1] = np.nan
    s.set(capi.BUF_X, broken)
    assert quant() == RN_E_STATE and "not finite" in lib.rn_last_error(s.h).decode()
    assert quant_dev() == 0
    s.synchronize()
    tab = _d2h(dev.value, N * s.nx * len(LEVELS), "f64").reshape(N, s.nx, len(LEVELS))
    assert np.isnan(tab[N - 1, 1]).all() and np.isnan(tab).sum() == len(LEVELS)
    s.set(capi.BUF_X, x)
    want = bo.quantiles(x.reshape(-1, s.nx), s.getTreeData()["prob"], bo.tree_arrays(p["tree"])[1], LEVELS)
    assert quant() == 0 and np.array_equal(bits(out.ravel()[: want.size]), bits(want.ravel()))
    s.close()


def test_a_batch_that_failed_half_way_is_refused_until_the_reset():
    """a shard whose all-reduce fails abandons its batch: the plan is that of no iteration, and the bands say so"""
    name = "medium"
    p, fc = problem(name)
    s = capi.Solver(p["network"], p["tree"], p["config"], rank=0, nranks=2)
    s.debugSetAllreduce(lambda *a: 0)                    # the sum of one rank: the buffer as it stands
    s.initialiseSmpcController(*fc)
    s.apgReset()
    s.apgIterate(2)
    q = np.array(LEVELS)
    out = np.zeros((s.N, s.nx, len(LEVELS)))
    assert s.lib.rn_plan_quantiles(s.h, capi.BAND_X, len(LEVELS), q.ctypes.data, s.N, out.ctypes.data) == 0
    s.debugSetAllreduce(lambda *a: 7)
    with pytest.raises(capi.RapidNetError):
        s.apgIterate(2)
    s.debugSetAllreduce(lambda *a: 0)
    assert s.lib.rn_plan_quantiles(s.h, capi.BAND_X, len(LEVELS), q.ctypes.data, s.N, out.ctypes.data) == RN_E_STATE
    assert "half-way" in s.lib.rn_last_error(s.h).decode()
    pth = np.zeros((s.bandLeaves(), s.N, s.nx))
    assert s.lib.rn_plan_paths(s.h, capi.BAND_X, s.bandLeaves(), pth.ctypes.data, None) == RN_E_STATE
    s.apgReset()
    s.apgIterate(2)
    assert s.lib.rn_plan_quantiles(s.h, capi.BAND_X, len(LEVELS), q.ctypes.data, s.N, out.ctypes.data) == 0
    s.close()


# ---- 5. guard mode -----------------------------------------------------------------------------------------------------------------------------
def test_under_the_buffer_guard(monkeypatch):
    """RAPIDNET_GUARD=1 (read when a context is created): every buffer between red zones and NaN until written.  A row read outside the arrays
    would bring a NaN into a table (compared bit for bit with the restatement), a write outside a buffer changes a red zone."""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    for name, mode, kind in (("bigfan", "dense", "f64"), ("ragged", "structured", "f32")):
        s = solved(name, mode, kind)
        check_a("guard: %s %s %s" % (name, mode, kind), s, problem(name)[0]["tree"], kind)
        assert s.guardCheck() == 0
        s.close()
    after = capi.guard_report()
    assert after[0] - before[0] == 2 and after[1] == before[1]      # both contexts were checked once more when they went away: 0 bytes
