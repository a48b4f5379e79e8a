"""rn_apg_solve / rn_set_stop_tolerance: the APG solve ends at a batch boundary once the residual of the batch's last iteration is <= tol.

The decision is the host's, taken behind the synchronisation that closes a batch; the launch that closes the batch (k_finalize_optimistic, the
decideHere fix-up launch, k_batch_close_unpack) publishes the batch record it needs.  What is pinned here:
  * the iteration count, from the fp64 CPU oracle alone: the tolerance is placed in a factor-2 gap of the ORACLE's residuals at the batch
    boundaries (sqrt of the two neighbours: a factor sqrt(2) > 1.4 to either side, nine orders of magnitude above the 1e-9 parity of the
    histories), so the expected count is fixed before the GPU is touched;
  * the iterates, bit for bit those of rn_apg_reset + the same sequence of rn_apg_iterate(checkEvery) calls, and at 1e-9 those of the oracle
    stopped at the same count;
  * the fixed-count paths (tol = 0, a context that never set a tolerance), bit for bit.
vecPrimalInfs is the LARGER OF TWO SIGNED entries (the reference's quirk, SmpcController.cu:1480-1496), so a history can go negative: every
case below is a problem variant (step size, forecast instant) whose oracle residuals at the chosen boundaries are positive -- asserted."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT
from oracle.oracle import Oracle, forecast_at
from rapidnet_amd import capi, partition, synth

pytestmark = pytest.mark.gpu
REL_TOL = 1e-9
FP32_TOL = 2e-4          # the suite's fp32 tolerance (tests/test_gpu_parity.py)
M = 100
# (problem, checkEvery) -> (step size as a multiple of the generator's own, feasible, forecast instant): variants whose ORACLE history has a
# factor-2 drop between positive residuals at a batch boundary within 100 iterations (found on the CPU; asserted by _oracle_stop)
VARIANTS = {("small", 7): (1.0, None, 0), ("small", 16): (0.5, None, 1), ("small", 20): (2.0, None, 0),
            ("odd", 7): (0.5, None, 0), ("odd", 16): (0.5, None, 0), ("odd", 20): (1.0, None, 0),
            ("ragged", 7): (1.0, None, 0), ("ragged", 16): (0.5, None, 1), ("ragged", 20): (0.5, True, 1)}
ALL_BUFS = [getattr(capi, n) for n in ("BUF_X", "BUF_U", "BUF_V", "BUF_XI", "BUF_PSI", "BUF_ACC_XI", "BUF_ACC_PSI", "BUF_UPD_XI", "BUF_UPD_PSI",
                                        "BUF_PRIMAL_XI", "BUF_PRIMAL_PSI", "BUF_DUAL_XI", "BUF_DUAL_PSI", "BUF_RES_XI", "BUF_RES_PSI")]
ORACLE_PAIRS = [(capi.BUF_X, "x"), (capi.BUF_U, "u"), (capi.BUF_XI, "xi"), (capi.BUF_PSI, "psi"), (capi.BUF_UPD_XI, "updXi"),
                (capi.BUF_UPD_PSI, "updPsi"), (capi.BUF_DUAL_XI, "dualXi"), (capi.BUF_DUAL_PSI, "dualPsi")]


def relmax(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


_cache = {}


def _variant(name, c, precision="f64", **kw):
    """(problem, forecast, oracle history of M iterations) of a case: computed once, shared, never modified"""
    key = (name, c, precision, tuple(sorted(kw.items())))
    if key not in _cache:
        mult, feasible, t = VARIANTS[(name, c)]
        step = synth.make_problem(name)["config"]["stepSize"][0] * mult
        p = synth.make_problem(name, step_size=step, feasible=feasible, **kw)
        dh, ah = synth.forecast_at(p["forecast"], t)
        o = Oracle(p["network"], p["tree"], p["config"], precision=precision)
        o.initialise(dh, ah)
        r = o.apg(M)
        r.setflags(write=False)
        _cache[key] = (p, dh, ah, r)
    return _cache[key]


def _oracle_stop(r, c, floor=0.0):
    """(j*, tol) from the oracle's history alone: the first boundary j* >= 2 whose residual is below half the smallest earlier boundary
    residual, tol = their geometric mean.  Both residuals must be positive (and above `floor`), or the gap decides nothing."""
    b = [float(r[j * c - 1]) for j in range(1, len(r) // c + 1)]
    for j in range(2, len(b) + 1):
        lo = min(b[: j - 1])
        if b[j - 1] < 0.5 * lo:
            assert b[j - 1] > floor and lo > floor, "the oracle's residuals at the chosen boundaries are not positive: %r" % (b[:j],)
            return j, float(np.sqrt(b[j - 1] * lo))
    raise AssertionError("the oracle's history has no factor-2 drop at a batch boundary: %r" % (b,))


def _solver(p, dh, ah, structured=False, precision="f64", **kw):
    s = capi.Solver(p["network"], p["tree"], p["config"], structured=structured, precision=precision, **kw)
    s.initialiseSmpcController(dh, ah)
    return s


def _by_batches(s, c, total):
    """test 2's construction: rn_apg_reset and the batches an rn_apg_solve of `total` iterations is made of, as rn_apg_iterate calls"""
    s.apgReset()
    hist = [s.apgIterate(min(c, total - k)) for k in range(0, total, c)]
    return np.concatenate(hist) if hist else np.zeros(0)


def _same_bits(a, b):
    for bid in ALL_BUFS:
        assert np.array_equal(a.get(bid), b.get(bid)), bid


def _check_case(name, c, structured, precision="f64", tol_parity=REL_TOL, floor=0.0):
    p, dh, ah, r = _variant(name, c, precision)
    jstar, tol = _oracle_stop(r, c, floor)          # before the GPU is touched
    want = jstar * c
    s = _solver(p, dh, ah, structured, precision)
    run, hist = s.apg_solve(M, tol, c)
    print("%s c=%d %s %s: oracle j*=%d tol=%.6g -> %d iterations; GPU ran %d" % (name, c, "structured" if structured else "dense", precision, jstar, tol, want, run))
    assert run == want
    ls = s.last_solve()
    below = np.flatnonzero(hist <= tol)
    assert ls == {"iterations": want, "stopped": 1, "first_below": int(below[0]), "batches": jstar}, (ls, below[:3])
    assert np.abs(hist - r[:want]).max() <= tol_parity * np.abs(r[:want]).max()
    o = Oracle(p["network"], p["tree"], p["config"], precision=precision)
    o.initialise(dh, ah)
    o.apg(want)
    bad = {nm: relmax(s.get(bid), o.get(nm)) for bid, nm in ORACLE_PAIRS}
    assert all(v < tol_parity for v in bad.values()), bad
    return p, dh, ah, s, tol, want


@pytest.mark.parametrize("structured", [False, True], ids=["dense", "structured"])
@pytest.mark.parametrize("c", [7, 16, 20])
@pytest.mark.parametrize("name", ["small", "odd", "ragged"])
def test_stop_count_comes_from_the_oracle(name, c, structured):
    """c = 7: the exact path (the fix-up launch closes the batch), 16: the optimistic threshold, 20: the default"""
    _check_case(name, c, structured)


def test_stop_count_fp32():
    """against the fp32 oracle at the suite's fp32 tolerance; residuals at the boundaries above 1e-3, so the factor-2 gap still decides"""
    _check_case("small", 20, False, precision="f32", tol_parity=FP32_TOL, floor=1e-3)


@pytest.mark.parametrize("structured", [False, True], ids=["dense", "structured"])
@pytest.mark.parametrize("name,c", [("small", 7), ("odd", 16), ("ragged", 20)])
def test_bitwise_equal_to_its_batches(name, c, structured):
    p, dh, ah, s, tol, run = _check_case(name, c, structured)
    t = _solver(p, dh, ah, structured)
    _by_batches(t, c, run)
    _same_bits(s, t)
    assert s.counters() == t.counters()


@pytest.mark.parametrize("structured", [False, True], ids=["dense", "structured"])
def test_tolerance_zero_runs_every_iteration(structured):
    p, dh, ah, _ = _variant("small", 20)
    s, t = _solver(p, dh, ah, structured), _solver(p, dh, ah, structured)
    run, hist = s.apg_solve(50, 0.0, 20)
    assert run == 50 and hist.shape == (50,)
    ls = s.last_solve()
    assert ls["iterations"] == 50 and ls["stopped"] == 0 and ls["batches"] == 3
    ref = _by_batches(t, 20, 50)            # 20 + 20 + 10
    assert np.array_equal(hist, ref)
    _same_bits(s, t)


@pytest.mark.parametrize("structured", [False, True], ids=["dense", "structured"])
def test_default_is_untouched(structured):
    """a context that was told rn_set_stop_tolerance(0, 0) against one that never heard of the feature: control action and algorithmApg, bit for bit"""
    p, dh, ah, _ = _variant("small", 20)
    a = capi.Solver(p["network"], p["tree"], p["config"], structured=structured)
    b = capi.Solver(p["network"], p["tree"], p["config"], structured=structured)
    assert a.stopTolerance() == (0.0, 20)
    b.setStopTolerance(0.0, 0)
    assert b.stopTolerance() == (0.0, 20)
    for s in (a, b):
        s.factorStep()
    ua, ub = a.controlAction(dh, ah, maxIterations=45), b.controlAction(dh, ah, maxIterations=45)
    assert np.array_equal(ua, ub)
    _same_bits(a, b)
    assert a.last_solve() == b.last_solve() == {"iterations": 45, "stopped": 0, "first_below": -1, "batches": 1}
    ha, hb = a.algorithmApg(45), b.algorithmApg(45)
    assert np.array_equal(ha, hb)
    _same_bits(a, b)
    assert a.counters() == b.counters()
    # and both are what the batch construction gives for ONE batch of 45
    t = _solver(p, dh, ah, structured)
    assert np.array_equal(_by_batches(t, 45, 45), ha)
    _same_bits(a, t)


def _fixture_tol(o_hist, c, first=12):
    """a tolerance the fixture's cold first step reaches within its first boundaries: 1.5 x the smallest positive boundary residual there"""
    b = np.array([o_hist[j * c - 1] for j in range(1, first + 1)])
    assert (b > 0).any()
    j0 = int(np.flatnonzero(b > 0)[np.argmin(b[b > 0])])
    return 1.5 * float(b[j0]), (j0 + 1) * c


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
def test_control_action_under_a_tolerance(ref_fixture, warm):
    """the closed-loop fixture (the reference's 3-tank files, 500 iterations per control step), two control steps: u0 is the oracle's for the
    iteration counts the library reports.  (Whether the warm start needs fewer iterations is a measurement: tools/ab_stop_tolerance.py.)"""
    f = ref_fixture
    c = 20
    maxit = int(np.ravel(f["config"]["maxIterations"])[0])
    dh0, ah0 = forecast_at(f["forecast"], 0)
    dh1, ah1 = forecast_at(f["forecast"], 1)
    o = Oracle(f["network"], f["tree"], f["config"])
    o.factor_step()
    o.update_state_control()
    o.eliminate(dh0, ah0)
    tol, latest = _fixture_tol(o.apg(maxit), c)
    s = capi.Solver(f["network"], f["tree"], f["config"], stop_tolerance=tol, stop_check_every=c)
    assert s.stopTolerance() == (tol, c)
    s.factorStep()
    s.setWarmStart(warm)
    u0 = s.controlAction(dh0, ah0)
    n0 = s.last_solve()
    print("step 0: %r (tol %.6g)" % (n0, tol))
    assert 0 < n0["iterations"] <= min(maxit, latest) and n0["iterations"] % c == 0 and n0["stopped"] == 1
    o.apg(n0["iterations"])
    assert relmax(u0, o.get("u")[: o.nu]) < REL_TOL
    x1 = np.asarray(f["config"]["currentX"], float) * 0.97
    u1 = s.controlAction(dh1, ah1, currentX=x1, prevU=u0)
    n1 = s.last_solve()
    print("step 1 (%s): %r" % ("warm" if warm else "cold", n1))
    assert 0 < n1["iterations"] <= maxit and n1["batches"] == -(-n1["iterations"] // c)
    if warm:
        o.set("xi", o.get("updXi")); o.set("psi", o.get("updPsi"))      # y := y+ ; y+ kept
    o.update_state_control(x1, u0)
    o.eliminate(dh1, ah1)
    if warm:
        o.apg_continue(n1["iterations"], [1.0, 1.0])
    else:
        o.apg(n1["iterations"])
    assert relmax(u1, o.get("u")[: o.nu]) < REL_TOL


@pytest.mark.parametrize("structured", [False, True], ids=["dense", "structured"])
def test_replayed_batch_is_judged_on_the_replay(structured):
    """the penalties of tests/test_gpu_parity.py's tripped-replay case: the first optimistic batch trips and is replayed through the exact path,
    whose fix-up launch then closes the batches (the tripped iterations' records come from its last arriver)"""
    c = 20
    p = synth.make_problem("small", penalty_x=20.0, penalty_xs=5.0)
    dh, ah = synth.forecast_at(p["forecast"], 0)
    o = Oracle(p["network"], p["tree"], p["config"])
    o.initialise(dh, ah)
    r = o.apg(M)
    b = [float(r[j * c - 1]) for j in range(1, M // c + 1)]
    # first boundary (>= 2) at least 1.0 below every earlier one: the tolerance goes half-way (1e-9 parity of residuals of size 1e3: 1e-6)
    jstar = next(j for j in range(2, len(b) + 1) if b[j - 1] < min(b[: j - 1]) - 1.0)
    tol = 0.5 * (b[jstar - 1] + min(b[: jstar - 1]))
    assert tol > 0
    s, t = _solver(p, dh, ah, structured), _solver(p, dh, ah, structured)
    run, hist = s.apg_solve(M, tol, c)
    assert s.counters()["replayed"] >= 1, s.counters()
    assert run == jstar * c and s.last_solve()["batches"] == jstar and s.last_solve()["stopped"] == 1
    assert s.last_solve()["first_below"] == int(np.flatnonzero(hist <= tol)[0])
    assert np.abs(hist - r[:run]).max() <= REL_TOL * np.abs(r[:run]).max()
    ref = _by_batches(t, c, run)
    assert np.array_equal(hist, ref)
    _same_bits(s, t)
    assert s.counters() == t.counters()


def test_arguments_and_state():
    import ctypes as C

    p, dh, ah, _ = _variant("small", 20)
    s = capi.Solver(p["network"], p["tree"], p["config"])
    run = C.c_int(-1)
    assert s.lib.rn_apg_solve(s.h, 10, 1.0, 5, C.byref(run), None) == -3          # RN_E_STATE: before the factor step
    s.initialiseSmpcController(dh, ah)
    for tol in (-1.0, float("nan"), float("inf")):
        assert s.lib.rn_apg_solve(s.h, 10, tol, 5, C.byref(run), None) == -1, tol   # RN_E_ARG
        assert s.lib.rn_set_stop_tolerance(s.h, tol, 5) == -1, tol
    assert s.lib.rn_apg_solve(s.h, -1, 1.0, 5, C.byref(run), None) == -1
    assert s.lib.rn_apg_solve(s.h, 10, 1.0, 5, None, None) == -1
    assert s.lib.rn_get_last_solve(s.h, None) == -1
    assert s.stopTolerance() == (0.0, 20)
    assert s.apg_solve(0, 1.0, 5)[0] == 0 and s.last_solve() == {"iterations": 0, "stopped": 0, "first_below": -1, "batches": 0}
    # a solve inside the reserved iteration count allocates nothing (the leak check of SmpcController.cu:1612-1623 stays meaningful)
    s.reserveIterations(200)
    s.apg_solve(40, 0.0, 20)
    before = s.deviceMemoryInfo()["context_bytes"]
    assert s.apg_solve(200, 0.0, 0)[0] == 200 and s.last_solve()["batches"] == 10
    assert s.apg_solve(200, 1e30, 7)[0] == 7
    assert s.deviceMemoryInfo()["context_bytes"] == before


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_ranks_stop_together(world):
    """the in-process stand-in of tests/test_gpu_sharded_batched.py: the record every rank reads comes from the all-reduced history"""
    c = 20
    p, dh, ah, r = _variant("small", c)
    jstar, tol = _oracle_stop(r, c)
    full = _solver(p, dh, ah)
    want, _ = full.apg_solve(M, tol, c)
    assert want == jstar * c
    group = capi.local_group_create(world)
    shards = []
    try:
        for rk in range(world):
            s = capi.Solver(p["network"], p["tree"], p["config"], rank=rk, nranks=world, cut_stage=0)
            s.joinLocalGroup(group, rk)
            shards.append(s)
        out, errs = [None] * world, []

        def work(i):
            try:
                shards[i].initialiseSmpcController(dh, ah)
                out[i] = (shards[i].apg_solve(M, tol, c), shards[i].last_solve())
            except Exception as e:   # noqa: BLE001 -- reported below, with the rank
                errs.append((i, e))

        ts = [threading.Thread(target=work, args=(i,)) for i in range(world)]
        for th in ts:
            th.start()
        for th in ts:
            th.join()
        assert not errs, errs
        for (run, hist), ls in out:
            assert run == want and ls == out[0][1] and ls == full.last_solve(), (run, ls)
            assert np.array_equal(hist, out[0][0][1])
        dims = {capi.BUF_X: full.nx, capi.BUF_U: full.nu, capi.BUF_UPD_XI: 2 * full.nx, capi.BUF_UPD_PSI: full.nu, capi.BUF_DUAL_XI: 2 * full.nx}
        for bid, dim in dims.items():
            got = partition.scatter_to_global([s.get(bid) for s in shards], [s.global_nodes for s in shards], shards[0].full_nodes, dim)
            assert relmax(got, full.get(bid)) < REL_TOL, bid
    finally:
        for s in shards:
            s.close()
        capi.local_group_destroy(group)


_GUARD_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import test_gpu_stop_tolerance as t
from rapidnet_amd import capi
import gc, numpy as np
p, dh, ah, s, tol, run = t._check_case("odd", 16, False)
assert all(np.isfinite(s.get(b)).all() for b in t.ALL_BUFS)
assert s.guardCheck() == 0
s.close(); del s; gc.collect()
print("GUARD", *capi.guard_report())
"""


def test_one_case_under_guard_mode():
    """RAPIDNET_GUARD=1 (red zones around every device buffer, NaN poison) is read when the library first creates a context: a fresh process"""
    env = dict(os.environ, RAPIDNET_GUARD="1")
    r = subprocess.run([sys.executable, "-s", "-c", _GUARD_CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("GUARD ")][-1].split()
    assert int(line[1]) >= 1 and int(line[2]) == 0, line
