"""rn_set_restart(RN_RESTART_GRADIENT): the gradient test at the batch ends of an APG solve, and the momentum restart it decides.

  * the kernel alone (rn_debug_restart_test) against numpy on the buffers read back, |g_gpu - g_np| <= 1e-12 x sum |terms| (the sum is fp64
    whatever the context's type), repeatable bit for bit, clean under the buffer guard;
  * a solve in which the test never fires is the plain solve, bit for bit;
  * a solve in which it fires restarts where the CPU oracle's restatement does (tests/restart_oracle.py: the oracle driven through
    Oracle.apg_continue, g in numpy, the restart by hand) and has its iterates at every batch end: 1e-9 up to iteration 200, 1e-8 after;
  * with a stop tolerance, through rn_control_action with a warm start, on shards of 2 and 3 ranks, on an fp32 context; FBE / NAMA ignore it.

The iterates at a batch end are read behind a solve of that many iterations: a solve of k batches is the first k batches of a longer one, launch
for launch, so the solves of 1, 2, ... batches show every boundary of the long solve (and rn_get_restart_info of each shows whether its last
boundary fired).  Every boundary of every oracle run used here is far from marginal, |g| >= 1e-6 sqrt(na2 nb2) -- asserted, none skipped:
margins found on the CPU with checkEvery = 20: small |cos| >= 0.42 over 400 iterations (3e-2 over 1 200), tiny >= 0.099 over 600."""
import gc

import numpy as np
import pytest

import restart_oracle as ro
from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from test_gpu_sharded_batched import Ranks

pytestmark = pytest.mark.gpu
REL_TOL = 1e-9           # the project's level for fp64 iterates ...
LATE_TOL = 1e-8          # ... and behind iteration 200
FP32_TOL = 2e-4          # the suite's fp32 tolerance (tests/test_gpu_parity.py)
SUM_TOL = 1e-12          # the kernel's fp64 sum against numpy's, relative to the sum of the terms' magnitudes
MARGIN = 1e-6            # a boundary with |g| below this x sqrt(na2 nb2) would be marginal
W = (capi.BUF_ACC_XI, capi.BUF_ACC_PSI)
YP = (capi.BUF_UPD_XI, capi.BUF_UPD_PSI)
Y = (capi.BUF_XI, capi.BUF_PSI)
ALL_BUFS = [getattr(capi, n) for n in ("BUF_X", "BUF_U", "BUF_V", "BUF_XI", "BUF_PSI", "BUF_ACC_XI", "BUF_ACC_PSI", "BUF_UPD_XI", "BUF_UPD_PSI",
                                        "BUF_PRIMAL_XI", "BUF_PRIMAL_PSI", "BUF_DUAL_XI", "BUF_DUAL_PSI", "BUF_RES_XI", "BUF_RES_PSI")]
ORACLE_PAIRS = [(capi.BUF_X, "x"), (capi.BUF_U, "u"), (capi.BUF_XI, "xi"), (capi.BUF_PSI, "psi"), (capi.BUF_UPD_XI, "updXi"), (capi.BUF_UPD_PSI, "updPsi")]


def relmax(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


_cache = {}


def _problem(name):
    if ("p", name) not in _cache:
        p = synth.make_problem(name, feasible=True)
        _cache[("p", name)] = (p,) + tuple(synth.forecast_at(p["forecast"], 0))
    return _cache[("p", name)]


def _oracle_run(name, iterations, every=20, precision="f64", tol=0.0):
    """the restatement on the oracle, once per case: its result and the iterates behind every batch end -- shared, never modified"""
    key = ("o", name, iterations, every, precision, tol)
    if key not in _cache:
        p, dh, ah = _problem(name)
        o = Oracle(p["network"], p["tree"], p["config"], precision=precision)
        o.initialise(dh, ah)
        snaps = {}

        def snap(done, orc):
            snaps[done] = {nm: orc.get(nm) for _, nm in ORACLE_PAIRS}

        r = ro.restart_loop(o, iterations, every, restart=True, tol=tol, at_batch_end=snap)
        _cache[key] = (r, snaps)
    return _cache[key]


def _assert_no_boundary_is_marginal(r):
    assert r["tests"], "the oracle run tested no boundary"
    for k, t in enumerate(r["tests"]):
        assert abs(t[0]) >= MARGIN * np.sqrt(t[1] * t[2]), "boundary %d of the oracle run is marginal: %r" % (k + 1, t)


def _solver(name, structured=False, precision="f64", **kw):
    p, dh, ah = _problem(name)
    s = capi.Solver(p["network"], p["tree"], p["config"], structured=structured, precision=precision, **kw)
    s.initialiseSmpcController(dh, ah)
    return s


def _vectors(s):
    return tuple(np.concatenate([s.get(a), s.get(b)]) for a, b in (W, YP, Y))


def _check_kernel(s, label):
    """rn_debug_restart_test on the context's current w, y+, y against numpy on the same buffers; twice: the same bits"""
    g, na2, nb2, mag = ro.gradient_test(*_vectors(s))
    out = s.debugRestartTest()
    print("%s: g %.17g (numpy %.17g, sum |terms| %.3g), na2 %.17g (%.17g), nb2 %.17g (%.17g)" % (label, out[0], g, mag, out[1], na2, out[2], nb2))
    assert np.isfinite(out).all()
    assert abs(out[0] - g) <= SUM_TOL * mag and abs(out[1] - na2) <= SUM_TOL * na2 and abs(out[2] - nb2) <= SUM_TOL * nb2
    assert s.debugRestartTest() == out
    return out


# ---- the kernel alone -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("structured", [False, True], ids=["dense", "structured"])
@pytest.mark.parametrize("name", ["tiny", "odd", "ragged", "small"])
def test_kernel_against_numpy(name, structured, precision):
    """after 1, 5 and 20 iterations; n_tot = 228, 891, 2 185, 1 330: fewer elements than one grid, odd: no multiple of the 16-byte slot in
    either type (the tail loop), ragged: 2 185 = 546 fp32 slots + 1"""
    s = _solver(name, structured, precision)
    s.apgReset()
    assert s.debugRestartTest() == (0.0, 0.0, 0.0)          # all three vectors are zero behind a reset
    done = 0
    for upto in (1, 5, 20):
        s.apgIterate(upto - done, history=False)
        done = upto
        out = _check_kernel(s, "%s %s %s after %d" % (name, "structured" if structured else "dense", precision, upto))
        assert out[1] >= 0 and out[2] >= 0
    s.apgReset()
    s.apgIterate(20, history=False)          # ... and behind ONE batch of 20: the optimistic path's rotation
    _check_kernel(s, "%s behind one batch of 20" % name)
    assert s.last_restarts() == dict(restarts=0, last_at=-1, tested=0, g=0.0, na2=0.0, nb2=0.0)      # the hook is no solve
    assert s.restart() == "off"                                                                        # ... and no setting
    s.close()


def test_kernel_under_the_buffer_guard(monkeypatch):
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    s = _solver("odd", restart="gradient")
    s.apgReset()
    s.apgIterate(20, history=False)
    _check_kernel(s, "odd under the guard")
    run, hist = s.apg_solve(60, 0.0, 20)
    assert run == 60 and np.isfinite(hist).all() and s.last_restarts()["tested"] == 3
    assert np.isfinite([s.last_restarts()[k] for k in ("g", "na2", "nb2")]).all()
    assert s.guardCheck() == 0
    s.close()
    after = capi.guard_report()
    assert after[0] >= before[0] + 1 and after[1] == before[1]


# ---- argument validation on a live context ------------------------------------------------------------------------------------------------
def test_a_bad_mode_and_null_outputs_are_refused_on_a_live_context():
    """RN_E_ARG, nothing written and the setting unchanged -- in either state of the setting; the context goes on working"""
    RN_E_ARG = -1
    s = _solver("tiny")
    s.apgReset()
    s.apgIterate(5, history=False)
    want = s.debugRestartTest()
    for state in ("off", "gradient"):
        s.setRestart(state)
        for bad in (2, 7, -1):
            assert s.lib.rn_set_restart(s.h, bad) == RN_E_ARG and s.restart() == state, (state, bad)
        assert s.lib.rn_get_restart(s.h, None) == RN_E_ARG
        counts, last = np.full(4, 77, dtype=np.int64), np.full(3, 77.0)
        assert s.lib.rn_get_restart_info(s.h, None, last.ctypes.data) == RN_E_ARG
        assert s.lib.rn_get_restart_info(s.h, counts.ctypes.data, None) == RN_E_ARG
        assert s.lib.rn_get_restart_info(s.h, None, None) == RN_E_ARG
        assert (counts == 77).all() and (last == 77.0).all()          # a refused call writes neither array
        assert s.lib.rn_debug_restart_test(s.h, None) == RN_E_ARG
        assert s.restart() == state and s.debugRestartTest() == want
    run, hist = s.apg_solve(40, 0.0, 20)
    assert run == 40 and np.isfinite(hist).all() and s.last_restarts()["tested"] == 2
    s.close()


# ---- never fires: the plain solve ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structured", [False, True], ids=["dense", "structured"])
def test_a_solve_that_never_restarts_is_the_plain_solve(structured):
    """barcelona31, feasible: the oracle's loop does not fire within 1 200 iterations (profiles/ab_restart.txt)"""
    on, off = _solver("barcelona31", structured, restart="gradient"), _solver("barcelona31", structured)
    assert on.restart() == "gradient" and off.restart() == "off"
    run1, h1 = on.apg_solve(200, 0.0, 20)
    run0, h0 = off.apg_solve(200, 0.0, 20)
    assert run1 == run0 == 200 and np.array_equal(h1, h0)
    for bid in ALL_BUFS:
        assert np.array_equal(on.get(bid), off.get(bid)), bid
    info = on.last_restarts()
    assert (info["restarts"], info["last_at"], info["tested"]) == (0, -1, 10), info
    assert info["g"] < 0 and abs(info["g"]) >= MARGIN * np.sqrt(info["na2"] * info["nb2"])
    assert off.last_restarts() == dict(restarts=0, last_at=-1, tested=0, g=0.0, na2=0.0, nb2=0.0)
    assert on.last_solve() == off.last_solve() and on.counters() == off.counters()
    on.close(); off.close()


# ---- fires: against the oracle ---------------------------------------------------------------------------------------------------------------
def _walk_boundaries(s, name, iterations, every, precision="f64", tol_early=REL_TOL, tol_late=LATE_TOL):
    """solves of 1, 2, ... batches: the iterates behind every boundary against the oracle's, the boundaries that fired; returns (fires, last history)"""
    r, snaps = _oracle_run(name, iterations, every, precision)
    _assert_no_boundary_is_marginal(r)
    fires, hist = [], None
    for k in range(1, iterations // every + 1):
        done = k * every
        run, hist = s.apg_solve(done, 0.0, every)
        assert run == done
        info = s.last_restarts()
        assert info["tested"] == k and info["restarts"] >= len(fires)
        if info["restarts"] > len(fires):
            assert info["restarts"] == len(fires) + 1 and info["last_at"] == done and info["g"] > 0
            fires.append(done)
        else:
            assert info["g"] <= 0 and info["last_at"] == (fires[-1] if fires else -1)
        assert (info["g"] > 0) == (r["tests"][k - 1][0] > 0), (done, info, r["tests"][k - 1])
        tol = tol_early if done <= 200 else tol_late
        bad = {nm: relmax(s.get(bid), snaps[done][nm]) for bid, nm in ORACLE_PAIRS}
        assert all(v < tol for v in bad.values()), (done, bad)
    return fires, hist, r


@pytest.mark.parametrize("name,iterations,want,structured", [("small", 400, [180], False), ("small", 400, [180], True),
                                                              ("tiny", 600, [120, 300, 420, 540], False)])
def test_restarts_where_the_oracle_restarts(name, iterations, want, structured):
    s = _solver(name, structured, restart="gradient")
    fires, hist, r = _walk_boundaries(s, name, iterations, 20)
    print("%s: oracle fires %r, GPU fires %r" % (name, r["fires"], fires))
    assert r["fires"] == want and fires == want
    # the solve's bookkeeping runs through the restarts: the history covers every iteration, the count is the solve's
    assert len(hist) == iterations and np.abs(hist - r["hist"]).max() <= LATE_TOL * np.abs(r["hist"]).max()
    ls = s.last_solve()
    assert ls["iterations"] == iterations and ls["batches"] == iterations // 20 and ls["stopped"] == 0
    assert s.last_restarts()["restarts"] == len(want) and s.last_restarts()["last_at"] == want[-1]
    parts = s.historyParts(0, iterations)
    assert np.isfinite(parts).all() and np.array_equal(np.maximum(parts[:, 1], parts[:, 3]), hist)
    # rn_algorithm_apg under the setting is the same solve (batches of the stop tolerance's checkEvery, default 20)
    t = _solver(name, structured, restart="gradient")
    h2 = t.algorithmApg(iterations)
    assert np.array_equal(h2, hist) and t.last_restarts() == s.last_restarts()
    # ... with no tolerance set: rn_get_last_solve's "first iteration below the tolerance" is -1, whatever the residuals were (on `small` they
    # are exactly 0 over the first 140 iterations)
    assert t.last_solve() == {"iterations": iterations, "stopped": 0, "first_below": -1, "batches": iterations // 20}
    for bid in ALL_BUFS:
        assert np.array_equal(t.get(bid), s.get(bid)), bid
    s.close(); t.close()


def test_fp32_context_restarts_on_the_fp64_schedule():
    """small: every boundary of the fp64 oracle has |cos| >= 0.42, none is marginal, so the fp32 context must restart exactly where fp64 does;
    its iterates against the fp32 oracle's restatement at the suite's fp32 tolerance"""
    r64, _ = _oracle_run("small", 400, 20)
    _assert_no_boundary_is_marginal(r64)
    s = _solver("small", precision="f32", restart="gradient")
    fires, hist, r32 = _walk_boundaries(s, "small", 400, 20, precision="f32", tol_early=FP32_TOL, tol_late=FP32_TOL)
    assert fires == r64["fires"] == r32["fires"] == [180]
    assert len(hist) == 400
    s.close()


# ---- with a tolerance -----------------------------------------------------------------------------------------------------------------------
def test_with_a_tolerance_the_restart_saves_iterations_on_small():
    """The library stops on vecPrimalInfs, the larger of two SIGNED residual entries; on `small` that is exactly 0 over the first 140
    iterations, so with batches of 20 every solve stops at 20, restart or not.  Batches of 240 put the first boundary behind that prefix.
    CPU run (tests/test_host_restart.py), tol = 1e-3: plain 1 200 iterations, with the restart (it fires at 480) 720.  Asserted: the inequality."""
    every, tol, cap = 240, 1e-3, 1440
    on, off = _solver("small", restart="gradient"), _solver("small")
    run1, h1 = on.apg_solve(cap, tol, every)
    run0, h0 = off.apg_solve(cap, tol, every)
    print("iterations to %.0e on small, batches of %d: restart %d, plain %d" % (tol, every, run1, run0))
    assert run1 < run0
    for run, h, s in ((run1, h1, on), (run0, h0, off)):
        assert run % every == 0 and h[run - 1] <= tol and all(h[k - 1] > tol for k in range(every, run, every))     # the FIRST batch below tol
        assert s.last_solve()["stopped"] == 1 and s.last_solve()["iterations"] == run
    info = on.last_restarts()
    assert info["tested"] == run1 // every - 1 and info["restarts"] >= 1 and info["last_at"] < run1      # the batch that stopped did not restart
    on.close(); off.close()


# ---- rn_control_action, warm start on ---------------------------------------------------------------------------------------------------------
def test_control_action_with_warm_start_matches_the_oracle_sequence():
    p, dh0, ah0 = _problem("small")
    dh1, ah1 = synth.forecast_at(p["forecast"], 1)
    x1 = np.asarray(p["config"]["currentX"], float) * 0.97
    o = Oracle(p["network"], p["tree"], p["config"])
    o.factor_step()
    o.update_state_control()
    o.eliminate(dh0, ah0)
    r0 = ro.restart_loop(o, 200, 20)
    uo0 = o.get("u")[: o.nu].copy()
    o.set("xi", o.get("updXi")); o.set("psi", o.get("updPsi"))      # the warm start: y := y+ ; y+ kept; theta = {1, 1}
    o.update_state_control(x1, uo0)
    o.eliminate(dh1, ah1)
    r1 = ro.restart_loop(o, 200, 20, reset=False)
    _assert_no_boundary_is_marginal(r0); _assert_no_boundary_is_marginal(r1)
    assert r0["fires"] and r1["fires"], (r0["fires"], r1["fires"])      # (CPU: [180] and [160])
    s = capi.Solver(p["network"], p["tree"], p["config"], restart="gradient")
    s.factorStep()
    s.setWarmStart(True)
    u0 = s.controlAction(dh0, ah0, maxIterations=200)
    i0 = s.last_restarts()
    u1 = s.controlAction(dh1, ah1, currentX=x1, prevU=uo0, maxIterations=200)
    i1 = s.last_restarts()
    assert (i0["restarts"], i0["last_at"], i0["tested"]) == (len(r0["fires"]), r0["fires"][-1], 10), (i0, r0["fires"])
    assert (i1["restarts"], i1["last_at"], i1["tested"]) == (len(r1["fires"]), r1["fires"][-1], 10), (i1, r1["fires"])
    assert relmax(u0, uo0) < REL_TOL and relmax(u1, o.get("u")[: o.nu]) < REL_TOL
    assert s.last_solve() == {"iterations": 200, "stopped": 0, "first_below": -1, "batches": 10}      # no tolerance was set: -1
    s.close()


# ---- FBE / NAMA ignore the setting ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["globalFbeAlgorithm", "namaAlgorithm"])
def test_quasi_newton_loops_ignore_the_setting(alg):
    outs = []
    for mode in ("gradient", "off"):
        s = _solver("small", restart=mode)
        s.setAlgorithm(alg, 5)
        res = (s.algorithmGlobalFbe if alg == "globalFbeAlgorithm" else s.algorithmNama)(12)
        outs.append((res, [s.get(b) for b in (capi.BUF_X, capi.BUF_U, capi.BUF_XI, capi.BUF_PSI, capi.BUF_UPD_XI, capi.BUF_UPD_PSI)], s.last_restarts()["tested"]))
        s.close()
    for a, b in zip(outs[0][0], outs[1][0]):
        assert np.array_equal(a, b)
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(a, b)
    assert outs[0][2] == 0


# ---- shards -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,cut", [(2, 3), (3, 0)])
def test_shards_agree_with_each_other_and_with_the_whole_tree(world, cut, monkeypatch):
    monkeypatch.setenv("RAPIDNET_GROUP_TIMEOUT_S", "30")       # ranks that decided differently would wait for each other: fail soon
    p, dh, ah = _problem("small")
    r, _ = _oracle_run("small", 400, 20)
    _assert_no_boundary_is_marginal(r)
    full = _solver("small", restart="gradient")
    full.apgReset()
    full.apgIterate(20, history=False)
    mag = ro.gradient_test(*_vectors(full))[3]
    gfull = full.debugRestartTest()
    rk = Ranks(p, world, cut)
    try:
        def work(s):
            s.initialiseSmpcController(dh, ah)
            s.setRestart("gradient")
            s.apgReset()
            s.apgIterate(20, history=False)
            g = s.debugRestartTest()
            assert s.debugRestartTest() == g
            fires, upto = [], 400
            while upto > 0:          # a solve of `upto` iterations reports its last restart: walk the restarts from the last to the first
                run, _ = s.apg_solve(upto, 0.0, 20)
                info = s.last_restarts()
                assert run == upto and info["tested"] == upto // 20
                if upto == 400:
                    last = (info, s.last_solve())
                if info["restarts"] == 0:
                    break
                fires.insert(0, info["last_at"])
                upto = info["last_at"] - 20
            return g, fires, last

        res = rk.run(work)
        print("world %d: g per rank %r, unsharded %r; fires %r" % (world, [x[0] for x in res], gfull, [x[1] for x in res]))
        for g, fires, last in res:
            assert g == res[0][0]                                   # the same bits on every rank
            assert all(abs(a - b) <= SUM_TOL * m for a, b, m in zip(g, gfull, (mag, gfull[1], gfull[2])))
            assert fires == r["fires"] == [180]
            assert last == res[0][2] and last[1]["iterations"] == 400 and last[0]["restarts"] == 1
        # ... and the unsharded context on the same schedule, its iterates those of the shards
        run, _ = full.apg_solve(400, 0.0, 20)
        assert run == 400 and full.last_restarts()["last_at"] == 180 and full.last_restarts()["restarts"] == 1
        rk.run(lambda s: s.apg_solve(400, 0.0, 20))
        for bid, dim in ((capi.BUF_UPD_XI, 2 * full.nx), (capi.BUF_UPD_PSI, full.nu), (capi.BUF_U, full.nu)):
            assert relmax(rk.gathered(bid, dim), full.get(bid)) < LATE_TOL, bid
    finally:
        rk.close()
        full.close()
