"""rn_estimate_lipschitz / rn_get_lipschitz / rn_set_step_rule on the GPU against the numpy restatement (tests/lipschitz_oracle.py), which
tests/test_lipschitz_oracle.py holds to the dense definition M = K H^-1 K' on the CPU.  Every fp64 comparison is against the restatement fed
the same start vector and the same count.

1  history row by row (dense, structured, auto; 1, 2, 7, 40 iterations) and the three invariants.   2  a context of more than one block.
3  a caller's start.   4  own blocks, probabilities, fp32 storage: the estimate follows, staleness.   5  nothing else moves.   6  early stop.
7  shards.   8  fp32 contexts.   9  the step rule.   10  errors.   11  guard mode.

Bounds: NORM and RAYLEIGH 1e-9 relative (the project's fp64 bound: the power iteration contracts towards the dominant vector, rounding does not
accumulate); RESIDUAL 1e-6 absolute, the cancellation floor of s - t^2 in fp64.  $LIPSCHITZ_ERRORS names a file the measured worst values are
appended to (profiles/lipschitz_errors.txt)."""
import gc
import os

import numpy as np
import pytest

import lipschitz_oracle as lo
import test_lipschitz_oracle as tlo
from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from test_gpu_operator_storage import blocks_of, oracle_with_blocks
from test_gpu_sharded_batched import Ranks
from test_gpu_tree_data import make, reweighted

pytestmark = pytest.mark.gpu

RN_E_ARG, RN_E_STATE = -1, -3
REL, RES_ABS = 1e-9, 1e-6
COUNTS = (1, 2, 7, 40)
ALL_BUFS = tuple(range(capi.BUF_XMIN)) + tuple(range(capi.BUF_UMAX + 1, capi.BUF_UDIR + 1))      # every RN_BUF_*; the scaled bounds are in between
APG_BUFS = tuple(b for b in ALL_BUFS if b < capi.BUF_PREV_XI)
_WORST = {}


def record(line):
    print(line)
    path = os.environ.get("LIPSCHITZ_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def start_of(s, seed=0):
    return lo.hash_start(s.nodes, s.nx, s.nu, seed, global_nodes=getattr(s, "global_nodes", None))


def check_history(label, got, want, invariants_lam=None):
    """got, want: [rows][3]; returns the worst relative errors of NORM, RAYLEIGH and the worst absolute error of RESIDUAL"""
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert np.isfinite(got).all(), label
    e = [float(np.max(np.abs(got[:, c] - want[:, c]) / np.abs(want[:, c]))) for c in (lo.NORM, lo.RAYLEIGH)]
    e.append(float(np.max(np.abs(got[:, lo.RESIDUAL] - want[:, lo.RESIDUAL]))))
    print("%s: NORM %.2e RAYLEIGH %.2e RESIDUAL %.2e" % (label, *e))
    assert e[0] <= REL and e[1] <= REL and e[2] <= RES_ABS, (label, e)
    assert (got[:, lo.RAYLEIGH] <= got[:, lo.NORM] * (1 + 1e-12)).all(), label
    if invariants_lam is not None:
        assert (got[:, lo.NORM] <= invariants_lam * (1 + 1e-12)).all(), label
    return e


def oracle_apply(o):
    """apply(xi, psi) of the CPU oracle's Hessian sweep (a NAMA oracle: the sweep reads res)"""
    def apply(xi, psi):
        o.set("resXi", np.asarray(xi).ravel()); o.set("resPsi", np.asarray(psi).ravel())
        o.hessian_oracle()
        return o.get("primalXiDir").reshape(o.nodes, 2 * o.nx), o.get("primalPsiDir").reshape(o.nodes, o.nu)
    return apply


# ---- 1. history, row by row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "structured", "auto"])
@pytest.mark.parametrize("name", tlo.SHAPES)
def test_history_row_by_row_against_the_dense_definition(name, mode):
    p, fc = tlo.problem(name)
    M, lam, apply = tlo.dense(name)
    s = make(p, p["tree"], mode, "f64")
    s.factorStep()                                                          # the factor step alone: no affine terms yet
    xi, psi = start_of(s, tlo.SEED[name])
    want = lo.power_loop(apply, xi, psi, 40)
    worst = [0.0, 0.0, 0.0]
    for n in COUNTS:
        r = s.estimateLipschitz(n, seed=tlo.SEED[name], history=True)
        assert r["iterations"] == n and r["history"].shape == (n, 3)
        e = check_history("%s %s %d" % (name, mode, n), r["history"], want[:n], lam)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert np.array_equal(bits([r["norm"], r["rayleigh"], r["residual"]]), bits(r["history"][-1]))
        held = s.lipschitz()
        assert not held["stale"] and held["iterations"] == n and held["norm"] == r["norm"]
    assert r["norm"] >= 0.9999 * lam
    record("history %-7s %-10s worst over 1/2/7/40 iterations: NORM %.2e RAYLEIGH %.2e (rel), RESIDUAL %.2e (abs); NORM(40)/lambda_max %.8f"
           % (name, mode, *worst, r["norm"] / lam))
    s.close()


# ---- 2. more than one block of elements -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["medium", "barcelona31"])
def test_a_context_bigger_than_one_block_against_the_structured_operator(name):
    p, fc = tlo.problem(name)
    s = make(p, p["tree"], "structured", "f64")
    s.factorStep()
    assert s.nodes * s.ny > 4 * 256 * 4                                    # several workgroups of 16-byte vectors
    op = synth._Structured(p["network"], p["tree"], p["config"])
    xi, psi = start_of(s)
    want = lo.power_loop(op.apply, xi, psi, 10)
    r = s.estimateLipschitz(10, history=True)
    e = check_history("%s structured 10" % name, r["history"], want)
    record("blocks  %-11s structured, 10 iterations: NORM %.2e RAYLEIGH %.2e (rel), RESIDUAL %.2e (abs)" % (name, *e))
    s.close()


# ---- 3. a caller's start --------------------------------------------------------------------------------------------------------------------
def test_a_callers_start_reproduces_synths_estimate():
    name = "small"
    p, fc = tlo.problem(name)
    want = synth.lipschitz_estimate(p["network"], p["tree"], p["config"], iters=40, seed=0)
    nodes, nx, nu = tlo.dims(p)
    rng = np.random.default_rng(0)                                          # synth's own start: seed 0, xi drawn first
    xi = rng.standard_normal((nodes, 2 * nx))
    psi = rng.standard_normal((nodes, nu))
    for mode in ("dense", "structured"):
        s = make(p, p["tree"], mode, "f64")
        s.initialiseSmpcController(*fc)
        r = s.estimateLipschitz(40, start=(xi, psi))
        err = abs(r["norm"] - want) / want
        record("start   small %-10s the caller's start, 40 iterations against synth.lipschitz_estimate: %.2e" % (mode, err))
        assert err <= REL
        s.close()


# ---- 4. the estimate follows what the context holds; staleness ----------------------------------------------------------------------------------
def test_own_blocks_probabilities_and_fp32_storage():
    name = "small"
    p, fc = tlo.problem(name)
    s = make(p, p["tree"], "auto", "f64")
    s.initialiseSmpcController(*fc)
    base = s.estimateLipschitz(40)
    assert not s.lipschitz()["stale"]
    # bounds and errors alone do not enter M
    s.setBounds("shared", xmax=np.asarray(p["network"]["vecXmax"], float) * 0.9)
    assert not s.lipschitz()["stale"]
    s.setTreeData(errorDemand=np.asarray(p["tree"]["errorDemandNode"], float) * 1.5)
    assert not s.lipschitz()["stale"]
    # own blocks: Phi scaled by 1.1
    blk = blocks_of(s)
    blk["Phi"] = blk["Phi"] * 1.1
    s.setOperators(phi=blk["Phi"])
    assert s.lipschitz()["stale"] and s.lipschitz()["norm"] == base["norm"]
    o = oracle_with_blocks(p, fc, blk, alg="namaAlgorithm")
    xi, psi = start_of(s)
    want = lo.power_loop(oracle_apply(o), xi, psi, 40)
    r = s.estimateLipschitz(40, history=True)
    e = check_history("own blocks", r["history"], want)
    assert abs(r["norm"] - base["norm"]) > 1e-3 * base["norm"] and not s.lipschitz()["stale"]
    record("blocks  small Phi x 1.1 against the loop over the CPU oracle's Hessian sweep: NORM %.2e RAYLEIGH %.2e RESIDUAL %.2e" % tuple(e))
    s.close()
    # new probabilities
    s = make(p, p["tree"], "dense", "f64")
    s.initialiseSmpcController(*fc)
    base = s.estimateLipschitz(40)
    new = reweighted(p["tree"], fc, 3)
    s.setTreeData(prob=new["probNode"])
    assert s.lipschitz()["stale"]
    tree2 = dict(p["tree"], probNode=new["probNode"])
    o = Oracle(p["network"], tree2, p["config"])
    o.set_algorithm("namaAlgorithm", 5)
    o.initialise(*fc)
    o.fbe_reset()
    want = lo.power_loop(oracle_apply(o), xi, psi, 40)
    r = s.estimateLipschitz(40, history=True)
    e = check_history("probabilities", r["history"], want)
    # (lambda_max hardly depends on how the children share their parent's probability: 4e-7 relative here -- still 400 times the bound above)
    assert abs(r["norm"] - base["norm"]) > 100 * REL * base["norm"] and not s.lipschitz()["stale"]
    record("prob    small re-weighted tree against the loop over the CPU oracle's Hessian sweep: NORM %.2e RAYLEIGH %.2e RESIDUAL %.2e" % tuple(e))
    s.close()
    # fp32-stored blocks under fp64 iterates: the oracle on the blocks as stored
    s = make(p, p["tree"], "dense", "f64_store32")
    assert s.lib.rn_get_lipschitz(s.h, np.zeros(4).ctypes.data, None) == RN_E_STATE
    s.initialiseSmpcController(*fc)
    o = oracle_with_blocks(p, fc, blocks_of(s), alg="namaAlgorithm")
    want = lo.power_loop(oracle_apply(o), xi, psi, 40)
    r = s.estimateLipschitz(40, history=True)
    e = check_history("fp32 storage", r["history"], want)
    record("store32 small fp32-stored blocks against the loop over the CPU oracle on those blocks: NORM %.2e RAYLEIGH %.2e RESIDUAL %.2e" % tuple(e))
    s.factorStep()
    assert s.lipschitz()["stale"]
    s.close()


# ---- 5. nothing else moves ---------------------------------------------------------------------------------------------------------------------
def _fbe_iteration(s, fbe, it, probe):
    """one iteration of the step-wise global FBE / NAMA loop; probe(k) is called at every seam between two entry points"""
    s.solveStep(); probe(0)
    s.proximalFunG(); probe(1)
    s.computeFixedPointResidual(); probe(2)
    if fbe:
        s.computeGradientFbe()
    else:
        s.updateFixedPointResidualNamaAlgorithm()
    probe(3)
    if it > 0:
        v = s.computeValueFbe(); probe(4)
        s.computeLbfgsDirection(); probe(5)
        s.computeHessianOracalGlobalFbe(); probe(6)                         # (the step-wise API's own sweep: the line search repeats it)
        s.computeLineSearchLbfgsUpdate(v) if fbe else s.computeLineSearchAmeLbfgsUpdate(v)
        probe(6)
    s.dualUpdate(); probe(7)


@pytest.mark.parametrize("alg", ["proximalAlgorithm", "globalFbeAlgorithm", "namaAlgorithm"])
@pytest.mark.parametrize("mode", ["dense", "structured"])
def test_an_estimate_inside_a_solve_moves_nothing(alg, mode):
    name = "small"
    p, fc = tlo.problem(name)
    a, b = (make(p, p["tree"], mode, "f64") for _ in range(2))
    for s in (a, b):
        s.initialiseSmpcController(*fc)
        if alg != "proximalAlgorithm":
            s.setAlgorithm(alg, 5)
    bufs = APG_BUFS if alg == "proximalAlgorithm" else ALL_BUFS
    first = {}

    def estimate(s):
        r = s.estimateLipschitz(7, history=True)
        first.setdefault("r", r)
        assert np.array_equal(bits(r["history"]), bits(first["r"]["history"])) and r["norm"] == first["r"]["norm"]      # two estimates: the same bits

    if alg == "proximalAlgorithm":
        for s in (a, b):
            s.apgReset()
            h1 = s.apgIterate(9)
            if s is a:
                before = {bid: s.get(bid) for bid in bufs}
                estimate(s)
                estimate(s)
                for bid in bufs:
                    assert np.array_equal(bits(before[bid]), bits(s.get(bid))), (alg, mode, bid)
            h2 = s.apgIterate(11)
            s.hist = np.concatenate([h1, h2])
        assert np.array_equal(bits(a.hist), bits(b.hist))
    else:
        fbe = alg == "globalFbeAlgorithm"
        for it in range(12):
            # the estimate sits at every seam of iteration 9 and 10 in turn (between the direction -- its Hessian sweep included -- and the line search too)
            _fbe_iteration(a, fbe, it, (lambda k: estimate(a)) if it in (9, 10) else (lambda k: None))
            _fbe_iteration(b, fbe, it, lambda k: None)
        assert a.lbfgsState()[:3] == b.lbfgsState()[:3]
        for which in (0, 1):
            for col in range(1, 6):
                assert np.array_equal(bits(a.lbfgsColumn(which, col)), bits(b.lbfgsColumn(which, col)))
    for bid in bufs:
        assert np.array_equal(bits(a.get(bid)), bits(b.get(bid))), (alg, mode, bid)
    assert "r" in first
    a.close(); b.close()


def test_a_context_that_never_asks_allocates_nothing_and_the_first_estimate_keeps_its_buffers():
    p, fc = tlo.problem("small")
    s, twin = (make(p, p["tree"], "dense", "f64") for _ in range(2))
    for c in (s, twin):
        c.initialiseSmpcController(*fc)
        c.apgReset(); c.apgIterate(5)
    m0 = s.deviceMemoryInfo()["context_bytes"]
    assert twin.deviceMemoryInfo()["context_bytes"] == m0
    s.estimateLipschitz(3)
    m1 = s.deviceMemoryInfo()["context_bytes"]
    per_node = 2 * s.ny + s.nx + s.nu + s.nv + max(s.nu, s.nx, s.nv)           # v, w; x, u, v of the sweep; the zero block of an APG context
    assert m1 - m0 == 8 * (s.nodes * per_node + 1024 * 6 + 2 + 3 * 64), (m1 - m0)
    s.estimateLipschitz(40); s.estimateLipschitz(64)
    assert s.deviceMemoryInfo()["context_bytes"] == m1                         # kept
    u_s, u_t = s.controlAction(*fc, maxIterations=20), twin.controlAction(*fc, maxIterations=20)
    assert np.array_equal(bits(u_s), bits(u_t)) and twin.deviceMemoryInfo()["context_bytes"] == m0
    s.close(); twin.close()


# ---- 6. early stop ---------------------------------------------------------------------------------------------------------------------------------
def test_early_stop_at_the_multiple_the_restatement_stops_at():
    name = "small"
    p, fc = tlo.problem(name)
    M, lam, apply = tlo.dense(name)
    s = make(p, p["tree"], "dense", "f64")
    s.factorStep()
    xi, psi = start_of(s)
    want = lo.power_loop(apply, xi, psi, 40, tol=1e-4, check_every=5)
    full = lo.power_loop(apply, xi, psi, 40)
    assert 5 <= len(want) < 40 and len(want) % 5 == 0
    # (the decision must not sit on the tolerance: the records at the multiples of 5 keep clear of it by more than RESIDUAL's bound;
    #  the closest is 9.65e-5 at iteration 35, where the loop stops)
    assert all(abs(full[k - 1, lo.RESIDUAL] - 1e-4) > RES_ABS for k in range(5, 40, 5))
    r = s.estimateLipschitz(40, tol=1e-4, check_every=5, history=True)
    assert r["iterations"] == len(want) and r["residual"] <= 1e-4
    check_history("early stop", r["history"], want, lam)
    r0 = s.estimateLipschitz(40, tol=0.0, check_every=5, history=True)
    assert r0["iterations"] == 40
    assert np.array_equal(bits(r0["history"][: r["iterations"]]), bits(r["history"]))      # the checks change no bits
    record("stop    small tol 1e-4 every 5: stopped after %d iterations (restatement: %d), residual %.3e" % (r["iterations"], len(want), r["residual"]))
    s.close()


# ---- 7. shards -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,world,cut", [("small", 2, 1), ("small", 3, 2), ("ragged", 2, 2), ("ragged", 3, 1)])
def test_shards_hold_the_same_bits_and_the_one_gpu_contexts_history(name, world, cut):
    p, fc = tlo.problem(name)
    one = make(p, p["tree"], "dense", "f64")
    one.factorStep()
    want = one.estimateLipschitz(40, history=True)
    want_stop = one.estimateLipschitz(40, tol=1e-4, check_every=5)
    one.close()
    rk = Ranks(p, world, cut, False)
    try:
        def run(s):
            s.factorStep()
            r = s.estimateLipschitz(40, history=True)
            r2 = s.estimateLipschitz(40, tol=1e-4, check_every=5)
            return r, r2, s.guardCheck()
        out = rk.run(run)
        for rank, (r, r2, bad) in enumerate(out):
            assert bad == 0
            assert np.array_equal(bits(r["history"]), bits(out[0][0]["history"])), (name, world, rank)
            assert r2["iterations"] == out[0][1]["iterations"] == want_stop["iterations"] and r2["norm"] == out[0][1]["norm"]
        got = out[0][0]["history"]
        e = float(np.max(np.abs(got - want["history"])[:, :2] / np.abs(want["history"][:, :2])))
        record("shards  %-6s %d ranks cut %d: history against the one-GPU context's, NORM / RAYLEIGH %.2e (rel)" % (name, world, cut, e))
        assert e <= 1e-12
        assert np.max(np.abs(got[:, 2] - want["history"][:, 2])) <= RES_ABS
    finally:
        rk.close()


def test_a_shard_without_a_communicator_and_a_failed_batch_are_refused():
    p, fc = tlo.problem("medium")
    s = capi.Solver(p["network"], p["tree"], p["config"], rank=0, nranks=2)
    s.initialiseSmpcController(*fc)
    out = np.zeros(4)
    args = (40, 0.0, 0, None, None, 0, out.ctypes.data, None)
    assert s.lib.rn_estimate_lipschitz(s.h, *args) == RN_E_STATE and "communicator" in s.lib.rn_last_error(s.h).decode()
    s.debugSetAllreduce(lambda *a: 0)
    s.apgReset(); s.apgIterate(2)
    assert s.lib.rn_estimate_lipschitz(s.h, *args) == 0
    s.debugSetAllreduce(lambda *a: 7)
    with pytest.raises(capi.RapidNetError):
        s.apgIterate(2)
    s.debugSetAllreduce(lambda *a: 0)
    assert s.lib.rn_estimate_lipschitz(s.h, *args) == RN_E_STATE and "half-way" in s.lib.rn_last_error(s.h).decode()
    s.apgReset()
    assert s.lib.rn_estimate_lipschitz(s.h, *args) == 0
    s.close()


# ---- 8. fp32 contexts ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_fp32_contexts_against_the_rounded_restatement(name, mode):
    p, fc = tlo.problem(name)
    M, lam, apply = tlo.dense(name)
    s = make(p, p["tree"], mode, "f32")
    s.factorStep()
    xi64, psi64 = start_of(s)
    exact = lo.power_loop(apply, xi64, psi64, 40)[-1, lo.NORM]
    xi, psi = lo.hash_start(s.nodes, s.nx, s.nu, 0, dtype=np.float32)
    e_cpu = abs(lo.power_loop(apply, xi, psi, 40, round_to=np.float32)[-1, lo.NORM] - exact) / exact
    r = s.estimateLipschitz(40, history=True)
    r2 = s.estimateLipschitz(40, history=True)
    assert np.array_equal(bits(r["history"]), bits(r2["history"]))
    err = abs(r["norm"] - exact) / exact
    bound = 4 * e_cpu + 32 * 2.0 ** -24
    record("fp32    %-6s %-10s NORM against the fp64 restatement: %.3e, e_cpu %.3e, bound %.3e, ratio %.3f" % (name, mode, err, e_cpu, bound, err / bound))
    assert err <= bound
    # |t| <= |v| |w|, and the fp32 v is a unit vector only up to its two roundings per element (the reciprocal, the product): |v| <= (1 + 2^-24)^2
    assert r["rayleigh"] <= r["norm"] * (1 + 3 * 2.0 ** -24)
    s.close()


# ---- 9. the step rule ------------------------------------------------------------------------------------------------------------------------------------
def test_step_rule_is_bitwise_set_parameters_with_margin_over_norm():
    name = "small"
    p, fc = tlo.problem(name)
    cfg = dict(p["config"], stepSize=[1e-4])                                # a deliberately wrong configured step size
    px, pxs = float(cfg["penaltyStateX"][0]), float(cfg["penaltySafetyX"][0])
    n = 30
    a = capi.Solver(p["network"], p["tree"], cfg, operator_mode="dense")
    a.initialiseSmpcController(*fc)
    assert a.stepRule() == dict(rule="fixed", margin=0.9, iterations=40, step_size_in_force=1e-4)
    off = a.controlAction(*fc, maxIterations=n)
    base = capi.Solver(p["network"], p["tree"], cfg, operator_mode="dense")
    base.initialiseSmpcController(*fc)
    assert np.array_equal(bits(off), bits(base.controlAction(*fc, maxIterations=n)))      # the rule off: today's bits
    assert a.lib.rn_get_lipschitz(a.h, np.zeros(4).ctypes.data, None) == RN_E_STATE        # ... and nothing was estimated
    a.setStepRule("lipschitz", 0.95, 40)
    u = a.controlAction(*fc, maxIterations=n)
    L = a.lipschitz()
    assert not L["stale"] and L["iterations"] == 40
    step = 0.95 / L["norm"]
    assert a.stepRule()["step_size_in_force"] == step and abs(step * tlo.dense(name)[1] - 0.95) < 1e-3
    b = capi.Solver(p["network"], p["tree"], cfg, operator_mode="dense")
    b.initialiseSmpcController(*fc)
    b._check(b.lib.rn_set_parameters(b.h, step, px, pxs))
    ub = b.controlAction(*fc, maxIterations=n)
    assert np.array_equal(bits(u), bits(ub))
    for bid in APG_BUFS:
        assert np.array_equal(bits(a.get(bid)), bits(b.get(bid))), bid
    # the CPU oracle at that step size, stage by stage
    from stagewise import stage_relmax
    o = Oracle(p["network"], p["tree"], dict(cfg, stepSize=[step]))
    o.initialise(*fc)
    o.control_action(*fc, max_iterations=n, project=False)
    for bid, nm, dim in ((capi.BUF_X, "x", a.nx), (capi.BUF_U, "u", a.nu), (capi.BUF_UPD_XI, "updXi", 2 * a.nx), (capi.BUF_UPD_PSI, "updPsi", a.nu)):
        e = float(np.max(stage_relmax(a.get(bid), o.get(nm), p["tree"], dim)))
        record("rule    small %-7s against the CPU oracle at 0.95 / NORM, worst stage: %.2e" % (nm, e))
        assert e <= REL, (nm, e)
    # new probabilities: the next control action re-estimates
    new = reweighted(p["tree"], fc, 3)
    a.setTreeData(prob=new["probNode"])
    assert a.lipschitz()["stale"]
    a.controlAction(*fc, maxIterations=n)
    L2 = a.lipschitz()
    assert not L2["stale"] and L2["norm"] != L["norm"] and a.stepRule()["step_size_in_force"] == 0.95 / L2["norm"]
    # back to the fixed rule: rn_set_parameters' own figure returns
    a.setStepRule("fixed")
    assert a.stepRule()["step_size_in_force"] == 1e-4
    # the other solves take the rule too
    a.setStepRule("lipschitz", 0.5, 10)
    a.updateStateControl(); a.eliminateInputDistubanceCoupling(*fc)
    a.apg_solve(10)
    assert a.stepRule()["step_size_in_force"] == 0.5 / a.lipschitz()["norm"] and a.lipschitz()["iterations"] == 40      # held and fresh: not re-estimated
    # ... and the constructor's form is the call
    c = capi.Solver(p["network"], p["tree"], cfg, operator_mode="dense", step_rule=("lipschitz", 0.95, 40))
    c.initialiseSmpcController(*fc)
    assert c.stepRule() == dict(rule="lipschitz", margin=0.95, iterations=40, step_size_in_force=1e-4)      # nothing estimated yet
    assert np.array_equal(bits(c.controlAction(*fc, maxIterations=n)), bits(u)) and c.stepRule()["step_size_in_force"] == step
    for s in (a, b, base, c):
        s.close()


# ---- 10. errors ---------------------------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_state():
    p, fc = tlo.problem("small")
    s = make(p, p["tree"], "dense", "f64")
    lib = s.lib
    out, hist = np.zeros(4), np.zeros((40, 3))
    xi, psi = np.ones(s.nodes * 2 * s.nx), np.ones(s.nodes * s.nu)
    o, x, ps = out.ctypes.data, xi.ctypes.data, psi.ctypes.data
    assert lib.rn_estimate_lipschitz(s.h, 40, 0.0, 0, None, None, 0, o, None) == RN_E_STATE      # before the factor step
    assert "rn_factor_step" in lib.rn_last_error(s.h).decode()
    assert lib.rn_get_lipschitz(s.h, o, None) == RN_E_STATE
    s.factorStep()
    m0 = s.deviceMemoryInfo()["context_bytes"]
    assert lib.rn_estimate_lipschitz(s.h, 0, 0.0, 0, None, None, 0, o, None) == RN_E_ARG
    assert lib.rn_estimate_lipschitz(s.h, -3, 0.0, 0, None, None, 0, o, None) == RN_E_ARG
    assert lib.rn_estimate_lipschitz(s.h, 40, -1e-3, 0, None, None, 0, o, None) == RN_E_ARG
    assert lib.rn_estimate_lipschitz(s.h, 40, float("nan"), 0, None, None, 0, o, None) == RN_E_ARG
    assert lib.rn_estimate_lipschitz(s.h, 40, 0.0, 0, x, None, 0, o, None) == RN_E_ARG
    assert lib.rn_estimate_lipschitz(s.h, 40, 0.0, 0, None, ps, 0, o, None) == RN_E_ARG
    assert lib.rn_estimate_lipschitz(s.h, 40, 0.0, 0, None, None, 0, None, None) == RN_E_ARG
    assert lib.rn_estimate_lipschitz(None, 40, 0.0, 0, None, None, 0, o, None) == RN_E_ARG
    assert s.deviceMemoryInfo()["context_bytes"] == m0                      # none of the refused calls allocated anything
    assert lib.rn_get_lipschitz(s.h, o, None) == RN_E_STATE
    for bad in (0.0, float("nan"), float("inf")):                            # a start whose norm is 0 or not finite: seen in the first record
        xi[:] = bad; psi[:] = bad
        assert lib.rn_estimate_lipschitz(s.h, 5, 0.0, 0, x, ps, 0, o, None) == RN_E_ARG and "start" in lib.rn_last_error(s.h).decode()
        assert lib.rn_estimate_lipschitz(s.h, 20, 1e-3, 5, x, ps, 0, o, None) == RN_E_ARG
        assert lib.rn_get_lipschitz(s.h, o, None) == RN_E_STATE             # a refused start leaves no record
    xi[:] = 1.0; psi[:] = 1.0
    assert lib.rn_estimate_lipschitz(s.h, 5, 0.0, 0, x, ps, 0, o, hist.ctypes.data) == 0 and out[3] == 5 and (hist[5:] == 0).all()
    assert lib.rn_get_lipschitz(s.h, None, None) == RN_E_ARG
    st = capi.C.c_int(-1)
    assert lib.rn_get_lipschitz(s.h, o, capi.C.byref(st)) == 0 and st.value == 0
    for rule, margin in ((2, 0.9), (-1, 0.9), (1, 0.0), (1, -0.5), (1, 1.5), (1, float("nan"))):
        assert lib.rn_set_step_rule(s.h, rule, margin, 0) == RN_E_ARG
    assert lib.rn_set_step_rule(s.h, 1, 1.0, 0) == 0 and s.stepRule()["iterations"] == 40
    assert lib.rn_set_step_rule(None, 1, 1.0, 0) == RN_E_ARG
    s.close()


# ---- 11. guard mode ---------------------------------------------------------------------------------------------------------------------------------------
def test_under_the_buffer_guard(monkeypatch):
    """RAPIDNET_GUARD=1 (read when a context is created): every buffer between red zones and NaN until written.  A read outside v or w, or of an
    element nobody wrote, would bring a NaN into the records (held to the restatement); a write outside a buffer changes a red zone."""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    for name, mode, kind in (("odd", "dense", "f64"), ("ragged", "structured", "f32"), ("toy", "auto", "f64")):
        p, fc = tlo.problem(name)
        M, lam, apply = tlo.dense(name)
        s = make(p, p["tree"], mode, kind)
        s.factorStep()
        r = s.estimateLipschitz(7, history=True)
        xi, psi = start_of(s)
        want = lo.power_loop(apply, xi, psi, 7)
        assert np.isfinite(r["history"]).all()
        assert np.max(np.abs(r["history"][:, 0] - want[:, 0]) / want[:, 0]) <= (REL if kind == "f64" else 1e-4)
        assert s.guardCheck() == 0
        s.close()
    gc.collect()
    after = capi.guard_report()
    assert after[0] - before[0] == 3 and after[1] == before[1]      # the three contexts were checked once more when they went away: 0 bytes
