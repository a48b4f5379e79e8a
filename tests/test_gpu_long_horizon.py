"""Horizons beyond 24 stages against the fp64 oracle, stage by stage.

The chain kernels of csrc/k_walks.hpp walk a chain in batches of prefetched stages (UP_PF = 24, LIN_PF = CHAIN_PF = 12) and the longest
chain of any other test is 23 stages long: every "next batch" path past the first (UP_PF) or the second (the others) runs here only.  The
shapes -- chains of L = 24, 25, 36, 37, 48, 49 stages, a full last batch and one stage past it, and the Barcelona network on either side
of the 64 KB of LDS the fused walk + dual update may take -- and every reference are those of tests/test_long_horizon_shapes.py, which
guards them without a GPU; the chain length of every context is asserted from kernelInfo(), not assumed.

Measure: stagewise.worst_by_buffer -- per stage, against that stage's own magnitude -- at the project's tolerances: REL_TOL = 1e-9 in fp64,
e_gpu <= 4 e_cpu + 32 * 2^-24 against the fp32 oracle's own error in fp32 (test_gpu_apg_f32.py), bit for bit between knob pairs.

 1. one step from non-trivial duals (random xi, psi, updXi, updPsi of scale 50): every shape, dense and structured; every form of the
    structured up walk (struct_linear 0, 2, 3, 4, 5) at L = 25 and 37; fp32-stored blocks on a medium shape
 2. short APG runs in batches of (20, 17, 3) -- two optimistic batches, which take the fused launch where the shape allows it, with the
    chain walk riding in it in structured mode, and an exact tail: every shape; fused on / off and fuse_split 1, 2, 3, 4, L bit for bit;
    unscaled_walk 0 against the default bit for bit
 3. the split last round of the streaming kernel above a chain of 26 stages or more (k_up_chain<SPLIT> adds the second partial in its
    first batch only), on a tree built from the device's CU count
 4. shards in one process: cut right above the chains (k_up_chain_cut, 3 and 4 batches) on 2 and 3 ranks, and one stage higher
 5. fp32 contexts: one exact iteration and one optimistic batch from the fp64 loop's fp32-rounded states
 6. global FBE and NAMA on the medium L = 37 shape
 7. what rides on the iterates at L = 49: plan report, plan bands, shifted warm start, a two-step control loop -- each held as its own
    test file holds it

When LONG_HORIZON_ERRORS names a file, every case appends its worst per-stage error and the stage it is in:
profiles/long_horizon_errors.txt is such a file."""
import os

import numpy as np
import pytest

import horizon_oracle as ho
import test_gpu_apg_f32 as apg32
import test_gpu_fbe_nama as fbe
import test_gpu_fused_walk_dual as fwd
import test_gpu_plan_bands as bands
import test_gpu_plan_report as report
import test_gpu_receding_horizon as rh
import test_gpu_shift_warm_start as shift
import test_gpu_stream_split as spl
import test_long_horizon_shapes as lh
from rapidnet_amd import capi, synth
from test_gpu_operator_storage import blocks_of, oracle_with_blocks
from test_gpu_parity import PAIRS
from test_gpu_sharded_batched import Ranks

pytestmark = pytest.mark.gpu

REL_TOL = lh.REL_TOL
BID = {nm: bid for bid, nm in PAIRS}
MODES = ("dense", "structured")
DUAL_BIDS = (capi.BUF_XI, capi.BUF_PSI, capi.BUF_UPD_XI, capi.BUF_UPD_PSI)
SEAM_SMALL = ("s22_25", "s3_25", "s22_37", "s3_37")      # one stage past a full batch of UP_PF, and of three batches of LIN_PF / CHAIN_PF


def record(line):
    print(line)
    path = os.environ.get("LONG_HORIZON_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def context(name, mode="dense", precision="f64", **kw):
    """an initialised context of a long shape whose chain length is the one the shape is named for"""
    p, fc = lh.problem(name)
    s = capi.Solver(p["network"], p["tree"], p["config"], precision=precision, operator_mode=mode, **kw)
    s.initialiseSmpcController(*fc)
    assert s.N - s.kernelInfo()["chain_stage"] == lh.SHAPES[name][1], (name, s.N, s.kernelInfo())
    assert s.operatorMode()[1] == mode
    return s


def check(what, got, ref, p, tol=REL_TOL, hist=None, ohist=None):
    """every buffer of `got` per stage against `ref`; records the worst buffer, its error and the stage it is in, then asserts"""
    nx, nu, nv = lh.dims(p)
    e = lh.stage_errors(got, ref, p["tree"], nx, nu, nv)
    nm = max(e, key=lambda k: e[k][0])
    line = "%-66s worst per-stage error %.2e  %-9s stage %2d" % (what, e[nm][0], nm, e[nm][1])
    herr = None
    if hist is not None:
        assert hist.shape == ohist.shape and np.isfinite(hist).all()
        herr = float(np.abs(hist - ohist).max() / np.abs(ohist).max())
        line += "  history %.2e" % herr
    record(line)
    bad = {k: v for k, v in e.items() if not v[0] <= tol}
    assert not bad, (what, bad)
    assert herr is None or herr <= tol, (what, herr)


def one_step(s, lam=0.618):
    for bid, v in zip(DUAL_BIDS, lh.duals(s.nodes, s.nx, s.nu)):
        s.set(bid, v)
    s.dualExtrapolationStep(lam); s.solveStep(); s.proximalFunG(); s.computeFixedPointResidual(); s.dualUpdate()


# ---------------------------------------------------------------------------------------------------------------
# 1. one step from non-trivial duals
# ---------------------------------------------------------------------------------------------------------------
def step_case(name, mode, what, ref=None, **kw):
    p, _ = lh.problem(name)
    ref = lh.step_reference(name) if ref is None else ref
    s = context(name, mode, **kw)
    try:
        one_step(s)
        check("step %s %s" % (name, what), {nm: s.get(BID[nm]) for nm in lh.compared(name)}, ref, p)
        inf = s.updatePrimalInfeasibity()
        assert abs(inf - ref["infeasibility"]) <= REL_TOL * abs(ref["infeasibility"]), (inf, ref["infeasibility"])
        assert s.guardCheck() == 0
    finally:
        s.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(lh.SHAPES))
def test_one_step_from_non_trivial_duals(name, mode):
    step_case(name, mode, mode)


@pytest.mark.parametrize("linear", [0, 2, 3, 4, 5])
@pytest.mark.parametrize("name", SEAM_SMALL)
def test_one_step_in_every_form_of_the_structured_up_walk(name, linear):
    """struct_linear 0: k_gemm_prep_m2 + k_up_chain; 2 ... 5: the linear form without the riding walk, without the constant operand, with the
    two products kept apart, with the composite operator but the affine terms in the walk (the default, 1, is the case above)"""
    step_case(name, "structured", "structured struct_linear=%d" % linear, knobs={"struct_linear": linear})


def test_one_step_over_fp32_stored_blocks():
    """fp64 iterates over fp32-stored blocks: the oracle holds the context's own blocks"""
    name = "m42_37"
    p, fc = lh.problem(name)
    probe = context(name, "dense", operator_storage="f32")
    assert probe.operatorStorage()[1] == "f32"
    o = oracle_with_blocks(p, fc, blocks_of(probe))
    probe.close()
    lh.one_step(o)
    ref = {nm: o.get(nm) for nm in lh.NAMES}
    ref["infeasibility"] = o.primal_infeasibility()
    step_case(name, "dense", "dense, fp32-stored blocks", ref=ref, operator_storage="f32")


# ---------------------------------------------------------------------------------------------------------------
# 2. short APG runs
# ---------------------------------------------------------------------------------------------------------------
def batches(s):
    s.apgReset()
    return np.concatenate([s.apgIterate(n) for n in lh.BATCHES])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(lh.SHAPES))
def test_short_apg_run(name, mode):
    p, _ = lh.problem(name)
    ref, ohist = lh.apg_reference(name)
    s = context(name, mode)
    try:
        hist = batches(s)
        c = s.counters()
        assert c == {"optimistic": 2, "exact": 1, "replayed": 0, "hold": 0}, c
        check("apg  %s %s, %d iterations" % (name, mode, lh.ITERS), {nm: s.get(BID[nm]) for nm in lh.NAMES}, ref, p, hist=hist, ohist=ohist)
        assert s.guardCheck() == 0
    finally:
        s.close()


# (shape, structured): the small shapes one stage past a seam and at the longest chain, the medium shapes, Barcelona on both sides of the
# fused launch's LDS limit.  s3_* (ny = 19) cannot fuse -- the flat dual update -- and pins the fall-back; structured mode carries the
# next sweep's chain walk in the fused launch (fuse_split = 1 only)
FUSE_CASES = [("s22_25", False), ("s3_25", True), ("s22_37", True), ("s3_37", False), ("s22_49", False), ("s22_49", True), ("s3_49", True),
              ("m42_36", False), ("m42_37", True), ("m5_25", True), ("b5_33", False), ("b5_33", True), ("b5_34", False), ("b5_34", True)]


@pytest.mark.parametrize("name,structured", FUSE_CASES)
def test_fused_launch_forms_are_bitwise_the_two_launches(monkeypatch, name, structured):
    p, _ = lh.problem(name)
    L = lh.SHAPES[name][1]
    probe = context(name, MODES[structured])
    k, ny, N = probe.kernelInfo(), probe.ny, probe.N
    probe.close()
    if name.startswith("s3_"):
        assert k["dual_stage"] == 0 and ny % 2 == 1, k
    else:
        assert k["dual_stage"] == 1 and k["dual_pipe"] != 0 and 1 <= k["chain_stage"] <= 8 and ny % 2 == 0, k
    if name in lh.BARCELONA:      # the fused launch's tile: N ny sizeof(double) against 64 KB
        assert (N * ny * 8 <= 64 * 1024) == (name == "b5_33"), (N, ny)
    monkeypatch.setenv("RAPIDNET_FUSE_DOWN_DUAL", "0")
    h0, o0, c0 = fwd.run(p, structured, "f64", lh.BATCHES)
    assert c0 == {"optimistic": 2, "exact": 1, "replayed": 0, "hold": 0}, c0
    monkeypatch.setenv("RAPIDNET_FUSE_DOWN_DUAL", "1")
    for split in (1, 2, 3, 4, L, None):
        h1, o1, c1 = fwd.run(p, structured, "f64", lh.BATCHES, knobs=None if split is None else {"fuse_split": split})
        assert c0 == c1, (split, c0, c1)
        assert np.array_equal(h0, h1), split
        for b in fwd.BUFS:
            assert np.array_equal(o0[b], o1[b]), (split, b)


@pytest.mark.parametrize("structured", [False, True])
def test_unscaled_walk_is_bitwise_the_scaled_one(monkeypatch, structured):
    """k_down_chain<UNSC> + k_dual_stage<SCALE> against the walk that applies the preconditioner itself (the fused launch off: it would
    replace both)"""
    p, _ = lh.problem("m42_37")
    monkeypatch.setenv("RAPIDNET_FUSE_DOWN_DUAL", "0")
    h0, o0, c0 = fwd.run(p, structured, "f64", lh.BATCHES, knobs={"unscaled_walk": 0})
    h1, o1, c1 = fwd.run(p, structured, "f64", lh.BATCHES)
    assert c0 == c1 == {"optimistic": 2, "exact": 1, "replayed": 0, "hold": 0}, (c0, c1)
    assert np.array_equal(h0, h1)
    for b in fwd.BUFS:
        assert np.array_equal(o0[b], o1[b]), b


# ---------------------------------------------------------------------------------------------------------------
# 3. the split last round above a long chain
# ---------------------------------------------------------------------------------------------------------------
def long_split_tree(cus, most=301):
    """(r, K, N) of a tree of test_gpu_stream_split.split_tree's family (cus + r nodes) whose chains are at least 26 stages long (N >= 28)
    and whose split round reaches the third stage from the end (2K < r <= 3K, 2r <= cus): the shortest such horizon -- the second batch of
    UP_PF stages is then two stages long -- and of those the smallest tree, within `most` nodes where the CU count allows it (256 CUs:
    r = 33, K = 11, N = 28: 289 nodes).  Two crown nodes at least: behind a single-child root stage the step size that synth estimates
    undershoots on a long horizon (tests/test_long_horizon_shapes.py)"""
    found = [(1 + a + K * (N - 2) - cus, K, N) for N in range(28, 80) for K in range(2, cus) for a in range(2, K + 1)
             if 2 * K < 1 + a + K * (N - 2) - cus <= 3 * K and 2 * (1 + a + K * (N - 2) - cus) <= cus]
    assert found, cus
    within = [c for c in found if cus + c[0] <= most] or found
    return min(within, key=lambda c: (c[2], c[0]))


def test_split_last_round_above_a_long_chain():
    """k_up_chain<SPLIT>: the second partial m2 of the last three stages is added in the FIRST batch of UP_PF stages and never again -- one
    step from non-trivial duals (m2 is then far from zero), then a short APG run"""
    cus = spl.num_cus()
    r, K, N = long_split_tree(cus)
    branching, N = spl.split_tree(cus, r, K, N)
    p, fc = spl.problem("b240", "long", branching, N)
    s = spl.solver(p, fc)
    try:
        spl.expect_split(s, r, "long chain")
        assert s.N - s.kernelInfo()["chain_stage"] >= lh.UP_PF + 2, (s.N, s.kernelInfo())
        o = spl.oracle_of(p, fc)
        lh.one_step(o)
        one_step(s)
        ref = {nm: o.get(nm) for nm in lh.NAMES}
        check("split last round, L = %d, one step" % (N - 2), {nm: s.get(BID[nm]) for nm in lh.NAMES}, ref, p)
        ref, ohist = spl.reference(("b240", "long"), p, fc)
        assert np.isfinite(ohist).all() and np.abs(ohist).max() <= 10 * abs(ohist[0]), ohist      # (the tree is built here: the CPU file's guard)
        hist = s.algorithmApg(spl.ITERS)
        spl.compare("split last round, L = %d" % (N - 2), spl.local_get(s), s, p["tree"], ref, REL_TOL, hist, ohist)
        check("split last round, L = %d, %d iterations" % (N - 2, spl.ITERS), {nm: s.get(bid) for nm, bid, _ in spl.VECS}, ref, p, hist=hist, ohist=ohist)
        spl.expect_split(s, r)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. shards in one process
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", ["optimistic", "exact"])
@pytest.mark.parametrize("name,world,cut,structured", [("s3_25", 2, 1, False), ("s3_25", 3, 1, True), ("s3_37", 2, 1, True), ("s3_37", 3, 1, False),
                                                        ("s22_25", 2, 1, False), ("s22_37", 2, 2, True)])
def test_shards_match_the_oracle(name, world, cut, structured, exchange):
    """cut == chain stage: the chain walks and the cut parents' sums are one launch (k_up_chain_cut, batches of CHAIN_PF stages);
    s22_25 is cut one stage higher (k_up_chain on every shard, crown stage 1 behind the exchange)"""
    p, fc = lh.problem(name)
    ref, ohist = lh.apg_reference(name)
    L = lh.SHAPES[name][1]
    rk = Ranks(p, world, cut, structured, optimistic=exchange == "optimistic")
    try:
        def solve(s):
            s.initialiseSmpcController(*fc)
            return batches(s), s.counters()

        res = rk.run(solve)
        for s in rk.shards:
            # (a shard with ONE chain below the cut is a chain from its root on: its walks start at max(local chain stage, cut stage))
            top = max(s.kernelInfo()["chain_stage"], s.shardInfo()["cut_stage"])
            assert s.N - top == L and s.shardInfo()["cut_stage"] == cut, (s.kernelInfo(), s.shardInfo())
            assert (cut == top) == (name != "s22_25")
        for hist, c in res:
            assert c == res[0][1] and c["replayed"] == 0, (c, res[0][1])
            assert np.array_equal(hist, res[0][0])
        d = {"x": rk.shards[0].nx, "u": rk.shards[0].nu, "v": rk.shards[0].nv}
        dim = lambda nm: d.get(nm, rk.shards[0].nu if nm.endswith("Psi") or nm == "psi" else 2 * rk.shards[0].nx)
        got = {nm: rk.gathered(BID[nm], dim(nm)) for nm in lh.NAMES}
        check("shards %s %d ranks cut %d %s %s" % (name, world, cut, MODES[structured], exchange), got, ref, p, hist=res[0][0], ohist=ohist)
        u0 = [s.get(capi.BUF_U)[: s.nu] for s in rk.shards]          # the root control: the same bits on every rank
        for u in u0[1:]:
            assert np.array_equal(u, u0[0])
    finally:
        rk.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. fp32 contexts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", lh.F32_SHAPES)
def test_f32_iteration_and_batch(name, mode):
    """forms B (one exact iteration) and C (one optimistic batch of 16) of test_gpu_apg_f32.py from the fp64 loop's fp32-rounded states"""
    case = lh.f32_case(name)
    s = apg32.make_solver(case, operator_mode=mode)
    led = apg32.Ledger("%s %s" % (name, mode))
    try:
        assert s.N - s.kernelInfo()["chain_stage"] == lh.SHAPES[name][1]
        assert s.kernelInfo()["dual_stage"] == (1 if s.ny % 4 == 0 else 0)      # m42_37: the stage-tiled dual update and the fused launch; s3_49: flat
        apg32.run_case(case, s, led, forms=("B", "C"))
    finally:
        s.close()
    form, step, k = max(led.rows, key=lambda key: led.rows[key][3])
    e_gpu, e_cpu, it, share = led.rows[(form, step, k)]
    record("f32  %-61s worst share of 4 e_cpu + 32 * 2^-24: %.3f  (form %s %s state %d: e_gpu %.2e, e_cpu %.2e)" % ("%s %s" % (name, mode), share, form, k, it, e_gpu, e_cpu))
    led.finish()


# ---------------------------------------------------------------------------------------------------------------
# 6. global FBE and NAMA
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", fbe.ALGS)
@pytest.mark.parametrize("structured", [False, True])
def test_quasi_newton_loops(structured, alg):
    """12 iterations as test_gpu_fbe_nama.test_loop_matches_oracle holds them: the oracle's step lengths exactly, values at 1e-9, every
    buffer of the loops at 1e-8, the line searches in batches"""
    with lh.registered("m42_37"):
        fbe.test_loop_matches_oracle("m42_37", structured, alg)
    record("fbe  %-61s held as tests/test_gpu_fbe_nama.py holds its loops" % ("m42_37 %s %s, 12 iterations" % (MODES[structured], alg)))


# ---------------------------------------------------------------------------------------------------------------
# 7. what rides on the iterates, at L = 49
# ---------------------------------------------------------------------------------------------------------------
RIDES = "s22_49"


def into_the_table(monkeypatch, var):
    """the lines the body's own file records (under its own variable) go to the table of this file"""
    if os.environ.get("LONG_HORIZON_ERRORS"):
        monkeypatch.setenv(var, os.environ["LONG_HORIZON_ERRORS"])


@pytest.mark.parametrize("mode,iters", [("dense", 5), ("structured", 40)])
def test_plan_report(monkeypatch, mode, iters):
    into_the_table(monkeypatch, "PLAN_REPORT_ERRORS")
    with lh.registered(RIDES):
        report.test_tables_after_a_cold_solve(RIDES, mode, "f64", iters, "stage")


def test_plan_bands(monkeypatch):
    into_the_table(monkeypatch, "PLAN_BANDS_ERRORS")
    with lh.registered(RIDES):
        bands.test_bands_after_a_cold_solve(RIDES)


@pytest.mark.parametrize("mode", MODES)
def test_shift_warm_start(monkeypatch, mode):
    into_the_table(monkeypatch, "SHIFT_WARM_START_ERRORS")
    with lh.registered(RIDES):
        shift.test_one_shift_is_the_restatements(RIDES, mode, "f64")


@pytest.mark.parametrize("mode", MODES)
def test_two_step_control_loop(mode):
    """two warm rn_control_action calls (23 and 16 iterations) against tests/horizon_oracle.py, every buffer per stage"""
    p, _ = lh.problem(RIDES)          # (forecasts of time 0 and 1: synth's default simulation horizon)
    recs = ho.run_horizon(rh.oracle_of(p), ho.steps_of(p["forecast"], synth.forecast_at, ho.COUNTS[:2]), True)
    s = rh.solver(p, mode, True)
    try:
        assert s.N - s.kernelInfo()["chain_stage"] == lh.SHAPES[RIDES][1]
        worst = max(rh.assert_step(rh.step_of(s, rec), rec, p, "%s %s warm" % (RIDES, mode)) for rec in recs)
        assert s.guardCheck() == 0
    finally:
        s.close()
    record("loop %-61s worst error of either step %.2e" % ("%s %s, 23 + 16 iterations, warm" % (RIDES, mode), worst))


# ---------------------------------------------------------------------------------------------------------------
# guard mode's body (tests/test_gpu_guard.py)
# ---------------------------------------------------------------------------------------------------------------
def guard_body(name="m42_37"):
    """the step and the batches on the medium L = 37 shape (four batches of CHAIN_PF stages, the fused launch and its riding walk), dense
    and structured; returns the number of contexts"""
    for mode in MODES:
        step_case(name, mode, mode + " (guard)")
        test_short_apg_run(name, mode)
    return 4
