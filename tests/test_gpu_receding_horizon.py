"""Sequences of control steps on ONE context against the CPU oracle: every operator form, cold and warm, one GPU and shards.

A model-predictive controller calls rn_control_action step after step on one context; with rn_set_warm_start the duals of the previous
step are carried over.  What a step inherits -- which of the two rotating dual buffers holds y+, whether the accelerated dual is current,
the iteration counters, the checkpoints and the hold of the optimistic path, the constants the structured form derives from the affine
terms -- shows only from the second step on and depends on how the previous step ended.  tests/horizon_oracle.py runs the loop on the
oracle around the oracle's own plant; the context under test is handed the oracle's (x_t, u_{t-1}, d_{t-1}) at every step, so both sides
solve the same problem at every step and a step's error is that step's own.

Iteration counts per step: horizon_oracle.COUNTS = (23, 16, 37, 5, 1) -- an odd count above one batch of 16, exactly one batch, two
batches plus an odd tail, less than a batch, one iteration; the plant mode alternates 0 / 1.

Checked at EVERY step, fp64: the root control (before and after the projection) at 1e-9, every buffer of test_gpu_parity.PAIRS per stage
(stagewise.worst_by_buffer) at 1e-9, the step's primal-infeasibility history at 1e-9 of its maximum.  rn_control_action returns no history:
it is read back through rn_get_history_parts (the larger of the two signed entries, as the library's write_history forms it); on shards
the parts are rank-local and the tree-global history is the entry at the arg-max over the ranks.

Values chosen on the CPU oracle (test_oracle_side_choices checks them without a GPU):
  * soft penalties of `medium`: penalty_x = 32, penalty_xs = 2.5.  lambda x the largest prox distances of the first three steps are, cold,
    (27.2, 1.94), (19.4, 1.52), (36.5, 1.37) and, warm, (27.2, 1.94), (27.0, 0.92), (40.5, 1.81): no threshold trips in steps 0 and 1,
    the state threshold trips in step 2 (37 iterations: one optimistic batch, replayed), cold and warm.
  * stop tolerance on `ragged`, warm: tol = 300 on the signed residual, batches of 10, at most 40 iterations per step: the steps stop
    behind 20, 30, 40, 40 and 40 iterations (residuals at the batch ends: 689, -468 | 425, 345, 257 | 868 ... 576 | ...).
  * fp32, section 5: e_cpu of the batch is 1e-7 ... 1e-5 on every buffer (never 0 on all of them), see profiles/receding_horizon_errors.txt.
"""
import gc

import numpy as np
import pytest

import horizon_oracle as ho
from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from test_gpu_parity import PAIRS

gpu = pytest.mark.gpu

TOL = 1e-9
T = len(ho.COUNTS)
SOFT = {"penalty_x": 32.0, "penalty_xs": 2.5}
STOP = dict(name="ragged", tol=300.0, every=10, most=40)
BID = {nm: bid for bid, nm in PAIRS}
AFFINE_BID = {"uhat": capi.BUF_UHAT, "e": capi.BUF_E, "beta": capi.BUF_BETA, "alpha": capi.BUF_ALPHA}
DUAL_BIDS = (capi.BUF_XI, capi.BUF_PSI, capi.BUF_UPD_XI, capi.BUF_UPD_PSI)

_PROBLEMS, _RECORDS = {}, {}


def problem(name, soft=False):
    key = (name, soft)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = synth.make_problem(name, sim_horizon=T, **(SOFT if soft else {}))
    return _PROBLEMS[key]


def steps_of(p, counts=ho.COUNTS):
    return ho.steps_of(p["forecast"], synth.forecast_at, counts)


def oracle_of(p, tree=None):
    o = Oracle(p["network"], p["tree"] if tree is None else tree, p["config"])
    o.factor_step()
    return o


def records(name, warm, soft=False, **kw):
    """the oracle's loop of a problem, computed once and left unchanged (run_horizon makes every array read-only)"""
    key = (name, warm, soft, tuple(sorted(kw.items())))
    if key not in _RECORDS:
        p = problem(name, soft)
        counts = kw.pop("counts", ho.COUNTS)
        _RECORDS[key] = ho.run_horizon(oracle_of(p), steps_of(p, counts), warm, **kw)
    return _RECORDS[key]


# ---------------------------------------------------------------------------------------------------------------
# the context's side of one step
# ---------------------------------------------------------------------------------------------------------------
def history_of(s, n):
    """vecPrimalInfs of the last n iterations' step from rn_get_history_parts (one GPU)"""
    parts = s.historyParts(0, n)
    return np.where(parts[:, 1] > parts[:, 3], parts[:, 1], parts[:, 3])


def control_step(s, rec, most=None):
    """rn_control_action with the oracle's (x_t, u_{t-1}, d_{t-1}); the projected control is the call's result, the unprojected one the
    root's rows of BUF_U"""
    return s.controlAction(rec["dh"], rec["ah"], currentX=rec["x"], prevU=rec["prevU"], prevDemand=rec["prevD"],
                           maxIterations=rec["n"] if most is None else most, project=True)


def step_of(s, rec, most=None):
    u = control_step(s, rec, most)
    n = s.last_solve()["iterations"]
    assert n == rec["n"], ("iterations", rec["t"], n, rec["n"])
    return dict(u=u, u_raw=s.get(capi.BUF_U)[: s.nu], hist=history_of(s, n), bufs={nm: s.get(bid) for bid, nm in PAIRS})


def assert_step(got, rec, p, what):
    nx, nu, nv = int(p["network"]["nx"][0]), int(p["network"]["nu"][0]), int(p["config"]["nv"][0])
    e = ho.step_errors(got, rec, p["tree"], nx, nu, nv)
    bad = {k: v for k, v in e.items() if not v <= TOL}
    assert not bad, "%s, step %d (%d iterations): %s" % (what, rec["t"], rec["n"], bad)
    return max(e.values())


def solver(p, mode, warm, tree=None, **kw):
    s = capi.Solver(p["network"], p["tree"] if tree is None else tree, p["config"], operator_mode=mode, **kw)
    s.factorStep()
    s.setWarmStart(warm)
    return s


# ---------------------------------------------------------------------------------------------------------------
# 1. the helper, without a GPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "medium", "ragged"])
def test_cold_loop_is_the_oracles_own_control_actions(name):
    """T independent Oracle.control_action calls around move_forward (test_gpu_closed_loop._oracle_loop), bit for bit"""
    p = problem(name)
    recs = records(name, False)
    o = oracle_of(p)
    o.update_state_control()
    for rec, (dh, ah, n) in zip(recs, steps_of(p)):
        x, u, d = (o.get(k) for k in ("curX", "prevU", "prevD"))
        assert np.array_equal(x, rec["x"]) and np.array_equal(u, rec["prevU"]) and np.array_equal(d, rec["prevD"])
        up = o.control_action(dh, ah, max_iterations=n, project=True)
        assert np.array_equal(up, rec["u"]) and np.array_equal(o.get("u")[: o.nu], rec["u_raw"])
        for nm in ho.NAMES:
            assert np.array_equal(o.get(nm), rec["bufs"][nm]), (rec["t"], nm)
        o.move_forward(dh, ah, weight_economical=1.0, plant_mode=rec["plant_mode"])
    assert [r["n"] for r in recs] == list(ho.COUNTS) and [r["plant_mode"] for r in recs] == [0, 1, 0, 1, 0]


@pytest.mark.parametrize("name", ["small", "medium", "ragged"])
def test_warm_loops_second_step_is_the_two_step_recipe(name):
    """test_warm_start_against_the_oracle_started_from_the_same_duals, bit for bit; and the loop moves: duals non-zero at every step, the
    state by more than 1 % between steps of plant mode 0, a warm and a cold run apart by more than 1e-6 from the second step on"""
    p = problem(name)
    warm, cold = records(name, True), records(name, False)
    (dh0, ah0, n0), (dh1, ah1, n1) = steps_of(p)[:2]
    o = oracle_of(p)
    o.update_state_control()
    o.eliminate(dh0, ah0)
    o.apg(n0)
    o.set("xi", o.get("updXi")); o.set("psi", o.get("updPsi"))
    o.update_state_control(warm[1]["x"], warm[1]["prevU"], warm[1]["prevD"])
    o.eliminate(dh1, ah1)
    o.apg_continue(n1, [1.0, 1.0])
    for nm in ho.NAMES:
        assert np.array_equal(o.get(nm), warm[1]["bufs"][nm]), nm
    assert np.array_equal(warm[0]["u_raw"], cold[0]["u_raw"])
    for t in range(1, T):
        assert ho.relmax(warm[t]["u_raw"], cold[t]["u_raw"]) > 1e-6, t
        assert max(ho.relmax(warm[t]["bufs"][nm], cold[t]["bufs"][nm]) for nm in ("x", "updXi", "updPsi")) > 1e-6, t
    for rec in warm:
        assert max(np.abs(rec["bufs"]["updXi"]).max(), np.abs(rec["bufs"]["updPsi"]).max()) > 1e-3, rec["t"]
    assert max(ho.relmax(warm[t]["x"], warm[t - 1]["x"]) for t in range(1, T)) > 0.01


def test_one_iteration_at_a_time_is_the_batch():
    """the loop with a stop tolerance or a distance record runs one iteration at a time: bit for bit the cold and warm loops"""
    for warm in (False, True):
        a, b = records("ragged", warm), records("ragged", warm, track_dist=True)
        for ra, rb in zip(a, b):
            assert np.array_equal(ra["hist"], rb["hist"]) and len(rb["dists"]) == ra["n"]
            for nm in ho.NAMES:
                assert np.array_equal(ra["bufs"][nm], rb["bufs"][nm]), (warm, ra["t"], nm)


def first_trip(recs, p):
    """(step, iteration) of the first iteration whose prox distance exceeds a threshold, or None"""
    lam = p["config"]["stepSize"][0]
    thr = (p["config"]["penaltyStateX"][0] / lam, p["config"]["penaltySafetyX"][0] / lam)
    for rec in recs:
        for k, (dx, ds) in enumerate(rec["dists"]):
            if dx > thr[0] or ds > thr[1]:
                return rec["t"], k
    return None


REPLAYED_IN = {False: 2, True: 2}       # the step whose optimistic batch trips first on the soft-penalty problem, cold / warm


def test_oracle_side_choices():
    """the penalties trip for the first time in a step other than the first, in a step that is one optimistic batch (>= 16 iterations);
    the stop tolerance stops the steps at different batch boundaries"""
    p = problem("medium", True)
    for warm in (False, True):
        trip = first_trip(records("medium", warm, True, track_dist=True), p)
        assert trip is not None and trip[0] == REPLAYED_IN[warm] and ho.COUNTS[trip[0]] >= ho.BATCH, (warm, trip)
    stops = [r["n"] for r in stop_records()]
    print("iterations per step under the stop tolerance:", stops)
    assert stops == STOP_COUNTS and all(n % STOP["every"] == 0 for n in stops) and len(set(stops)) >= 3


STOP_COUNTS = [20, 30, 40, 40, 40]


def stop_records():
    return records(STOP["name"], True, tol=STOP["tol"], every=STOP["every"], counts=(STOP["most"],) * T)


# ---- sharpness: what the suite's former checks of a warm step let through ----------------------------------------------------------------
def former_check(corrupt):
    """the suite's one warm step against the oracle, test_warm_start_against_the_oracle_started_from_the_same_duals (`small`, 30 then 25
    iterations, forecasts 0 and 1, the state moved 3 %), with the corrupted oracle in the library's place: the errors of what it compares"""
    p = synth.make_problem("small")
    steps = [synth.forecast_at(p["forecast"], 0) + (30,), synth.forecast_at(p["forecast"], 1) + (25,)]
    x1 = np.asarray(p["config"]["currentX"], float) * 0.97

    def run(c):
        o = oracle_of(p)
        first = ho.run_horizon(o, steps[:1], True, corrupt=c)[0]
        # the second step from the test's own state: the loop's plant is not part of that test
        o.update_state_control(x1, first["u_raw"])
        if c != "stale_affine":
            o.eliminate(*steps[1][:2])
        if c == "wrong_buffer" and first["n"] % 2 == 1:
            o.set("updXi", o.get("xi")); o.set("updPsi", o.get("psi"))
        ho.keep_duals(o)
        th = [1.0, 1.0]
        if c == "stale_theta":
            probe = oracle_of(p)
            probe.update_state_control(); probe.eliminate(*steps[0][:2])
            _, th = ho.solve(probe, 30)
        o.apg_continue(25, th)
        return dict(u_raw=o.get("u")[: o.nu], bufs={nm: o.get(nm) for nm in ho.NAMES})

    good, bad = run(None), run(corrupt)
    return ho.old_step_errors(bad, good)


@pytest.mark.parametrize("name", ["medium", "ragged"])
@pytest.mark.parametrize("corrupt", ho.CORRUPTIONS)
def test_new_checks_refuse_a_wrong_second_step(corrupt, name):
    """three oracles that are wrong from the second step on stand in for the library: a warm start that takes the other of the two
    rotating buffers for y+ after an odd iteration count, one that keeps theta, a step that keeps the previous step's affine terms.
    The per-step, per-stage checks refuse each at the first step it can show at (step 1: the first step ran 23 iterations), by more than
    five orders of magnitude."""
    p = problem(name)
    good = records(name, True)
    bad = ho.run_horizon(oracle_of(p), steps_of(p)[:2], True, corrupt=corrupt)
    nx, nu, nv = int(p["network"]["nx"][0]), int(p["network"]["nu"][0]), int(p["config"]["nv"][0])
    errors = []
    for t in (0, 1):        # (the first step is clean, so step 1 is handed the good loop's state -- as a context under test would be)
        assert all(np.array_equal(bad[t][k], good[t][k]) for k in ("x", "prevU", "prevD"))
        got = dict(u_raw=bad[t]["u_raw"], u=bad[t]["u"], hist=bad[t]["hist"], bufs={nm: bad[t]["bufs"][nm] for nm in ho.NAMES})
        errors.append(ho.step_errors(got, good[t], p["tree"], nx, nu, nv))
    assert max(errors[0].values()) == 0.0
    e = errors[1]
    print("%s %s step 1: worst %.1e (%s), root control %.1e" % (name, corrupt, max(e.values()), max(e, key=e.get), e["u_raw"]))
    assert max(e.values()) > 1e6 * TOL and e["u_raw"] > 1e5 * TOL, (corrupt, e)


def test_former_check_passes_a_wrong_buffer_after_an_odd_count():
    """... while the suite's former check of a warm step (`small`, an EVEN count of 30 before the warm start, whole-buffer relmax of four
    buffers) is blind to the first of them: the corrupted oracle is the good one there, bit for bit.  The other two it does refuse -- in
    the one configuration it runs: dense, one GPU, cold-started first step of one batch."""
    e = former_check("wrong_buffer")
    assert max(e.values()) == 0.0, e
    for c in ("stale_theta", "stale_affine"):
        e = former_check(c)
        print("former check, %s: %s" % (c, {k: "%.1e" % v for k, v in e.items()}))
        assert max(e.values()) > TOL


# ---------------------------------------------------------------------------------------------------------------
# 2. one GPU, fp64: every operator form, cold and warm
# ---------------------------------------------------------------------------------------------------------------
FUSES = {"medium": (0, -1)}      # ny = 80 runs k_dual_stage: the fused walk + dual update off / by default; small (19), ragged (23), odd (27): flat
FORMS = ["dense", "structured", "auto", "auto+block"]
BLOCK_AT = 2                     # the step in front of which the auto context is handed a block


def block_of(o):
    """(node, block): 1.2 x the factor step's own D block of a node in the middle of the tree"""
    node = o.nodes // 2
    return node, 1.2 * o.get("D").reshape(o.nodes, -1)[node]


def _block_hook(t, o):
    if t == BLOCK_AT:
        node, blk = block_of(o)
        o.buf("D").reshape(o.nodes, -1)[node] = blk


def block_records(name, warm):
    return records(name, warm, before_step=_block_hook)


def run_loop(name, form, warm, fuse=-1, soft=False, what="", **kw):
    p = problem(name, soft)
    recs = block_records(name, warm) if form == "auto+block" else records(name, warm, soft, **({"track_dist": True} if soft else {}))
    s = solver(p, form.split("+")[0], warm, **kw)
    if fuse != -1:
        s.setFusedWalkDual(fuse)
    counters, worst = [], 0.0
    try:
        for rec in recs:
            if form == "auto+block" and rec["t"] == BLOCK_AT:
                assert s.operatorMode() == ("auto", "structured")
                node, blk = block_of(oracle_of(p))
                s.setOperator(capi.OP_D, node, blk)
            if form == "auto+block":
                assert s.operatorMode() == ("auto", "dense" if rec["t"] >= BLOCK_AT else "structured")
            worst = max(worst, assert_step(step_of(s, rec), rec, p, "%s %s %s fuse %d%s" % (name, form, "warm" if warm else "cold", fuse, what)))
            counters.append(s.counters())
        assert s.guardCheck() == 0
    finally:
        s.close()
    print("%s %s %s fuse %d: worst error of any step %.1e" % (name, form, "warm" if warm else "cold", fuse, worst))
    return counters


@gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,fuse", [(n, f) for n in ("small", "ragged", "medium", "odd") for f in FUSES.get(n, (-1,))])
def test_control_steps_match_the_oracle(name, fuse, form, warm):
    counters = run_loop(name, form, warm, fuse)
    # 23, 16 and 37 iterations are one optimistic batch each, 5 and 1 an exact one; nothing trips
    assert [c["optimistic"] for c in counters] == [1, 2, 3, 3, 3] and [c["exact"] for c in counters] == [0, 0, 0, 1, 2], counters
    assert counters[-1]["replayed"] == 0 and counters[-1]["hold"] == 0


@gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("form", ["dense", "structured"])
def test_a_replayed_batch_in_a_later_step(form, warm):
    """the soft-penalty problem: the first optimistic batch that trips is in step 2, cold and warm; it is replayed through the
    exact path, the next step warm-starts from what the replay left, and the batches behind it back off to the exact path"""
    counters = run_loop("medium", form, warm, soft=True, what=" soft")
    k = REPLAYED_IN[warm]
    assert [c["replayed"] for c in counters[:k]] == [0] * k and counters[k]["replayed"] == 1 and counters[k]["hold"] > 0, counters
    assert counters[-1]["replayed"] == 1 and counters[-1]["exact"] >= T - 1 - k, counters


@gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("name", ["odd", "medium"])
def test_f32_stored_blocks_across_control_steps(name, warm):
    """operator_storage="f32" under fp64 iterates: the oracle runs the loop on the blocks as the context stores them
    (test_gpu_operator_storage.blocks_of / oracle_with_blocks)"""
    import test_gpu_operator_storage as sto

    p = problem(name)
    s = solver(p, "dense", warm, operator_storage="f32")
    try:
        assert s.operatorStorage() == ("f32", "f32")
        o = oracle_of(p)
        for nm, b in sto.blocks_of(s).items():
            view = o.buf(nm).reshape(o.nodes, b.shape[1])
            assert 1e-9 < ho.relmax(b, view) < 1e-7, nm                         # fp32 roundings of the oracle's own blocks
            view[:] = b
        recs = ho.run_horizon(o, steps_of(p), warm)
        for rec in recs:
            assert_step(step_of(s, rec), rec, p, "%s f32-stored blocks %s" % (name, "warm" if warm else "cold"))
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. in-place updates between steps
# ---------------------------------------------------------------------------------------------------------------
def update_plan(name):
    """(problem, re-weighted tree, per-stage rows, per-node rows): per-stage bounds in front of step 1, the re-weighted tree in front of
    step 2, per-node bounds in front of step 3"""
    import test_gpu_bounds as bnd
    import test_gpu_tree_data as td

    p = problem(name)
    new = td.reweighted(p["tree"], synth.forecast_at(p["forecast"], 0), 7)
    rows = bnd.staged(p)
    return p, new, rows, bnd.per_node(rows, p["tree"], True)


def updated_records(name, warm, upto=3):
    import test_gpu_bounds as bnd

    key = ("updates", name, warm, upto)
    if key not in _RECORDS:
        p, new, _, _ = update_plan(name)

        def hook(t, o):
            if t == 1 and upto >= 1:
                bnd.oracle_scale(o, p["tree"])
            elif t == 2 and upto >= 2:
                o2 = oracle_of(p, new)
                bnd.oracle_scale(o2, new)
                return o2
            elif t == 3 and upto >= 3:
                xs = o.get("xs").reshape(o.nodes, o.nx)
                xs[bnd.second_of_last_stage(p["tree"])] *= 1.25
                o.set("xs", xs)
            return None

        _RECORDS[key] = ho.run_horizon(oracle_of(p), steps_of(p), warm, before_step=hook)
    return _RECORDS[key]


def apply_update(s, t, plan, local=None):
    p, new, rows, nodes = plan
    if t == 1:
        s.setBounds("stage", **rows)
    elif t == 2:
        s.updateTree(new)
    elif t == 3:
        s.setBounds("node", **({k: v[local] for k, v in nodes.items()} if local is not None else nodes))


@gpu
@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("form", ["dense", "structured", "auto"])
@pytest.mark.parametrize("name", ["medium", "ragged"])
def test_in_place_updates_between_control_steps(name, form, warm):
    """one long-lived context: per-stage bounds, a re-weighted tree and per-node bounds between its steps, every step against an oracle
    given the same data; and, from the last update on, bit for bit a context created on the final data and fed the same duals"""
    plan = update_plan(name)
    p, new = plan[0], plan[1]
    recs = updated_records(name, warm)
    for t in (1, 2, 3):                                                            # every update matters: the loop without it is another one
        without = updated_records(name, warm, upto=t - 1)[t]
        assert max(ho.relmax(recs[t]["bufs"][nm], without["bufs"][nm]) for nm in ("x", "u", "updXi", "updPsi")) > 1e-6, t
    s = solver(p, form, warm)
    fresh = None
    try:
        for rec in recs:
            apply_update(s, rec["t"], plan)
            if rec["t"] == 3:
                duals = [s.get(b) for b in DUAL_BIDS]
                fresh = solver(p, form, warm, tree=new)
                fresh.setBounds("node", **plan[3])
                if warm:
                    control_step(fresh, recs[0], most=1)                        # (a context that has never iterated cold-starts)
                    for b, v in zip(DUAL_BIDS, duals):
                        fresh.set(b, v)
            got = step_of(s, rec)
            assert_step(got, rec, p, "%s %s %s in-place updates" % (name, form, "warm" if warm else "cold"))
            if fresh is not None:
                other = step_of(fresh, rec)
                assert np.array_equal(got["u"], other["u"]) and np.array_equal(got["hist"], other["hist"]), rec["t"]
                for nm in got["bufs"]:
                    assert np.array_equal(got["bufs"][nm], other["bufs"][nm]), (rec["t"], nm)
        assert s.guardCheck() == 0
    finally:
        s.close()
        if fresh is not None:
            fresh.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. shards across control steps
# ---------------------------------------------------------------------------------------------------------------
def global_history(parts):
    """the tree-global vecPrimalInfs from the ranks' parts [rank, iteration, (absXi, valXi, absPsi, valPsi)]: the signed entry at the
    arg-max over the ranks of each half, the larger of the two (test_gpu_sharded_batched)"""
    n = parts.shape[1]
    ix, ip = parts[:, :, 0].argmax(0), parts[:, :, 2].argmax(0)
    vx, vp = parts[ix, np.arange(n), 1], parts[ip, np.arange(n), 3]
    return np.where(vx > vp, vx, vp)


def run_shards(name, world, cut, structured, optimistic, warm, soft=False, recs=None, most=None, plan=None, solver_kw=None, what=""):
    from test_gpu_sharded_batched import Ranks

    p = problem(name, soft)
    recs = records(name, warm, soft, **({"track_dist": True} if soft else {})) if recs is None else recs
    rk = Ranks(p, world, cut, structured, optimistic=optimistic)
    label = "%s %d ranks cut %d %s %s %s%s" % (name, world, cut, "structured" if structured else "dense", "optimistic" if optimistic else "exact",
                                                "warm" if warm else "cold", what)
    counters = []
    try:
        def setup(s):
            for k, v in (solver_kw or {}).items():
                getattr(s, k)(*v)
            s.factorStep()
            s.setWarmStart(warm)

        rk.run(setup)
        nx, nu, nv = rk.shards[0].nx, rk.shards[0].nu, rk.shards[0].nv
        dims = {"nx": nx, "nu": nu, "nv": nv, "2nx": 2 * nx}
        from stagewise import DIM_OF
        for rec in recs:
            def step(s):
                if plan is not None:
                    apply_update(s, rec["t"], plan, np.asarray(s.global_nodes, int))
                u = control_step(s, rec, most)
                last = s.last_solve()
                return u, s.get(capi.BUF_U)[: s.nu].copy(), last, s.historyParts(0, last["iterations"]), s.counters()

            res = rk.run(step)
            for r, (u, u_raw, last, _, c) in enumerate(res):
                assert np.array_equal(u, res[0][0]) and np.array_equal(u_raw, res[0][1]), (label, rec["t"], "rank %d: another root control" % r)
                assert last == res[0][2] and last["iterations"] == rec["n"], (label, rec["t"], r, last, res[0][2], rec["n"])
                assert c == res[0][4], (label, rec["t"], r, c, res[0][4])
            hist = global_history(np.stack([x[3] for x in res]))
            got = dict(u=res[0][0], u_raw=res[0][1], hist=hist, bufs={nm: rk.gathered(bid, dims[DIM_OF[nm]]) for bid, nm in PAIRS})
            assert_step(got, rec, p, label)
            counters.append(res[0][4])
        assert [s.guardCheck() for s in rk.shards] == [0] * world
    finally:
        rk.close()
    return counters


SHARD_CASES = [
    # name, world, cut (0: the partitioner's own), structured, optimistic, warm
    ("medium", 2, 0, False, True, True), ("medium", 2, 1, True, False, False), ("medium", 2, 2, False, False, True),
    ("medium", 3, 0, False, False, True), ("medium", 3, 1, False, True, False), ("medium", 3, 2, True, True, True),
    ("medium", 4, 0, True, True, False), ("medium", 4, 1, False, True, True), ("medium", 4, 2, True, False, True),
    ("ragged", 2, 0, True, False, True), ("ragged", 2, 1, False, False, False), ("ragged", 2, 2, False, True, True),
    ("ragged", 3, 1, False, False, True), ("ragged", 3, 1, True, True, False), ("ragged", 3, 2, True, True, True),
    ("ragged", 4, 2, False, True, True), ("ragged", 4, 2, True, False, False),
]


def test_shard_cases_cover_every_value():
    """worlds 2, 3, 4; cuts 0, 1, 2; both forms; both exchanges; cold and warm; both trees -- and every pair (world, cut) the trees allow"""
    cols = list(zip(*SHARD_CASES))
    assert set(cols[0]) == {"medium", "ragged"} and set(cols[1]) == {2, 3, 4} and set(cols[2]) == {0, 1, 2}
    assert all(set(c) == {False, True} for c in cols[3:])
    for name in ("medium", "ragged"):
        mine = [c for c in SHARD_CASES if c[0] == name]
        for col in (3, 4, 5):
            assert {c[col] for c in mine} == {False, True}, (name, col)
        assert {c[1] for c in mine} == {2, 3, 4}
    assert {(c[1], c[2]) for c in SHARD_CASES if c[0] == "medium"} == {(w, c) for w in (2, 3, 4) for c in (0, 1, 2)}


@gpu
@pytest.mark.parametrize("name,world,cut,structured,optimistic,warm", SHARD_CASES)
def test_shards_across_control_steps(name, world, cut, structured, optimistic, warm):
    counters = run_shards(name, world, cut, structured, optimistic, warm)
    assert counters[-1]["replayed"] == 0, counters


@gpu
@pytest.mark.parametrize("world,cut,structured,warm", [(2, 1, False, True), (3, 0, True, True), (4, 2, False, False)])
def test_shards_replay_a_batch_in_a_later_step(world, cut, structured, warm):
    """the soft-penalty problem on shards: the verdict vote refuses the optimistic batch of step 2 on every rank, the
    batch is replayed through the exact two-collective path, and the following steps start from what the replay left"""
    counters = run_shards("medium", world, cut, structured, True, warm, soft=True, what=" soft")
    k = REPLAYED_IN[warm]
    assert [c["replayed"] for c in counters[:k]] == [0] * k and counters[k]["replayed"] >= 1, counters


@gpu
def test_shards_stop_at_the_oracles_batch_boundaries():
    """a stop tolerance on 3 ranks, warm: every rank reports the same iteration count at every step (asserted in run_shards), the counts are
    the oracle's (20, 30, 40, 40, 40), and the iterates those of the oracle run for exactly that count"""
    recs = stop_records()
    assert [r["n"] for r in recs] == STOP_COUNTS
    run_shards(STOP["name"], 3, 1, False, True, True, recs=recs, most=STOP["most"], solver_kw={"setStopTolerance": (STOP["tol"], STOP["every"])}, what=" stop tolerance")


@gpu
def test_shards_updated_in_place_between_control_steps():
    """per-stage bounds, the re-weighted tree and the ranks' local per-node rows between the steps of 3 rank contexts"""
    run_shards("medium", 3, 0, False, True, True, recs=updated_records("medium", True), plan=update_plan("medium"), what=" in-place updates")


# ---------------------------------------------------------------------------------------------------------------
# 5. fp32 iterates at a later step
# ---------------------------------------------------------------------------------------------------------------
F32_STEPS = (1, 2)
_F32 = {}


def f32_case(name):
    """for t in F32_STEPS of the fp64 oracle's warm loop: the fp32-rounded duals the step starts from, and -- for the constants, a cold and
    a warm batch of 16 -- the fp64 reference's buffers with the fp32 oracle's per-stage errors against them.  Computed once."""
    import test_gpu_apg_f32 as a32

    if name in _F32:
        return _F32[name]
    p = problem(name)
    loop = ho.run_horizon(oracle_of(p), steps_of(p)[: max(F32_STEPS) + 1], True)
    stages = np.asarray(p["tree"]["stages"], int)[: int(p["tree"]["nodes"][0])]
    lam = float(p["config"]["stepSize"][0])
    ref, cpu = oracle_of(p), Oracle(p["network"], p["tree"], p["config"], precision="f32")
    cpu.factor_step()
    d = {"x": ref.nx, "u": ref.nu, "v": ref.nv, "uhat": ref.nu, "e": ref.nx, "beta": ref.nv, "alpha": ref.nu}
    dim = lambda nm: d.get(nm, ref.nu if nm.endswith("Psi") or nm == "psi" else 2 * ref.nx)
    case = dict(p=p, dim=dim, stages=stages, lam=lam, steps={})
    for t in F32_STEPS:
        rec, prev = loop[t], loop[t - 1]
        duals = {nm: a32.round32(prev["bufs"][nm]) for nm in ho.DUALS}
        snaps = {}
        for kind in ("cold", "warm"):
            for o in (ref, cpu):
                o.apg_reset()
                for nm in ho.DUALS:
                    o.set(nm, duals[nm])
                o.update_state_control(rec["x"], rec["prevU"], rec["prevD"])
                o.eliminate(rec["dh"], rec["ah"])
            if kind == "cold":                                              # the constants once: they are the same for both kinds
                aff = {nm: ref.get(nm) for nm in ho.AFFINE}
                snaps["constants"] = (aff, {nm: a32.stage_metric({nm: cpu.get(nm)}, dict(aff, **{k: ref.get(k) for k in a32.Z_SOURCES}), (nm,), stages, lam, dim)[nm] for nm in ho.AFFINE})
                for o in (ref, cpu):
                    o.apg(ho.BATCH)
            else:
                for o in (ref, cpu):
                    ho.keep_duals(o)
                    o.apg_continue(ho.BATCH, [1.0, 1.0])
            r = {nm: ref.get(nm) for nm in a32.ALL}
            snaps[kind] = (r, a32.stage_metric({nm: cpu.get(nm) for nm in a32.ALL}, r, a32.ALL, stages, lam, dim))
        case["steps"][t] = dict(rec=rec, duals=duals, snaps=snaps)
    _F32[name] = case
    return case


@pytest.mark.parametrize("name", ["medium", "barcelona31"])
def test_f32_yardstick_is_not_degenerate(name):
    """e_cpu, the fp32 oracle's own error at steps 1 and 2, is a real fp32 error -- not 0, where the floor alone would be the bound -- on
    the constants and on nearly every buffer of both batches.  (Measured: 1e-7 ... 1e-5 of the stage's scale; beta, a difference of
    sums, is the largest of the constants at 1e-5.)"""
    import test_gpu_apg_f32 as a32

    case = f32_case(name)
    for t, st in case["steps"].items():
        for kind in ("cold", "warm"):
            e = {nm: v[0] for nm, v in st["snaps"][kind][1].items()}
            assert max(e.values()) > a32.EPS32 and sum(v > 0 for v in e.values()) >= len(e) - 3, (name, t, kind, e)
            assert max(e.values()) < 1e-3, (name, t, kind, e)              # ... and an fp32 error, not a disagreement
        e = {nm: v[0] for nm, v in st["snaps"]["constants"][1].items()}
        assert e["beta"] > a32.EPS32 and max(e.values()) < 1e-3, (name, t, e)
        print("%s step %d: e_cpu constants %.1e, cold %.1e, warm %.1e" % (name, t, max(e.values()), max(v[0] for v in st["snaps"]["cold"][1].values()),
                                                                          max(v[0] for v in st["snaps"]["warm"][1].values())))


@gpu
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name", ["medium", "barcelona31"])
def test_f32_control_step_at_a_later_state(name, mode):
    """an fp32 context at steps 1 and 2 of the fp64 oracle's loop: the constants of the control step behind updateStateControl +
    eliminateInputDistubanceCoupling (k_affine_demand, k_affine_beta, k_fold_affine; structured: the refreshed linear constants show in the
    batch), then one 16-iteration batch through rn_control_action, cold and warm from the step's fp32-rounded duals; bound per stage:
    e_gpu <= 4 e_cpu + 32 * 2^-24 (test_gpu_apg_f32)"""
    import test_gpu_apg_f32 as a32

    case = f32_case(name)
    p = case["p"]
    led = a32.Ledger("horizon %s %s" % (name, mode))
    s = capi.Solver(p["network"], p["tree"], p["config"], precision="f32", operator_mode=mode)
    s.factorStep()
    try:
        for t, st in case["steps"].items():
            rec = st["rec"]
            s.updateStateControl(rec["x"], rec["prevU"], rec["prevD"])
            s.eliminateInputDistubanceCoupling(rec["dh"], rec["ah"])
            aff, e_cpu = st["snaps"]["constants"]
            for nm in ho.AFFINE:
                ref = dict(aff, **{k: st["snaps"]["cold"][0][k] for k in a32.Z_SOURCES})
                e = a32.stage_metric({nm: s.get(AFFINE_BID[nm])}, ref, (nm,), case["stages"], case["lam"], case["dim"])[nm]
                led.add("constants", "step %d" % t, t, nm, e[0], e_cpu[nm][0], " (stage %d)" % e[1])
            for kind in ("cold", "warm"):
                s.setWarmStart(kind == "warm")
                if kind == "warm":
                    s.setWarmStart(False)
                    control_step(s, rec, most=1)                                 # a context that has iterated: the next call keeps its duals
                    s.setWarmStart(True)
                    for nm in ho.DUALS:
                        s.set(BID[nm], st["duals"][nm])
                before = s.counters()
                control_step(s, rec, most=ho.BATCH)
                c = s.counters()
                assert (c["optimistic"] - before["optimistic"], c["replayed"] - before["replayed"]) == (1, 0), (kind, before, c)
                r, e_cpu_b = st["snaps"][kind]
                e = a32.stage_metric({nm: s.get(BID[nm]) for nm in a32.ALL}, r, a32.ALL, case["stages"], case["lam"], case["dim"])
                for nm in a32.ALL:
                    led.add(kind, "step %d" % t, t, nm, e[nm][0], e_cpu_b[nm][0], " (stage %d; the fp32 oracle's worst: stage %d)" % (e[nm][1], e_cpu_b[nm][1]))
    finally:
        s.close()
    print("%s %s: worst share of the bound %.3f" % (name, mode, led.worst()))
    led.finish()


# ---------------------------------------------------------------------------------------------------------------
# guard mode's body (tests/test_gpu_guard.py)
# ---------------------------------------------------------------------------------------------------------------
def guard_body():
    """one warm structured loop and one warm loop on 3 ranks; returns the number of contexts"""
    run_loop("medium", "structured", True)
    run_shards("medium", 3, 1, False, True, True)
    gc.collect()
    return 4
