"""k_stream_gemv's split last round (StreamSplit, SPLIT = true, second partials in my2) against the fp64 oracle.

Ctx::stream_split_setup() turns the split on for dense contexts whose launch is one round of workgroups plus a last round that is at
most half full, whose leftover blocks r = nodes % numCUs lie in the last three stages of the chain region, and whose blocks have at
least two groups of spans.  None of the named trees of the suite meets that on a 256-CU device except the 1/8 shards and the fp32
run of the 493-scenario tree, and no test could tell whether the path was taken.  Here the trees are BUILT from the device's CU
count (split_tree: nodes = numCUs + r exactly, the smallest trees at which the split can exist) and every positive case first
asserts through rn_debug_stream_info (Solver.streamInfo) that the split is on and where: a case that fell back to the unsplit
launch fails.  WHICH half takes the odd group is asserted from the hook only (splitSpanHalf == (groups + 1) / 2 * D, the library's
own rule restated): wherever the boundary lies the two halves together cover every span, so no sum depends on it.

The comparison is per stage (the split touches three stages only; a whole-tree maximum hides them behind the root's magnitudes):
max |got - ref| over the nodes of a stage / max |ref| over that stage, at the project's own tolerances (test_gpu_parity.py:
REL_TOL in fp64, FP32_TOL in fp32, both against the fp64 oracle).  No floor under a stage's scale is needed on these problems: every
stage of every compared vector has a maximum within two decades of the vector's, and the fp64 oracle against its own fp32 build
(precision="f32": no kernel involved) differs per stage by at most 1.6e-5 (resXi; 4.3e-6 dualXi, 2e-6 and less elsewhere) after
ITERS iterations on the b236 / b240 / nv129 trees -- a decade inside FP32_TOL."""
import numpy as np
import pytest

import test_gpu_fbe_nama as fbe
from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from test_gpu_parity import FP32_TOL, REL_TOL, relmax
from test_gpu_sharded_batched import Ranks

pytestmark = pytest.mark.gpu

ITERS = 14
STREAM_D, STREAM_D_WIDE, SPLIT_STAGES = 5, 3, 3      # RN_STREAM_D, RN_STREAM_D_WIDE, STREAM_SPLIT_STAGES (csrc/common.hpp)

# (nx, nu, nd, ne): the smallest networks with two groups of spans.  b240: Barcelona's dimensions, ny = 240 -- fp64 G = 8, 6 groups,
# fp32 G = 16, 3 groups (odd).  b236: ny = 236 -- fp64 29 whole spans = 5 groups (odd) + 4 whole spans outside the groups + a ragged
# span of 4 columns.  nv129: 2 nv = 258 rows, fp64 129 slots per column (odd): G = 8 is the only line-aligned span, 1032 slots,
# NL = 3, D = 3, ny = 201 = 25 spans + 1 column
NETS = {"b240": (50, 63, 114, 88, 17), "b236": (51, 61, 114, 88, 17), "nv129": (52, 30, 141, 40, 12)}
VECS = (("x", capi.BUF_X, "nx"), ("u", capi.BUF_U, "nu"), ("v", capi.BUF_V, "nv"), ("updXi", capi.BUF_UPD_XI, "2nx"), ("updPsi", capi.BUF_UPD_PSI, "nu"),
        ("primalXi", capi.BUF_PRIMAL_XI, "2nx"), ("primalPsi", capi.BUF_PRIMAL_PSI, "nu"), ("dualXi", capi.BUF_DUAL_XI, "2nx"),
        ("resXi", capi.BUF_RES_XI, "2nx"), ("resPsi", capi.BUF_RES_PSI, "nu"))
ALL_BUFS = tuple(b for _, b, _ in VECS) + (capi.BUF_XI, capi.BUF_PSI, capi.BUF_ACC_XI, capi.BUF_ACC_PSI, capi.BUF_DUAL_PSI)

_CUS = []


def num_cus():
    """the device's CU count as the library sees it (valid from rn_create on): from a throw-away context"""
    if not _CUS:
        p = synth.make_problem("tiny")
        s = capi.Solver(p["network"], p["tree"], p["config"])
        info = s.streamInfo()
        assert info["splitFirst"] == -1 and info["numCUs"] > 0, info          # the factor step has not decided yet
        _CUS.append(info["numCUs"])
        s.close()
    return _CUS[0]


def split_tree(cus, r, K=None, N=None):
    """(branching list for synth, N) of a tree with cus + r nodes exactly: the root, one crown stage of a nodes (1 <= a <= K) whose
    children are dealt raggedly to K chains, then N - 2 stages of K nodes: 1 + a + K (N - 2) = cus + r.  Give K (N follows) or N
    (K = the widest that leaves a >= 1)."""
    total = cus + r
    if K is None:
        K = (total - 2) // (N - 2)
    if N is None:
        N = (total - 2) // K + 2
    a = total - 1 - K * (N - 2)
    assert 1 <= a <= K and N >= 3, (cus, r, K, N, a)
    deal = [K // a + (1 if j < K % a else 0) for j in range(a)]
    assert sum(deal) == K and min(deal) >= 1
    return [a, deal], N


def position(pos, cus):
    """(r, K, N) of the named position of the split round in the tree; K or N is None where split_tree derives it"""
    k0 = max(cus // 16, 4)
    return {
        "r1": (1, k0 + 2, None),                              # one block in the split round (K = 18 on 256 CUs: four crown nodes)
        "last": (k0 - 6 if k0 > 8 else 2, k0, None),          # r < K: inside the last stage
        "two": (k0 + k0 // 2, k0, None),                      # K < r <= 2K: the last stage and a part of the one before
        "three": (2 * k0 + k0 // 2, k0, None),                # 2K < r <= 3K: three stages
        "half": (cus // 2, -(-(cus // 2) // 3), None),        # 2r == numCUs exactly, in three stages (K = 43 on 256 CUs)
        "short": (cus // 2 - 2, None, 5),                     # N - chainStage == 3: the chain region IS the three stages
        # negative controls
        "over_half": (cus // 2 + 1, -(-(cus // 2 + 1) // 3), None),   # 2r == numCUs + 2
        "four": (3 * k0 + 1, k0, None),                       # r = 3K + 1: a block of the round in a fourth stage
    }[pos]


_PROBLEMS, _REFS = {}, {}


def problem(net, pos=None, branching=None, N=None):
    """the problem of a network on the tree of a position (or on a given tree), built once per module"""
    key = (net, pos, str(branching), N)
    if key not in _PROBLEMS:
        if branching is None:
            r, K, N = position(pos, num_cus())
            branching, N = split_tree(num_cus(), r, K, N)
        idx, nx, nu, nd, ne = NETS[net]
        name = "split_%s_%s" % (net, pos)
        synth.CONFIGS[name] = (idx, nx, nu, nd, ne, N, branching)
        try:
            p = synth.make_problem(name)
        finally:
            del synth.CONFIGS[name]
        _PROBLEMS[key] = (p, synth.forecast_at(p["forecast"], 0))
    return _PROBLEMS[key]


def aliasing(p):
    """the reference's Omega / Theta aliasing (Engine.cu:210-221) needs a tree that branches from the root on: a CU count that leaves
    ONE crown node gives the oracle per-node blocks instead (test_gpu_parity.py, "late")"""
    return int(p["tree"]["nodesPerStage"][1]) > 1


def oracle_of(p, fc, precision="f64"):
    o = Oracle(p["network"], p["tree"], p["config"], precision=precision, alias_operators=aliasing(p))
    o.initialise(*fc)
    return o


def reference(key, p, fc, iters=ITERS):
    """the fp64 oracle's iterates and history after `iters` APG iterations, computed once per problem and left unchanged"""
    k = (key, iters)
    if k not in _REFS:
        o = oracle_of(p, fc)
        hist = o.apg(iters)
        ref = {nm: o.get(nm) for nm, _, _ in VECS}
        for a in ref.values():
            a.setflags(write=False)
        _REFS[k] = (ref, hist)
    return _REFS[k]


def stage_errors(got, ref, tree, dim):
    """[max |got - ref| over the nodes of stage k / max |ref| over the nodes of stage k, for every stage k]"""
    nodes = int(tree["nodes"][0])
    st = np.asarray(tree["stages"], int)[:nodes]
    got, ref = np.asarray(got, float).reshape(nodes, dim), np.asarray(ref, float).reshape(nodes, dim)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    n = int(st.max()) + 1
    err, mag = np.zeros(n), np.zeros(n)
    np.maximum.at(err, st, np.abs(got - ref).max(axis=1))
    np.maximum.at(mag, st, np.abs(ref).max(axis=1))
    return err / np.maximum(mag, 1e-300)


def dims_of(s):
    return {"nx": s.nx, "nu": s.nu, "nv": s.nv, "2nx": 2 * s.nx}


def compare(tag, get, s, tree, ref, tol, hist=None, ohist=None, first_stages=None):
    """every vector of VECS, stage by stage, against the reference; prints the worst stage of every vector before it asserts"""
    d, worst = dims_of(s), {}
    for nm, bid, dm in VECS:
        if nm in ref:
            e = stage_errors(get(bid, d[dm]), ref[nm], tree, d[dm])[:first_stages]
            worst[nm] = (float(e.max()), int(e.argmax()))
    print("\n%s: worst per-stage error (stage): %s" % (tag, {k: "%.1e (%d)" % v for k, v in worst.items()}))
    bad = {k: v for k, v in worst.items() if not v[0] <= tol}
    assert not bad, (tag, bad)
    if hist is not None:
        assert np.abs(hist - ohist).max() <= tol * np.abs(ohist).max(), (tag, hist, ohist)


def stage_of(tree, node):
    return int(np.asarray(tree["stages"], int)[node])


def expect_split(s, r, tag=""):
    """the hook's account of the launch: split on, at nodes - r, in the two-per-CU instantiation, inside the last three stages and
    with the first half taking the odd group; returns (streamInfo, kernelInfo, groups)"""
    info, k = s.streamInfo(), s.kernelInfo()
    G, NL = k["stream_G"], k["stream_NL"]
    D = STREAM_D if NL <= 2 else STREAM_D_WIDE
    groups = (s.ny // G) // D
    print("\n%s nodes %d r %d K %d N %d G %d NL %d groups %d ragged %d %s" % (tag, s.nodes, r, s.K, s.N, G, NL, groups, s.ny % G, info))
    assert info["splitFirst"] == s.nodes - r, (info, s.nodes, r)
    assert info["twoPerCU"] == 1, info
    assert groups >= 2 and info["splitSpanHalf"] == (groups + 1) // 2 * D, (info, groups, D)
    assert s.nodes == info["numCUs"] + r and 2 * r <= info["numCUs"]
    assert s.N - k["chain_stage"] >= SPLIT_STAGES and stage_of(s.tree, info["splitFirst"]) >= s.N - SPLIT_STAGES
    return info, k, groups


def expect_no_split(s):
    info = s.streamInfo()
    assert info["splitFirst"] == s.nodes and info["splitSpanHalf"] == 0, info
    return info


def solver(p, fc, precision="f64", **kw):
    s = capi.Solver(p["network"], p["tree"], p["config"], precision=precision, **kw)
    s.initialiseSmpcController(*fc)
    return s


def local_get(s):
    return lambda bid, dim: s.get(bid)


# what a case is named for, checked from the hooks: (network, precision) -> property of the span walk; position -> stages of the round
def span_property(net, precision, s, k, groups):
    G, NL = k["stream_G"], k["stream_NL"]
    if (net, precision) == ("b240", "f64"):
        assert groups % 2 == 0 and s.ny % G == 0 and NL <= 2, (k, groups)                  # the plain case: even groups, no ragged span
    elif net == "b240":
        assert groups % 2 == 1 and NL <= 2, (k, groups)                                    # odd group count
    elif (net, precision) == ("b236", "f64"):
        assert groups % 2 == 1 and s.ny % G != 0 and (s.ny // G) % STREAM_D != 0, (k, groups)   # odd groups, whole spans outside the groups, ragged span
    elif net == "b236":
        assert s.ny % G != 0, (k, groups)                                                  # ragged span
    else:
        assert NL >= 3 and s.ny % G != 0, (k, groups)                                      # RN_STREAM_D_WIDE, ragged span


def stage_property(pos, s, info, r):
    first, last = stage_of(s.tree, info["splitFirst"]), s.N - 1
    if pos == "r1":
        assert r == 1 and first == last
    elif pos == "last":
        assert 1 < r < s.K and first == last
    elif pos == "two":
        assert s.K < r <= 2 * s.K and first == last - 1
    elif pos == "three":
        assert 2 * s.K < r <= 3 * s.K and first == last - 2
    elif pos == "half":
        assert 2 * r == info["numCUs"] and first == last - 2
    elif pos == "short":
        assert s.N - s.kernelInfo()["chain_stage"] == SPLIT_STAGES


CASES = [("b240", "r1", "f64"), ("b240", "last", "f64"), ("b240", "two", "f64"), ("b240", "three", "f64"), ("b240", "half", "f64"), ("b240", "short", "f64"),
         ("b240", "two", "f32"), ("b240", "half", "f32"),
         ("b236", "r1", "f64"), ("b236", "three", "f64"), ("b236", "two", "f32"),
         ("nv129", "two", "f64"), ("nv129", "half", "f64")]


@pytest.mark.parametrize("net,pos,precision", CASES)
def test_split_round_matches_the_oracle(net, pos, precision):
    """ITERS iterations of one control step on a tree whose last round is split: every iterate and the primal-infeasibility history,
    stage by stage, against the fp64 oracle on the same inputs"""
    p, fc = problem(net, pos)
    ref, ohist = reference((net, pos), p, fc)
    s = solver(p, fc, precision)
    r = position(pos, num_cus())[0]
    info, k, groups = expect_split(s, r, "%s %s %s" % (net, pos, precision))
    span_property(net, precision, s, k, groups)
    stage_property(pos, s, info, r)
    hist = s.algorithmApg(ITERS)
    compare("%s %s %s" % (net, pos, precision), local_get(s), s, p["tree"], ref, REL_TOL if precision == "f64" else FP32_TOL, hist, ohist)
    s.close()


def test_one_solve_step_from_a_non_trivial_dual():
    """a single rn_solve_step (and the steps behind it) from the oracle's duals after 3 iterations, on the tree whose split round
    spans three stages with an odd group count and a ragged span: an error of the split has had no iteration to be averaged away"""
    p, fc = problem("b236", "three")
    o, s = oracle_of(p, fc), solver(p, fc)
    expect_split(s, position("three", num_cus())[0])
    o.apg(3); s.algorithmApg(3)
    for bid, nm in ((capi.BUF_XI, "xi"), (capi.BUF_PSI, "psi"), (capi.BUF_UPD_XI, "updXi"), (capi.BUF_UPD_PSI, "updPsi")):
        s.set(bid, o.get(nm))
    s.dualExtrapolationStep(0.618); o.extrapolate(0.618)
    s.solveStep(); o.solve_step()
    s.proximalFunG(); o.prox()
    s.computeFixedPointResidual(); o.residual()
    s.dualUpdate(); o.dual_update()
    compare("one solve step", local_get(s), s, p["tree"], {nm: o.get(nm) for nm, _, _ in VECS}, REL_TOL)
    assert abs(s.updatePrimalInfeasibity() - o.primal_infeasibility()) <= REL_TOL * abs(o.primal_infeasibility())
    s.close()


@pytest.mark.parametrize("net,pos,precision,kw", [("b240", "over_half", "f64", {}), ("b240", "four", "f64", {}),
                                                  ("b240", "two", "f64", {"knobs": {"stream_two_per_cu": 0}}), ("b240", "two", "f64", {"structured": True})])
def test_negative_controls_are_not_split_and_match_the_oracle(net, pos, precision, kw):
    """2r = numCUs + 2; a block of the round in a fourth stage; the one-per-CU instantiation in fp64; structured mode on a tree that
    splits when dense: no split, and the same solve"""
    p, fc = problem(net, pos)
    ref, ohist = reference((net, pos), p, fc)
    s = solver(p, fc, precision, **kw)
    r = position(pos, num_cus())[0]
    info = expect_no_split(s)
    assert s.nodes == info["numCUs"] + r
    if pos == "over_half":
        assert 2 * r == info["numCUs"] + 2
    elif pos == "four":
        assert r == 3 * s.K + 1
    elif "knobs" in kw:
        assert info["twoPerCU"] == 0
    else:
        assert s.operatorMode()[1] == "structured"
    hist = s.algorithmApg(ITERS)
    compare("negative %s %s" % (pos, kw), local_get(s), s, p["tree"], ref, REL_TOL, hist, ohist)
    s.close()


def run_all(p, fc, precision, knobs, iters=ITERS):
    s = solver(p, fc, precision, knobs=knobs)
    info = s.streamInfo()
    hist = s.algorithmApg(iters)
    out = {b: s.get(b) for b in ALL_BUFS}
    s.close()
    return info, hist, out


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_two_instantiations_are_bitwise_the_same_without_the_split(precision):
    """stream_split = 0: SPLIT = true and SPLIT = false walk the columns in the same order"""
    p, fc = problem("b236", "three")
    i0, h0, o0 = run_all(p, fc, precision, {"stream_split": 0, "stream_two_per_cu": 0})
    i1, h1, o1 = run_all(p, fc, precision, {"stream_split": 0, "stream_two_per_cu": 1})
    nodes = i0["numCUs"] + position("three", i0["numCUs"])[0]
    assert (i0["splitFirst"], i0["twoPerCU"]) == (nodes, 0) and (i1["splitFirst"], i1["twoPerCU"]) == (nodes, 1), (i0, i1)
    assert np.array_equal(h0, h1)
    for b in ALL_BUFS:
        assert np.array_equal(o0[b], o1[b]), b


def test_split_on_and_off_agree_above_the_split_stages():
    """the split changes the order of the sums in the last three stages only: both forms match the oracle, and after ONE
    rn_solve_step from a non-trivial dual the stages before the split round's first agree to the fp64 tolerance"""
    p, fc = problem("b236", "three")
    ref, ohist = reference(("b236", "three"), p, fc)
    o = oracle_of(p, fc)
    o.apg(3)
    acc = o.get("accXi"), o.get("accPsi")
    o.solve_step()
    oref = {nm: o.get(nm) for nm in ("x", "u", "v", "primalXi", "primalPsi")}
    got = []
    for split in (1, 0):
        s = solver(p, fc, knobs={"stream_split": split})
        info = s.streamInfo()
        if split:
            expect_split(s, position("three", num_cus())[0])
        else:
            expect_no_split(s)
            assert info["twoPerCU"] == 1
        s.set(capi.BUF_ACC_XI, acc[0]); s.set(capi.BUF_ACC_PSI, acc[1])
        s.solveStep()
        compare("one step, split %d" % split, local_get(s), s, p["tree"], oref, REL_TOL)
        got.append({"primalXi": s.get(capi.BUF_PRIMAL_XI), "primalPsi": s.get(capi.BUF_PRIMAL_PSI)})
        if not split:
            hist = s.algorithmApg(ITERS)
            compare("split off", local_get(s), s, p["tree"], ref, REL_TOL, hist, ohist)
        s.close()
    first = stage_of(p["tree"], num_cus())          # splitFirst = numCUs on these trees
    assert first >= 1
    nx, nu = int(p["network"]["nx"][0]), int(p["network"]["nu"][0])
    for nm, dim in (("primalXi", 2 * nx), ("primalPsi", nu)):
        e = stage_errors(got[0][nm], got[1][nm], p["tree"], dim)[:first]
        print("split on against off, %s, stages < %d: %.1e" % (nm, first, e.max()))
        assert e.max() <= REL_TOL, (nm, e)


UPCUT_THREADS = 1024          # k_up_chain_cut's workgroup (csrc/k_walks.hpp)


def sharded_tree(cus, lanes_per, world=2):
    """(branching, N, cut stage, [r of every rank]) of a tree whose two shards take the MERGED up walk k_up_chain_cut (Ctx::up_cut_lanes: the
    cut lies right above the chains, and every cut parent's local chains fit side by side in one workgroup of UPCUT_THREADS lanes,
    lanes_per each) and whose shards' own node counts put their last rounds into the split range, in the third stage from the end:
    root -> a cut parents -> chains, cut below stage 2.  The chains are dealt round-robin, so a parent with an even child count gives
    each rank half; the last parent has one more, which goes to rank 0: K1 + 1 and K1 local chains.  On 256 CUs with 5 chains per
    workgroup: 4 parents with 10, 10, 8, 9 children, 16 chain stages, shards of 309 and 293 nodes (r = 53 and 37)."""
    most = UPCUT_THREADS // lanes_per
    assert most >= 2 and world == 2
    for a in range(4, 33):
        for k1 in range(2 * a, most * a):              # rank 1's chains; rank 0 has one more
            for L in range(3, 64):
                rs = [1 + a + k * L - cus for k in (k1 + 1, k1)]
                if all(2 * k < r <= 3 * k and 2 * r <= cus for k, r in zip((k1 + 1, k1), rs)):
                    deal = [2 * (k1 // a + (1 if j < k1 % a else 0)) for j in range(a)]
                    deal[-1] += 1
                    if (max(deal) + 1) // 2 <= most:
                        return [a, deal], L + 2, 2, rs
    raise AssertionError("no two-rank tree for %d CUs" % cus)


def sharded_split_problem():
    """(problem, forecast, cut stage, expect) of the b240 network on sharded_tree; expect(shards) asserts, from the two shard contexts behind a
    run, the split last round of each and the conditions of the merged launch (Ctx::up_cut_lanes)"""
    idx, nx, nu, nd, ne = NETS["b240"]
    lanes_per = (nu - ne + nx + 63) // 64 * 64
    branching, N, cut, rs = sharded_tree(num_cus(), lanes_per)
    p, fc = problem("b240", "sharded", branching, N)

    def expect(shards):
        for rank, (s, r) in enumerate(zip(shards, rs)):
            info, k = s.streamInfo(), s.kernelInfo()
            print("\nrank %d nodes %d r %d %s %s" % (rank, s.nodes, r, info, k))
            assert info["splitFirst"] == s.nodes - r and s.nodes == info["numCUs"] + r and info["twoPerCU"] == 1, (info, s.nodes, r)
            # the merged launch: cut stage == first chain stage, and the most local children of a cut parent fit one workgroup
            local = capi.partition_tree(p["tree"], rank, 2, cut)["tree"]
            kids = np.bincount(np.asarray(local["ancestor"], int)[1:] - 1, minlength=s.nodes)
            cum = local["nodesPerStageCumul"]
            assert s.shardInfo()["cut_stage"] == cut == k["chain_stage"], (s.shardInfo(), k)
            assert 2 <= kids[cum[cut - 1]:cum[cut]].max() <= UPCUT_THREADS // lanes_per and lanes_per <= UPCUT_THREADS
            k_local = cum[N] - cum[N - 1]
            assert 2 * k_local < r <= 3 * k_local                       # the split round reaches the third stage from the end

    return p, fc, cut, expect


@pytest.mark.parametrize("exchange", ["optimistic", "exact"])
def test_sharded_up_walk_adds_the_second_partial(exchange):
    """k_up_chain_cut<SPLIT>: two ranks whose cut lies right above the chains, so that the chain
    walks and the cut parents' sums are ONE launch, each shard's OWN node count putting its last round in the split range, three
    stages deep.  The conditions of the merged launch (Ctx::up_cut_lanes) are asserted from the shards."""
    p, fc, cut, expect = sharded_split_problem()
    ref, ohist = reference(("b240", "sharded"), p, fc)
    rk = Ranks(p, 2, cut, optimistic=exchange != "exact")
    try:
        def solve(s):
            s.initialiseSmpcController(*fc)
            s.apgReset()
            return s.apgIterate(ITERS)

        hists = rk.run(solve)
        expect(rk.shards)
        for h in hists:
            assert np.abs(h - ohist).max() <= REL_TOL * np.abs(ohist).max()
        compare("sharded, %s" % exchange, rk.gathered, rk.shards[0], p["tree"], ref, REL_TOL)
    finally:
        rk.close()


def test_sharded_up_walk_with_the_one_shot_exchange():
    """k_up_chain_cut<SPLIT, GATHER>: the same two shards with the one-shot transport, whose merged launch also pushes the cut parents' sums to
    the peer and gathers the peer's.  In a process of its own, as every in-process one-shot run (tests/oneshot_worker.py, `split`): the split
    and the merged launch are asserted from the shards behind each transport's run, the one-shot iterates, histories and batch counters are
    bitwise the stand-in transport's, and both are the oracle's at REL_TOL."""
    from test_gpu_oneshot import run

    out = run(("split",))
    assert "oneshot inprocess ok" in out, out


@pytest.mark.parametrize("knobs", [{"fuse_split": 1}, {"fuse_split": 3}, {"unscaled_walk": 0}])
def test_fused_walk_forms_on_a_split_tree(knobs):
    """the forward walk + dual update in one launch (k_down_chain_dual with 1 and 3 workgroups per chain; optimistic batches of >= 16
    iterations take it) and the walk that applies the preconditioner itself (the knob selects it directly), behind a split streaming
    launch.  Whether the one launch HAPPENED is the sweep's answer to the batch and is not reported; what is asserted is everything
    it depends on -- forced on, an optimistic batch, the stage-tiled dual update, a crown the chain workgroups fold (1 <= chainStage
    <= 8)."""
    p, fc = problem("b236", "three")
    iters = 20
    ref, ohist = reference(("b236", "three"), p, fc, iters)
    s = capi.Solver(p["network"], p["tree"], p["config"], knobs=knobs)
    if "fuse_split" in knobs:
        s.setFusedWalkDual(1)
    s.initialiseSmpcController(*fc)
    expect_split(s, position("three", num_cus())[0])
    hist = s.algorithmApg(iters)
    k, c = s.kernelInfo(), s.counters()
    assert c["optimistic"] == 1 and c["replayed"] == 0 and c["exact"] == 0, c
    assert k["dual_stage"] == 1 and k["dual_pipe"] != 0 and 1 <= k["chain_stage"] <= 8, k
    compare("fused walk %s" % knobs, local_get(s), s, p["tree"], ref, REL_TOL, hist, ohist)
    s.close()


@pytest.mark.parametrize("alg", fbe.ALGS)
def test_quasi_newton_loops_on_a_split_context(alg):
    """global FBE and NAMA: stream_pair_ok() must send NAMA's two Hessian sweeps through two (split) launches instead of the
    two-right-hand-side launch, which exists unsplit only"""
    p, fc = problem("b240", "two")
    o = Oracle(p["network"], p["tree"], p["config"], alias_operators=aliasing(p))
    o.set_algorithm(alg, 5)
    o.initialise(*fc)
    o.fbe_reset()
    s = solver(p, fc)
    s.setAlgorithm(alg, 5)
    expect_split(s, position("two", num_cus())[0])
    iters = 6
    ho, vo, to = o.fbe_nama(iters)
    hs, vs, ts = (s.algorithmGlobalFbe if alg == "globalFbeAlgorithm" else s.algorithmNama)(iters)
    assert np.array_equal(ts, to), (ts, to)
    assert relmax(vs, vo) < REL_TOL
    assert relmax(hs, ho) < 1e-7
    fbe.compare_fbe(s, o, alg, 1e-8, "%s on a split context" % alg)
    c = s.fbeCounters()
    assert c["sweep_pairs"] == 0 and c["sequential"] == 0, c
    expect_split(s, position("two", num_cus())[0])
    s.close()


def test_refactor_by_set_operator_decides_the_split_again():
    """operator_mode auto: structured (no split) until a block is handed in; rn_set_operator then runs the factor step again, which
    must decide the split and allocate my2 again -- from there on the bits of a context that was dense from the start"""
    p, fc = problem("b236", "three")
    ref, ohist = reference(("b236", "three"), p, fc)
    r = position("three", num_cus())[0]
    a, d = solver(p, fc, operator_mode="auto"), solver(p, fc, operator_mode="dense")
    assert a.operatorMode() == ("auto", "structured")
    expect_no_split(a)
    expect_split(d, r)
    a.algorithmApg(ITERS); d.algorithmApg(ITERS)
    node = a.nodes - 2                        # a block of the split round
    a.setOperator(capi.OP_PSI, node, a.getOperator(capi.OP_PSI, node))
    assert a.operatorMode() == ("auto", "dense")
    expect_split(a, r)
    ha, hd = a.algorithmApg(ITERS), d.algorithmApg(ITERS)
    assert np.array_equal(ha, hd)
    for b in ALL_BUFS:
        assert np.array_equal(a.get(b), d.get(b)), b
    compare("after the re-factor", local_get(a), a, p["tree"], ref, REL_TOL, ha, ohist)
    a.close(); d.close()
