"""Dense operator blocks stored in fp32 under fp64 iterates (rn_set_operator_storage(RN_STORE_F32), k_stream_gemv<double, ..., float>).

The contract: an fp64 context with fp32 block storage computes the fp64 solution of the problem WITH THE ROUNDED BLOCKS.  So the
reference of the parity tests is the fp64 oracle holding the context's own blocks: every per-node block (Phi, Psi, D, Ftil) is read
back with rn_get_operator and written into the oracle's arrays (Oracle.buf is a view), and from there on the tolerance is REL_TOL,
the fp64 tolerance of test_gpu_parity.  Taking the blocks from the context instead of rounding the oracle's own keeps an entry from
landing on the neighbouring float because the two factor steps differ by 1e-12.  The distance from the UNROUNDED problem is a test
of its own, at FP32_TOL.

Shapes: the smallest that reach each path of the kernel (the set's properties are asserted in test_shapes_cover_the_kernels_paths);
`even4` is Barcelona's operator width on a 5-node tree with ny = 320: 20 spans of 16 columns = 4 groups."""
import ctypes as C
import gc

import numpy as np
import pytest

import test_gpu_fbe_nama as fbe
import test_gpu_stream_split as spl
from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from test_gpu_parity import FP32_TOL, PAIRS, REL_TOL, compare_all, relmax
from test_gpu_sharded_batched import Ranks

pytestmark = pytest.mark.gpu

OPS = ((capi.OP_PHI, "Phi"), (capi.OP_D, "D"), (capi.OP_PSI, "Psi"), (capi.OP_F, "Ftil"))
SHAPES = ["tiny", "odd", "medium", "tall", "ragged", "even4"]
EXTRA = {"even4": (31, 103, 114, 88, 17, 3, [2])}      # (seed index, nx, nu, nd, ne, N, branching): nv = 97, ny = 320
STREAM_D, STREAM_D_WIDE = 5, 3                          # RN_STREAM_D, RN_STREAM_D_WIDE (csrc/common.hpp)
ITERS = 25
RN_E_ARG, RN_E_STATE = -1, -3

_PROBLEMS = {}


def problem(name):
    if name not in _PROBLEMS:
        if name in EXTRA:
            synth.CONFIGS[name] = EXTRA[name]
            try:
                p = synth.make_problem(name)
            finally:
                del synth.CONFIGS[name]
        else:
            p = synth.make_problem(name)
        _PROBLEMS[name] = (p, synth.forecast_at(p["forecast"], 0))
    return _PROBLEMS[name]


def solver(p, fc, storage="f32", init=True, **kw):
    s = capi.Solver(p["network"], p["tree"], p["config"], operator_storage=storage, **kw)
    if init:
        s.initialiseSmpcController(*fc)
    return s


def op_dims(s):
    return {"Phi": s.nv * 2 * s.nx, "D": s.nv * 2 * s.nx, "Psi": s.nv * s.nu, "Ftil": s.nv * s.nu}


def blocks_of(s):
    """{name: [nodes][dim]} every per-node block as the context stores it"""
    d = op_dims(s)
    return {nm: np.stack([s.getOperator(op, node) for node in range(s.nodes)]).reshape(s.nodes, d[nm]) for op, nm in OPS}


def oracle_with_blocks(p, fc, blocks, nodes_of=None, alias=True, alg=None):
    """the fp64 oracle of the problem, initialised, with its per-node blocks overwritten by `blocks` (rows nodes_of: global node ids)"""
    o = Oracle(p["network"], p["tree"], p["config"], alias_operators=alias)
    if alg:
        o.set_algorithm(alg, 5)
    o.initialise(*fc)
    for nm, b in blocks.items():
        view = o.buf(nm).reshape(o.nodes, b.shape[1])
        if nodes_of is None:
            view[:] = b
        else:
            view[np.asarray(nodes_of, int)] = b
    if alg:
        o.fbe_reset()
    return o


def shape_info(s):
    k = s.kernelInfo()
    G, NL = k["stream_G"], k["stream_NL"]
    D = STREAM_D if NL <= 2 else STREAM_D_WIDE
    return G, NL, (s.ny // G) // D, s.ny % G


def test_shapes_cover_the_kernels_paths():
    """G, NL and the group count of every shape with fp32 storage; the set must hold a block shorter than one group (the prologue's
    clamp), an odd and an even (>= 4) number of groups (both tails of the double-buffered loop), a ragged last span, a padded slot
    (2 nv no multiple of four) and more than one slot per thread"""
    seen = {}
    for name in SHAPES:
        p, fc = problem(name)
        s = solver(p, fc, init=False)
        G, NL, groups, rag = shape_info(s)
        seen[name] = (G, NL, groups, rag, 2 * s.nv % 4)
        print("\n%-7s nodes %4d ny %3d 2nv %3d  G %2d NL %d groups %2d ny %% G %2d" % (name, s.nodes, s.ny, 2 * s.nv, G, NL, groups, rag))
        s.close()
    gr = [v[2] for v in seen.values()]
    assert 0 in gr and any(g % 2 == 1 for g in gr) and any(g % 2 == 0 and g >= 4 for g in gr), seen
    assert any(v[3] != 0 for v in seen.values()) and any(v[1] >= 2 for v in seen.values()) and any(v[4] != 0 for v in seen.values()), seen
    assert seen["tiny"][2] == 0 and seen["tall"][2] >= 5, seen


@pytest.mark.parametrize("name", SHAPES)
def test_parity_with_the_oracle_on_the_same_blocks(name):
    p, fc = problem(name)
    s = solver(p, fc)
    assert s.operatorStorage() == ("f32", "f32")
    print("\n%s: G %d NL %d groups %d ragged %d" % ((name,) + shape_info(s)))
    o = oracle_with_blocks(p, fc, blocks_of(s))
    # step-wise, from a non-trivial dual (test_gpu_parity.test_stepwise_known_answer)
    rng = np.random.default_rng(7)
    nxi, nps = o.nodes * 2 * o.nx, o.nodes * o.nu
    for bx, bp, ox, op_ in ((capi.BUF_XI, capi.BUF_PSI, "xi", "psi"), (capi.BUF_UPD_XI, capi.BUF_UPD_PSI, "updXi", "updPsi")):
        vx, vp = rng.standard_normal(nxi) * 50, rng.standard_normal(nps) * 50
        s.set(bx, vx); s.set(bp, vp); o.set(ox, vx); o.set(op_, vp)
    s.dualExtrapolationStep(0.618); o.extrapolate(0.618)
    s.solveStep(); o.solve_step()
    s.proximalFunG(); o.prox()
    s.computeFixedPointResidual(); o.residual()
    s.dualUpdate(); o.dual_update()
    w = compare_all(s, o, REL_TOL, "%s, one step" % name)
    print("one step: worst %.1e" % max(w.values()))
    assert abs(s.updatePrimalInfeasibity() - o.primal_infeasibility()) <= REL_TOL * abs(o.primal_infeasibility())
    # device-resident iterations
    hist, ohist = s.algorithmApg(ITERS), o.apg(ITERS)
    w = compare_all(s, o, REL_TOL, "%s, %d iterations" % (name, ITERS))
    print("%d iterations: worst %.1e, history %.1e" % (ITERS, max(w.values()), np.abs(hist - ohist).max() / np.abs(ohist).max()))
    assert np.abs(hist - ohist).max() <= REL_TOL * np.abs(ohist).max()
    s.close()


@pytest.mark.parametrize("name", ["odd", "medium"])
def test_stored_blocks_are_what_was_promised(name):
    p, fc = problem(name)
    s, n = solver(p, fc), solver(p, fc, storage="native")
    assert n.operatorStorage() == ("native", "native")
    bs, bn = blocks_of(s), blocks_of(n)
    for nm in bs:
        v, ref = bs[nm], bn[nm]
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), nm                 # fp32-representable
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert (np.abs(v - ref) <= ulp).all(), (nm, float((np.abs(v - ref) / ulp).max()))     # within one fp32 ulp of the fp64 block
    rng = np.random.default_rng(3)
    for op, nm in OPS:
        node = s.nodes // 2
        x = bn[nm][node] * (1.0 + 0.3 * rng.standard_normal(bn[nm].shape[1]))
        s.setOperator(op, node, x)
        assert np.array_equal(s.getOperator(op, node), x.astype(np.float32).astype(np.float64)), nm
        other = s.getOperator(op, node - 1)
        assert np.array_equal(other, bs[nm][node - 1]), nm                                     # the neighbour is untouched
    s.close(); n.close()


@pytest.mark.parametrize("net,pos", [("b236", "three"), ("nv129", "two")])
def test_split_last_round(net, pos):
    """a tree of numCUs + r nodes: the second workgroup of a split block and my2, stage by stage against the oracle on the same blocks;
    split on against split off on the stages above the split"""
    p, fc = spl.problem(net, pos)
    r = spl.position(pos, spl.num_cus())[0]
    got, o = [], None
    for split in (1, 0):
        s = solver(p, fc, knobs={"stream_split": split})
        if split:
            info, k, groups = spl.expect_split(s, r, "%s %s fp32 storage" % (net, pos))
            o = oracle_with_blocks(p, fc, blocks_of(s), alias=spl.aliasing(p))
            o.apg(3)
            acc = o.get("accXi"), o.get("accPsi")
            o.solve_step()
            oref = {nm: o.get(nm) for nm in ("x", "u", "v", "primalXi", "primalPsi")}
            ohist = o.apg(spl.ITERS)
            ref = {nm: o.get(nm) for nm, _, _ in spl.VECS}
        else:
            spl.expect_no_split(s)
            assert s.streamInfo()["twoPerCU"] == 1
        assert s.operatorStorage() == ("f32", "f32")
        s.set(capi.BUF_ACC_XI, acc[0]); s.set(capi.BUF_ACC_PSI, acc[1])
        s.solveStep()
        spl.compare("one step, split %d" % split, spl.local_get(s), s, p["tree"], oref, REL_TOL)
        got.append({"primalXi": s.get(capi.BUF_PRIMAL_XI), "primalPsi": s.get(capi.BUF_PRIMAL_PSI)})
        hist = s.algorithmApg(spl.ITERS)
        spl.compare("%d iterations, split %d" % (spl.ITERS, split), spl.local_get(s), s, p["tree"], ref, REL_TOL, hist, ohist)
        s.close()
    first = spl.stage_of(p["tree"], spl.num_cus())
    assert first >= 1
    nx, nu = int(p["network"]["nx"][0]), int(p["network"]["nu"][0])
    for nm, dim in (("primalXi", 2 * nx), ("primalPsi", nu)):
        e = spl.stage_errors(got[0][nm], got[1][nm], p["tree"], dim)[:first]
        print("split on against off, %s, stages < %d: %.1e" % (nm, first, e.max()))
        assert e.max() <= REL_TOL, (nm, e)


def test_distance_from_the_unrounded_problem():
    """the same context against the UNMODIFIED fp64 oracle: the rounding of the blocks moves the iterates by far less than the fp32
    context's arithmetic does (both printed; DESIGN.md section 4 quotes them)"""
    p, fc = problem("medium")
    o = Oracle(p["network"], p["tree"], p["config"])
    o.initialise(*fc)
    ohist = o.apg(ITERS)
    errs = {}
    for tag, kw in (("f64 + fp32 blocks", {"operator_storage": "f32"}), ("f32 context", {"precision": "f32"})):
        s = capi.Solver(p["network"], p["tree"], p["config"], **kw)
        s.initialiseSmpcController(*fc)
        hist = s.algorithmApg(ITERS)
        w = {nm: relmax(s.get(bid), o.get(nm)) for bid, nm in PAIRS}
        errs[tag] = (max(w.values()), float(np.abs(hist - ohist).max() / np.abs(ohist).max()))
        s.close()
    print("\nmedium, %d iterations, against the unmodified fp64 oracle (worst vector, history): %s" % (ITERS, {k: "%.2e, %.2e" % v for k, v in errs.items()}))
    assert errs["f64 + fp32 blocks"][0] < FP32_TOL and errs["f64 + fp32 blocks"][1] < FP32_TOL, errs


def block_bytes(s, elem):
    """bytes of the dense blocks as the library lays them out: LD = 2 nv in whole 16-byte slots, node stride in whole 128-byte lines"""
    per16, per128 = 16 // elem, 128 // elem
    LD = -(-2 * s.nv // per16) * per16
    stride = -(-s.ny * LD // per128) * per128
    return s.nodes * stride * elem


def test_modes_and_state():
    p, fc = problem("medium")
    lib = capi.load()
    # requested / active under the three operator modes
    d, st, a = (solver(p, fc, operator_mode=m) for m in ("dense", "structured", "auto"))
    n = solver(p, fc, storage="native", operator_mode="dense")
    fresh = solver(p, fc, init=False, operator_mode="dense")
    assert fresh.operatorStorage() == ("f32", "native")                      # no blocks yet
    assert d.operatorStorage() == ("f32", "f32") and st.operatorStorage() == ("f32", "native") and a.operatorStorage() == ("f32", "native")
    assert n.operatorStorage() == ("native", "native")
    f32 = capi.Solver(p["network"], p["tree"], p["config"], precision="f32", operator_storage="f32", operator_mode="dense")
    f32.initialiseSmpcController(*fc)
    assert f32.operatorStorage() == ("f32", "f32")
    f32.close()
    # errors
    assert lib.rn_set_operator_storage(fresh.h, 7) == RN_E_ARG and lib.rn_set_operator_storage(fresh.h, -1) == RN_E_ARG
    assert lib.rn_set_operator_storage(fresh.h, capi.STORE_NATIVE) == 0 and fresh.operatorStorage() == ("native", "native")
    assert lib.rn_set_operator_storage(fresh.h, capi.STORE_F32) == 0
    for s in (d, st, a):
        assert lib.rn_set_operator_storage(s.h, capi.STORE_F32) == RN_E_STATE and lib.rn_set_operator_storage(s.h, capi.STORE_NATIVE) == RN_E_STATE
    # bytes: the blocks at 4, the vectors at 8; the context holds half the blocks' bytes less
    bwd, dual = d.algorithmicBytes()
    assert bwd == d.nodes * (2 * d.nv * d.ny * 4 + (d.ny + 2 * d.nv + d.nx) * 8)
    assert n.algorithmicBytes() == (d.nodes * (2 * d.nv * d.ny + d.ny + 2 * d.nv + d.nx) * 8, dual)
    assert st.algorithmicBytes()[0] == 0
    own_d, own_n = d.deviceMemoryInfo()["context_bytes"], n.deviceMemoryInfo()["context_bytes"]
    assert own_n - own_d == block_bytes(d, 8) - block_bytes(d, 4) > 0.49 * block_bytes(d, 8), (own_n, own_d, block_bytes(d, 8), block_bytes(d, 4))
    # two runs give identical bits; the structured context is the structured context
    d2 = solver(p, fc, operator_mode="dense")
    h1, h2 = d.algorithmApg(ITERS), d2.algorithmApg(ITERS)
    assert np.array_equal(h1, h2)
    for bid, _ in PAIRS:
        assert np.array_equal(d.get(bid), d2.get(bid))
    # AUTO: active with the first block handed in, and from then on the bits of the context that was dense from the start
    a.algorithmApg(ITERS)
    node = a.nodes // 2
    a.setOperator(capi.OP_PSI, node, a.getOperator(capi.OP_PSI, node))
    assert a.operatorMode() == ("auto", "dense") and a.operatorStorage() == ("f32", "f32")
    blk = a.getOperator(capi.OP_PSI, node)
    assert np.array_equal(blk.astype(np.float32).astype(np.float64), blk) and np.array_equal(blk, d.getOperator(capi.OP_PSI, node))
    ha = a.algorithmApg(ITERS)
    assert np.array_equal(ha, h1)
    for bid, _ in PAIRS:
        assert np.array_equal(a.get(bid), d.get(bid))
    assert a.algorithmicBytes() == d.algorithmicBytes()
    for s in (d, d2, st, a, n, fresh):
        s.close()


@pytest.mark.parametrize("alg", fbe.ALGS)
def test_quasi_newton_loops(alg):
    """global FBE and NAMA on fp32 blocks: the two Hessian sweeps of NAMA run one after the other (no two-right-hand-side pass)"""
    p, fc = problem("small")
    s = solver(p, fc)
    s.setAlgorithm(alg, 5)
    o = oracle_with_blocks(p, fc, blocks_of(s), alg=alg)
    iters = 8      # (as test_gpu_operator_mode's quasi-Newton case)
    ho, vo, to = o.fbe_nama(iters)
    hs, vs, ts = (s.algorithmGlobalFbe if alg == "globalFbeAlgorithm" else s.algorithmNama)(iters)
    assert np.array_equal(ts, to), (ts, to)
    assert relmax(vs, vo) < REL_TOL
    assert relmax(hs, ho) < REL_TOL
    fbe.compare_fbe(s, o, alg, REL_TOL, "%s on fp32 blocks" % alg)
    out = (C.c_long * 4)()
    assert s.lib.rn_fbe_counters(s.h, C.addressof(out)) == 0
    assert out[3] == 0 and s.fbeCounters()["sequential"] == 0, list(out)
    assert s.operatorStorage() == ("f32", "f32")
    s.close()


def test_three_ranks_through_the_stand_in():
    p, fc = problem("medium")
    rk = Ranks(p, 3, 2)
    try:
        for s in rk.shards:
            assert s.lib.rn_set_operator_storage(s.h, capi.STORE_F32) == 0      # after rn_create_sharded, before the factor step

        def solve(s):
            s.initialiseSmpcController(*fc)
            s.apgReset()
            return np.concatenate([s.apgIterate(20), s.apgIterate(ITERS - 20)])

        hists = rk.run(solve)
        o = Oracle(p["network"], p["tree"], p["config"])
        o.initialise(*fc)
        for s in rk.shards:
            assert s.operatorStorage() == ("f32", "f32")
            for nm, b in blocks_of(s).items():
                o.buf(nm).reshape(o.nodes, b.shape[1])[np.asarray(s.global_nodes, int)] = b
        ohist = o.apg(ITERS)
        for h in hists:
            assert np.array_equal(h, hists[0]) and np.abs(h - ohist).max() <= REL_TOL * np.abs(ohist).max()
        d = spl.dims_of(rk.shards[0])
        for nm, bid, dm in spl.VECS:
            assert relmax(rk.gathered(bid, d[dm]), o.get(nm)) < REL_TOL, nm
    finally:
        rk.close()


@pytest.mark.parametrize("name", ["odd", "tall"])
def test_under_the_buffer_guard(monkeypatch, name):
    """RAPIDNET_GUARD=1: the fp32 block buffer sits between red zones and starts as NaN like every other buffer -- a read outside a
    block (the clamped first group, the idle slots, the padded tail of a column) would carry a NaN into the iterates, a write outside
    a buffer changes a red zone"""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    p, fc = problem(name)
    s = solver(p, fc)
    o = oracle_with_blocks(p, fc, blocks_of(s))
    hist, ohist = s.algorithmApg(ITERS), o.apg(ITERS)
    compare_all(s, o, REL_TOL, "%s under the guard" % name)                  # (relmax asserts finiteness)
    assert np.isfinite(hist).all() and np.abs(hist - ohist).max() <= REL_TOL * np.abs(ohist).max()
    assert s.guardCheck() == 0
    s.close()
    after = capi.guard_report()
    assert after[0] == before[0] + 1 and after[1] == before[1], (before, after)
