"""NAMA's two Hessian sweeps in ONE pass over fp32-stored operator blocks (rn_set_sweep_pairing(RN_PAIR_ON), k_stream_gemv over fp32 storage with two
right-hand sides; the oracles are SmpcController.cu:1331 and :1341-1345).

The contract: the pair is bitwise the two sweeps run one after the other (each right-hand side's sums are formed as the unsplit one-vector
kernel forms them), it is opt-in (RN_PAIR_AUTO, the default, leaves fp32-stored blocks unpaired), and on a context whose streaming launch
has a split last round the pair sweep alone runs unsplit while every other sweep keeps its split -- there the comparison with the
sequential path is to rounding (the split kernel adds its halves in another order), not bitwise.

Shapes, helpers and tolerances are those of test_gpu_operator_storage / test_gpu_fbe_nama / test_gpu_stream_split."""
import ctypes as C
import gc

import numpy as np
import pytest

import test_gpu_fbe_nama as fbe
import test_gpu_stream_split as spl
from rapidnet_amd import capi
from test_gpu_operator_storage import EXTRA, SHAPES, blocks_of, oracle_with_blocks, problem, shape_info, solver  # noqa: F401 (EXTRA: the shapes' source)
from test_gpu_parity import REL_TOL, relmax
from test_gpu_sharded_batched import Ranks

pytestmark = pytest.mark.gpu

NAMA = "namaAlgorithm"
RN_E_ARG = -1
YVECS = (capi.BUF_LBFGS_CUR_YVEC_XI, capi.BUF_LBFGS_CUR_YVEC_PSI, capi.BUF_LBFGS_PREV_YVEC_XI, capi.BUF_LBFGS_PREV_YVEC_PSI)
FBE_BUFS = tuple(b for b, _ in fbe.FBE_PAIRS) + YVECS          # every buffer compare_fbe reads


def pairs_of(s):
    out = (C.c_long * 4)()
    assert s.lib.rn_fbe_counters(s.h, C.addressof(out)) == 0
    return int(out[3])


def nama(p, fc, iters, pairing, storage="f32", knobs=None, keep=False):
    """a context of the problem with the given pairing, NAMA selected, `iters` iterations: what it computed and how"""
    s = solver(p, fc, storage=storage, sweep_pairing=pairing, knobs=knobs)
    s.setAlgorithm(NAMA, 5)
    state = s.sweepPairing()
    h, v, t = s.algorithmNama(iters)
    run = {"hist": h, "values": v, "tau": t, "bufs": {b: s.get(b) for b in FBE_BUFS}, "pairs": pairs_of(s), "state": state, "after": s.sweepPairing()}
    if keep:
        return run, s
    s.close()
    return run


def assert_bitwise(a, b, what):
    assert np.array_equal(a["tau"], b["tau"]), (what, a["tau"], b["tau"])
    assert np.array_equal(a["values"], b["values"]), (what, a["values"], b["values"])
    assert np.array_equal(a["hist"], b["hist"]), (what, a["hist"], b["hist"])
    for bid in FBE_BUFS:
        assert np.array_equal(a["bufs"][bid], b["bufs"][bid]), (what, bid)


def test_shapes_cover_the_pair_kernels_paths():
    """NL and G of every shape: the set must hold more than one slot per thread (NL >= 2) and a ragged last span"""
    seen = {}
    for name in SHAPES:
        p, fc = problem(name)
        s = solver(p, fc, init=False, sweep_pairing="on")
        G, NL, groups, rag = shape_info(s)
        seen[name] = (G, NL, groups, rag)
        print("\n%-7s nodes %4d ny %3d 2nv %3d  G %2d NL %d groups (one vector) %2d ny %% G %2d" % (name, s.nodes, s.ny, 2 * s.nv, G, NL, groups, rag))
        s.close()
    assert any(v[1] >= 2 for v in seen.values()) and any(v[3] != 0 for v in seen.values()), seen


@pytest.mark.parametrize("name", SHAPES)
def test_pair_is_bitwise_the_two_sweeps(name):
    """stream_split = 0 on both contexts: the sequential path's launches are unsplit, so every sum of the pair has a twin formed in the
    same order -- histories, accepted steps and every buffer to the last bit"""
    p, fc = problem(name)
    on = nama(p, fc, 6, "on", knobs={"stream_split": 0})
    off = nama(p, fc, 6, "off", knobs={"stream_split": 0})
    print("\n%s: pairs on %d off %d, tau %s" % (name, on["pairs"], off["pairs"], on["tau"]))
    assert on["state"] == ("on", 1) and on["after"] == ("on", 1), on["state"]
    assert off["state"] == ("off", 0) and off["after"] == ("off", 0), off["state"]
    assert on["pairs"] > 0 and off["pairs"] == 0, (on["pairs"], off["pairs"])
    assert_bitwise(on, off, name)


def test_pair_against_the_oracle_on_the_same_blocks():
    p, fc = problem("small")
    iters = 8
    run, s = nama(p, fc, iters, "on", keep=True)
    o = oracle_with_blocks(p, fc, blocks_of(s), alg=NAMA)
    ho, vo, to = o.fbe_nama(iters)
    assert run["pairs"] > 0 and run["state"] == ("on", 1)
    assert np.array_equal(run["tau"], to), (run["tau"], to)
    assert relmax(run["values"], vo) < REL_TOL
    assert relmax(run["hist"], ho) < REL_TOL
    fbe.compare_fbe(s, o, NAMA, REL_TOL, "paired NAMA on fp32 blocks")
    s.close()


@pytest.mark.parametrize("storage,pairing", [("f32", "on"), ("native", "auto")])
def test_pair_under_the_profiler_runs_its_halves_in_turn(storage, pairing):
    """While rn_profile_enable is set every interval is bracketed on the context's one stream: the second right-hand side's steps run BEHIND
    the first's, on the first's scratch set, instead of beside them on a stream of their own.  Same kernels, same inputs: bitwise the
    pair of a context that is not profiled, and the oracle's iterates on the same blocks at REL_TOL."""
    p, fc = problem("small")
    iters, runs = 6, {}
    for prof in (0, 1):
        s = solver(p, fc, storage=storage, sweep_pairing=pairing)
        s.setAlgorithm(NAMA, 5)
        s.profileEnable(prof)
        h, v, t = s.algorithmNama(iters)
        s.profileEnable(0)
        runs[prof] = {"hist": h, "values": v, "tau": t, "bufs": {b: s.get(b) for b in FBE_BUFS}, "pairs": pairs_of(s)}
        if prof:
            o = oracle_with_blocks(p, fc, blocks_of(s), alg=NAMA)
            ho, vo, to = o.fbe_nama(iters)
            assert np.array_equal(t, to), (t, to)
            assert relmax(v, vo) < REL_TOL and relmax(h, ho) < REL_TOL
            fbe.compare_fbe(s, o, NAMA, REL_TOL, "paired NAMA under the profiler, %s blocks" % storage)
        s.close()
    assert runs[0]["pairs"] > 0 and runs[1]["pairs"] == runs[0]["pairs"], (runs[0]["pairs"], runs[1]["pairs"])
    assert_bitwise(runs[1], runs[0], "profiled pair, %s blocks" % storage)


def test_pair_on_a_context_with_a_split_last_round():
    """the context's APG launch is split; the pair sweep runs unsplit and leaves the split state alone"""
    p, fc = spl.problem("b236", "three")
    r = spl.position("three", spl.num_cus())[0]
    on, s = nama(p, fc, 4, "on", keep=True)
    spl.expect_split(s, r, "b236 three fp32 storage, pairing on")      # still split after the loop
    assert on["state"] == ("on", 1) and on["pairs"] > 0, (on["state"], on["pairs"])
    off, so = nama(p, fc, 4, "off", keep=True)
    spl.expect_split(so, r, "b236 three fp32 storage, pairing off")
    assert off["pairs"] == 0
    so.close()
    if not np.array_equal(on["tau"], off["tau"]):
        print("\nvalue histories: on %s\n                 off %s" % (on["values"], off["values"]))
    assert np.array_equal(on["tau"], off["tau"]), (on["tau"], off["tau"])
    worst = {bid: relmax(on["bufs"][bid], off["bufs"][bid]) for bid in FBE_BUFS}
    print("\npair (unsplit) against two split sweeps: values %.1e history %.1e worst buffer %.1e" %
          (relmax(on["values"], off["values"]), relmax(on["hist"], off["hist"]), max(worst.values())))
    assert relmax(on["values"], off["values"]) < REL_TOL and relmax(on["hist"], off["hist"]) < REL_TOL
    assert not {k: v for k, v in worst.items() if v > REL_TOL}, worst
    # the APG sweeps of the context that paired: bit for bit those of a context that never did
    s.setAlgorithm("proximalAlgorithm")
    hist = s.algorithmApg(spl.ITERS)
    spl.expect_split(s, r)
    fresh = solver(p, fc, sweep_pairing="off")
    spl.expect_split(fresh, r)
    href = fresh.algorithmApg(spl.ITERS)
    assert np.array_equal(hist, href)
    for b in spl.ALL_BUFS:
        assert np.array_equal(s.get(b), fresh.get(b)), b
    s.close(); fresh.close()


def test_defaults_are_unchanged():
    p, fc = problem("small")
    lib = capi.load()
    # the default: fp32-stored blocks do not pair, native blocks do
    for storage, paired in (("f32", False), ("native", True)):
        s = solver(p, fc, storage=storage)
        assert s.sweepPairing() == ("auto", 0)                # NAMA not selected yet
        s.setAlgorithm(NAMA, 5)
        assert s.sweepPairing() == ("auto", 1 if paired else 0)
        s.algorithmNama(6)
        n = pairs_of(s)
        assert (n > 0) == paired, (storage, n)
        # errors; the setting at any time: the buffers come with the call when NAMA is selected already
        assert lib.rn_set_sweep_pairing(s.h, 7) == RN_E_ARG and lib.rn_set_sweep_pairing(s.h, -1) == RN_E_ARG
        assert s.sweepPairing()[0] == "auto"
        if storage == "f32":
            assert lib.rn_set_sweep_pairing(s.h, capi.PAIR_ON) == 0 and s.sweepPairing() == ("on", 1)
            s.algorithmNama(6)
            assert pairs_of(s) > n
        assert lib.rn_set_sweep_pairing(s.h, capi.PAIR_OFF) == 0 and s.sweepPairing() == ("off", 0)
        n = pairs_of(s)
        s.algorithmNama(6)
        assert pairs_of(s) == n
        s.close()
    # the knob that forces the sequential path wins over RN_PAIR_ON
    run = nama(p, fc, 6, "on", knobs={"nama_pair": 0})
    assert run["pairs"] == 0 and run["state"] == ("on", 0), run["state"]


def test_sharded_contexts_stay_unpaired():
    p, fc = problem("medium")
    rk = Ranks(p, 3, 2)
    try:
        for s in rk.shards:
            assert s.lib.rn_set_operator_storage(s.h, capi.STORE_F32) == 0
            assert s.lib.rn_set_sweep_pairing(s.h, capi.PAIR_ON) == 0
            s.setAlgorithm(NAMA, 5)
            assert s.sweepPairing() == ("on", 0)
    finally:
        rk.close()


@pytest.mark.parametrize("name", ["ragged", "tall"])
def test_pair_under_the_buffer_guard(monkeypatch, name):
    """RAPIDNET_GUARD=1: every buffer between red zones and NaN at first -- a read outside a block or of a pair buffer nobody wrote would
    carry a NaN into the iterates, a write outside a buffer changes a red zone"""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    p, fc = problem(name)
    run, s = nama(p, fc, 6, "on", knobs={"stream_split": 0}, keep=True)
    assert run["pairs"] > 0 and run["state"] == ("on", 1)
    assert np.isfinite(run["hist"]).all() and np.isfinite(run["values"]).all() and np.isfinite(run["tau"]).all()
    for bid in FBE_BUFS:
        assert np.isfinite(run["bufs"][bid]).all(), bid
    assert s.guardCheck() == 0
    s.close()
    after = capi.guard_report()
    assert after[0] == before[0] + 1 and after[1] == before[1], (before, after)
