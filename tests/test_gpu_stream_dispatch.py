"""Every instantiation of k_stream_gemv is reached by the launch that should reach it.

The host picks the kernel from (block storage, two workgroups per CU or one, one right-hand side or two, NL) in one selector
(Ctx::stream_kernel).  These cases walk that whole table -- the three forms {fp64, fp32, fp64 iterates over fp32-stored blocks} x NL = 1 .. 4 x
{SPLIT = false, SPLIT = true, NR = 2} -- and hold each launch to what the project holds that kernel to elsewhere: a selector that hands back a
neighbouring instantiation walks a block with the wrong slot count, group depth or element size, and none of that survives REL_TOL.

NR = 1: one step from a non-trivial dual and a short APG run against the fp64 oracle (for fp32 storage the oracle holds the context's own
blocks), at REL_TOL, the fp32 context at FP32_TOL: test_gpu_operator_storage.test_parity_with_the_oracle_on_the_same_blocks, per form and knob.
NR = 2: NAMA with its pair of Hessian sweeps in one pass, bitwise the run with RN_PAIR_OFF (test_gpu_sweep_pairing, test_gpu_fbe_nama).

Shapes: `small`, `medium`, `tall` are NL = 1, 2, 3 in every form; `wide4` (nv = 386, ny = 412, 5 nodes) is NL = 4 in every form -- fp64 G = 4,
4-byte blocks G = 8 -- and its paired fp32-storage launch needs 105 408 B of LDS plus the mask: the launch behind the function attribute."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from test_gpu_operator_storage import blocks_of, oracle_with_blocks
from test_gpu_parity import FP32_TOL, PAIRS, REL_TOL, relmax
from test_gpu_sweep_pairing import FBE_BUFS, NAMA, assert_bitwise, pairs_of

pytestmark = pytest.mark.gpu

EXTRA = {"wide4": (33, 8, 396, 40, 10, 3, [2])}      # (seed index, nx, nu, nd, ne, N, branching)
NL_OF = {"small": 1, "medium": 2, "tall": 3, "wide4": 4}
G_OF = {("wide4", 8): 4, ("wide4", 4): 8}               # (shape, bytes of a stored block entry): columns per span
# form: (precision, operator storage, tolerance against the fp64 oracle, pairing that pairs it)
FORMS = {"f64": ("f64", "native", REL_TOL, "auto"), "f32": ("f32", "native", FP32_TOL, "auto"), "f64_store32": ("f64", "f32", REL_TOL, "on")}
ITERS = 10

_PROBLEMS, _REFS = {}, {}


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


def duals(o):
    """the non-trivial duals of the one step (test_gpu_parity.test_stepwise_known_answer)"""
    rng = np.random.default_rng(7)
    nxi, nps = o.nodes * 2 * o.nx, o.nodes * o.nu
    return [rng.standard_normal(n) * 50 for n in (nxi, nps, nxi, nps)]


def reference(name, blocks=None):
    """what the fp64 oracle computes on the shape -- with its own blocks, or with `blocks` (a context's fp32-stored ones): computed once per
    shape and kind of blocks, and read only from then on"""
    key = (name, blocks is not None)
    if key not in _REFS:
        p, fc = problem(name)
        if blocks is None:
            o = Oracle(p["network"], p["tree"], p["config"])
            o.initialise(*fc)
        else:
            o = oracle_with_blocks(p, fc, blocks)
        for nm, v in zip(("xi", "psi", "updXi", "updPsi"), duals(o)):
            o.set(nm, v)
        o.extrapolate(0.618); o.solve_step(); o.prox(); o.residual(); o.dual_update()
        ref = {"step": {nm: o.get(nm).copy() for _, nm in PAIRS}, "infeasibility": o.primal_infeasibility()}
        ref["hist"] = o.apg(ITERS).copy()
        ref["apg"] = {nm: o.get(nm).copy() for _, nm in PAIRS}
        ref["blocks"] = blocks
        _REFS[key] = ref
    elif blocks is not None:      # the same rounding of the same blocks, whichever kernel the context runs
        for nm, b in blocks.items():
            assert np.array_equal(b, _REFS[key]["blocks"][nm]), nm
    return _REFS[key]


def context(name, form, **kw):
    p, fc = problem(name)
    precision, storage = FORMS[form][:2]
    s = capi.Solver(p["network"], p["tree"], p["config"], precision=precision, operator_storage=storage, **kw)
    s.initialiseSmpcController(*fc)
    k = s.kernelInfo()
    elem = 4 if "32" in form else 8
    print("\n%s %s: G %d NL %d, %d nodes, ny %d, 2nv %d" % (name, form, k["stream_G"], k["stream_NL"], s.nodes, s.ny, 2 * s.nv))
    assert k["stream_NL"] == NL_OF[name], k
    assert k["stream_G"] == G_OF.get((name, elem), k["stream_G"]), k
    assert s.operatorStorage()[1] == ("f32" if elem == 4 else "native"), s.operatorStorage()      # (active: the fp32 context's own blocks are fp32)
    return s


def compare(s, ref, tol, what):
    worst = {nm: relmax(s.get(bid), ref[nm]) for bid, nm in PAIRS}
    print("%s: worst %.2e (%s)" % (what, max(worst.values()), max(worst, key=worst.get)))
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, "%s mismatch vs oracle: %s" % (what, bad)


@pytest.mark.parametrize("two_per_cu", [0, 1])
@pytest.mark.parametrize("name", list(NL_OF))
@pytest.mark.parametrize("form", list(FORMS))
def test_one_right_hand_side(form, name, two_per_cu):
    """SPLIT = false (one workgroup per CU) and SPLIT = true (two) of every NL and form"""
    tol = FORMS[form][2]
    s = context(name, form, knobs={"stream_two_per_cu": two_per_cu})
    assert s.streamInfo()["twoPerCU"] == two_per_cu, s.streamInfo()
    ref = reference(name, blocks_of(s) if FORMS[form][1] == "f32" else None)
    vals = duals(s)
    for bid, v in zip((capi.BUF_XI, capi.BUF_PSI, capi.BUF_UPD_XI, capi.BUF_UPD_PSI), vals):
        s.set(bid, v)
    s.dualExtrapolationStep(0.618); s.solveStep(); s.proximalFunG(); s.computeFixedPointResidual(); s.dualUpdate()
    compare(s, ref["step"], tol, "%s %s two per CU %d, one step" % (name, form, two_per_cu))
    assert abs(s.updatePrimalInfeasibity() - ref["infeasibility"]) <= tol * abs(ref["infeasibility"])
    hist = s.algorithmApg(ITERS)
    compare(s, ref["apg"], tol, "%s %s two per CU %d, %d iterations" % (name, form, two_per_cu, ITERS))
    print("history: %.2e" % (np.abs(hist - ref["hist"]).max() / np.abs(ref["hist"]).max()))
    assert np.abs(hist - ref["hist"]).max() <= tol * np.abs(ref["hist"]).max()
    s.close()


def nama(name, form, pairing, iters=6):
    s = context(name, form, sweep_pairing=pairing)
    s.setAlgorithm(NAMA, 5)
    state = s.sweepPairing()      # rn_get_sweep_pairing: (requested, active)
    h, v, t = s.algorithmNama(iters)
    run = {"hist": h, "values": v, "tau": t, "bufs": {b: s.get(b) for b in FBE_BUFS}, "pairs": pairs_of(s), "state": state}
    s.close()
    return run


@pytest.mark.parametrize("name", list(NL_OF))
@pytest.mark.parametrize("form", list(FORMS))
def test_two_right_hand_sides(form, name):
    """NR = 2 of every NL and form: the NAMA loop with its two Hessian sweeps in one pass, bitwise the loop that runs them one after the other"""
    pairing = FORMS[form][3]
    on, off = nama(name, form, pairing), nama(name, form, "off")
    print("%s %s: pairs %d | %d, tau %s" % (name, form, on["pairs"], off["pairs"], on["tau"]))
    assert on["state"] == (pairing, 1), on["state"]
    assert off["state"] == ("off", 0), off["state"]
    assert on["pairs"] > 0 and off["pairs"] == 0, (on["pairs"], off["pairs"])
    assert_bitwise(on, off, "%s %s" % (name, form))
