"""The wide network (200 states, 360 inputs, nv = 306) in fp64 on the 256-scenario tree (5 649 nodes, ~20 GB of fp64 blocks), dense
and structured, against the block-free fp64 oracle (Oracle(..., lazy_operators=True)), stage by stage.

This is the first fp64 run of the wide network at a size where the library picks its own launch shapes: the streaming kernel's
span for 2 448-byte columns, the lean MFMA loop or the multi-slab kernel, the fused walk.  kernelInfo() is printed so that the
choice is visible in the test log.  The error is measured per stage (tests/stagewise.py): the dual-side vectors carry sqrt(p_i),
1/16 at the leaves of this tree, and a global relmax would dilute a leaf-stage error by as much."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from stagewise import worst_by_buffer

pytestmark = pytest.mark.gpu
ITERS = 25
STAGE_TOL = 1e-9
PAIRS = {"x": capi.BUF_X, "u": capi.BUF_U, "v": capi.BUF_V, "xi": capi.BUF_XI, "psi": capi.BUF_PSI, "accXi": capi.BUF_ACC_XI,
         "accPsi": capi.BUF_ACC_PSI, "updXi": capi.BUF_UPD_XI, "updPsi": capi.BUF_UPD_PSI, "primalXi": capi.BUF_PRIMAL_XI,
         "primalPsi": capi.BUF_PRIMAL_PSI, "dualXi": capi.BUF_DUAL_XI, "dualPsi": capi.BUF_DUAL_PSI, "resXi": capi.BUF_RES_XI,
         "resPsi": capi.BUF_RES_PSI}


def oracle_run(p, iters):
    """the lazy fp64 oracle after iters APG iterations: (buffers, history, iterations in which both soft thresholds tripped)"""
    dh, ah = synth.forecast_at(p["forecast"], 0)
    o = Oracle(p["network"], p["tree"], p["config"], lazy_operators=True)
    o.initialise(dh, ah)
    lam = p["config"]["stepSize"][0]
    gx, gs = p["config"]["penaltyStateX"][0] / lam, p["config"]["penaltySafetyX"][0] / lam
    o.apg_reset()
    th, hist, both = [1.0, 1.0], [], 0
    for _ in range(iters):
        th = o.apg_continue(1, th)
        hist.append(o.primal_infeasibility())
        dx, ds = o.dist()
        both += int(dx > gx and ds > gs)
    return {nm: o.get(nm) for nm in PAIRS}, np.array(hist), both


@pytest.fixture(scope="module")
def wide256():
    p = synth.make_problem("wide256")
    return p, oracle_run(p, ITERS)


def check(tag, s, p, ref, ohist, hist):
    w = worst_by_buffer({nm: s.get(bid) for nm, bid in PAIRS.items()}, ref, p["tree"], s.nx, s.nu, s.nv)
    print("\n%s kernelInfo %s\n%s worst per-stage error against the lazy fp64 oracle: %s"
          % (tag, s.kernelInfo(), tag, {k: "%.1e" % v for k, v in w.items()}))
    assert max(w.values()) <= STAGE_TOL, (tag, w)
    assert np.abs(hist - ohist).max() <= 1e-9 * np.abs(ohist).max()


@pytest.mark.parametrize("structured", [False, True])
def test_wide256_fp64_against_the_lazy_oracle(wide256, structured):
    p, (ref, ohist, _) = wide256
    dh, ah = synth.forecast_at(p["forecast"], 0)
    s = capi.Solver(p["network"], p["tree"], p["config"], precision="f64", structured=structured)
    s.initialiseSmpcController(dh, ah)
    assert s.nodes == 5649 and s.nv == 306
    hist = s.algorithmApg(ITERS)
    check("wide256 f64 %s" % ("structured" if structured else "dense"), s, p, ref, ohist, hist)
    s.close()


def test_wide256_fp64_both_soft_thresholds_trip(wide256):
    """penalties small enough that dist_x > gamma_x / lambda and dist_s > gamma_s / lambda: the device-resident batch runs
    optimistically, trips and is replayed through the exact fix-up kernels, and must still match the oracle"""
    p0 = wide256[0]
    p = synth.make_problem("wide256", penalty_x=2e-3, penalty_xs=2e-3, step_size=p0["config"]["stepSize"][0])
    ref, ohist, both = oracle_run(p, ITERS)
    assert both >= 20, "only %d of %d iterations exceed both thresholds at once" % (both, ITERS)
    dh, ah = synth.forecast_at(p["forecast"], 0)
    s = capi.Solver(p["network"], p["tree"], p["config"], precision="f64", structured=True)
    s.initialiseSmpcController(dh, ah)
    hist = s.algorithmApg(ITERS)
    check("wide256 f64 structured, both thresholds tripped", s, p, ref, ohist, hist)
    assert s.counters()["replayed"] >= 1, s.counters()
    s.close()
