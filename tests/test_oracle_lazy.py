"""The oracle's block-free operator mode (Oracle(..., lazy_operators=True), oracle_config_lazy in oracle/apg_oracle.c) pinned to its
stored-block mode, and tests/stagewise.py pinned on synthetic arrays.

The lazy mode applies every per-node block of the factor step from the shared matrices, the stage diagonals and p_i, so that the
wide network can be checked against an fp64 oracle at its full size (tests/test_gpu_wide_network.py).  The two modes compute the
same operator in another order of summation (Rinv / p_a against (p_a Rbar)^-1), so they must agree to rounding on every buffer
the GPU tests read, stage by stage, over 25 APG iterations."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from rapidnet_amd import partition, synth
from stagewise import DIM_OF, stage_relmax, worst_by_buffer

ITERS = 25
TOL = {"f64": 1e-12, "f32": 1e-5}
BUFFERS = tuple(DIM_OF)   # every buffer the GPU tests read


def lambdas(n):
    th0, th1, out = 1.0, 1.0, []
    for _ in range(n):
        out.append(th1 * (1 / th0 - 1))
        th0, th1 = th1, 0.5 * (np.sqrt(th1 ** 4 + 4 * th1 ** 2) - th1 ** 2)
    return out


def pair(name, precision="f64", alias=True, **kw):
    p = synth.make_problem(name, **kw)
    dh, ah = synth.forecast_at(p["forecast"], 0)
    out = []
    for lazy in (False, True):
        o = Oracle(p["network"], p["tree"], p["config"], precision=precision, alias_operators=alias, lazy_operators=lazy)
        o.initialise(dh, ah)
        out.append(o)
    return p, out[0], out[1]


def worst(stored, lazy, tree):
    ref = {nm: stored.get(nm) for nm in BUFFERS}
    return worst_by_buffer({nm: lazy.get(nm) for nm in BUFFERS}, ref, tree, stored.nx, stored.nu, stored.nv)


# the reference's aliasing rule (Omega/Theta of the last branching stage reused below it, Engine.cu:210-221) is defined only for
# trees that branch from the root on: on "late" and "horizon1" it indexes before the first Omega, so they run with aliasing off
CASES = [(nm, True) for nm in ("small", "odd", "ragged", "fan", "widecrown", "wide16")] + \
        [(nm, False) for nm in ("small", "odd", "ragged", "late", "fan", "horizon1", "widecrown", "wide16")]


@pytest.mark.parametrize("name,alias", CASES)
def test_lazy_operators_match_the_stored_blocks(name, alias):
    p, s, z = pair(name, alias=alias)
    hs, hz = s.apg(ITERS), z.apg(ITERS)
    w = worst(s, z, p["tree"])
    assert max(w.values()) <= TOL["f64"], w
    assert np.abs(hz - hs).max() <= TOL["f64"] * np.abs(hs).max()
    for nm in ("sysF", "sysG", "Omega", "Theta", "Phi", "D", "Psi", "Ftil"):   # no per-node block is held
        with pytest.raises(KeyError):
            z.buf(nm)


@pytest.mark.parametrize("name,tol", [("small", TOL["f32"]), ("ragged", TOL["f32"]), ("wide16", 5e-5)])
def test_lazy_operators_match_the_stored_blocks_fp32(name, tol):
    """wide16: dualXi = proj(primalXi + accXi / lambda) with lambda = 1.6e-6 cancels down to the box, and its fp32 rounding of the
    two orders of summation is measured at 2.0e-5 of the stage's primal (1.7e-5 for resXi); the bound is 2.5x that."""
    p, s, z = pair(name, precision="f32")
    hs, hz = s.apg(ITERS), z.apg(ITERS)
    w = worst(s, z, p["tree"])
    print(name, "fp32 lazy vs stored, worst stage:", {k: "%.1e" % v for k, v in w.items()})
    assert max(w.values()) <= tol, w
    assert np.abs(hz - hs).max() <= TOL["f32"] * np.abs(hs).max()


def test_lazy_operators_with_both_soft_constraint_thresholds_tripped():
    """penalties small enough that dist_x > gamma_x / lambda AND dist_s > gamma_s / lambda in every iteration (the case of
    tests/test_gpu_parity.py::test_both_soft_constraint_thresholds_trip_at_once)"""
    px, ps = 0.5, 0.2
    p, s, z = pair("medium", penalty_x=px, penalty_xs=ps)
    lam = p["config"]["stepSize"][0]
    s.apg_reset(); z.apg_reset()
    th_s = th_z = [1.0, 1.0]
    for _ in range(ITERS):
        th_s, th_z = s.apg_continue(1, th_s), z.apg_continue(1, th_z)
        for o in (s, z):
            dx, ds = o.dist()
            assert dx > px / lam and ds > ps / lam
    w = worst(s, z, p["tree"])
    assert max(w.values()) <= TOL["f64"], w


@pytest.mark.parametrize("name", ["ragged", "small"])
def test_lazy_operators_around_a_cut(name):
    """the two phases of solve_step_phase: the children sums of the cut parents that phase 0 leaves in q / r (what the ranks
    all-reduce) and the iterates after phase 1"""
    p, s, z = pair(name, alias=False)
    cut = partition.default_cut_stage(p["tree"])
    pn = p["tree"]["nodesPerStage"][cut - 1]
    s.apg_reset(); z.apg_reset()
    for lam in lambdas(ITERS):
        for o in (s, z):
            o.extrapolate(lam)
            o.solve_step_phase(0, cut)
        for nm, dim in (("q", s.nx), ("r", s.nv)):
            ref = s.get(nm)[: pn * dim]
            assert np.abs(z.get(nm)[: pn * dim] - ref).max() <= TOL["f64"] * np.abs(ref).max(), nm
        for o in (s, z):
            o.solve_step_phase(1, cut)
            o.prox(); o.residual(); o.dual_update()
    w = worst(s, z, p["tree"])
    assert max(w.values()) <= TOL["f64"], w


def test_lazy_oracle_refuses_fbe_and_nama():
    p = synth.make_problem("small")
    o = Oracle(p["network"], p["tree"], p["config"], lazy_operators=True)
    o.initialise(*synth.forecast_at(p["forecast"], 0))
    for name in ("globalFbeAlgorithm", "namaAlgorithm"):
        with pytest.raises(RuntimeError, match="lazy_operators"):
            o.set_algorithm(name)
    with pytest.raises(RuntimeError, match="lazy_operators"):
        o.hessian_oracle()
    o.set_algorithm("proximalAlgorithm")


# ---- tests/stagewise.py ------------------------------------------------------------------------------------------------
def _wide_like_tree():
    """root, 8, 64 and 4 096 nodes per stage: the sqrt(p_i) of the last stage is 1/64"""
    counts = [1, 8, 64, 4096]
    return {"nodes": [sum(counts)], "stages": np.repeat(np.arange(len(counts)), counts).tolist()}, counts


def test_stage_relmax_sees_an_error_confined_to_a_small_stage():
    tree, counts = _wide_like_tree()
    rng = np.random.default_rng(3)
    dim = 5
    scale = np.repeat([1.0, 1 / 8 ** 0.5, 1 / 8, 1 / 64], counts)[:, None]
    ref = rng.standard_normal((sum(counts), dim)) * scale
    got = ref.copy()
    leaves = slice(sum(counts[:-1]), None)
    got[leaves] *= 1 + 1e-8                                  # a 1e-8 relative error in the leaf stage only (scale 1/64)
    glob = np.abs(got - ref).max() / np.abs(ref).max()
    per_stage = stage_relmax(got, ref, tree, dim)
    assert glob < 1e-9                                       # the global measure passes it ...
    assert per_stage.max() > 1e-9 and int(np.argmax(per_stage)) == 3   # ... the per-stage one does not, and names the stage
    assert (per_stage[:3] == 0).all()
    assert per_stage[3] == pytest.approx(1e-8, rel=1e-3)


def test_stage_relmax_floor_keeps_rounding_noise_out():
    """a stage whose reference sits at rounding level is measured against 1e-3 of the tree's scale, not against itself"""
    tree, counts = _wide_like_tree()
    dim = 3
    ref = np.ones((sum(counts), dim))
    ref[sum(counts[:-1]):] = 1e-21
    got = ref.copy()
    got[sum(counts[:-1]):] = 3e-21                           # noise against noise: 200 % of itself, 2e-18 of the floor
    e = stage_relmax(got, ref, tree, dim)
    assert e[3] == pytest.approx(2e-21 / 1e-3)
    got[0, 0] += 1e-6
    assert stage_relmax(got, ref, tree, dim)[0] == pytest.approx(1e-6)
