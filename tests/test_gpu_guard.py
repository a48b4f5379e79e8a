"""Device-buffer guard mode ("race detection / sanitizers"; no GPU address sanitizer exists on this pool).

With RAPIDNET_GUARD=1 every device buffer of a context sits between two 128 KiB red zones; red zones and payloads of the
floating-point buffers start as NaN.  A kernel that reads outside its buffer -- the streaming kernel's clamped re-reads of the
last slot, the slab products' prefetches past the last group, the zero-padded operator columns are all meant to stay INSIDE --
or reads something nobody wrote, drags a NaN into the iterates: the parity checks below then fail (`relmax` asserts finiteness).
A kernel that writes outside its buffer changes a red zone: every context is checked when it is destroyed and the process-wide
tally (rn_guard_report) must stay at zero.  The bodies are the parity tests themselves, run once more under the guard."""
import gc

import numpy as np
import pytest

import test_gpu_apg_f32 as apg32
import test_gpu_fbe_nama as fbe
import test_gpu_fbe_nama_f32 as f32
import test_gpu_first_principles as fpg
import test_gpu_parity as par
import test_gpu_receding_horizon as rh
import test_gpu_sharded_batched as shb
import test_gpu_stream_split as spl
from rapidnet_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture()
def guard(monkeypatch):
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    box = {}
    yield box
    gc.collect()
    after = capi.guard_report()
    assert after[0] - before[0] >= box.get("contexts", 1), "no context was created (and checked) under the guard: %s -> %s" % (before, after)
    assert after[1] == before[1], "a kernel wrote outside its buffer: %d red-zone bytes overwritten" % (after[1] - before[1])


def test_guard_mode_detects_an_overwritten_red_zone(monkeypatch):
    """The detector itself: payloads start as NaN (a buffer nobody has written reads back as NaN), a clean solve leaves every
    red zone intact, and a deliberate write behind a buffer (rn_debug_guard_poke: 24 bytes right behind the payload of the
    context's first buffer) is counted by rn_guard_check and by the tally rn_destroy keeps."""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    p = synth.make_problem("tiny")
    s2 = capi.Solver(p["network"], p["tree"], p["config"])
    assert np.isnan(s2.get(capi.BUF_BETA)).all()
    s2.close()
    s = capi.Solver(p["network"], p["tree"], p["config"])
    s.initialiseSmpcController(*synth.forecast_at(p["forecast"], 0))
    s.algorithmApg(20)
    assert s.guardCheck() == 0
    assert np.isfinite(s.get(capi.BUF_X)).all()
    s.debugGuardPoke(24)
    assert s.guardCheck() == 24
    before = capi.guard_report()
    s.close()
    after = capi.guard_report()
    assert after[0] == before[0] + 1 and after[1] == before[1] + 24
    monkeypatch.delenv("RAPIDNET_GUARD")
    s3 = capi.Solver(p["network"], p["tree"], p["config"])          # outside guard mode: nothing to check, nothing counted
    assert s3.guardCheck() == 0
    s3.close()
    assert capi.guard_report() == after


@pytest.mark.parametrize("name", ["toy", "odd", "medium"])
def test_stepwise_under_guard(guard, name):
    par.test_factor_step_and_affine_terms(name)
    par.test_stepwise_known_answer(name)
    guard["contexts"] = 2


@pytest.mark.parametrize("name,iters", [("small", 40), ("odd", 40), ("medium", 25)])
def test_apg_dense_and_structured_under_guard(guard, name, iters):
    par.test_apg_iterates_match_oracle(name, iters)
    par.test_structured_operator_mode(name, iters)
    guard["contexts"] = 2


@pytest.mark.parametrize("structured", [False, True])
@pytest.mark.parametrize("name,alias", [("widecrown", True), ("ragged", True), ("horizon1", False), ("fan", True), ("late", False)])
def test_edge_shapes_under_guard(guard, name, alias, structured):
    par.test_edge_tree_shapes(name, alias, structured)


def test_fp32_and_soft_branch_under_guard(guard):
    par.test_fp32_path()
    par.test_structured_fp32_and_soft_branch()
    par.test_soft_constraint_branch()
    guard["contexts"] = 4


@pytest.mark.parametrize("name,world,cut,structured,kw,trips", [("medium", 3, 2, False, {}, False), ("ragged", 3, 1, False, {}, False),
                                                                ("medium", 2, 1, True, {"penalty_x": 20.0, "penalty_xs": 5.0}, True)])
def test_sharded_batches_under_guard(guard, name, world, cut, structured, kw, trips):
    shb.test_batched_sharded_solve_matches_oracle(name, world, cut, structured, kw, trips)
    guard["contexts"] = world


@pytest.mark.parametrize("alg", fbe.ALGS)
def test_fbe_nama_loops_under_guard(guard, alg):
    fbe.test_loop_matches_oracle("small", False, alg)
    fbe.test_loop_matches_oracle("odd", False, alg)          # odd ny: the streaming kernel's two right-hand sides (NAMA) and k_value_mfma on ragged tiles
    fbe.test_loop_matches_oracle("medium", True, alg)
    fbe.test_line_search_direction_rule(alg, "positive")
    guard["contexts"] = 4


@pytest.mark.parametrize("alg", fbe.ALGS)
def test_f32_direction_and_line_search_under_guard(guard, alg):
    """the fp32 element kernels on `odd` (n = 891 = 3 mod 4): the scalar walks of L-BFGS columns that start off a 16-byte boundary and the
    tails behind the vector bodies are where a store one element past n would land in a red zone"""
    guard["contexts"] = f32.guard_body(alg)


def test_f32_apg_batches_under_guard(guard):
    """the fp32 APG kernels on `small` (n = 1330 = 2 mod 4), dense and structured: one exact iteration and one optimistic batch of 16 from each
    of the fp64 loop's fp32-rounded states -- the re-derived w behind rn_set, the checkpoint copies and the batch close are where a vector
    body's last store or a tail would land in a red zone"""
    guard["contexts"] = apg32.guard_body()


def test_control_steps_under_guard(guard):
    """five warm control steps on one structured context and on 3 rank contexts of `medium`: the warm start's copy between the rotating
    dual buffers, the checkpoints of the optimistic batches and the exchange buffers at the cut, step after step"""
    guard["contexts"] = rh.guard_body()


def test_first_principles_under_guard(guard):
    """`small`, dense and structured, against the problem's definition (tests/first_principles.py): the solve step from random and from
    9-iteration duals, and the state behind an exact iteration and an optimistic batch"""
    guard["contexts"] = fpg.guard_body()


@pytest.mark.parametrize("cases", [(("b236", "three", "f64"), ("nv129", "two", "f64"))])
def test_split_last_round_under_guard(guard, cases):
    """k_stream_gemv's split last round: the second halves' partials in my2 (r * 2 nv values, indexed by node - splitFirst), the second
    half's first group requested unconditionally and clamped into the block -- on the tree with an odd group count and a ragged last
    span, and on the one with three slots per thread"""
    spl.num_cus()            # (its throw-away context is not one of the two counted below)
    before = capi.guard_report()[0]
    for net, pos, precision in cases:
        spl.test_split_round_matches_the_oracle(net, pos, precision)
    gc.collect()
    assert capi.guard_report()[0] - before == len(cases)
    guard["contexts"] = len(cases)


def test_long_horizon_under_guard(guard):
    """a chain of 37 stages (`m42_37` of tests/test_long_horizon_shapes.py), dense and structured: the second and later batches of prefetched
    stages of the chain walks -- requests past the chain's end are clamped into it --, the fused walk + dual update's LDS tile of N rows and
    the chain walk riding in it; one step from non-trivial duals and two optimistic batches + an exact one"""
    import test_gpu_long_horizon as lhz

    guard["contexts"] = lhz.guard_body()


def test_slab_products_under_guard(guard):
    """rn_debug_slab_product's scratch operators, operand rows and outputs between red zones (tests/test_gpu_slab_product.py): a last slab of one
    node, the wide kernel's last workgroup of one node, the linear form's reads at an offset into longer rows, the first structured product and
    the tile kernel's 64-row groups past m -- payloads start as NaN, so a read outside what the hook wrote shows in the exact comparisons"""
    import test_gpu_slab_product as slp

    guard["contexts"] = slp.guard_body()


def test_dual_update_hook_under_guard(guard):
    """rn_debug_dual_update's scratch outputs, partials, iteration state and history slot between red zones (tests/test_gpu_dual_update.py): the
    stage-tiled kernel's partial last tile of two vectors and its idle trips, the flat kernel's scalar tail, the fix-up launch and the bookkeeping
    kernels writing into the hook's own state -- payloads start as NaN, so a read of something nobody wrote shows in the exact comparisons"""
    import test_gpu_dual_update as du

    guard["contexts"] = du.guard_body()


def test_barcelona31_under_guard(guard):
    """The full-size K = 31 Barcelona config: the kernel instantiations and launch shapes of the headline workload (G = 8 spans,
    two slots per thread, pipelined slab products, k_dual_stage tiles)."""
    par.test_barcelona31_full_size()
