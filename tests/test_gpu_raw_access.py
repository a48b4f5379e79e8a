"""rn_get / rn_set / rn_get_range / rn_set_range: the whole-buffer forms are the range forms over [0, all), with one difference that is meant.
v is an output computed on demand where the structured linear form is active (rapidnet_capi.hip, v_flush): a whole-buffer rn_set(RN_BUF_V)
drops the pending product, a partial rn_set_range(RN_BUF_V) computes it first, because the rest of the buffer has to be the sweep's.  Every
message names the entry point that was called; the texts are those of the library before the four functions shared their implementation."""
import functools

import numpy as np
import pytest

from rapidnet_amd import capi, synth

pytestmark = pytest.mark.gpu

PRECISIONS = ["f64", "f32"]
MODES = ["auto", "dense"]      # auto: structured, unsharded -- v is pending after a sweep that stores the primal iterates; dense: never pending


def round32(v):
    return np.asarray(v, np.float32).astype(np.float64)


problem = functools.lru_cache(maxsize=None)(synth.make_problem)      # (read only)


def stepped(name, precision, mode):
    """a context after three APG iterations, an extrapolation and one solveStep (which stores x, u and -- on demand -- v)"""
    p = problem(name)
    s = capi.Solver(p["network"], p["tree"], p["config"], precision=precision, operator_mode=mode)
    s.initialiseSmpcController(*synth.forecast_at(p["forecast"], 0))
    s.algorithmApg(3)
    s.dualExtrapolationStep(0.5)
    s.solveStep()
    return s


@pytest.fixture(scope="module")
def v0():
    """v after the step, read with rn_get, per (precision, mode): computed once, never written"""
    out = {}
    for precision in PRECISIONS:
        for mode in MODES:
            s = stepped("small", precision, mode)
            out[precision, mode] = s.get(capi.BUF_V)
            out[precision, mode].setflags(write=False)
            s.close()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_whole_set_of_v_replaces_a_pending_product(precision, mode, v0):
    s = stepped("small", precision, mode)
    vals = np.random.default_rng(1).standard_normal(v0[precision, mode].size)
    if precision == "f32":
        vals = round32(vals)
    s.set(capi.BUF_V, vals)
    assert np.array_equal(s.get(capi.BUF_V), vals)
    assert np.array_equal(s.getRange(capi.BUF_V, 0, vals.size), vals)
    s.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_partial_set_of_v_keeps_the_sweeps_values_around_it(precision, mode, v0):
    ref = v0[precision, mode]
    assert np.any(ref != 0.0)
    s = stepped("small", precision, mode)
    first, n = ref.size // 2 + 1, 7
    assert first % 4 and n % 4 and first + n < ref.size
    vals = np.random.default_rng(2).standard_normal(n)
    if precision == "f32":
        vals = round32(vals)
    s.setRange(capi.BUF_V, first, vals)
    want = ref.copy()
    want[first:first + n] = vals
    assert np.array_equal(s.get(capi.BUF_V), want)
    s.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_whole_get_is_the_range_from_zero(precision, mode, v0):
    s = stepped("small", precision, mode)
    bufs = (capi.BUF_X, capi.BUF_XI, capi.BUF_PSI, capi.BUF_ACC_XI, capi.BUF_ACC_PSI, capi.BUF_XMIN, capi.BUF_UMAX)
    for bid in bufs:
        whole = s.get(bid)
        assert whole.size == s.lib.rn_buffer_size(s.h, bid) > 0, bid
        assert np.array_equal(s.getRange(bid, 0, whole.size), whole), bid
    assert np.array_equal(s.getRange(capi.BUF_V, 0, v0[precision, mode].size), v0[precision, mode])     # (a pending v: computed by the range form too)
    s.close()


OBSERVED = (capi.BUF_X, capi.BUF_U, capi.BUF_V, capi.BUF_XI, capi.BUF_PSI, capi.BUF_UPD_XI, capi.BUF_UPD_PSI, capi.BUF_ACC_XI, capi.BUF_ACC_PSI,
            capi.BUF_PRIMAL_XI, capi.BUF_PRIMAL_PSI)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_whole_set_is_the_range_from_zero(precision, mode):
    """rn_set(values) and rn_set_range(0, values) on twin contexts, then the same two iterations: the same bits.  The twins stand behind an APG
    batch, where the ACC view is not the sweep's input buffer (the set swaps them), and RN_BUF_UHAT marks the control-step constants dirty."""
    rng = np.random.default_rng(3)
    groups = ((capi.BUF_X,), (capi.BUF_UHAT,), (capi.BUF_XI, capi.BUF_PSI), (capi.BUF_ACC_XI, capi.BUF_ACC_PSI))
    for group in groups:
        a, b = stepped("small", precision, mode), stepped("small", precision, mode)
        a.algorithmApg(2); b.algorithmApg(2)
        for bid in group:
            vals = a.get(bid) + 0.25 * rng.standard_normal(a.get(bid).size)
            a.set(bid, vals)
            b.setRange(bid, 0, vals)
            assert np.array_equal(a.get(bid), b.get(bid)), bid
            assert np.array_equal(a.get(bid), round32(vals) if precision == "f32" else vals), bid
        ha, hb = a.apgIterate(2), b.apgIterate(2)
        assert np.array_equal(ha, hb), group
        for bid in OBSERVED:
            ga, gb = a.get(bid), b.get(bid)
            assert np.all(np.isfinite(ga)) and np.array_equal(ga, gb), (group, bid)
        a.close(); b.close()


def message(s, rc):
    """the library's text for a refused call, without the wrapper's prefix"""
    assert rc != 0
    with pytest.raises(capi.RapidNetError) as e:
        s._check(rc)
    text = str(e.value)
    print(text)
    assert text.startswith("rapidnet error %d: " % rc)
    return text.split(": ", 1)[1]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_messages_name_the_entry_point_that_was_called(precision):
    p = problem("tiny")
    s = capi.Solver(p["network"], p["tree"], p["config"], precision=precision, operator_mode="auto")
    s.initialiseSmpcController(*synth.forecast_at(p["forecast"], 0))
    s.algorithmApg(2)
    lib, h = s.lib, s.h
    nX, nXi, dimXi = s.nodes * s.nx, s.nodes * 2 * s.nx, 2 * s.nx
    buf = np.zeros(nXi + 2 * dimXi)
    ptr = buf.ctypes.data
    unknown = 10 ** 6
    before = {bid: s.get(bid) for bid in (capi.BUF_X, capi.BUF_XI, capi.BUF_XMIN)}
    # a wrong size or range: plain and dual-shaped buffers
    assert message(s, lib.rn_get(h, capi.BUF_X, ptr, nX + 1)) == "rn_get: size mismatch"
    assert message(s, lib.rn_get(h, capi.BUF_XI, ptr, nXi - 1)) == "rn_get: size mismatch"
    assert message(s, lib.rn_set(h, capi.BUF_X, ptr, nX - 1)) == "rn_set: size mismatch"
    assert message(s, lib.rn_set(h, capi.BUF_XI, ptr, nXi + dimXi)) == "rn_set: size mismatch"
    assert message(s, lib.rn_get_range(h, capi.BUF_X, nX - 3, 4, ptr)) == "rn_get_range: range outside the buffer"
    assert message(s, lib.rn_set_range(h, capi.BUF_X, nX, 1, ptr)) == "rn_set_range: range outside the buffer"
    for first, n in ((3, dimXi), (dimXi, dimXi + 1), (nXi - dimXi, 2 * dimXi)):
        assert message(s, lib.rn_get_range(h, capi.BUF_XI, first, n, ptr)) == "rn_get_range: dual-shaped buffers are addressed in whole nodes"
        assert message(s, lib.rn_set_range(h, capi.BUF_XI, first, n, ptr)) == "rn_set_range: dual-shaped buffers are addressed in whole nodes"
    # an unknown id; the FBE / NAMA vectors are unknown until rn_set_algorithm selected one of them
    for bid in (unknown, capi.BUF_PREV_XI, capi.BUF_LBFGS_DIR_PSI):
        assert lib.rn_buffer_size(h, bid) == 0
        assert message(s, lib.rn_get(h, bid, ptr, 1)) == "rn_get: unknown buffer id"
        assert message(s, lib.rn_set(h, bid, ptr, 1)) == "rn_set: unknown buffer id"
        assert message(s, lib.rn_get_range(h, bid, 0, 1, ptr)) == "rn_get_range: unknown buffer id"
        assert message(s, lib.rn_set_range(h, bid, 0, 1, ptr)) == "rn_set_range: unknown buffer id"
    # the scaled bounds are read-only, whatever the size says
    for bid, dim in ((capi.BUF_XMIN, s.nx), (capi.BUF_XS, s.nx), (capi.BUF_UMAX, s.nu)):
        for n in (s.nodes * dim, 1):
            assert message(s, lib.rn_set(h, bid, ptr, n)) == "rn_set: the scaled bounds are read-only"
            assert message(s, lib.rn_set_range(h, bid, 0, n, ptr)) == "rn_set_range: the scaled bounds are read-only"
        assert np.array_equal(s.getRange(bid, dim, 2 * dim), s.get(bid)[dim:3 * dim])
    # no host array
    assert message(s, lib.rn_get(h, capi.BUF_X, None, nX)) == "rn_get: null host pointer"
    assert message(s, lib.rn_set(h, capi.BUF_X, None, nX)) == "rn_set: null host pointer"
    assert message(s, lib.rn_get_range(h, capi.BUF_X, 0, nX, None)) == "rn_get_range: null host pointer"
    assert message(s, lib.rn_set_range(h, capi.BUF_X, 0, nX, None)) == "rn_set_range: null host pointer"
    for bid, want in before.items():      # a refused call changes nothing
        assert np.array_equal(s.get(bid), want), bid
    s.setAlgorithm("namaAlgorithm")
    assert lib.rn_buffer_size(h, capi.BUF_PREV_XI) == nXi and s.get(capi.BUF_LBFGS_DIR_PSI).size == s.nodes * s.nu
    s.close()
