"""k_stream_gemv's skip of operator spans that meet no nonzero entry of the dual vector (csrc/k_stream.hpp, stream_walk; RN_KNOB_STREAM_SKIP).

The contract of the skip is that it changes no bit: a dead span adds a * (+-0) = +-0 to partial sums that started at +0.  So every case here
runs the same sweep in two contexts, knob 0 (every span) and knob 1 (the default), asks for BITWISE equal outputs, and holds one of them
against the fp64 oracle at the tolerances of test_gpu_parity.py (REL_TOL in fp64; FP32_TOL for the fp32 context and for fp64 iterates over
fp32-stored blocks, as test_gpu_stream_split.py does).  What the launch walked is read back through rn_debug_stream_live and must EQUAL
the counts numpy derives from the vector the test set (integers), and rn_algorithmic_bytes must equal the bytes of exactly those spans.

The dual patterns are the ones at which the walk can go wrong: nothing live (the outputs are still written), everything live, a single
live column at the first index, at the last one and inside the ragged last span, alternate spans, one half of the spans, -0.0 everywhere
(zero), one denormal (live), a random 10 %.  The small trees have one or two spans per block (the ragged one on `odd` and `small`); the wide
network gives more than 64 spans per block (several ballots), the trees of test_gpu_stream_split.py the split last round, where a pattern
leaves one workgroup of a block without a live span."""
import numpy as np
import pytest

import test_gpu_fbe_nama as fbe
import test_gpu_stream_split as ss
from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from test_gpu_parity import FP32_TOL, REL_TOL, relmax

pytestmark = pytest.mark.gpu

FORMS = {"f64": dict(precision="f64"), "f32": dict(precision="f32"), "f64_on_f32": dict(precision="f64", operator_storage="f32")}
TOL = {"f64": REL_TOL, "f32": FP32_TOL, "f64_on_f32": FP32_TOL}
OUT = ((capi.BUF_X, "x"), (capi.BUF_U, "u"), (capi.BUF_V, "v"), (capi.BUF_PRIMAL_XI, "primalXi"), (capi.BUF_PRIMAL_PSI, "primalPsi"))
PATTERNS = ("zero", "dense", "col_first", "col_last", "col_in_last_span", "alternate_spans", "first_half", "second_half", "neg_zero", "denormal", "random10")


def pattern(name, nodes, ny, G, half, f32):
    """W [nodes][ny] in fp64; `half`: the span at which the second half starts"""
    rng = np.random.default_rng(PATTERNS.index(name) + 11)
    val = rng.standard_normal((nodes, ny)) * 50
    val[val == 0] = 1.0
    span = np.arange(ny) // G
    W = np.zeros((nodes, ny))
    if name == "dense":
        W = val
    elif name == "col_first":
        W[:, 0] = val[:, 0]
    elif name == "col_last":
        W[:, ny - 1] = val[:, ny - 1]
    elif name == "col_in_last_span":       # the first column of the last span: the ragged one where ny % G != 0
        c = (ny - 1) // G * G
        W[:, c] = val[:, c]
    elif name == "alternate_spans":        # even spans in even nodes, odd spans in odd nodes
        W = np.where((span[None, :] + np.arange(nodes)[:, None]) % 2 == 0, val, 0.0)
    elif name == "first_half":
        W = np.where(span[None, :] < half, val, 0.0)
    elif name == "second_half":
        W = np.where(span[None, :] >= half, val, 0.0)
    elif name == "neg_zero":
        W = -W
        assert np.signbit(W).all()
    elif name == "denormal":               # of the context's type; in the last block's last column
        W[nodes - 1, ny - 1] = 1e-45 if f32 else 5e-324
    elif name == "random10":
        W = np.where(rng.random((nodes, ny)) < 0.1, val, 0.0)
    return W


def counts(W, G, f32):
    """{live spans, spans, live columns, columns} and the live ragged last spans, as rn_debug_stream_live defines them: any bit but the sign"""
    nz = (W.astype(np.float32) if f32 else W) != 0
    nodes, ny = W.shape
    spans = -(-ny // G)
    pad = np.zeros((nodes, spans * G), bool)
    pad[:, :ny] = nz
    live = pad.reshape(nodes, spans, G).any(axis=2)
    ragged = int(live[:, -1].sum()) if ny % G else 0
    return {"liveSpans": int(live.sum()), "spans": nodes * spans, "liveColumns": int(nz.sum()), "columns": nodes * ny}, ragged


def sweep_bytes(s, form, G, live, ragged):
    """rn_algorithmic_bytes' streaming figure: whole live spans at G * LD entries, ragged ones at ny % G columns, plus the vectors"""
    elem, real = (8 if form == "f64" else 4), (4 if form == "f32" else 8)
    per = 16 // elem
    LD = (2 * s.nv + per - 1) // per * per
    vectors = s.nodes * (s.ny + 2 * s.nv + s.nx) * real
    dense = s.nodes * 2 * s.nv * s.ny * elem + vectors
    return ((live - ragged) * G + ragged * (s.ny % G)) * LD * elem + vectors, dense


def context(p, fc, form, skip, **kw):
    s = capi.Solver(p["network"], p["tree"], p["config"], knobs=dict(kw.pop("knobs", {}), stream_skip=skip), **dict(FORMS[form], **kw))
    s.initialiseSmpcController(*fc)
    return s


def one_sweep(s, W):
    s.set(capi.BUF_ACC_XI, np.ascontiguousarray(W[:, :2 * s.nx]).ravel())
    s.set(capi.BUF_ACC_PSI, np.ascontiguousarray(W[:, 2 * s.nx:]).ravel())
    s.solveStep()
    return {nm: s.get(b) for b, nm in OUT}


_ORACLE_OUT = {}


def oracle_sweep(key, make_oracle, W, nx):
    """the fp64 oracle's sweep at the dual W: computed once per (problem, pattern, span), left unchanged"""
    if key not in _ORACLE_OUT:
        o = make_oracle()
        o.set("accXi", np.ascontiguousarray(W[:, :2 * nx]).ravel()); o.set("accPsi", np.ascontiguousarray(W[:, 2 * nx:]).ravel())
        o.solve_step()
        ref = {nm: o.get(nm) for _, nm in OUT}
        for a in ref.values():
            a.setflags(write=False)
        _ORACLE_OUT[key] = ref
    return _ORACLE_OUT[key]


def check_patterns(tag, p, fc, form, make_oracle, patterns=PATTERNS, min_spans=1, split=False, **kw):
    s0, s1 = context(p, fc, form, 0, **kw), context(p, fc, form, 1, **kw)
    try:
        k, info = s1.kernelInfo(), s1.streamInfo()
        G, f32 = k["stream_G"], form == "f32"
        spans = -(-s1.ny // G)
        assert spans >= min_spans, (tag, k, spans)
        assert (info["splitFirst"] < s1.nodes) == split and s0.streamInfo() == info, (tag, info)
        half = info["splitSpanHalf"] if split else spans // 2
        print("\n%s %s: nodes %d ny %d G %d NL %d spans %d half %d %s" % (tag, form, s1.nodes, s1.ny, G, k["stream_NL"], spans, half, info))
        # before any launch: the dense figure, and nothing to report
        assert s1.algorithmicBytes()[0] == sweep_bytes(s1, form, G, 0, 0)[1]
        with pytest.raises(capi.RapidNetError):
            s1.streamLive()
        for name in patterns:
            W = pattern(name, s1.nodes, s1.ny, G, half, f32)
            want, ragged = counts(W, G, f32)
            a, b = one_sweep(s0, W), one_sweep(s1, W)
            live0, live1 = s0.streamLive(), s1.streamLive()
            print("%-17s live spans %d of %d, live columns %d of %d, ragged %d" % (name, want["liveSpans"], want["spans"], want["liveColumns"], want["columns"], ragged))
            assert live1 == want, (tag, name, live1, want)
            assert live0 == dict(want, liveSpans=want["spans"], liveColumns=want["columns"]), (tag, name, live0)      # knob 0 walks everything
            skipped, dense = sweep_bytes(s1, form, G, want["liveSpans"], ragged)
            assert s1.algorithmicBytes()[0] == skipped and s0.algorithmicBytes()[0] == dense, (tag, name, s1.algorithmicBytes(), skipped, dense)
            for nm in a:
                assert np.array_equal(a[nm], b[nm]), (tag, name, nm, "knob 0 and knob 1 differ")
            ref = oracle_sweep((tag, name, G), make_oracle, W, s1.nx)
            worst = {nm: relmax(b[nm], ref[nm]) for nm in b}
            assert max(worst.values()) <= TOL[form], (tag, name, worst)
    finally:
        s0.close(); s1.close()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("tree", ["tiny", "odd", "ragged", "small"])
def test_one_sweep_is_bitwise_the_walk_over_every_span(tree, form):
    p = synth.make_problem(tree)
    fc = synth.forecast_at(p["forecast"], 0)

    def make_oracle():
        o = Oracle(p["network"], p["tree"], p["config"])
        o.initialise(*fc)
        return o

    check_patterns(tree, p, fc, form, make_oracle)
    if tree == "odd":
        s = context(p, fc, form, 1)
        assert s.ny % s.kernelInfo()["stream_G"] != 0       # the ragged last span is among the cases
        s.close()


_WIDE = []


def wide_problem():
    """the wide network (2 nv = 612 rows per column) on five nodes: 19 MB of fp64 blocks, and more spans per block than one ballot holds"""
    if not _WIDE:
        synth.CONFIGS["skip_wide5"] = (4, 200, 360, 280, 54, 3, [2])
        try:
            p = synth.make_problem("skip_wide5")
        finally:
            del synth.CONFIGS["skip_wide5"]
        _WIDE.append((p, synth.forecast_at(p["forecast"], 0)))
    return _WIDE[0]


@pytest.mark.parametrize("form", list(FORMS))
def test_more_than_64_spans_per_block(form):
    p, fc = wide_problem()
    check_patterns("wide5", p, fc, form, lambda: ss.oracle_of(p, fc), min_spans=65)


@pytest.mark.parametrize("net,pos,form", [("b240", "two", "f64"), ("b236", "three", "f64"), ("b240", "two", "f32")])
def test_split_round_with_a_dead_half(net, pos, form):
    """the split last round: `first_half` / `second_half` cut at splitSpanHalf, so one of a split block's two workgroups has no live span"""
    p, fc = ss.problem(net, pos)
    check_patterns("%s_%s" % (net, pos), p, fc, form, lambda: ss.oracle_of(p, fc), split=True,
                   patterns=("zero", "dense", "col_first", "col_in_last_span", "alternate_spans", "first_half", "second_half", "random10"))


@pytest.mark.parametrize("form", list(FORMS))
def test_forty_apg_iterations_from_reset(form):
    """iterates and history bit for bit between the knobs, from the all-zero duals of a reset on"""
    p = synth.make_problem("small")
    fc = synth.forecast_at(p["forecast"], 0)
    runs = []
    for skip in (0, 1):
        s = context(p, fc, form, skip)
        hist = s.algorithmApg(40)
        runs.append((hist, {b: s.get(b) for b in ss.ALL_BUFS}, s.streamLive()))
        s.close()
    (h0, b0, l0), (h1, b1, l1) = runs
    print("\nlive after 40 iterations: knob 0 %s, knob 1 %s" % (l0, l1))
    assert np.array_equal(h0, h1)
    for b in ss.ALL_BUFS:
        assert np.array_equal(b0[b], b1[b]), b
    assert l0["liveSpans"] == l0["spans"] and 0 < l1["liveColumns"] <= l1["columns"] and l1["liveSpans"] <= l1["spans"]


@pytest.mark.parametrize("tree,form", [("odd", "f64"), ("small", "f32"), ("odd", "f64_on_f32")])
def test_nama_pair_of_sweeps_stays_bitwise(tree, form):
    """NR = 2 (rn_set_sweep_pairing(RN_PAIR_ON)): the union mask of the two vectors.  The pair with the skip against the two sweeps with
    the skip, and against the pair without it: every buffer, value and accepted step"""
    p = synth.make_problem(tree)
    fc = synth.forecast_at(p["forecast"], 0)
    runs = {}
    for skip, pair in ((1, 1), (1, 0), (0, 1)):
        s = context(p, fc, form, skip, sweep_pairing="on", knobs={"nama_pair": pair, "stream_split": 0})
        s.setAlgorithm("namaAlgorithm", 5)
        h, v, t = s.algorithmNama(4)
        runs[(skip, pair)] = (h, v, t, [s.get(b) for b, _ in fbe.FBE_PAIRS] + [s.get(capi.BUF_X), s.get(capi.BUF_U)], s.fbeCounters())
        s.close()
    assert runs[(1, 1)][4]["sweep_pairs"] >= 1 and runs[(0, 1)][4]["sweep_pairs"] >= 1 and runs[(1, 0)][4]["sweep_pairs"] == 0, {k: v[4] for k, v in runs.items()}
    for other in ((1, 0), (0, 1)):
        for i in range(3):
            assert np.array_equal(runs[(1, 1)][i], runs[other][i]), (other, i)
        for x, y in zip(runs[(1, 1)][3], runs[other][3]):
            assert np.array_equal(x, y), other
