"""k_stream_gemv's skip at HALF-span granularity (csrc/k_stream.hpp, stream_walk_half; RN_KNOB_STREAM_HALF).

Every NL = 2 launch walks units of one load per thread: with an even span G a unit is half a span (G / 2 columns) and, where half a span is
whole 128-byte lines, the skip leaves out single halves.  The contract is that of the skip: no bit changes.  So every case runs the same sweep
in THREE contexts -- stream_skip = 0 (everything walked), stream_half = 0 (live spans walked whole) and the default -- asks for BITWISE equal
outputs and holds the default to the fp64 oracle at test_gpu_stream_skip.py's tolerances (its machinery is reused by import).  What the launch
walked is read back through rn_debug_stream_units and must EQUAL numpy's count of the vector the test set at G / 2 columns (integers);
rn_debug_stream_live keeps its meaning, the live SPANS, in all three, and rn_algorithmic_bytes must equal the bytes of exactly the units walked
(halves of a ragged span at the columns they have).  (A context with stream_skip = 1 FORCED skips whole spans: test_gpu_stream_skip.py.)

Shapes: the split-round trees of test_gpu_stream_split.py (b240 / two in the three forms, b236 / three with its ragged span: in fp64 the ragged
span is one half, in fp32 a whole first half and a partial second); a network of 2 nv = 256 rows (G = 8, 71 units per block: more units than
one ballot holds, a ragged span of 2 columns); one of 2 nv = 176 rows whose line-aligned span is G = 11 (NL = 2 with an ODD span: the units
are the two slots of the span walk and never skipped by themselves); an NL = 1 tree and the wide network (NL >= 3), where nothing changed and
the hook reports whole spans.

Patterns: the first half of every span, the second, halves alternating by node parity, a single live column at G / 2 - 1 and at G / 2, one
column at each end of the ragged span, one live unit, everything live (more than 64 live units on the 71-unit shape), -0.0 everywhere, a
denormal in the last column, a random 10 %."""
import numpy as np
import pytest

import test_gpu_stream_skip as sk
import test_gpu_stream_split as ss
from oracle.oracle import Oracle
from rapidnet_amd import capi, synth

pytestmark = pytest.mark.gpu

HALF_PATTERNS = ("first_halves", "second_halves", "halves_by_parity", "col_before_middle", "col_at_middle", "ragged_ends", "one_unit")
REUSED = ("zero", "dense", "neg_zero", "denormal", "random10")      # test_gpu_stream_skip.pattern
# (nx, nu, nd, ne) of networks built for this file: nv = nu - ne
NETS = {"nv128": (60, 71, 140, 40, 12),      # 2 nv = 256: fp64 G = 8 (1024 slots, NL = 2), ny = 282 = 35 spans + 2 columns = 71 units
        "nv88": (61, 20, 100, 30, 12),       # 2 nv = 176: fp64 G = 11 (968 slots, NL = 2, odd), ny = 140 = 12 spans + 8 columns
        "b240s": (62, 63, 114, 88, 17)}      # Barcelona's dimensions (fp64 G = 8, fp32 G = 16, NL = 2) on a small tree
_PROBLEMS = {}


def net_problem(net, N=3, branching=(2,)):
    if net not in _PROBLEMS:
        idx, nx, nu, nd, ne = NETS[net]
        name = "half_%s" % net
        synth.CONFIGS[name] = (idx, nx, nu, nd, ne, N, list(branching))
        try:
            p = synth.make_problem(name)
        finally:
            del synth.CONFIGS[name]
        _PROBLEMS[net] = (p, synth.forecast_at(p["forecast"], 0))
    return _PROBLEMS[net]


def half_pattern(name, nodes, ny, G, f32):
    """W [nodes][ny] in fp64; halves of G // 2 columns"""
    if name in REUSED:
        return sk.pattern(name, nodes, ny, G, 0, f32)
    Gh = G // 2
    rng = np.random.default_rng(HALF_PATTERNS.index(name) + 101)
    val = rng.standard_normal((nodes, ny)) * 50
    val[val == 0] = 1.0
    second = (np.arange(ny) % G) >= Gh
    W = np.zeros((nodes, ny))
    if name == "first_halves":
        W = np.where(~second[None, :], val, 0.0)
    elif name == "second_halves":
        W = np.where(second[None, :], val, 0.0)
    elif name == "halves_by_parity":       # first halves in even nodes, second halves in odd nodes
        W = np.where(second[None, :] == (np.arange(nodes)[:, None] % 2 == 1), val, 0.0)
    elif name == "col_before_middle":      # the last column of a first half (of the second span where there is one)
        c = (G if ny >= 2 * G else 0) + Gh - 1
        W[:, c] = val[:, c]
    elif name == "col_at_middle":          # the first column of a second half
        c = (G if ny >= 2 * G else 0) + Gh
        W[:, c] = val[:, c]
    elif name == "ragged_ends":            # the first and the last column of the last span (the ragged one where ny % G != 0): its two halves where it has two
        c = (ny - 1) // G * G
        W[:, c] = val[:, c]
        W[:, ny - 1] = val[:, ny - 1]
    elif name == "one_unit":               # one whole unit of one block
        W[nodes // 2, 3 * Gh:4 * Gh] = val[nodes // 2, 3 * Gh:4 * Gh]
    return W


def unit_counts(W, cols, f32):
    """{live units, units, columns per unit} as rn_debug_stream_units defines them, at units of `cols` columns: any bit but the sign"""
    nz = (W.astype(np.float32) if f32 else W) != 0
    nodes, ny = W.shape
    units = -(-ny // cols)
    pad = np.zeros((nodes, units * cols), bool)
    pad[:, :ny] = nz
    return {"liveUnits": int(pad.reshape(nodes, units, cols).any(axis=2).sum()), "units": nodes * units, "columnsPerUnit": cols}


def halves_skipped(s, form, G, NL):
    """the library's rule restated (Ctx::stream_half_on): two slots per thread, an even span, half a span a whole number of 64-byte half lines"""
    elem = 8 if form == "f64" else 4
    per = 16 // elem
    LD = (2 * s.nv + per - 1) // per * per
    return NL == 2 and G % 2 == 0 and (G // 2 * LD * elem) % 64 == 0


def context(p, fc, form, knobs):
    s = capi.Solver(p["network"], p["tree"], p["config"], knobs=knobs, **sk.FORMS[form])
    s.initialiseSmpcController(*fc)
    return s


def unit_bytes(s, form, W, cols, f32):
    """rn_algorithmic_bytes' streaming figure where units of `cols` columns are skipped by themselves: every live unit at the columns it has"""
    elem, real = (8 if form == "f64" else 4), (4 if form == "f32" else 8)
    per = 16 // elem
    LD = (2 * s.nv + per - 1) // per * per
    nz = (W.astype(np.float32) if f32 else W) != 0
    live_cols = sum(min(cols, s.ny - c0) * int(nz[:, c0:c0 + cols].any(axis=1).sum()) for c0 in range(0, s.ny, cols))
    return live_cols * LD * elem + s.nodes * (s.ny + 2 * s.nv + s.nx) * real


def check_halves(tag, p, fc, form, make_oracle, patterns, two_slots=None, want_half=None, split=False, min_units=1):
    ctx = {"all": context(p, fc, form, {"stream_skip": 0}), "span": context(p, fc, form, {"stream_half": 0}), "half": context(p, fc, form, {})}
    try:
        s = ctx["half"]
        k, info = s.kernelInfo(), s.streamInfo()
        G, NL, f32 = k["stream_G"], k["stream_NL"], form == "f32"
        half = halves_skipped(s, form, G, NL)
        spans = -(-s.ny // G)
        print("\n%s %s: nodes %d ny %d G %d NL %d spans %d halves skipped %s %s" % (tag, form, s.nodes, s.ny, G, NL, spans, half, info))
        assert (two_slots is None or (NL == 2) == two_slots) and (want_half is None or half == want_half), (tag, k, half)
        assert (info["splitFirst"] < s.nodes) == split, (tag, info)
        for c in ctx.values():      # the hooks still speak in spans, with the same values whatever the knobs
            assert c.kernelInfo() == k and c.streamInfo() == info, (tag, c.kernelInfo(), c.streamInfo())
        ucols = G // 2 if half else G
        assert -(-s.ny // ucols) >= min_units, (tag, s.ny, ucols)
        with pytest.raises(capi.RapidNetError):
            s.streamUnits()
        for name in patterns:
            W = half_pattern(name, s.nodes, s.ny, G, f32)
            want, ragged = sk.counts(W, G, f32)
            out = {key: sk.one_sweep(c, W) for key, c in ctx.items()}
            units = {key: c.streamUnits() for key, c in ctx.items()}
            wantU = unit_counts(W, ucols, f32)
            print("%-17s live units %d of %d (%d columns each), live spans %d of %d" % (name, wantU["liveUnits"], wantU["units"], ucols, want["liveSpans"], want["spans"]))
            assert units["half"] == wantU, (tag, name, units["half"], wantU)
            assert units["span"] == {"liveUnits": want["liveSpans"], "units": want["spans"], "columnsPerUnit": G}, (tag, name, units["span"], want)
            assert units["all"] == {"liveUnits": want["spans"], "units": want["spans"], "columnsPerUnit": G}, (tag, name, units["all"], want)
            # the span hook: unchanged meaning (an upper bound on what the half walk requested); the bytes: those of the units walked
            assert ctx["half"].streamLive() == want and ctx["span"].streamLive() == want, (tag, name, ctx["half"].streamLive(), want)
            skipped, dense = sk.sweep_bytes(s, form, G, want["liveSpans"], ragged)
            assert ctx["span"].algorithmicBytes()[0] == skipped and ctx["all"].algorithmicBytes()[0] == dense, (tag, name, ctx["span"].algorithmicBytes(), skipped, dense)
            assert ctx["half"].algorithmicBytes()[0] == unit_bytes(s, form, W, ucols, f32), (tag, name, ctx["half"].algorithmicBytes(), unit_bytes(s, form, W, ucols, f32), skipped)
            for nm in out["half"]:
                assert np.array_equal(out["all"][nm], out["half"][nm]), (tag, name, nm, "stream_skip = 0 and the default differ")
                assert np.array_equal(out["span"][nm], out["half"][nm]), (tag, name, nm, "stream_half = 0 and the default differ")
            ref = sk.oracle_sweep(("half", tag, name, G), make_oracle, W, s.nx)
            worst = {nm: sk.relmax(out["half"][nm], ref[nm]) for nm in ref}
            assert max(worst.values()) <= sk.TOL[form], (tag, name, worst)
    finally:
        for c in ctx.values():
            c.close()


@pytest.mark.parametrize("net,pos,form", [("b240", "two", "f64"), ("b240", "two", "f32"), ("b240", "two", "f64_on_f32"), ("b236", "three", "f64"), ("b236", "three", "f32")])
def test_halves_on_the_split_round_trees(net, pos, form):
    """NL = 2 with a split last round (an odd group count on b236 / three); b236's ragged span: 4 of 8 columns in fp64, 12 of 16 in fp32"""
    p, fc = ss.problem(net, pos)
    check_halves("%s_%s" % (net, pos), p, fc, form, lambda: ss.oracle_of(p, fc), HALF_PATTERNS + REUSED, two_slots=True, want_half=True, split=True)


def test_more_than_64_live_units_in_a_block():
    """71 units per block: two chunks of the walk, `dense` and the half patterns cross the first one with more than 64 (35) live units"""
    p, fc = net_problem("nv128")
    check_halves("nv128", p, fc, "f64", lambda: ss.oracle_of(p, fc), ("dense", "first_halves", "second_halves", "halves_by_parity", "ragged_ends", "one_unit", "random10"),
                 two_slots=True, want_half=True, min_units=65)


def test_an_odd_span_walks_units_but_skips_whole_spans():
    p, fc = net_problem("nv88")
    check_halves("nv88", p, fc, "f64", lambda: ss.oracle_of(p, fc), ("dense", "first_halves", "col_at_middle", "ragged_ends", "one_unit", "random10", "zero"),
                 two_slots=True, want_half=False)
    s = sk.context(p, fc, "f64", 1)
    assert s.kernelInfo()["stream_G"] % 2 == 1      # the odd span is the case
    s.close()


@pytest.mark.parametrize("tree", ["small", "wide5"])
def test_other_slot_counts_report_whole_spans(tree):
    """NL = 1 (`small`) and NL >= 3 (the wide network): the span walk as it was, and rn_debug_stream_units in spans"""
    if tree == "small":
        p = synth.make_problem("small")
        fc = synth.forecast_at(p["forecast"], 0)

        def make_oracle():
            o = Oracle(p["network"], p["tree"], p["config"])
            o.initialise(*fc)
            return o
    else:
        p, fc = sk.wide_problem()

        def make_oracle():
            return ss.oracle_of(p, fc)
    check_halves(tree, p, fc, "f64", make_oracle, ("dense", "first_halves", "halves_by_parity", "random10"), two_slots=False, want_half=False)


@pytest.mark.parametrize("form", list(sk.FORMS))
def test_forty_apg_iterations_from_reset(form):
    """iterates and history bit for bit between the three knob settings on an NL = 2 shape, from the all-zero duals of a reset on"""
    p, fc = net_problem("b240s", N=5, branching=(3, 2))
    runs = []
    for knobs in ({"stream_skip": 0}, {"stream_half": 0}, {}):
        s = context(p, fc, form, knobs)
        assert s.kernelInfo()["stream_NL"] == 2
        hist = s.algorithmApg(40)
        runs.append((hist, {b: s.get(b) for b in ss.ALL_BUFS}, s.streamLive(), s.streamUnits()))
        s.close()
    print("\nafter 40 iterations: %s" % [(r[2], r[3]) for r in runs])
    for h, b, _, _ in runs[:2]:
        assert np.array_equal(h, runs[2][0])
        for k in ss.ALL_BUFS:
            assert np.array_equal(b[k], runs[2][1][k]), k
    (_, _, l1, u1), (_, _, l2, u2) = runs[1:]
    assert l1 == l2 and u1["liveUnits"] == l1["liveSpans"] and u1["units"] == l1["spans"]
    assert u2["columnsPerUnit"] * 2 == u1["columnsPerUnit"] and l2["liveSpans"] <= u2["liveUnits"] <= 2 * l2["liveSpans"] and 0 < u2["liveUnits"]
