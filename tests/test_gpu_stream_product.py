"""k_stream_gemv's product [m1_i; m2_i] = A_i w_i ALONE (rn_debug_stream_product) against an exact GEMV, at every live-unit count.

Every chunk of up to 64 units of the walk (csrc/k_stream.hpp, RN_STREAM_GROUPS) runs one schedule: nLive live units are a partial group of
nHead = nLive % group in front of nGroups = nLive / group full ones, and the code has a tail of its own for nGroups = 0, 1, 2, odd > 2 and even
> 2, each with or without a head, the guarded loads of a ragged last span behind them.  The other stream tests reach a handful of those cells and
compare sweep OUTPUTS at REL_TOL; here the product itself is read out and one launch on a tree of U + 1 nodes gives node i exactly i mod (U + 1)
live units in the chunk under test (stream_product_ref.live_count_duals), so every head meets every tail.  Each case prints the (nHead, nGroups)
cells it ran, and where the shape allows it asserts that they are the whole table {0 .. group - 1} x {0 .. 4}.

Two data sets per case:
 (a) exact: blocks of integers in [-4, 4] (read back from the context: fp32 storage included), live dual entries nonzero integers in [-8, 8]
     (read back and asserted).  With ny <= 1 600 every partial sum stays below 4 * 8 * 1 600 < 2^24: exact in fp32 and fp64 in any order, so
     the assertion is np.array_equal against the int64 product.  A unit left out, met twice, met against the wrong column or consumed before
     it landed cannot pass.
 (b) real: normal deviates, per row |my_r - ref_r| <= (ny + G) u sum_c |A_rc| |w_c| with u = 2^-53 where the sums are fp64 (fp32-stored blocks
     included) and 2^-24 in the fp32 context: the textbook bound of a sum of that many terms in any order, against np.longdouble.  Nothing in
     it is measured.  $STREAM_PRODUCT_ERRORS names a file every case appends its worst fraction of the bound to
     (profiles/stream_product_errors.txt).
Both also hold rn_debug_stream_units to numpy's count of the live units, and the rows of nodes without a live unit to exactly +0.  The real-valued
product must further be the same BITS through the one-per-CU and the two-per-CU instantiation (groups of different sizes over the same columns in
the same order), and a pair of right-hand sides the bits of two one-vector launches.  (The fp32 kernels once were not: the compiler had fused
most of their multiply-adds and left some as a product and a sum, different ones in each instantiation; k_stream.hpp, stream_fma.)

Shapes: NL = 2 Barcelona's dimensions (fp64: 60 half-spans) and for 4-byte blocks the network of 2 nv = 258 rows (50 half-spans and a ragged
span of one column); NL = 3 `tall`'s network, NL = 4 `wide4`'s (test_gpu_stream_dispatch.py); NL = 1 a network of 2 nv = 8 rows and 765 tanks:
G = 64, 24 whole spans and a ragged one of 6 columns.  Only rn_create and the factor step see them: the hook launches nothing else."""
import os

import numpy as np
import pytest

import stream_product_ref as ref
import test_gpu_stream_dispatch as sd
import test_gpu_stream_half as sh
import test_gpu_stream_skip as sk
import test_gpu_stream_split as ss
from rapidnet_amd import capi, synth

pytestmark = pytest.mark.gpu

# (seed index, nx, nu, nd, ne) and the tree (N, branching): 1 + 11 * 6 = 67 nodes (every count 0 .. 64 of a full chunk), 1 + 9 * 7 = 64 for the wide network
NETS = {"b240": ((80, 63, 114, 88, 17), (7, [11])), "nv129": ((81,) + ss.NETS["nv129"][1:], (7, [11])), "tall": ((82,) + synth.CONFIGS["tall"][1:5], (7, [11])),
        "wide4": ((83,) + sd.EXTRA["wide4"][1:5], (7, [11])), "flat": ((84, 765, 12, 6, 8), (7, [11])), "nv128": ((85,) + sh.NETS["nv128"][1:], (7, [11])),
        "wide5": ((86, 200, 360, 280, 54), (8, [9]))}
NET_OF = {1: lambda form: "flat", 2: lambda form: "b240" if form == "f64" else "nv129", 3: lambda form: "tall", 4: lambda form: "wide4"}
UNIT_ROUNDOFF = {"f64": 2.0 ** -53, "f64_on_f32": 2.0 ** -53, "f32": 2.0 ** -24}
_PROBLEMS, _REAL_PRODUCTS = {}, {}


def problem(net):
    if net not in _PROBLEMS:
        (idx, nx, nu, nd, ne), (N, branching) = NETS[net]
        name = "product_%s" % net
        synth.CONFIGS[name] = (idx, nx, nu, nd, ne, N, branching)
        try:
            p = synth.make_problem(name)
        finally:
            del synth.CONFIGS[name]
        _PROBLEMS[net] = p
    return _PROBLEMS[net]


def factored(p, form, knobs=None, **kw):
    s = capi.Solver(p["network"], p["tree"], p["config"], knobs=knobs, **dict(sk.FORMS[form], **kw))
    s.factorStep()
    return s


def record(tag, what):
    print("%s: %s" % (tag, what))
    path = os.environ.get("STREAM_PRODUCT_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write("%s: %s\n" % (tag, what))


def set_blocks(s, seed, integer):
    """hands random blocks in and returns what the context STORES, as [nodes][ny][2 nv]"""
    rng = np.random.default_rng(seed)
    dims = s._opDims()
    b = {nm: rng.integers(-4, 5, (s.nodes, n)).astype(np.float64) if integer else rng.standard_normal((s.nodes, n)) for nm, n in dims.items()}
    s.setOperators(b["Phi"], b["Psi"], b["D"], b["Ftil"])
    got = s.getOperators()
    if integer:
        for nm in b:
            assert np.array_equal(got[nm], b[nm]), nm
    return ref.block_columns(got, s.nx, s.nu, s.nv)


def set_dual(s, W, xi=capi.BUF_ACC_XI, psi=capi.BUF_ACC_PSI):
    """sets a dual-shaped vector and returns what the context holds"""
    s.set(xi, np.ascontiguousarray(W[:, :2 * s.nx]).ravel())
    s.set(psi, np.ascontiguousarray(W[:, 2 * s.nx:]).ravel())
    return np.concatenate([s.get(xi).reshape(s.nodes, 2 * s.nx), s.get(psi).reshape(s.nodes, s.nu)], axis=1)


def geometry(s, form, knobs):
    """(G, NL, columns per unit of liveness, such units per chunk of the walk, units of the schedule per unit of liveness)"""
    k = s.kernelInfo()
    G, NL = k["stream_G"], k["stream_NL"]
    if NL != 2:
        return G, NL, G, 64, 1
    if sh.halves_skipped(s, form, G, NL) and (knobs or {}).get("stream_half", -1) != 0 and (knobs or {}).get("stream_skip", -1) < 0:
        return G, NL, G // 2, 64, 1
    return G, NL, G, 32, 2      # both units of a span share its liveness: chunks of 32 spans, even counts


def check_product(tag, exact, form, got, At, W, G, rows=slice(None), col_range=None, where=None):
    """got against A w over col_range for the nodes `rows`; returns the worst fraction of the bound (0 where exact)"""
    ny = At.shape[1]
    want = ref.reference(At[rows], W[rows], col_range)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    c0, c1 = col_range or (0, ny)
    dead = ~(W[rows][:, c0:c1] != 0).any(axis=1)
    assert not got[dead].any() and not np.signbit(got[dead]).any(), (tag, "rows of nodes without a live unit are not +0")
    if exact:
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (tag, "first wrong node of the range", int(bad[0]), None if where is None else where(int(bad[0])), got[bad[0]][:8], want[bad[0]][:8])
        return 0.0
    bound = (ny + G) * UNIT_ROUNDOFF[form] * ref.magnitude(At[rows], W[rows], col_range)
    err = np.abs(got.astype(np.longdouble) - want)
    assert np.isfinite(got).all()
    frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    bad = np.flatnonzero((err > bound).any(axis=1))
    assert bad.size == 0, (tag, "first node over the bound", int(bad[0]), None if where is None else where(int(bad[0])), frac)
    return frac


def sweep_case(tag, net, form, knobs=None, chunk=0, full=True, chunks_at_least=1, same_bits_as=None):
    """one context, both data sets, the live count of chunk `chunk` swept over the nodes.  same_bits_as: a key under which the real-valued product is
    kept; a later case with the same key (the same data through another instantiation) must give the same bits"""
    p = problem(net)
    s = factored(p, form, knobs)
    try:
        info = s.streamInfo()
        assert info["splitFirst"] == s.nodes, info
        G, NL, ucols, cu, mult = geometry(s, form, knobs)
        group = ref.group_size(form, NL, info["twoPerCU"] == 1, 1)
        first, U = ref.chunk_capacity(s.ny, G, ucols, chunk, cu)
        print("\n%s: nodes %d ny %d 2nv %d G %d NL %d, units of %d columns, chunk at unit %d holds %d, group %d, %s" % (tag, s.nodes, s.ny, 2 * s.nv, G, NL, ucols, first, U, group, info))
        assert s.ny <= 1600
        if full:      # every head 0 .. group - 1 with every tail nGroups = 0 .. 4
            assert U * mult >= 5 * group - 1 and s.nodes >= min(65, U + 1) and (s.nodes - 1) * mult >= min(U * mult, 5 * group - 1), (tag, U, mult, group, s.nodes)
        assert -(-ref.whole_units(s.ny, G, ucols) // cu) >= chunks_at_least and s.nodes >= U + 1, (tag, G, ucols, s.nodes, U)
        for exact in (True, False):
            At = set_blocks(s, 3 if exact else 4, exact)
            W, counts = ref.live_count_duals(s.nodes, s.ny, G, ucols, chunk, seed=17 if exact else 18, integer=exact, chunk_units=cu)
            held = set_dual(s, W)
            if exact and not np.array_equal(held, W):
                record(tag, "(a) skipped: rn_set does not hold the integers that were set")
                continue
            W = held      # (the fp32 context rounds real values: the reference is of what it holds)
            counts, _, live = ref.live_counts(W, G, ucols, cu)
            out = s.streamProduct()
            units = s.streamUnits()
            assert set(out) == {"my"} and units == {"liveUnits": int(live.sum()), "units": s.nodes * live.shape[1], "columnsPerUnit": ucols}, (tag, units, int(live.sum()))
            col = chunk % counts.shape[1]
            frac = check_product(tag, exact, form, out["my"], At, W, G, where=lambda i: ("live per chunk", counts[i] * mult, "cell", (counts[i, col] * mult % group, counts[i, col] * mult // group)))
            cells = ref.cells(counts[:, col] * mult, group)
            want = {(n % group, n // group) for n in range(0, 5 * group, mult)}
            print("%s %s: cells (nHead, nGroups) run in the chunk: %s" % (tag, "(a)" if exact else "(b)", sorted(cells)))
            if full:
                assert want <= cells, (tag, sorted(want - cells))
            record(tag, "(a) exact" if exact else "(b) worst fraction of the bound %.3g" % frac)
            if not exact and same_bits_as is not None:
                first_tag, kept = _REAL_PRODUCTS.setdefault(same_bits_as, (tag, out["my"]))
                assert np.array_equal(kept, out["my"]), (tag, "not the bits of", first_tag)
    finally:
        s.close()


@pytest.mark.parametrize("two_per_cu", [0, 1])
@pytest.mark.parametrize("form", list(sk.FORMS))
@pytest.mark.parametrize("NL", [1, 2, 3, 4])
def test_every_head_and_tail_of_one_right_hand_side(NL, form, two_per_cu):
    net = NET_OF[NL](form)
    sweep_case("NL%d %s %s two per CU %d" % (NL, net, form, two_per_cu), net, form, {"stream_two_per_cu": two_per_cu}, same_bits_as=(net, form))


@pytest.mark.parametrize("net", ["nv128", "wide5"])
def test_last_of_several_chunks(net):
    """71 half-spans (the second chunk: a few whole units and the ragged one) and 190 spans of NL = 3 (three chunks): the sweep goes over the LAST chunk,
    the earlier ones are random"""
    sweep_case("%s f64 last chunk" % net, net, "f64", None, chunk=-1, full=False, chunks_at_least=2 if net == "nv128" else 3)


@pytest.mark.parametrize("knobs", [{"stream_half": 0}, {"stream_skip": 1}])
def test_spans_walked_whole_by_the_walk_over_units(knobs):
    """NL = 2 without the half-span skip: both units of a span are live or dead together, so the live SPANS are swept and only even counts arise"""
    sweep_case("NL2 b240 f64 %s" % knobs, "b240", "f64", knobs, same_bits_as="spans walked whole")


@pytest.mark.parametrize("net,pos,form", [("b240", "two", "f64"), ("b236", "three", "f64"), ("b240", "two", "f32")])
def test_split_round(net, pos, form):
    """the split last round: live counts 0 .. 3 group - 1 (or all the half holds) in each HALF of the split blocks, the other half and the unsplit
    blocks random; my[splitFirst:] is the product over the first workgroup's columns, my2 over the second's"""
    p, fc = ss.problem(net, pos)
    s = ss.solver(p, fc, sk.FORMS[form]["precision"])
    try:
        r = ss.position(pos, ss.num_cus())[0]
        info, _, _ = ss.expect_split(s, r)
        G, NL, ucols, cu, mult = geometry(s, form, None)
        assert NL == 2 and mult == 1 and s.ny <= 1600
        group = ref.group_size(form, NL, True, 1)
        first, cut = info["splitFirst"], info["splitSpanHalf"] * (G // ucols)      # the unit at which the second workgroup starts
        tag = "split %s %s %s" % (net, pos, form)
        for exact in (True, False):
            At = set_blocks(s, 5 if exact else 6, exact)
            for half, rng_units in enumerate(({"unit1": cut}, {"unit0": cut})):
                U = ref.chunk_capacity(s.ny, G, ucols, 0, cu, **rng_units)[1]
                top = min(3 * group - 1, U)
                seen = set()
                for launch in range(-(-(top + 1) // r)):
                    want = np.full(s.nodes, -1)
                    want[first:] = (np.arange(r) + launch * r) % (top + 1)
                    W, _ = ref.live_count_duals(s.nodes, s.ny, G, ucols, 0, seed=100 + 10 * half + launch, integer=exact, chunk_units=cu, want=want, **rng_units)
                    held = set_dual(s, W)
                    if exact:
                        assert np.array_equal(held, W), tag
                    W = held
                    counts, _, live = ref.live_counts(W, G, ucols, cu, **rng_units)
                    assert np.array_equal(counts[first:, 0], want[first:])
                    out = s.streamProduct()
                    assert set(out) == {"my", "my2"} and s.streamUnits()["liveUnits"] == int(live.sum()), (tag, s.streamUnits(), int(live.sum()))
                    where = lambda i: ("split block", i, "live per chunk of the swept half", counts[first + i])      # noqa: E731
                    fr = [check_product(tag + " unsplit blocks", exact, form, out["my"][:first], At, W, G, rows=slice(0, first)),
                          check_product(tag + " first workgroups", exact, form, out["my"][first:], At, W, G, rows=slice(first, None), col_range=(0, info["splitSpanHalf"] * G), where=where),
                          check_product(tag + " second workgroups", exact, form, out["my2"], At, W, G, rows=slice(first, None), col_range=(info["splitSpanHalf"] * G, s.ny), where=where)]
                    seen |= ref.cells(counts[first:, 0], group)
                    record("%s half %d launch %d" % (tag, half, launch), "(a) exact" if exact else "(b) worst fraction of the bound %.3g" % max(fr))
                print("%s %s half %d (%d units, group %d): cells %s" % (tag, "(a)" if exact else "(b)", half, U, group, sorted(seen)))
                assert {(n % group, n // group) for n in range(top + 1)} <= seen
    finally:
        s.close()


@pytest.mark.parametrize("form", list(sk.FORMS))
@pytest.mark.parametrize("NL", [1, 2, 3, 4])
def test_every_head_and_tail_of_two_right_hand_sides(NL, form):
    """NR = 2: the walk follows the UNION of the two vectors' live sets, which differ; my = A w and myB = A y, each bitwise the one-vector product"""
    net = NET_OF[NL](form)
    tag = "NR2 NL%d %s %s" % (NL, net, form)
    s = factored(problem(net), form, sweep_pairing="on" if form == "f64_on_f32" else "auto")
    try:
        s.setAlgorithm("namaAlgorithm", 5)
        assert s.sweepPairing()[1] == 1 and s.streamInfo()["splitFirst"] == s.nodes, (tag, s.sweepPairing(), s.streamInfo())
        G, NL_, ucols, cu, mult = geometry(s, form, None)
        group = ref.group_size(form, NL, False, 2)
        U = ref.chunk_capacity(s.ny, G, ucols, 0, cu)[1]
        print("\n%s: nodes %d ny %d 2nv %d G %d NL %d, units of %d columns, chunk 0 holds %d, group %d" % (tag, s.nodes, s.ny, 2 * s.nv, G, NL_, ucols, U, group))
        assert NL_ == NL and mult == 1 and s.ny <= 1600 and U >= 5 * group - 1 and s.nodes >= min(U, 5 * group) + 1, (tag, U, group)
        for exact in (True, False):
            At = set_blocks(s, 7 if exact else 8, exact)
            Wu, _ = ref.live_count_duals(s.nodes, s.ny, G, ucols, 0, seed=27 if exact else 28, integer=exact, chunk_units=cu)
            w, y = ref.split_pair(Wu, ucols, seed=29, integer=exact)
            y, w = set_dual(s, y, capi.BUF_XI, capi.BUF_PSI), set_dual(s, w)
            if exact:
                assert np.array_equal(ref.split_pair(Wu, ucols, seed=29)[0], w) and np.array_equal(ref.split_pair(Wu, ucols, seed=29)[1], y), tag
            counts, _, live = ref.live_counts(np.where(w != 0, w, y), G, ucols, cu)      # the union
            lw, ly = ref.live_counts(w, G, ucols, cu)[2], ref.live_counts(y, G, ucols, cu)[2]
            assert np.array_equal(lw | ly, live) and (lw & ~ly).any() and (ly & ~lw).any() and np.array_equal(counts[:, 0], np.arange(s.nodes) % (U + 1))
            out = s.streamProduct(pair=True)
            assert set(out) == {"my", "myB"} and s.streamUnits()["liveUnits"] == int(live.sum()), (tag, s.streamUnits(), int(live.sum()))
            where = lambda i: ("live per chunk, union", counts[i], "cell", (counts[i, 0] % group, counts[i, 0] // group))      # noqa: E731
            fr = [check_product(tag + " my", exact, form, out["my"], At, w, G, where=where), check_product(tag + " myB", exact, form, out["myB"], At, y, G, where=where)]
            one = s.streamProduct()["my"]
            assert s.streamUnits()["liveUnits"] == int(lw.sum())
            set_dual(s, y)
            other = s.streamProduct()["my"]
            assert np.array_equal(out["my"], one) and np.array_equal(out["myB"], other), (tag, "the pair is not bitwise the two one-vector products")
            cells = ref.cells(counts[:, 0], group)
            print("%s %s: cells (nHead, nGroups) run in chunk 0: %s" % (tag, "(a)" if exact else "(b)", sorted(cells)))
            assert {(h, g) for h in range(group) for g in range(5)} <= cells
            record(tag, "(a) exact" if exact else "(b) worst fraction of the bound %.3g" % max(fr))
    finally:
        s.close()


def test_refusals():
    p = synth.make_problem("small")
    st = capi.Solver(p["network"], p["tree"], p["config"], structured=True)
    st.factorStep()
    with pytest.raises(capi.RapidNetError, match="error -3"):      # RN_E_STATE: no blocks
        st.streamProduct()
    st.close()
    s = capi.Solver(p["network"], p["tree"], p["config"])
    with pytest.raises(capi.RapidNetError, match="error -3"):      # before the factor step
        s.streamProduct()
    s.factorStep()
    assert s.streamInfo()["splitFirst"] == s.nodes
    with pytest.raises(capi.RapidNetError):                        # nothing launched yet
        s.streamUnits()
    out = s.streamProduct()
    assert set(out) == {"my"} and out["my"].shape == (s.nodes, 2 * s.nv) and s.streamUnits()["units"] > 0
    with pytest.raises(capi.RapidNetError, match="error -3"):      # pair = 1 without the pair buffers
        s.streamProduct(pair=True)
    my, my2 = np.zeros((s.nodes, 2 * s.nv)), np.zeros((s.nodes, 2 * s.nv))
    assert s.lib.rn_debug_stream_product(s.h, 0, my.ctypes.data, my2.ctypes.data, None) == -1      # RN_E_ARG: my2 on an unsplit context
    assert s.lib.rn_debug_stream_product(s.h, 0, None, None, None) == -1
    s.close()
