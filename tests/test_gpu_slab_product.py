"""The products with the SHARED operators on the matrix cores (csrc/k_slab.hpp) ALONE, against a plain GEMM, at every edge of their schedule.

rn_debug_slab_product uploads the test's own operators through the context's padded and fragment-ordered uploads, lays the test's operands out
as the sweep's buffers are, and runs ONE launch step of the sweep's own launching code (sweep.inc: run_v_lv, run_comp, run_prep_m2, run_gemm).
Every case holds what comes back to tests/slab_product_ref.py in three ways:
 (a) integer data (and the signed patterns: one live input column per node, a marked last operator row): every sum of |terms| is below 2^24
     (fp32) or 2^53 (fp64) -- asserted on the int64 reference by the builder -- so any order of accumulation gives the reference's BITS;
 (b) normal deviates: per entry |out - ref| <= (k + 4) u (|aux| + sum_k |s M_rk in_k|), u = 2^-53 | 2^-24 -- the bound of a sum of k terms in
     any order, the epilogue's three roundings and the rounding of s = -1 / (2 p) itself; each product by itself (the second product's
     reference is taken of the v the kernel stored).  Nothing in the bound is measured.  $SLAB_PRODUCT_ERRORS names a file that receives
     the worst fraction of the bound per kernel and precision (profiles/slab_product_errors.txt);
 (c) the output buffers arrive pre-filled: rows of nodes >= nodes (the absent nodes of a last slab, the absent slabs of a last wide
     workgroup) and outputs the launch does not produce must still hold the fill; a row >= m of the last node would land there too.
The hook's info[] is held to the restated launch rules (ref.expected_launch) in every case, and every case ASSERTS the cells of the schedule
it must reach (ref.cells; the table is printed): a shape that stops reaching its cell -- another wave count, another kernel -- fails."""
import os

import numpy as np
import pytest

import slab_product_ref as ref
import test_gpu_stream_split as ss
from rapidnet_amd import capi, synth

pytestmark = pytest.mark.gpu

FORMS = ("f64", "f32")
FILL = -12345.0
# (seed index, nx, nu, nd, ne); nv = nu - ne, the v product is nv x (nv + nx), the second (nu + nx) x nv
NETS = {"g1": (60, 2, 3, 4, 1),          # k_V = 4: one group, one tile in both products
        "g16": (61, 4, 13, 5, 1),        # k_V = 16: a full single group; m_L = 17
        "g17": (62, 4, 14, 5, 1),        # k_V = 17: G = 2 with 15 padding columns; m_L = 18
        "t16": (63, 16, 17, 5, 1),       # m_V = 16 exactly, m_L = 33
        "t17": (64, 15, 18, 5, 1),       # m_V = 17
        "k48": (65, 16, 33, 5, 1),       # k_V = 48: G = 3
        "k64": (66, 20, 45, 6, 1),       # k_V = 64: one whole 64-element chunk per slab row, G = 4
        "k65": (67, 20, 46, 6, 1),       # k_V = 65: two chunks, G = 5; 3 tiles against 5
        "r2": (68, 40, 90, 8, 5),        # 6 tiles against 9: two tiles per wave with a remainder
        "r3": (69, 60, 200, 30, 20),     # 12 tiles against 17, 57 KB of LDS in fp64: three tiles per wave with a remainder
        "e48": (70, 16, 32, 5, 4),       # nu + nx = 48: the composite operator on a tile edge
        "b": (71, 63, 114, 88, 17),      # Barcelona's dimensions
        "big": (72, 30, 500, 20, 10),    # k_V = 520, k_L = 490: past the 64 KB slab in fp64 (the tile kernel); in fp32 two slab launches
        "big32": (73, 30, 1040, 20, 10)}  # k_V = 1060: past the slab in fp32 too
_PROBLEMS, _WORST = {}, {}


def problem(net, nodes):
    key = (net, nodes)
    if key not in _PROBLEMS:
        name = "slab_%s_%d" % key
        synth.CONFIGS[name] = NETS[net] + (nodes, [])      # a tree without branching: N nodes
        try:
            _PROBLEMS[key] = synth.make_problem(name)
        finally:
            del synth.CONFIGS[name]
    return _PROBLEMS[key]


def context(p, form, structured=False, knobs=None):
    s = capi.Solver(p["network"], p["tree"], p["config"], precision=form, structured=structured, knobs=knobs)
    s.factorStep()
    return s


@pytest.fixture(scope="module", autouse=True)
def error_table():
    yield
    path = os.environ.get("SLAB_PRODUCT_ERRORS")
    if path and _WORST:
        with open(path, "w") as f:
            f.write("worst |out - ref| / ((k + 4) u sum|terms|) over the cases of tests/test_gpu_slab_product.py, per kernel and precision\n")
            for (kernel, form), (frac, tag) in sorted(_WORST.items()):
                f.write("%-16s %s  %.3g  (%s)\n" % (kernel, form, frac, tag))


def layout(s, structured, knobs):
    """the launch_v_lv of this context: launch, (m, k) of the first and second product, the aux row length, ldin and the input's offset"""
    nx, nu, nv = s.nx, s.nu, s.nv
    second = (nu + nx, nv)
    if not structured:
        return dict(launch="pair", first=(nv, nv + nx), second=second, aux_rows=2 * nv, ldin=nv + nx, off=0, ldA=nv, ldB=nu + nx)
    sl = (knobs or {}).get("struct_linear", -1)
    if sl == 0:
        return dict(launch="pair", first=(nv, nv + nx), second=second, aux_rows=0, ldin=nv + nx, off=0, ldA=nv, ldB=nu + nx)
    if sl == 3:
        return dict(launch="pair", first=(nv, nv + nx + nu), second=second, aux_rows=0, ldin=nv + nx + nu, off=0, ldA=nv, ldB=nu + nx)
    if sl == 4:
        return dict(launch="pair", first=(nv, nx + nu), second=second, aux_rows=nv, ldin=nv + nx + nu, off=nv, ldA=nv, ldB=nu + nx)
    return dict(launch="comp", first=(nu + nx, nx + nu), second=None, aux_rows=nu + nx, ldin=nv + nx + nu, off=nv, ldA=None, ldB=nu + nx)


def hold_info(tag, s, form, info, lay, knobs, kind=None):
    want = ref.expected_launch(form, s.nodes, info["numCUs"], lay["first"], lay.get("second"), knobs, kind or lay["launch"])
    got = {key: info[key] for key in want}
    assert got == want, (tag, "the hook's launch is not the restated rules'", got, want)
    assert info["ldin"] == lay["ldin"] and info["inOffset"] == lay["off"] and info["outNodes"] == s.slabOutNodes(), (tag, info, lay)


def note(tag, kernel, form, frac):
    if frac > _WORST.get((kernel, form), (-1.0, ""))[0]:
        _WORST[(kernel, form)] = (frac, tag)


def hold(tag, form, got, want, k, what):
    """got [nodes][m] against the reference (value, sum of |terms|); returns the fraction of the bound (0: exact data, bits)"""
    val, mag = want
    assert got.shape == val.shape and np.isfinite(got).all(), (tag, what, got.shape, val.shape)
    if val.dtype == np.int64:
        bad = np.argwhere(got != val)
        assert bad.size == 0, (tag, what, "first wrong (node, row) of %d" % len(bad), tuple(bad[0]), "got", got[tuple(bad[0])], "want", val[tuple(bad[0])],
                               "wrong nodes", sorted(set(bad[:, 0]))[:8], "wrong rows", sorted(set(bad[:, 1]))[:8])
        return 0.0
    err, bnd = np.abs(got.astype(np.longdouble) - val), ref.bound(mag, k, form)
    frac = float(np.max(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), np.where(err > 0, np.inf, 0))))
    bad = np.argwhere(err > bnd)
    assert bad.size == 0, (tag, what, "first (node, row) over the bound", tuple(bad[0]), "fraction", frac)
    return frac


def untouched(tag, out, nodes, what, cols=slice(None)):
    rest = out[nodes:, cols] if nodes is not None else out[:, cols]
    assert (rest == FILL).all(), (tag, what, "written outside the product: %d entries, first at %s" % (int((rest != FILL).sum()), tuple(np.argwhere(rest != FILL)[0])))


def data_sets(form, nodes, lay, split, aux_on, seed):
    aux_rows = lay["aux_rows"] if aux_on else 0
    kw = dict(aux_rows=aux_rows or None, split=split, second=lay["second"])
    yield "integers", ref.integer_data(seed, form, nodes, lay["first"], **kw)
    pat = ref.signed_patterns(nodes, lay["first"], lay["second"])
    if aux_rows:      # the patterns with an aux that marks its node and row
        pat["aux"] = np.add.outer(np.arange(nodes) % 7, np.arange(aux_rows) % 5).astype(float)
        if split is not None:
            pat["aux2"] = 100.0 + np.add.outer(np.arange(nodes - split), np.arange(aux_rows) % 3).astype(float)
    v = ref.product(pat["MA"], pat["X"], pat["p"], pat["aux"], pat["aux2"], split)
    assert v[0].dtype == np.int64 and (v[1] @ np.abs(pat["MB"]).astype(np.int64).T if lay["second"] else v[1]).max() < ref.EXACT_BELOW[form]
    yield "patterns", pat
    yield "deviates", ref.real_data(seed + 1, form, nodes, lay["first"], **kw)


def run_v_lv(tag, s, form, structured, knobs, must, aux_on=True, store_modes=(True, False), seed=1):
    """the context's launch_v_lv through the hook: all data sets, v stored and not; returns the cells that ran"""
    lay = layout(s, structured, knobs)
    nodes, (m, k) = s.nodes, lay["first"]
    split = None
    if not structured:
        first = s.streamInfo()["splitFirst"]
        split = first if 0 <= first < nodes else None
    ran = set()
    for name, d in data_sets(form, nodes, lay, split, aux_on, seed):
        kept = None
        for store in (store_modes if lay["launch"] == "pair" else (True,)):
            outA, outB, info = s.slabProduct(lay["launch"], d["MA"], d["MB"], d["X"], d["aux"], d["aux2"], d["p"], storeV=store, ldA=lay["ldA"], ldB=lay["ldB"], fill=FILL)
            hold_info(tag, s, form, info, lay, knobs)
            assert info["auxSplit"] == (split if split is not None else nodes), (tag, info, split)
            t = "%s %s v %s" % (tag, name, "stored" if store else "in LDS only")
            in_lds = info["kernel"] in ("k_gemm_vlv", "k_gemm_vlv_wide")
            ran |= ref.cells({"nodes": nodes, "form": form}, info, stored_v=store or not in_lds, aux=bool(d["aux"] is not None), split=split is not None,
                             pipe2=ref.few_slabs(nodes, info["numCUs"], form, (knobs or {}).get("slab_pipe", -1)))
            if lay["launch"] == "comp":
                frac = hold(t, form, outB[:nodes], ref.product(d["MA"], d["X"], d["p"], d["aux"]), k, "[Lv; BLv] by the composite operator")
                untouched(t, outB, nodes, "[Lv; BLv]")
                note(t, info["kernel"], form, frac)
                continue
            if store or not in_lds:
                fv = hold(t, form, outA[:nodes], ref.product(d["MA"], d["X"], d["p"], d["aux"], d["aux2"], split), k, "v")
                untouched(t, outA, nodes, "v")
                fl = hold(t, form, outB[:nodes], ref.product(d["MB"], outA[:nodes], None), lay["second"][1], "[Lv; BLv] of the stored v")
                note(t, info["kernel"], form, fv)
                note(t, info["kernel2"] or info["kernel"], form, fl)
                kept = outB
            else:
                untouched(t, outA, None, "v, which this launch keeps in LDS")
                assert kept is not None and np.array_equal(outB, kept), (t, "[Lv; BLv] is not the bits of the launch that stores v")
            untouched(t, outB, nodes, "[Lv; BLv]")
    print("\n%s: %s nodes %d, %s\n   cells: %s" % (tag, form, nodes, {key: info[key] for key in ("kernel", "kernel2", "nw", "pipe", "frag", "ct", "grid", "lds", "m", "k", "kp", "ldin",
                                                                                                     "m2", "k2", "kp2")}, sorted(ran)))
    missing = set(must) - ran
    assert not missing, (tag, "cells this case must reach and did not", sorted(missing), sorted(ran))
    return ran


LOOPS = [{"slab_pipe": pipe, "slab_frag": frag} for pipe in (0, 1) for frag in (0, 1)]
# the cells each shape is there for (17 nodes: a last slab of one node behind a full one)
SHAPES = {
    "g1": {"V: G=1", "L: G=1", "V: idle waves", "L: idle waves", "V: tg=1", "L: k%4!=0", "V: m%4!=0", "L: m%4!=0", "V: chunks/row=1"},
    "g16": {"V: G=1", "V: k%16=0", "L: m%16=1"},
    "g17": {"V: G=2", "V: k%16=1", "L: m%16=other"},
    "t16": {"V: m%16=0", "L: m%16=1", "V: G=2"},
    "t17": {"V: m%16=1", "L: m%16=1"},
    "k48": {"V: G=>2", "V: k%16=0"},
    "k64": {"V: chunks/row=1", "V: k%16=0", "L: m%16=1"},
    "k65": {"V: chunks/row=2", "V: k%16=1", "V: k%4!=0", "V: m%4!=0", "L: tg=1"},
    "r2": {"L: tg=2", "L: have remainder", "V: tg=1"},
    "r3": {"V: tg=2", "L: tg=3", "L: have remainder"},
}
PIPE_CELLS = {"k48": "V: pipelined G%3=0", "k64": "V: pipelined G%3=1", "k65": "V: pipelined G%3=2", "g1": "V: pipelined G%3=1", "g17": "V: pipelined G%3=2"}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("net", list(SHAPES))
def test_pair_every_shape_loop_and_operand_copy(net, form):
    """the dense context's k_gemm_vlv on 17 nodes: SLAB_PIPE 0 | 1 x SLAB_FRAG 0 | 1, v stored and kept in LDS"""
    p = problem(net, 17)
    for knobs in LOOPS:
        s = context(p, form, knobs=knobs)
        try:
            must = set(SHAPES[net]) | {"V: k_gemm_vlv", "last slab 1 node", "V: aux yes", "v tile in LDS, v not stored", "v tile in LDS, v stored",
                                       "frag" if knobs["slab_frag"] else "column-major", "V: pipelined G%%3=%d" % (ref.pad_cols(s.nv + s.nx) // 16 % 3) if knobs["slab_pipe"] else "V: lean"}
            if knobs["slab_pipe"] and net in PIPE_CELLS:
                must.add(PIPE_CELLS[net])
            run_v_lv("pair %s %s" % (net, knobs), s, form, False, knobs, must)
        finally:
            s.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("net", ["g1", "k65"])
@pytest.mark.parametrize("nodes,cell", [(1, "last slab 1 node"), (15, "last slab 15 nodes"), (16, "last slab full"), (17, "last slab 1 node"), (33, "last slab 1 node"),
                                        (129, "rotation b>=8")])
def test_pair_node_counts(nodes, cell, net, form):
    s = context(problem(net, nodes), form)
    try:
        ran = run_v_lv("pair %s %d nodes" % (net, nodes), s, form, False, None, {cell, "V: k_gemm_vlv"})
        assert ("rotation b>=8" in ran) == (nodes > 112)
    finally:
        s.close()


@pytest.mark.parametrize("form", FORMS)
def test_pair_on_more_slabs_than_cus(form):
    """4 100+ nodes on the smallest network, a structured context (no blocks) whose sweep keeps the two dense-form products (STRUCT_LINEAR 0, no
    aux): more slabs than CUs -- the lean loop by default in fp64 and the throughput rule of slab_waves --, and the rotation's last term"""
    cus = ss.num_cus()
    nodes = 16 * max(cus, 256) + 4
    s = context(problem("g1", nodes), form, structured=True, knobs={"struct_linear": 0})
    try:
        must = {"rotation b>=8", "rotation b>=256", "V: aux none", "V: k_gemm_vlv", "V: lean" if form == "f64" else "V: pipelined G%3=1"}
        run_v_lv("pair g1 %d nodes structured" % nodes, s, form, True, {"struct_linear": 0}, must, aux_on=False)
    finally:
        s.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("net", ["g1", "k65"])
@pytest.mark.parametrize("ct,nodes,cell", [(2, 31, "2 slab(s), last slab 15 nodes"), (2, 32, "2 slab(s), last slab full"), (2, 33, "1 slab(s), last slab 1 node"),
                                           (2, 47, "1 slab(s), last slab 15 nodes"), (2, 48, "1 slab(s), last slab full"), (2, 49, "2 slab(s), last slab 1 node"),
                                           (3, 31, "2 slab(s), last slab 15 nodes"), (3, 32, "2 slab(s), last slab full"), (3, 33, "3 slab(s), last slab 1 node"),
                                           (3, 47, "3 slab(s), last slab 15 nodes"), (3, 48, "3 slab(s), last slab full"), (3, 49, "1 slab(s), last slab 1 node")])
def test_pair_wide_kernel(ct, nodes, cell, net, form):
    """k_gemm_vlv_wide<2 | 3>: last workgroups of one, two and three slabs, the last slab of 1, 15 and 16 nodes; both operand copies"""
    for frag in (0, 1):
        knobs = {"vlv_wide": ct, "slab_frag": frag}
        s = context(problem(net, nodes), form, knobs=knobs)
        try:
            run_v_lv("wide CT %d %s %d nodes frag %d" % (ct, net, nodes, frag), s, form, False, knobs,
                     {"V: k_gemm_vlv_wide", "wide CT=%d last workgroup: %s" % (ct, cell), "v tile in LDS, v not stored"})
        finally:
            s.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("aux_on", [True, False])
@pytest.mark.parametrize("sl,first_cell", [(3, "V: k_gemm_vlv"), (4, "V: k_gemm_vlv"), (-1, "C: k_gemm_comp")])
@pytest.mark.parametrize("net", ["e48", "b"])
def test_linear_forms(net, sl, first_cell, aux_on, form):
    """structured contexts: the whole linear product (knob 3: k = nv + nx + nu, no aux), the product behind the constant (knob 4: k = nx + nu read at
    offset nv of rows of nv + nx + nu, aux = c_i or none) and the default composite product (EPI_VT), on 33 nodes"""
    if sl == 3 and aux_on:
        aux_on = False      # (the form has no aux: the case runs once more with the other loop instead)
        knobs = {"struct_linear": 3, "slab_pipe": 0}
    else:
        knobs = {"struct_linear": sl} if sl >= 0 else {}
    s = context(problem(net, 33), form, structured=True, knobs=knobs)
    try:
        tg = "C" if sl < 0 else "V"
        must = {first_cell, "%s: aux %s" % (tg, "yes" if aux_on else "none"), "last slab 1 node"}
        if sl != 3:
            must.add("ldin != k, offset > 0")
        if net == "e48" and sl < 0:
            must.add("C: m%16=0")
        if net == "b" and sl < 0:
            must |= {"C: m%16=1", "C: tg=2"}
        run_v_lv("linear %s knob %d aux %s" % (net, sl, aux_on), s, form, True, knobs, must, aux_on=aux_on)
    finally:
        s.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["odd", "medium", "k65"])
def test_first_structured_product(name, form):
    """k_gemm_prep_m2 from duals of scale 50: m2 within (k + 7) u sum|terms| -- the product's (k + 4) u plus the three roundings behind every slab
    entry (d w, the sum of the two, times sqrt(p)) -- and qa_i = a_i within 3 u (1 + 3 u) of its own terms; both loops and operand copies"""
    p = synth.make_problem(name) if name in synth.CONFIGS else problem(name, 33)
    u = ref.UNIT_ROUNDOFF[form]
    for knobs in ({"struct_linear": 0}, {"struct_linear": 0, "slab_pipe": 0, "slab_frag": 0}):
        s = context(p, form, structured=True, knobs=knobs)
        try:
            nx, nu, nv, nodes = s.nx, s.nu, s.nv, s.nodes
            rng = np.random.default_rng(5)
            W = 50.0 * rng.standard_normal((nodes, 2 * nx + nu))
            s.set(capi.BUF_ACC_XI, np.ascontiguousarray(W[:, :2 * nx]).ravel())
            s.set(capi.BUF_ACC_PSI, np.ascontiguousarray(W[:, 2 * nx:]).ravel())
            W = np.concatenate([s.get(capi.BUF_ACC_XI).reshape(nodes, 2 * nx), s.get(capi.BUF_ACC_PSI).reshape(nodes, nu)], axis=1)
            M = ref.round_to(form, rng.standard_normal((nv, nx + nu)))
            outA, outB, info = s.slabProduct("prep_m2", M, ldA=2 * nv, ldB=nx, fill=FILL)
            tag = "prep_m2 %s %s %s" % (name, form, knobs)
            hold_info(tag, s, form, info, {"first": (nv, nx + nu), "ldin": nx + nu, "off": 0}, knobs, kind="prep_m2")
            stage = np.asarray(p["tree"]["stages"], int).ravel()[:nodes]
            prob = np.asarray(p["tree"]["probNode"], float).ravel()[:nodes]
            (m2, m2mag), (qa, qamag) = ref.prep_m2(M, W, stage, prob, p["config"]["matDiagPrecnd"], nx, nu, form)
            got_m2, got_qa = outA[:nodes, nv:], outB[:nodes]
            assert np.isfinite(got_m2).all() and np.isfinite(got_qa).all()
            e_qa = np.abs(got_qa.astype(np.longdouble) - qa)
            assert (e_qa <= 3 * u * (1 + 3 * u) * qamag).all(), (tag, "qa", float(np.max(e_qa / qamag)) / u)
            e_m2, bnd = np.abs(got_m2.astype(np.longdouble) - m2), ref.bound(m2mag, nx + nu, form, extra=3)
            frac = float(np.max(e_m2 / bnd))
            assert (e_m2 <= bnd).all(), (tag, "m2", frac)
            untouched(tag, outA, nodes, "m2")
            untouched(tag, outA[:nodes], None, "the m1 half of the rows", cols=slice(0, nv))
            untouched(tag, outB, nodes, "qa")
            note(tag, info["kernel"], form, frac)
            cells = ref.cells({"nodes": nodes, "form": form}, info, aux=False)
            print("\n%s: %s\n   cells: %s, m2 at %.3g of its bound" % (tag, info, sorted(cells), frac))
            assert {"M2: k_gemm_prep_m2", "M2: aux none", "frag" if knobs.get("slab_frag", 1) else "column-major"} <= cells
        finally:
            s.close()


@pytest.mark.parametrize("form", FORMS)
def test_pair_behind_a_split_last_round(form):
    """a dense context whose streaming launch splits its last round: the v product adds the second partial aux2[(i - auxSplit) ldaux + r],
    here with values of its own"""
    p, fc = ss.problem("b240", "two")
    s = ss.solver(p, fc, form)
    try:
        r = ss.position("two", ss.num_cus())[0]
        first = s.streamInfo()["splitFirst"]
        assert first == s.nodes - r, (first, s.nodes, r)
        run_v_lv("split b240 two", s, form, False, None, {"V: aux split", "V: k_gemm_vlv"}, store_modes=(True,))
    finally:
        s.close()


@pytest.mark.parametrize("net,form,kernels", [("big", "f64", ("k_gemm_shared", "k_gemm_shared")), ("big", "f32", ("k_gemm_slab", "k_gemm_slab")),
                                              ("big32", "f32", ("k_gemm_shared", "k_gemm_shared")), ("widecrown", "f64", ("k_gemm_shared", "k_gemm_slab")),
                                              ("widecrown", "f32", ("k_gemm_slab", "k_gemm_slab"))])
def test_pair_as_two_launches(net, form, kernels):
    """the pair that does not fit 64 KB: two launch_gemm calls, each k_gemm_slab or the tile kernel k_gemm_shared (fp64 from k = 509, fp32 from
    k = 1021 on); v is always stored there"""
    p = synth.make_problem(net) if net in synth.CONFIGS else problem(net, 5)
    s = context(p, form)
    try:
        must = {"V: %s" % kernels[0], "L: %s" % kernels[1]}
        if net == "big" and form == "f64":
            must |= {"V: shared mp/64=8", "L: shared mp/64=9"}
        if form == "f32" and net != "big32":      # 31 and 25 tiles on 8 waves: a second pass of the tile loop
            must |= {"V: several passes", "V: tg=3"}
        run_v_lv("two launches %s" % net, s, form, False, None, must)
    finally:
        s.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("net", ["g17", "k65"])
def test_single_products(net, form):
    """launch_gemm alone (k_gemm_slab): EPI_V with m1, EPI_LV, EPI_Z with e, and EPI_V in the linear form's layout (ldin != k)"""
    for structured, roles in ((False, (0, 1, 2)), (True, (3,))):
        s = context(problem(net, 33), form, structured=structured)
        try:
            nx, nu, nv, nodes = s.nx, s.nu, s.nv, s.nodes
            for role in roles:
                (m, k), aux_rows, scaled, ldin, off = {0: ((nv, nv + nx), 2 * nv, True, nv + nx, 0), 1: ((nu + nx, nv), 0, False, nv, 0), 2: ((nx, nu), nx, False, nu, 0),
                                                       3: ((nv, nx + nu), nv, True, nv + nx + nu, nv)}[role]
                for name, build in (("integers", ref.integer_data), ("deviates", ref.real_data)):
                    d = build(7 + role, form, nodes, (m, k), aux_rows=aux_rows or None, with_p=scaled)
                    outA, _, info = s.slabProduct("single", d["MA"], None, d["X"], d["aux"], None, d["p"], role=role, ldA=m, fill=FILL)
                    tag = "single role %d %s %s %s" % (role, net, form, name)
                    hold_info(tag, s, form, info, {"first": (m, k), "ldin": ldin, "off": off}, None, kind="single")
                    note(tag, info["kernel"], form, hold(tag, form, outA[:nodes], ref.product(d["MA"], d["X"], d["p"], d["aux"]), k, "out"))
                    untouched(tag, outA, nodes, "out")
                    assert info["kernel"] == "k_gemm_slab" and info["frag"] == 0
        finally:
            s.close()


def test_refusals():
    p = problem("g17", 17)
    s = capi.Solver(p["network"], p["tree"], p["config"])
    nv, nx, nu, nodes = s.nv, s.nx, s.nu, s.nodes
    d = ref.integer_data(1, "f64", nodes, (nv, nv + nx), aux_rows=2 * nv, second=(nu + nx, nv))
    args = lambda **kw: dict(dict(MA=d["MA"], MB=d["MB"], inp=d["X"], aux=d["aux"], prob=d["p"], ldA=nv, ldB=nu + nx), **kw)      # noqa: E731
    with pytest.raises(capi.RapidNetError, match="error -3"):      # RN_E_STATE: before the factor step
        s.slabProduct("pair", **args())
    s.factorStep()
    s.slabProduct("pair", **args())
    for wrong in (dict(aux=None), dict(aux2=d["aux"]), dict(prob=None), dict(MB=None), dict(ldA=nv + 1), dict(inp=None)):
        with pytest.raises(capi.RapidNetError, match="error -1"):      # RN_E_ARG: an operand the launch lacks or does not read, a wrong size
            s.slabProduct("pair", **args(**wrong))
    with pytest.raises(capi.RapidNetError, match="error -1"):      # a dense context's sweep never runs the composite product
        s.slabProduct("comp", d["MA"], None, d["X"], None, None, d["p"], ldB=nu + nx)
    with pytest.raises(capi.RapidNetError, match="error -1"):      # ... nor the first structured product
        s.slabProduct("prep_m2", d["MA"], ldA=2 * nv, ldB=nx)
    with pytest.raises(capi.RapidNetError, match="error -1"):      # EPI_LV has no aux and no scale
        s.slabProduct("single", d["MB"], None, d["X"][:, :nv], d["aux"], None, None, role=1, ldA=nu + nx)
    s.close()
    st = context(p, "f64", structured=True)
    with pytest.raises(capi.RapidNetError, match="error -1"):      # the default linear form runs the composite product, not the pair
        st.slabProduct("pair", **args(aux=None))
    with pytest.raises(capi.RapidNetError, match="error -1"):      # role 0 is the dense contexts'
        st.slabProduct("single", d["MA"], None, d["X"], d["aux"], None, d["p"], role=0, ldA=nv)
    st.close()


def guard_body():
    """for tests/test_gpu_guard.py: the hook's scratch buffers between red zones -- partial last slabs, the wide kernel's last workgroup, the
    linear form's offset reads, the first structured product and the tile kernel; returns the contexts it made"""
    test_pair_every_shape_loop_and_operand_copy("k65", "f64")
    test_pair_wide_kernel(3, 49, "1 slab(s), last slab 1 node", "k65", "f32")
    test_linear_forms("e48", 4, "V: k_gemm_vlv", True, "f64")
    test_linear_forms("e48", -1, "C: k_gemm_comp", True, "f32")
    test_first_structured_product("odd", "f64")
    test_pair_as_two_launches("big", "f64", ("k_gemm_shared", "k_gemm_shared"))
    return 4 + 2 + 1 + 1 + 2 + 1
