"""Box and safety bounds per stage or per node, replaced in place (rn_set_bounds, rn_set_bounds_device, rn_get_bounds_layout, rn_get_bounds;
k_tree_data writes the tables and the scaled bounds, the dual kernels find a node's row by two strides).

The contract: a set with the factor step's own vectors changes nothing, a shared set is bit for bit a context whose network carries those
vectors, equal rows give the same bits at every granularity, and distinct rows agree with the CPU oracle whose scaled per-node bounds were
overwritten in the same way -- in every operator mode and storage type, through the flat dual update (`odd`, `ragged`, `small`: ny is no
whole number of 16-byte vectors), the stage-tiled one (`tiny`, `medium` with the fused walk off) and the fused walk + dual update (the
same two with the default), after 5 iterations (the exact path) and after 40 (device-resident batches), unsharded and sharded.

Reference snapshots are computed once per (tree, mode, kind, fused walk) and shared."""
import gc

import numpy as np
import pytest
import torch

from oracle.oracle import Oracle
from rapidnet_amd import capi
from test_gpu_device_pointer import _d2h
from test_gpu_fbe_nama import compare_fbe
from test_gpu_parity import FP32_TOL, REL_TOL, compare_all, relmax
from test_gpu_sharded_batched import Ranks
from test_gpu_tree_data import ALL_BUFS, KINDS, MODES, TREES, last_four, make, problem, same

pytestmark = pytest.mark.gpu

RN_E_ARG, RN_E_STATE = -1, -3
KEYS = ("xmin", "xmax", "xsafe", "umin", "umax")
NET = {"xmin": "vecXmin", "xmax": "vecXmax", "xsafe": "vecXsafe", "umin": "vecUmin", "umax": "vecUmax"}
BOUND_BUFS = {"xmin": capi.BUF_XMIN, "xmax": capi.BUF_XMAX, "xsafe": capi.BUF_XS, "umin": capi.BUF_UMIN, "umax": capi.BUF_UMAX}
SHORT, LONG = 5, 40

ALL_TREES = TREES + ["medium"]        # ny = 12, 27, 23, 19 and 80: of TREES only `tiny` is eligible for the stage-tiled kernels
STAGE_TILED = ("tiny", "medium")

_REF = {}


def fuses(name):
    """settings of the fused walk + dual update a case runs with: a tree whose ny is odd takes the flat k_dual_fused whatever the setting;
    the others run k_dual_stage with the fused walk off (0) and k_down_chain_dual with the default (-1)"""
    return (0, -1) if name in STAGE_TILED else (-1,)


def own_bounds(p):
    return {k: np.asarray(p["network"][NET[k]], float)[None, :].copy() for k in KEYS}


def moved(b):
    """new values for a shared set"""
    out = {k: v.copy() for k, v in b.items()}
    out["xsafe"] *= 1.15
    out["xmax"] *= 0.9
    out["umax"] *= 0.8
    return out


def stage_factors(N):
    s = np.arange(N)
    t = s / (N - 1)
    return {"xsafe": 1 + 0.5 * t, "xmax": 1 - 0.2 * t, "umax": 1 - 0.4 * (s % 3) / 2}


def staged(p):
    """distinct rows per stage: xsafe_t = xsafe (1 + 0.5 t), xmax_t = xmax (1 - 0.2 t), umax_t = umax (1 - 0.4 (stage mod 3) / 2), t = stage / (N - 1)"""
    N = int(p["tree"]["N"][0])
    f = stage_factors(N)
    return {k: np.repeat(v, N, axis=0) * (f[k][:, None] if k in f else 1.0) for k, v in own_bounds(p).items()}


def stages_of(tree):
    return np.asarray(tree["stages"], int)


def second_of_last_stage(tree):
    """every second node of the last stage"""
    st = stages_of(tree)
    return np.flatnonzero(st == st.max())[::2]


def per_node(rows, tree, extra=False):
    out = {k: v[stages_of(tree)].copy() for k, v in rows.items()}
    if extra:
        out["xsafe"][second_of_last_stage(tree)] *= 1.25
    return out


def oracle_scale(o, tree, extra=False):
    """the same factors on the oracle's scaled per-node bounds (after its factor step)"""
    st = stages_of(tree)
    f = stage_factors(o.N)
    for key, name, dim in (("xsafe", "xs", o.nx), ("xmax", "xmax", o.nx), ("umax", "umax", o.nu)):
        v = o.get(name).reshape(o.nodes, dim) * f[key][st][:, None]
        if extra and key == "xsafe":
            v[second_of_last_stage(tree)] *= 1.25
        o.set(name, v)


def context(name, mode, kind, fuse, network=None, tree=None):
    p, fc, _ = problem(name)
    s = make(p if network is None else dict(p, network=network), p["tree"] if tree is None else tree, mode, kind)
    if fuse != -1:
        s.setFusedWalkDual(fuse)
    s.initialiseSmpcController(*fc)
    return s


def snap(s, hist):
    out = {"history": np.array(hist)}
    for bid, nm in ALL_BUFS:
        out[nm] = s.get(bid)
    return out


def run(s, fc):
    """5 iterations (the exact path), then a fresh solve of 40 (device-resident batches)"""
    a = snap(s, last_four(s, fc, SHORT))
    b = snap(s, last_four(s, fc, LONG))
    return a, b


def same2(got, want, what):
    for g, w, n in zip(got, want, (SHORT, LONG)):
        same(g, w, "%s, %d iterations" % (what, n))


def reference(name, mode, kind, fuse, which):
    """which = "untouched": the factor step's own bounds; "moved": a fresh context whose network JSON carries moved(own)"""
    key = (name, mode, kind, fuse, which)
    if key not in _REF:
        p, fc, _ = problem(name)
        net = None
        if which == "moved":
            net = dict(p["network"])
            for k, v in moved(own_bounds(p)).items():
                net[NET[k]] = v[0].tolist()
        s = context(name, mode, kind, fuse, network=net)
        _REF[key] = run(s, fc)
        s.close()
    return _REF[key]


# ---- 0. the three dual kernels are in fact covered ---------------------------------------------------------------------------------------
def test_the_trees_cover_the_three_dual_kernels():
    for name in ALL_TREES:
        p, fc, _ = problem(name)
        s = context(name, "dense", "f64", -1)
        ki = s.kernelInfo()
        ny = 2 * s.nx + s.nu
        if name not in STAGE_TILED:
            assert ny % 2 != 0 and ki["dual_stage"] == 0, (name, ki)          # the flat k_dual_fused, regen branch
        else:
            assert ki["dual_stage"] == 1 and ki["dual_pipe"] > 0, (name, ki)  # k_dual_stage; with the fused walk on: k_down_chain_dual
            assert 0 <= ki["chain_stage"] < s.N, (name, ki)                   # there are chains for the fused walk to take
        s.close()
        f = make(p, p["tree"], "dense", "f32")
        f.initialiseSmpcController(*fc)
        assert f.kernelInfo()["dual_stage"] == (1 if name in STAGE_TILED else 0), name
        f.close()


# ---- 1. no-op ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ALL_TREES)
def test_a_set_with_the_factor_steps_own_vectors_changes_nothing(name, mode, kind):
    p, fc, _ = problem(name)
    for fuse in fuses(name):
        s = context(name, mode, kind, fuse)
        s.setBounds("shared", **own_bounds(p))
        assert s.boundsLayout() == (capi.BOUNDS_SHARED, 1)
        same2(run(s, fc), reference(name, mode, kind, fuse, "untouched"), "%s %s %s fuse %d: no-op" % (name, mode, kind, fuse))
        if mode == "auto":
            assert s.operatorMode() == ("auto", "structured")
        s.close()


# ---- 2. shared, new values -----------------------------------------------------------------------------------------------------------------
# ---- 3. granularity equivalence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ALL_TREES)
def test_shared_set_is_bitwise_a_fresh_context_and_equal_rows_give_the_same_bits(name, mode, kind):
    p, fc, _ = problem(name)
    new = moved(own_bounds(p))
    N = int(p["tree"]["N"][0])
    for fuse in fuses(name):
        want = reference(name, mode, kind, fuse, "moved")
        s = context(name, mode, kind, fuse)
        s.apgReset()
        s.apgIterate(7)                                   # a context in use
        s.setBounds("shared", **new)
        same2(run(s, fc), want, "%s %s %s fuse %d: shared" % (name, mode, kind, fuse))
        # per stage with N equal rows
        s.setBounds("stage", **{k: np.repeat(v, N, axis=0) for k, v in new.items()})
        assert s.boundsLayout() == (capi.BOUNDS_PER_STAGE, N)
        same2(run(s, fc), want, "%s %s %s fuse %d: per stage, equal rows" % (name, mode, kind, fuse))
        # distinct rows per stage, and per node built from them
        rows = staged(p)
        s.setBounds("stage", **rows)
        st = run(s, fc)
        assert not np.array_equal(st[1]["u"], want[1]["u"])
        s.setBounds("node", **per_node(rows, p["tree"]))
        assert s.boundsLayout() == (capi.BOUNDS_PER_NODE, s.nodes)
        same2(run(s, fc), st, "%s %s %s fuse %d: per node from the per-stage rows" % (name, mode, kind, fuse))
        s.setBounds("stage", **rows)                      # and back (the per-stage table is kept)
        same2(run(s, fc), st, "%s %s %s fuse %d: per stage again" % (name, mode, kind, fuse))
        s.close()


# ---- 4. parity with the fp64 oracle on distinct rows ---------------------------------------------------------------------------------------
def oracle_runs(name, precision, extra):
    """the oracle with the stage factors on its scaled bounds, after 5 and after 40 iterations; asserts first that the factors have teeth"""
    p, fc, _ = problem(name)

    def solve(scale, iters):
        o = Oracle(p["network"], p["tree"], p["config"], precision=precision)
        o.factor_step()
        if scale:
            oracle_scale(o, p["tree"], extra)
        o.update_state_control()
        o.eliminate(*fc)
        hist = o.apg(iters)
        return o, hist

    plain, _ = solve(False, LONG)
    o40, h40 = solve(True, LONG)
    du = np.abs(o40.get("u") - plain.get("u")).max() / np.abs(plain.get("u")).max()
    dx = np.abs(o40.get("x") - plain.get("x")).max() / np.abs(plain.get("x")).max()
    print("\n%s %s: the per-stage bounds move u by %.1e and x by %.1e of their maxima" % (name, precision, du, dx))
    assert du >= 1e-2, (name, du)
    o5, h5 = solve(True, SHORT)
    return (o5, h5), (o40, h40)


def check_parity(name, mode, precision, gran, extra=False, guard=False):
    p, fc, _ = problem(name)
    tol = REL_TOL if precision == "f64" else FP32_TOL
    oracles = oracle_runs(name, precision, extra)
    rows = staged(p)
    for fuse in fuses(name):
        s = context(name, mode, precision, fuse)
        if gran == "stage":
            s.setBounds("stage", **rows)
        else:
            s.setBounds("node", **per_node(rows, p["tree"], extra))
        for (o, ohist), iters in zip(oracles, (SHORT, LONG)):
            hist = last_four(s, fc, iters)
            what = "%s %s %s %s fuse %d, %d iterations" % (name, mode, precision, gran, fuse, iters)
            w = compare_all(s, o, tol, what)
            print("%s: worst %.1e, history %.1e" % (what, max(w.values()), np.abs(hist - ohist).max() / np.abs(ohist).max()))
            assert np.abs(hist - ohist).max() <= tol * np.abs(ohist).max(), what
            for key, nm in (("xsafe", "xs"), ("xmax", "xmax"), ("umax", "umax"), ("xmin", "xmin"), ("umin", "umin")):
                assert relmax(s.get(BOUND_BUFS[key]), o.get(nm)) <= (1e-15 if precision == "f64" else 1e-6), (what, nm)
        if guard:
            assert s.guardCheck() == 0
        s.close()


# `medium` (added to the four trees for the stage-tiled kernels at more than one workgroup per stage) is held to the oracle in fp64 only: FP32_TOL
# was set for the four small trees, and an fp32 residual of its 80-column rows after 40 iterations is noisier than that (the fp32 stage-tiled
# kernels are held to the oracle on `tiny` and, bit for bit across granularities, on `medium` above)
PARITY = [(n, pr) for n in ALL_TREES for pr in ("f64", "f32") if (n, pr) != ("medium", "f32")]


@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name,precision", PARITY)
def test_per_stage_bounds_match_the_oracle(name, mode, precision):
    check_parity(name, mode, precision, "stage")


@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name,precision", PARITY)
def test_per_node_bounds_match_the_oracle(name, mode, precision):
    check_parity(name, mode, precision, "node", extra=True)


# ---- 5. quasi-Newton loops -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("alg", ["globalFbeAlgorithm", "namaAlgorithm"])
@pytest.mark.parametrize("name", ["odd", "small"])
def test_quasi_newton_loops_after_a_per_stage_set(name, alg, mode):
    p, fc, _ = problem(name)
    iters = 10
    o = Oracle(p["network"], p["tree"], p["config"])
    o.set_algorithm(alg, 5)
    o.factor_step()
    oracle_scale(o, p["tree"])
    o.update_state_control()
    o.eliminate(*fc)
    o.fbe_reset()
    ho, vo, to = o.fbe_nama(iters)
    s = make(p, p["tree"], mode, "f64")
    s.initialiseSmpcController(*fc)
    s.setAlgorithm(alg, 5)
    s.setBounds("stage", **staged(p))
    s.fbeReset()
    hs, vs, ts = s._algorithmFbeNama(iters)
    assert np.array_equal(ts, to), (ts, to)
    assert relmax(vs, vo) < REL_TOL
    assert relmax(hs, ho) < 1e-7
    compare_fbe(s, o, alg, 1e-8, "%s %s %s after a per-stage set" % (alg, name, mode))
    s.close()


# ---- 6. routes -----------------------------------------------------------------------------------------------------------------------------
def on_device(b, dtype):
    t = {k: torch.from_numpy(np.ascontiguousarray(v.astype(dtype))).cuda() for k, v in b.items()}
    torch.cuda.synchronize()            # the producer is done before the call (the context's stream does not wait for torch's)
    return t


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["f64", "f32"])
@pytest.mark.parametrize("gran", ["shared", "stage", "node"])
@pytest.mark.parametrize("name", ["odd", "tiny"])
def test_device_form_is_bitwise_the_host_form(name, gran, kind, dtype):
    p, fc, _ = problem(name)
    rows = {"shared": moved(own_bounds(p)), "stage": staged(p), "node": per_node(staged(p), p["tree"], True)}[gran]
    if dtype == np.float32:            # values an fp32 array can hold, so that both routes are given the same numbers
        rows = {k: v.astype(np.float32).astype(np.float64) for k, v in rows.items()}
    h = context(name, "dense", kind, -1)
    h.setBounds(gran, **rows)
    want = run(h, fc)
    wb = h.getBounds()
    h.close()
    d = context(name, "dense", kind, -1)
    t = on_device(rows, dtype)
    d.setBoundsDevice(gran, "f64" if dtype == np.float64 else "f32", **{k: v.data_ptr() for k, v in t.items()})
    got = run(d, fc)                    # no synchronize in between: everything is ordered on the context's stream
    same2(got, want, "%s %s %s: device form (%s)" % (name, gran, kind, dtype.__name__))
    gb = d.getBounds()
    stored = (lambda v: v.astype(np.float32).astype(np.float64)) if kind == "f32" else (lambda v: v)
    for k in KEYS:
        assert np.array_equal(gb[k], wb[k]) and np.array_equal(gb[k], stored(rows[k])), k      # a get round-trips
    d.close()
    del t


# ---- 7. persistence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_bounds_persist_across_a_reweighting_and_the_factor_step_resets_them(mode, kind):
    name = "ragged"
    p, fc, new = problem(name)
    rows = staged(p)
    a = context(name, mode, kind, -1)
    a.setBounds("stage", **rows)
    a.setTreeData(prob=new["probNode"])
    assert a.boundsLayout() == (capi.BOUNDS_PER_STAGE, a.N)
    ra = run(a, fc)
    b = context(name, mode, kind, -1)
    b.setTreeData(prob=new["probNode"])
    b.setBounds("stage", **rows)
    same2(run(b, fc), ra, "%s %s: set bounds then re-weight, and the other order" % (mode, kind))
    for k, v in a.getBounds().items():
        assert np.array_equal(v, b.getBounds()[k]), k
    c = context(name, mode, kind, -1, tree=dict(p["tree"], probNode=new["probNode"]))       # a context created on the re-weighted tree
    c.setBounds("stage", **rows)
    same2(run(c, fc), ra, "%s %s: a context of the new tree" % (mode, kind))
    c.close(); b.close()
    # the factor step returns the context to the shared bounds of rn_system
    a.setTreeData(prob=p["tree"]["probNode"])
    a.factorStep()
    assert a.boundsLayout() == (capi.BOUNDS_SHARED, 1)
    for k, v in own_bounds(p).items():
        assert np.array_equal(a.getBounds()[k], v.astype(np.float32).astype(np.float64) if kind == "f32" else v), k
    same2(run(a, fc), reference(name, mode, kind, -1, "untouched"), "%s %s: after another factor step" % (mode, kind))
    a.close()


def test_an_auto_context_that_becomes_dense_keeps_its_bounds():
    name = "small"
    p, fc, _ = problem(name)
    rows = staged(p)
    d = context(name, "dense", "f64", -1)
    d.setBounds("stage", **rows)
    want = run(d, fc)
    ops = d.getOperators()
    d.close()
    a = context(name, "auto", "f64", -1)
    a.setBounds("stage", **rows)
    assert a.operatorMode() == ("auto", "structured")
    a.setOperators(phi=ops["Phi"])                         # the caller's own block: the context becomes dense
    assert a.operatorMode()[1] == "dense" and a.boundsLayout() == (capi.BOUNDS_PER_STAGE, a.N)
    same2(run(a, fc), want, "auto -> dense with per-stage bounds")
    a.close()


# ---- 8. partial update ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64", "f32"])
@pytest.mark.parametrize("gran", ["shared", "stage", "node"])
def test_partial_update(gran, kind):
    name = "odd"
    p, fc, _ = problem(name)
    rows = {"shared": own_bounds(p), "stage": staged(p), "node": per_node(staged(p), p["tree"])}[gran]
    s = context(name, "dense", kind, -1)
    ptr, n, prec = s.devicePointer(capi.BUF_XS)           # the node-major copies exist from here on
    s.setBounds(gran, **rows)
    m0 = s.deviceMemoryInfo()["context_bytes"]
    b0 = s.getBounds()
    scaled0 = {k: s.get(bid) for k, bid in BOUND_BUFS.items()}
    s.setBounds(gran, xsafe=rows["xsafe"] * 1.3)
    assert s.deviceMemoryInfo()["context_bytes"] == m0
    b1 = s.getBounds()
    stored = (lambda v: v.astype(np.float32).astype(np.float64)) if kind == "f32" else (lambda v: v)
    assert np.array_equal(b1["xsafe"], stored(rows["xsafe"] * 1.3))
    for k in ("xmin", "xmax", "umin", "umax"):
        assert np.array_equal(b1[k], b0[k]), k
        assert np.array_equal(s.get(BOUND_BUFS[k]), scaled0[k]), k
    xs = s.get(capi.BUF_XS)
    assert not np.array_equal(xs, scaled0["xsafe"])
    # the scaled values: sqrt(p_i) d_c xsafe, in the context's type
    assert relmax(xs, scaled0["xsafe"] * 1.3) < (1e-15 if kind == "f64" else 2e-7)
    s.synchronize()
    for k, bid in BOUND_BUFS.items():                     # the node-major copies show the new scaled values, the same arrays as before
        q, m, pr = s.devicePointer(bid)
        assert np.array_equal(_d2h(q, m, pr), s.get(bid)), k
    assert (ptr, n, prec) == s.devicePointer(capi.BUF_XS)
    s.close()


# ---- 9. controlAction(project=True) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gran", ["stage", "node"])
def test_control_action_projects_on_the_roots_row(gran):
    name = "small"
    p, fc, _ = problem(name)
    # the unprojected control, to choose a per-stage umax whose row 0 binds
    s = context(name, "dense", "f64", -1)
    u_free = s.controlAction(*fc, maxIterations=20)
    rows = staged(p)
    rows["umax"][0] = np.minimum(rows["umax"][0], np.maximum(0.5 * np.abs(u_free), 0.25 * rows["umax"][0]))
    assert (rows["umax"][0] >= rows["umin"][0]).all()
    f0 = rows["umax"][0] / own_bounds(p)["umax"][0]
    s.setBounds(gran, **(rows if gran == "stage" else per_node(rows, p["tree"])))
    u0 = s.controlAction(*fc, maxIterations=20, project=True)
    o = Oracle(p["network"], p["tree"], p["config"])
    o.factor_step()
    oracle_scale(o, p["tree"])
    um = o.get("umax").reshape(o.nodes, o.nu)
    um[0] = um[0] / stage_factors(o.N)["umax"][0] * f0
    o.set("umax", um)
    o.update_state_control()
    uo = o.control_action(*fc, max_iterations=20, project=True)
    raw = o.get("u")[: o.nu]
    assert (np.abs(raw - uo) > 1e-6 * np.abs(raw).max()).any(), "row 0 of umax must bind"
    assert relmax(u0, uo) < REL_TOL
    s.close()


# ---- 10. sharded ---------------------------------------------------------------------------------------------------------------------------
def check_shards(world, gran, structured=False):
    p, fc, _ = problem("medium")
    rows = staged(p)
    full = per_node(rows, p["tree"], True)
    u = make(p, p["tree"], "structured" if structured else "dense", "f64")
    u.initialiseSmpcController(*fc)
    u.setBounds(gran, **(rows if gran == "stage" else full))
    uh = last_four(u, fc, 24)
    dims = {"nx": u.nx, "nu": u.nu, "nv": u.nv, "2nx": 2 * u.nx}
    vecs = ((capi.BUF_X, "x", "nx"), (capi.BUF_U, "u", "nu"), (capi.BUF_V, "v", "nv"), (capi.BUF_UPD_XI, "updXi", "2nx"), (capi.BUF_UPD_PSI, "updPsi", "nu"),
            (capi.BUF_XS, "xs", "nx"), (capi.BUF_XMAX, "xmax", "nx"), (capi.BUF_UMAX, "umax", "nu"))
    want = {nm: u.get(bid) for bid, nm, _ in vecs}
    u.close()
    rk = Ranks(p, world, 0, structured)
    try:
        def solve(s):
            s.initialiseSmpcController(*fc)
            if gran == "stage":
                s.setBounds("stage", **rows)
            else:                                       # the LOCAL rows, in the order of rn_shard_global_nodes
                g = np.asarray(s.global_nodes, int)
                s.setBounds("node", **{k: v[g] for k, v in full.items()})
            return last_four(s, fc, 24)

        hists = rk.run(solve)
        for h in hists:
            assert np.array_equal(h, hists[0])
            assert np.abs(h - uh).max() <= 1e-9 * np.abs(uh).max()
        for bid, nm, dm in vecs:
            assert relmax(rk.gathered(bid, dims[dm]), want[nm]) < 1e-9, nm
        return [s.guardCheck() for s in rk.shards]
    finally:
        rk.close()


@pytest.mark.parametrize("gran", ["stage", "node"])
@pytest.mark.parametrize("world,structured", [(2, False), (3, False), (3, True)])
def test_shards_take_per_stage_rows_and_local_per_node_rows(world, structured, gran):
    check_shards(world, gran, structured)


# ---- 11. errors ----------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_state():
    name = "odd"
    p, fc, _ = problem(name)
    s = make(p, p["tree"], "dense", "f64")
    lib = s.lib
    b = {k: np.ascontiguousarray(v) for k, v in own_bounds(p).items()}
    ptrs = lambda d: [None if d[k] is None else d[k].ctypes.data for k in KEYS]      # noqa: E731
    assert lib.rn_set_bounds(s.h, capi.BOUNDS_SHARED, 1, *ptrs(b)) == RN_E_STATE                  # before the factor step
    g, r = capi.C.c_int(0), capi.C.c_size_t(0)
    assert lib.rn_get_bounds_layout(s.h, capi.C.byref(g), capi.C.byref(r)) == RN_E_STATE
    s.initialiseSmpcController(*fc)
    s.apgReset()
    s.apgIterate(6)
    rows = {k: np.ascontiguousarray(v) for k, v in staged(p).items()}
    s.setBounds("stage", **rows)
    N, n = s.N, s.nodes
    before = snap(s, [])
    before.update({"b." + k: v for k, v in s.getBounds().items()})
    m0 = s.deviceMemoryInfo()["context_bytes"]
    for gran, cnt in ((capi.BOUNDS_PER_STAGE, N + 1), (capi.BOUNDS_PER_STAGE, 1), (capi.BOUNDS_SHARED, N), (capi.BOUNDS_PER_NODE, N), (capi.BOUNDS_PER_NODE, n + 1), (3, N), (-1, 1)):
        assert lib.rn_set_bounds(s.h, gran, cnt, *ptrs(rows)) == RN_E_ARG, (gran, cnt)            # wrong rows / granularity
    assert lib.rn_set_bounds(s.h, capi.BOUNDS_PER_STAGE, N, None, None, None, None, None) == RN_E_ARG     # all NULL
    one_missing = dict(b, umin=None)
    assert lib.rn_set_bounds(s.h, capi.BOUNDS_SHARED, 1, *ptrs(one_missing)) == RN_E_ARG         # a changed granularity with one NULL array
    assert "all five" in lib.rn_last_error(s.h).decode()
    bad = {k: v.copy() for k, v in rows.items()}
    bad["xmin"][N // 2, 1] = bad["xmax"][N // 2, 1] * 1.5 + 1.0
    assert lib.rn_set_bounds(s.h, capi.BOUNDS_PER_STAGE, N, *ptrs(bad)) == RN_E_ARG               # xmin > xmax
    only = dict.fromkeys(KEYS)
    only["umax"] = rows["umin"] - 1.0
    assert lib.rn_set_bounds(s.h, capi.BOUNDS_PER_STAGE, N, *ptrs(only)) == RN_E_ARG              # umax alone, below the umin the context holds
    for v in (float("nan"), float("inf"), -float("inf")):
        bad = {k: w.copy() for k, w in rows.items()}
        bad["xsafe"][N - 1, 0] = v
        assert lib.rn_set_bounds(s.h, capi.BOUNDS_PER_STAGE, N, *ptrs(bad)) == RN_E_ARG, v
    with pytest.raises(ValueError):
        s.setBounds("stage", xsafe=np.ones(3))
    assert lib.rn_get_bounds(s.h, 1, *ptrs(b)) == RN_E_ARG
    assert lib.rn_get_bounds(s.h, N, None, None, None, None, None) == RN_E_ARG
    # the device form: precision and pointers
    t = on_device(rows, np.float64)
    dp = [t[k].data_ptr() for k in KEYS]
    for prec in (7, -1, 2):
        assert lib.rn_set_bounds_device(s.h, capi.BOUNDS_PER_STAGE, N, prec, *dp) == RN_E_ARG
    assert lib.rn_set_bounds_device(s.h, capi.BOUNDS_PER_STAGE, N, capi.RN_F64, rows["xmin"].ctypes.data, *dp[1:]) == RN_E_ARG    # a host pointer
    assert "device memory" in lib.rn_last_error(s.h).decode()
    assert lib.rn_set_bounds_device(s.h, capi.BOUNDS_PER_STAGE, N, capi.RN_F64, dp[0] + 4, *dp[1:]) == RN_E_ARG                  # misaligned
    assert lib.rn_set_bounds_device(s.h, capi.BOUNDS_PER_STAGE, N + 1, capi.RN_F64, *dp) == RN_E_ARG
    assert lib.rn_set_bounds_device(s.h, capi.BOUNDS_SHARED, 1, capi.RN_F64, dp[0], None, None, None, None) == RN_E_ARG
    after = snap(s, [])
    after.update({"b." + k: v for k, v in s.getBounds().items()})
    for k in before:
        assert np.array_equal(before[k], after[k]), k            # none of the refused calls changed anything
    assert s.boundsLayout() == (capi.BOUNDS_PER_STAGE, N)
    # host-form calls at a granularity already in force allocate nothing
    s.setBounds("stage", **rows)
    s.setBounds("stage", umax=rows["umax"])
    s.getBounds()
    assert s.deviceMemoryInfo()["context_bytes"] == m0
    s.setBoundsDevice("stage", "f64", **{k: v.data_ptr() for k, v in t.items()})
    assert s.deviceMemoryInfo()["context_bytes"] == m0
    s.apgIterate(1)
    s.close()
    del t


# ---- 12. guard mode ------------------------------------------------------------------------------------------------------------------------
def test_under_the_buffer_guard(monkeypatch):
    """RAPIDNET_GUARD=1: every buffer of the context between red zones and NaN until written: a row read outside the caller's arrays or the
    tables would bring a NaN into what is compared (same() and relmax() assert finiteness), a write outside a buffer changes a red zone"""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    saved = dict(_REF)
    _REF.clear()                       # (the reference contexts are made under the guard too)
    try:
        for name, mode, kind in (("tiny", "dense", "f64"), ("odd", "structured", "f32")):       # case 3
            p, fc, _ = problem(name)
            new, N = moved(own_bounds(p)), int(p["tree"]["N"][0])
            for fuse in fuses(name):
                s = context(name, mode, kind, fuse)
                s.setBounds("stage", **{k: np.repeat(v, N, axis=0) for k, v in new.items()})
                same2(run(s, fc), reference(name, mode, kind, fuse, "moved"), "guard: per stage, equal rows")
                rows = staged(p)
                s.setBounds("stage", **rows)
                st = run(s, fc)
                s.setBounds("node", **per_node(rows, p["tree"]))
                same2(run(s, fc), st, "guard: per node from the per-stage rows")
                assert s.guardCheck() == 0
                s.close()
        check_parity("tiny", "dense", "f64", "stage", guard=True)                                  # case 4
        check_parity("ragged", "dense", "f64", "node", extra=True, guard=True)
        check_parity("odd", "structured", "f32", "node", extra=True, guard=True)
        assert check_shards(3, "stage") == [0, 0, 0]                                               # case 10
        assert check_shards(2, "node") == [0, 0]
    finally:
        _REF.clear()
        _REF.update(saved)
    gc.collect()
    after = capi.guard_report()
    assert after[0] > before[0] and after[1] == before[1], (before, after)
