"""All per-node operator blocks set and read in one call, from host or device arrays in the reference's layout (rn_set_operators,
rn_get_operators, rn_set_operators_device, rn_get_operators_device; k_pack_operators).

The contract: the bulk calls store and return exactly the bits the per-node rn_set_operator / rn_get_operator do -- the caller's value,
rounded once to nearest where the stored (or the receiving) type is narrower -- leave what was not handed in bit for bit, and leave the
padding rows of the interleaved layout alone (the parity tests run the solver on bulk-set blocks against the fp64 oracle holding the
same blocks, at the fp64 tolerance).

Shapes, problems and helpers are test_gpu_operator_storage's; the set's properties are asserted in test_shapes_cover_the_kernels_paths."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import test_gpu_operator_storage as sto
import test_gpu_stream_split as spl
from rapidnet_amd import capi
from test_gpu_operator_storage import OPS, blocks_of, oracle_with_blocks, problem, solver
from test_gpu_parity import PAIRS, REL_TOL, compare_all, relmax
from test_gpu_sharded_batched import Ranks

pytestmark = pytest.mark.gpu

SHAPES = ["tiny", "odd", "medium", "ragged", "even4"]
KINDS = ["native", "f32", "f32ctx"]          # fp64 context with fp64 blocks, with fp32 blocks (RN_STORE_F32), fp32 context
NAMES = ("Phi", "Psi", "D", "Ftil")          # the order of the C ABI's four pointers
OP_OF = {nm: op for op, nm in OPS}
ITERS = 25
RN_E_ARG, RN_E_STATE = -1, -3


def make(kind, p, fc, **kw):
    if kind == "f32ctx":
        return solver(p, fc, storage="native", precision="f32", **kw)
    return solver(p, fc, storage=kind, **kw)


def stored(kind, v):
    """what a context of `kind` keeps of the fp64 values v"""
    return v if kind == "native" else v.astype(np.float32).astype(np.float64)


def perturbed(blocks, scale, seed):
    """random blocks around the factor step's own; (almost) no entry is fp32-representable"""
    rng = np.random.default_rng(seed)
    out = {nm: b * (1.0 + scale * rng.standard_normal(b.shape)) + 1e-3 * scale * rng.standard_normal(b.shape) for nm, b in blocks.items()}
    for nm, b in out.items():
        assert (b.astype(np.float32).astype(np.float64) != b).mean() > 0.99, nm
    return out


def on_device(blocks, dtype):
    return {nm: torch.from_numpy(np.ascontiguousarray(b.astype(dtype))).cuda() for nm, b in blocks.items()}


def addresses(t):
    return {k: (t[nm].data_ptr() if nm in t else 0) for k, nm in zip(("phi", "psi", "D", "F"), NAMES)}


def set_from_device(s, blocks, dtype):
    t = on_device(blocks, dtype)
    torch.cuda.synchronize()                              # the producer is done before the call (the context's stream does not wait for torch's)
    s.setOperatorsDevice("f64" if dtype == np.float64 else "f32", **addresses(t))
    s.synchronize()                                       # the tensors outlive the launch


def get_to_device(s, dtype, names=NAMES):
    d = sto.op_dims(s)
    t = {nm: torch.full((s.nodes, d[nm]), -7.0, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda") for nm in names}
    torch.cuda.synchronize()
    s.getOperatorsDevice("f64" if dtype == np.float64 else "f32", **addresses(t))
    s.synchronize()
    return {nm: v.cpu().numpy().astype(np.float64) for nm, v in t.items()}


def same(a, b, what):
    for nm in b:
        assert np.isfinite(a[nm]).all(), (what, nm)
        assert np.array_equal(a[nm], b[nm]), (what, nm, float(np.abs(a[nm] - b[nm]).max()))


def test_shapes_cover_the_kernels_paths():
    """the set must hold a 2 nv that is no multiple of 4 (fp32 slots reach into the padding rows), an odd nv (an fp64 slot straddles the Phi / D
    boundary, the caller's columns start off 16-byte boundaries), a block whose ny LD entries are no whole 128-byte lines (the node stride has a tail),
    unequal nu and 2 nx (the Psi / F arrays are strided differently from Phi / D), a non-uniform tree, and blocks of more than one workgroup's slots"""
    seen = {}
    for name in SHAPES:
        p, fc = problem(name)
        s = solver(p, fc, storage="native", init=False)
        nv, ny = s.nv, s.ny
        lines = {elem: (ny * (-(-2 * nv // (16 // elem)) * (16 // elem)) * elem) % 128 for elem in (8, 4)}
        nch, stage = np.asarray(p["tree"]["nChildren"], int), np.asarray(p["tree"]["stages"], int)[:len(p["tree"]["nChildren"])]
        uneven = any(len(set(nch[stage == k])) > 1 for k in set(stage))
        slots = ny * -(-2 * nv // 2)
        seen[name] = dict(nv=nv, pad4=2 * nv % 4, tail8=lines[8], tail4=lines[4], nu=s.nu, nx2=2 * s.nx, uneven=uneven, slots=slots, nodes=s.nodes)
        print("\n%-7s %s" % (name, seen[name]))
        s.close()
    v = seen.values()
    assert any(x["pad4"] != 0 for x in v) and any(x["nv"] % 2 == 1 for x in v) and any(x["nv"] % 2 == 0 for x in v), seen
    assert any(x["tail8"] != 0 for x in v) and any(x["tail4"] != 0 for x in v), seen
    assert any(x["nu"] != x["nx2"] for x in v), seen
    assert any(x["uneven"] for x in v) and seen["ragged"]["uneven"], seen
    assert any(x["slots"] > 256 for x in v) and any(x["slots"] < 256 for x in v) and any(x["nodes"] > 100 for x in v), seen


def check_bulk_equals_per_node(name, kind, guard=False):
    p, fc = problem(name)
    a, b, c = (make(kind, p, fc) for _ in range(3))
    src = perturbed(blocks_of(a), 0.3, 11)
    want = {nm: stored(kind, v) for nm, v in src.items()}
    for op, nm in OPS:
        for node in range(a.nodes):
            a.setOperator(op, node, src[nm][node])
    b.setOperators(phi=src["Phi"], psi=src["Psi"], D=src["D"], F=src["Ftil"])
    set_from_device(c, src, np.float64)
    ref = blocks_of(a)
    same(ref, want, "%s %s per node" % (name, kind))
    for tag, s in (("per node", a), ("host", b), ("device f64", c)):
        same(blocks_of(s), ref, "%s %s: %s, read per node" % (name, kind, tag))
        same(s.getOperators(), ref, "%s %s: %s, read in bulk" % (name, kind, tag))
    same(get_to_device(c, np.float64), ref, "%s %s: read into fp64 device arrays" % (name, kind))
    same(get_to_device(c, np.float32), {nm: v.astype(np.float32).astype(np.float64) for nm, v in ref.items()}, "%s %s: read into fp32 device arrays" % (name, kind))
    # fp32 arrays of the caller's: the float is what is stored (widened exactly under fp64 blocks)
    set_from_device(c, src, np.float32)
    ref32 = {nm: v.astype(np.float32).astype(np.float64) for nm, v in src.items()}
    same(blocks_of(c), ref32, "%s %s: device f32, read per node" % (name, kind))
    same(c.getOperators(), ref32, "%s %s: device f32, read in bulk" % (name, kind))
    same(get_to_device(c, np.float32), ref32, "%s %s: device f32, read into fp32 device arrays" % (name, kind))
    for s in (a, b, c):
        if guard:
            assert s.guardCheck() == 0
        s.close()


def check_partial_set(name, kind, route, guard=False):
    p, fc = problem(name)
    s = make(kind, p, fc)
    own = blocks_of(s)
    new = perturbed(own, 0.3, 5)
    want = {nm: stored(kind, v) for nm, v in new.items()}

    def put(names):
        part = {nm: new[nm] for nm in names}
        if route == "host":
            s.setOperators(**{k: part.get(nm) for k, nm in zip(("phi", "psi", "D", "F"), NAMES)})
        else:
            set_from_device(s, part, np.float64)

    put(("Phi", "Ftil"))
    for got in (blocks_of(s), s.getOperators()):
        same(got, {"Phi": want["Phi"], "Ftil": want["Ftil"], "D": own["D"], "Psi": own["Psi"]}, "%s %s %s: Phi and F given" % (name, kind, route))
    part = s.getOperators(ops=("D", "Ftil"))               # a partial get returns what was asked for
    assert sorted(part) == ["D", "Ftil"]
    same(part, {"D": own["D"], "Ftil": want["Ftil"]}, "partial get")
    if route == "device":
        same(get_to_device(s, np.float64, ("Psi",)), {"Psi": own["Psi"]}, "partial get, device")
    put(("Psi", "D"))
    for got in (blocks_of(s), s.getOperators()):
        same(got, want, "%s %s %s: then Psi and D" % (name, kind, route))
    if guard:
        assert s.guardCheck() == 0
    s.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", SHAPES)
def test_bulk_equals_per_node_bitwise(name, kind):
    check_bulk_equals_per_node(name, kind)


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("kind", ["native", "f32"])
@pytest.mark.parametrize("name", SHAPES)
def test_partial_set_leaves_the_rest_bitwise(name, kind, route):
    check_partial_set(name, kind, route)


@pytest.mark.parametrize("kind", ["native", "f32"])
@pytest.mark.parametrize("name", ["odd", "medium"])
def test_parity_with_the_oracle_on_bulk_set_blocks(name, kind):
    """test_gpu_operator_storage.test_parity_with_the_oracle_on_the_same_blocks on blocks that came in through one device-array call: a
    padding row or a neighbour's entry that the kernel had touched would show here"""
    p, fc = problem(name)
    s = make(kind, p, fc)
    set_from_device(s, perturbed(blocks_of(s), 0.02, 23), np.float64)
    o = oracle_with_blocks(p, fc, s.getOperators())
    rng = np.random.default_rng(7)
    nxi, nps = o.nodes * 2 * o.nx, o.nodes * o.nu
    for bx, bp, ox, op_ in ((capi.BUF_XI, capi.BUF_PSI, "xi", "psi"), (capi.BUF_UPD_XI, capi.BUF_UPD_PSI, "updXi", "updPsi")):
        vx, vp = rng.standard_normal(nxi) * 50, rng.standard_normal(nps) * 50
        s.set(bx, vx); s.set(bp, vp); o.set(ox, vx); o.set(op_, vp)
    s.dualExtrapolationStep(0.618); o.extrapolate(0.618)
    s.solveStep(); o.solve_step()
    s.proximalFunG(); o.prox()
    s.computeFixedPointResidual(); o.residual()
    s.dualUpdate(); o.dual_update()
    w = compare_all(s, o, REL_TOL, "%s %s, one step" % (name, kind))
    print("\none step: worst %.1e" % max(w.values()))
    assert abs(s.updatePrimalInfeasibity() - o.primal_infeasibility()) <= REL_TOL * abs(o.primal_infeasibility())
    hist, ohist = s.algorithmApg(ITERS), o.apg(ITERS)
    w = compare_all(s, o, REL_TOL, "%s %s, %d iterations" % (name, kind, ITERS))
    print("%d iterations: worst %.1e, history %.1e" % (ITERS, max(w.values()), np.abs(hist - ohist).max() / np.abs(ohist).max()))
    assert np.abs(hist - ohist).max() <= REL_TOL * np.abs(ohist).max()
    s.close()


@pytest.mark.parametrize("kind", ["native", "f32"])
@pytest.mark.parametrize("name", ["odd", "medium"])
def test_bulk_set_in_the_middle_of_a_solve(name, kind):
    """5 iterations, new blocks, 5 more: the device-array call between two batches gives the bits of the per-node calls"""
    p, fc = problem(name)
    x, y = make(kind, p, fc), make(kind, p, fc)
    new = perturbed(blocks_of(x), 0.02, 31)
    hists = []
    for s in (x, y):
        s.apgReset()
        h1 = s.apgIterate(5)
        if s is x:
            set_from_device(s, new, np.float64)
        else:
            for op, nm in OPS:
                for node in range(s.nodes):
                    s.setOperator(op, node, new[nm][node])
        hists.append(np.concatenate([h1, s.apgIterate(5)]))
    assert np.isfinite(hists[0]).all() and np.array_equal(hists[0], hists[1])
    for bid, nm in PAIRS:
        assert np.array_equal(x.get(bid), y.get(bid)), nm
    same(x.getOperators(), blocks_of(y), "blocks after the solve")
    x.close(); y.close()


@pytest.mark.parametrize("route", ["host", "device"])
def test_auto_context_becomes_dense_on_the_first_bulk_set(route):
    p, fc = problem("odd")
    a, d = solver(p, fc, storage="native", operator_mode="auto"), solver(p, fc, storage="native", operator_mode="dense")
    assert a.operatorMode() == ("auto", "structured")
    own = d.getOperators()
    new = perturbed(own, 0.3, 3)
    if route == "host":
        a.setOperators(phi=new["Phi"])
    else:
        set_from_device(a, {"Phi": new["Phi"]}, np.float64)
    assert a.operatorMode() == ("auto", "dense")
    same(a.getOperators(), {"Phi": new["Phi"], "Psi": own["Psi"], "D": own["D"], "Ftil": own["Ftil"]}, "auto, first bulk set (%s)" % route)
    a.factorStep()
    assert a.operatorMode() == ("auto", "dense")
    same(a.getOperators(), own, "auto, after the next factor step")
    same(blocks_of(a), own, "auto, after the next factor step, per node")
    a.close(); d.close()


def test_state_and_arguments():
    p, fc = problem("odd")
    lib = capi.load()
    fresh = solver(p, fc, storage="native", init=False)
    st, au, d = (solver(p, fc, storage="native", operator_mode=m) for m in ("structured", "auto", "dense"))
    dims = sto.op_dims(d)
    host = {nm: np.zeros((d.nodes, dims[nm])) for nm in NAMES}
    dev = on_device(host, np.float64)
    torch.cuda.synchronize()
    hp, dp = [host[nm].ctypes.data for nm in NAMES], [dev[nm].data_ptr() for nm in NAMES]
    n = d.nodes

    def rcs(s, nodes=n, prec=capi.RN_F64, hptr=hp, dptr=dp):
        return (lib.rn_set_operators(s.h, nodes, *hptr), lib.rn_get_operators(s.h, nodes, *hptr),
                lib.rn_set_operators_device(s.h, nodes, prec, *dptr), lib.rn_get_operators_device(s.h, nodes, prec, *dptr))

    before = d.getOperators()
    assert rcs(fresh) == (RN_E_STATE,) * 4                                       # before the factor step
    assert rcs(st) == (RN_E_STATE,) * 4                                          # no per-node blocks by request
    assert "rn_get_operator" in lib.rn_last_error(st.h).decode()
    # (gets only: a set would make the auto context dense)
    assert (lib.rn_get_operators(au.h, n, *hp), lib.rn_get_operators_device(au.h, n, capi.RN_F64, *dp)) == (RN_E_STATE, RN_E_STATE)
    assert rcs(d, nodes=n + 1) == (RN_E_ARG,) * 4 and rcs(d, nodes=n - 1) == (RN_E_ARG,) * 4 and rcs(d, nodes=0) == (RN_E_ARG,) * 4
    assert rcs(d, hptr=[None] * 4, dptr=[None] * 4) == (RN_E_ARG,) * 4
    for prec in (7, -1, 2):
        assert (lib.rn_set_operators_device(d.h, n, prec, *dp), lib.rn_get_operators_device(d.h, n, prec, *dp)) == (RN_E_ARG, RN_E_ARG)
    with pytest.raises(capi.RapidNetError):
        d.setOperators()
    with pytest.raises(ValueError):
        d.setOperators(phi=np.zeros(3))
    same(d.getOperators(), before, "after refused calls")                        # none of them wrote a block
    assert st.operatorMode() == ("structured", "structured") and au.operatorMode() == ("auto", "structured")
    for s in (fresh, st, au, d):
        s.close()


def test_auto_context_without_blocks_refuses_the_get():
    p, fc = problem("tiny")
    a = solver(p, fc, storage="native", operator_mode="auto")
    dims = sto.op_dims(a)
    out = np.zeros((a.nodes, dims["Phi"]))
    t = torch.zeros((a.nodes, dims["Phi"]), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert a.lib.rn_get_operators(a.h, a.nodes, out.ctypes.data, None, None, None) == RN_E_STATE
    assert "rn_get_operator" in a.lib.rn_last_error(a.h).decode()
    assert a.lib.rn_get_operators_device(a.h, a.nodes, capi.RN_F64, t.data_ptr(), None, None, None) == RN_E_STATE
    assert a.operatorMode() == ("auto", "structured")
    a.close()


def test_three_ranks_bulk_set_their_local_rows():
    p, fc = problem("medium")
    full = solver(p, fc, storage="native")
    glob = perturbed(full.getOperators(), 0.02, 41)              # [nodes of the full tree][dim]
    full.close()
    rk = Ranks(p, 3, 2)
    try:
        rk.run(lambda s: s.initialiseSmpcController(*fc))
        for i, s in enumerate(rk.shards):
            rows = np.asarray(s.global_nodes, int)
            mine = {nm: np.ascontiguousarray(b[rows]) for nm, b in glob.items()}
            if i == 1:
                s.setOperators(phi=mine["Phi"], psi=mine["Psi"], D=mine["D"], F=mine["Ftil"])
            else:
                set_from_device(s, mine, np.float64)
            same(s.getOperators(), mine, "rank %d" % i)

        def solve(s):
            s.apgReset()
            return np.concatenate([s.apgIterate(20), s.apgIterate(ITERS - 20)])

        hists = rk.run(solve)
        o = None
        for s in rk.shards:
            if o is None:
                o = oracle_with_blocks(p, fc, s.getOperators(), nodes_of=s.global_nodes)
            else:
                for nm, b in s.getOperators().items():
                    o.buf(nm).reshape(o.nodes, b.shape[1])[np.asarray(s.global_nodes, int)] = b
        ohist = o.apg(ITERS)
        for h in hists:
            assert np.array_equal(h, hists[0]) and np.abs(h - ohist).max() <= REL_TOL * np.abs(ohist).max()
        d = spl.dims_of(rk.shards[0])
        for nm, bid, dm in spl.VECS:
            assert relmax(rk.gathered(bid, d[dm]), o.get(nm)) < REL_TOL, nm
    finally:
        rk.close()


@pytest.mark.parametrize("name", ["odd", "ragged"])
def test_under_the_buffer_guard(monkeypatch, name):
    """RAPIDNET_GUARD=1: every buffer of the context between red zones and NaN until written.  The bitwise tests again: a slot read outside a
    block would bring a NaN into a block that is read back (same() asserts finiteness), a slot written outside a buffer changes a red zone"""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    for kind in KINDS:
        check_bulk_equals_per_node(name, kind, guard=True)
    for kind in ("native", "f32"):
        for route in ("host", "device"):
            check_partial_set(name, kind, route, guard=True)
    gc.collect()
    after = capi.guard_report()
    assert after[0] == before[0] + 3 * len(KINDS) + 4 and after[1] == before[1], (before, after)


def test_host_forms_leave_the_contexts_memory_as_it_was():
    p, fc = problem("medium")
    s = solver(p, fc, storage="f32")
    own = s.getOperators()                      # (first use: whatever the runtime sets up once is set up)
    m0 = s.deviceMemoryInfo()["context_bytes"]
    s.setOperators(phi=own["Phi"], psi=own["Psi"], D=own["D"], F=own["Ftil"])
    m1 = s.deviceMemoryInfo()["context_bytes"]
    again = s.getOperators()
    m2 = s.deviceMemoryInfo()["context_bytes"]
    assert m0 == m1 == m2 and m0 > 0, (m0, m1, m2)
    same(again, own, "a round trip of the stored values")
    info = (C.c_size_t * 4)()
    assert s.lib.rn_device_memory_info(s.h, C.addressof(info)) == 0 and info[2] == m0
    s.close()
