"""rn_solve_certificate / rn_solve_certificate_device (k_certificate, k_plan.hpp; csrc/certificate.inc): the dual bound and optimality gap of
the multiplier a context holds, against the numpy restatement tests/certificate_oracle.py.

B  end to end, fp64 contexts: every sum column (COST, INNER, SUPPORT, DIST_X^2, DIST_S^2, NORM_X^2, NORM_S^2) within 1e-9 -- the project's fp64
   tolerance -- of its own sum|terms| of the restatement on the CPU ORACLE's solve step at the oracle's y+, DUAL, PRIMAL and GAP within 1e-9
   ABS_TERMS; after 0 (reset), 1, 16, 23 and 37 iterations (both parities of the rotating buffers, inside and at the end of a batch).  Two
   places where these bounds contradict themselves are singled out and nothing else is widened: a squared column that is rounding dust on BOTH
   sides (is_dust), and PRIMAL / GAP where the penalty terms exceed ABS_TERMS, so that the tolerance granted to DIST^2 is already more than 1e-9
   ABS_TERMS of PRIMAL (derived_tol).  The kernel's Hz(y) is held to (F x(y), G u(y)) of the problem's definition entry by entry (check_hz).
A  the kernel alone.  The restatement is fed what the context itself holds, and every getter used returns doubles: RN_BUF_CERT_X / _CERT_U,
   RN_BUF_UPD_XI / _UPD_PSI, RN_BUF_ALPHA, the scaled bounds RN_BUF_XMIN ... _UMAX (the bits the prox and k_certificate form), Hz(y) through
   rn_debug_certificate_hz, the physical rows of rn_get_bounds for U_EXCESS, probNode of rn_get_tree_data (rounded to fp32 for an fp32 context,
   whose kernels read its fp32 copy); costW and prevU have no getter: what the test handed in, rounded likewise.  Both sides then sum the same
   exact fp64 terms.  Bound, derived from the kernel's operation count and not fitted: the kernel forms a term with at most 3 roundings (INNER,
   NORM^2: one product; SUPPORT: one product per candidate; DIST^2: one subtraction and one square; fp32 inputs: the products are exact) and
   adds it along a chain of at most m = m_lane + 18 + ceil(B / 256) additions -- m_lane terms of a lane's grid-stride positions (B = eltBlocks
   workgroups of 256 lanes over nodes * ny elements, 16 bytes at a time), 6 + 3 for the wave and the workgroup's 4 waves, ceil(B / 256) + 6 + 3
   for the last arriver's fold -- and the restatement rounds its longdouble sum once: |gpu - numpy| <= gamma(m + 4) sum|terms|, gamma(k) = k u /
   (1 - k u), u = 2^-53.  COST sums per node what k_plan_report's node phase leaves (nu products alpha u, nu^2 + nu of du' W du, 6 for its wave
   and 1 for its two waves), times p_i, along the same chain over the nodes: gamma(nu^2 + 2 nu + 8 + m + 4) of the sum of the |.| of the
   ELEMENTS' terms.  U_EXCESS and XIS_POS are bit for bit; DIST and NORM are compared squared (the record holds their correctly rounded roots:
   one more rounding each, 2 u relative on the square).
Invariance, other data and precisions, shards, refusals and guard mode: see each test.

When CERTIFICATE_ERRORS names a file, the worst ratios of every case are appended to it (profiles/certificate_errors.txt is such a file)."""
import gc
import os
import types

import numpy as np
import pytest

import certificate_oracle as co
import first_principles as fp
from oracle.oracle import Oracle
from rapidnet_amd import capi
from test_certificate_oracle import problem
from test_gpu_device_pointer import _d2h
from test_gpu_operator_storage import blocks_of
from test_gpu_parity import FP32_TOL
from test_gpu_sharded_batched import Ranks
from test_gpu_tree_data import make, reweighted
from test_plan_oracle import ORACLE_BUF, scaled_bounds, table_for, tree_arrays

pytestmark = pytest.mark.gpu

RN_E_ARG, RN_E_STATE = -1, -3
U = 2.0 ** -53
TOL = 1e-9
COUNTS = (0, 1, 16, 23, 37)
SQUARED = {"dist2X": "distX", "dist2S": "distS", "norm2X": "normX", "norm2S": "normS"}
ALL_BUFS = tuple(range(capi.BUF_UDIR + 1))      # every RN_BUF_* from before the certificate, the scaled bounds included
_ORACLE = {}


def record(line):
    print(line)
    path = os.environ.get("CERTIFICATE_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def f32_if(kind, a):
    a = np.asarray(a, float)
    return a.astype(np.float32).astype(np.float64) if kind == "f32" else a


def gamma(k):
    return k * U / (1.0 - k * U)


def sum_of(rec, col):
    """the value of a sum column of a record (dict by capi.CERT_COLUMNS): roots squared"""
    return rec[SQUARED[col]] ** 2 if col in SQUARED else rec[col]


def is_dust(want, col, got):
    """A squared column that is rounding dust on both sides.  y+ = w + lambda (Hx - z) and Hz - clamp(Hz) are differences: where a whole half of
    them cancels -- xi_s on `tiny`: 1e-17 beside 1e+3 in xi_b -- what is left is the rounding of the operands, at most u = 2^-53 of the
    largest |.| of the vector per entry, on the GPU and on the oracle alike, and dust does not agree with dust to 1e-9 of itself.  Only then,
    when BOTH sums are below n (u max)^2, is the column not compared further; every other case is held to 1e-9 of its own sum."""
    if col not in SQUARED:
        return False
    thr = want["terms"][col] * (U * want["maxY" if col.startswith("norm") else "maxHz"]) ** 2
    return want["sums"][col] < thr and got < thr


def derived_tol(want, col, tol):
    """tol ABS_TERMS for DUAL, PRIMAL and GAP -- wherever the penalty terms gamma_x DIST_X + gamma_s DIST_S of PRIMAL and GAP do not exceed
    ABS_TERMS.  Where they do (penalties of 1e+6: 1e+10 beside an ABS_TERMS of 1e+3 at y = 0) the bound contradicts the one on DIST^2: a DIST^2
    within tol of itself is a DIST within tol / 2 of itself (or within sqrt(tol DIST^2) where that is less), i.e. a PRIMAL that has moved by
    gamma times that -- more than tol ABS_TERMS.  There, and only there, PRIMAL and GAP are granted exactly that much on top."""
    out = tol * want["absTerms"]
    if col == "dual" or want["penalties"] <= want["absTerms"]:
        return out
    for g, d in ((want["gammaX"], want["distX"]), (want["gammaS"], want["distS"])):
        out += g * min(0.5 * tol * d * (1.0 + tol), np.sqrt(tol) * d)
    return out


def ubox_of(p, tree, gran):
    if gran is None:
        return co.physical_ubox(p["network"], int(tree["nodes"][0]))
    rows, brow = table_for(p, gran, tree)
    return rows["umin"][brow], rows["umax"][brow]


def oracle_records(name, gran=None, tree=None, tag=None, counts=COUNTS, blocks=None):
    """{count: restatement on the CPU oracle's solve step at its y+ after `count` iterations from cold}; computed once per case, not changed.
    blocks ({name: [nodes][dim]}, with a tag): the oracle's per-node operator blocks are overwritten by these -- a context's fp32-stored ones"""
    key = (name, gran, tag, counts)
    if key not in _ORACLE:
        p, fc = problem(name)
        tree = p["tree"] if tree is None else tree
        o = Oracle(p["network"], tree, p["config"])
        o.factor_step()
        bounds = None
        if gran is not None:
            rows, brow = table_for(p, gran, tree)
            for k, v in scaled_bounds(p, tree, rows, brow).items():
                o.set(ORACLE_BUF[k], v)
            bounds = dict(rows, granularity=gran)
        o.update_state_control()
        o.eliminate(*fc)
        for nm, b in (blocks or {}).items():
            o.buf(nm).reshape(o.nodes, b.shape[1])[:] = b
        m = fp.Model(p["network"], tree, p["config"], fc, probNode=tree["probNode"], errorDemandNode=tree["errorDemandNode"],
                     errorPriceNode=tree["errorPriceNode"], bounds=bounds)
        ubox = ubox_of(p, tree, gran)
        o.apg_reset()
        theta, done, out = [1.0, 1.0], 0, {}
        for c in counts:
            if c > done:
                theta = list(o.apg_continue(c - done, theta))
                done = c
            out[c] = co.oracle_certificate(o, m, ubox)
        _ORACLE[key] = out
    return _ORACLE[key]


def check_b(what, rec, want, tol=TOL):
    """a record against the restatement on the oracle's iterates; returns the worst ratio to the tolerance"""
    worst = 0.0
    for col in co.SUM_COLUMNS:
        if is_dust(want, col, sum_of(rec, col)):
            continue
        err, scale = abs(sum_of(rec, col) - want["sums"][col]), want["sumabs"][col]
        assert err <= tol * scale, (what, col, sum_of(rec, col), want["sums"][col], err / max(scale, 1e-300))
        worst = max(worst, err / (tol * scale) if scale > 0 else 0.0)
    for col in ("dual", "primal", "gap"):
        err, bound = abs(rec[col] - want[col]), derived_tol(want, col, tol)
        assert err <= bound, (what, col, rec[col], want[col], err / bound)
        worst = max(worst, err / bound)
    assert abs(rec["absTerms"] - want["absTerms"]) <= tol * want["absTerms"], what
    assert rec["valid"] == want["valid"], (what, rec, want["normX"], want["normS"], want["xisPos"])
    return worst


def held(s, p, tree, kind, prevU=None):
    """the restatement on what the context holds (A); returns (restatement, bound of every sum column)"""
    n, nx, nu = s.nodes, s.nx, s.nu
    parent, stage = tree_arrays(tree)
    sc = {k: s.get(b).reshape(n, -1) for k, b in (("xmin", capi.BUF_XMIN), ("xmax", capi.BUF_XMAX), ("xs", capi.BUF_XS), ("umin", capi.BUF_UMIN), ("umax", capi.BUF_UMAX))}
    m = types.SimpleNamespace(nodes=n, nx=nx, nu=nu, p=f32_if(kind, s.getTreeData()["prob"]), W=f32_if(kind, p["config"]["costW"]).reshape(nu, nu).T,
                              alpha=s.get(capi.BUF_ALPHA).reshape(n, nu), anc=parent, u_root=f32_if(kind, np.ravel(p["config"]["prevU"]) if prevU is None else prevU),
                              gammaX=float(np.ravel(p["config"]["penaltyStateX"])[0]), gammaS=float(np.ravel(p["config"]["penaltySafetyX"])[0]), **sc)
    b = s.getBounds()
    brow = {capi.BOUNDS_SHARED: np.zeros(n, int), capi.BOUNDS_PER_STAGE: stage, capi.BOUNDS_PER_NODE: np.arange(n)}[b["granularity"]]
    r = co.certificate(s.get(capi.BUF_CERT_X), s.get(capi.BUF_CERT_U), s.get(capi.BUF_UPD_XI), s.get(capi.BUF_UPD_PSI), m, (b["umin"][brow], b["umax"][brow]),
                       hz=s.debugCertificateHz())
    # sum|terms| of COST by ELEMENT (the node phase of k_plan_report sums elements, k_certificate sums nodes)
    u = s.get(capi.BUF_CERT_U).reshape(n, nu).astype(np.longdouble)
    du = u.copy()
    du[1:] -= u[parent[1:]]
    du[0] -= m.u_root
    elem = (m.p * (np.abs(m.alpha * u).sum(axis=1) + ((np.abs(du) @ np.abs(m.W).astype(np.longdouble)) * np.abs(du)).sum(axis=1))).sum()
    ntot = n * (2 * nx + nu)
    B = max(1, min(1024, -(-ntot // 1024)))      # eltBlocks

    def chain(items, per):
        """additions between a term and the result: a lane's positions (vectors of `per` elements and a scalar tail), then the folds"""
        vectors = -(-items // per)
        return per * -(-vectors // (256 * B)) + 1 + 18 + -(-B // 256)

    mflat, mnode = chain(ntot, 4 if kind == "f32" else 2), chain(n, 1)
    bound = {c: gamma(mflat + 4) * r["sumabs"][c] for c in co.SUM_COLUMNS}
    for c in SQUARED:
        bound[c] += 2 * U * r["sumabs"][c]
    bound["cost"] = gamma(nu * nu + 2 * nu + 8 + mnode + 4) * float(elem)
    return r, bound


def check_hz(what, s, p, tree, kind):
    """Hz(y) as k_certificate read it against (F x(y), G u(y)) of the definition (first_principles.Model's fx, fs, g on the probabilities the
    context holds) applied to RN_BUF_CERT_X / _CERT_U, entry by entry: the sweep forms an entry as (sqrt(p_i) d_c) * value -- a square root and
    two products in the context's type, 3 roundings -- and so does the model in fp64: bound 8 eps |entry|, eps = 2^-53 (fp32 contexts: eps =
    2^-24, and the stage diagonal is rounded to fp32 on its way in: 10 eps)"""
    fc = synth_forecast(p)
    t = s.getTreeData()
    m = fp.Model(p["network"], tree, p["config"], fc, probNode=f32_if(kind, t["prob"]))
    x, u = s.get(capi.BUF_CERT_X), s.get(capi.BUF_CERT_U)
    hxi, hpsi = s.debugCertificateHz()
    eps, k = (2.0 ** -24, 10.0) if kind == "f32" else (U, 8.0)
    for got, ref, nm in ((hxi, m.Fx(x).ravel(), "F x"), (hpsi, (m.g * u.reshape(m.nodes, m.nu)).ravel(), "G u")):
        bad = np.abs(got - ref) > k * eps * np.abs(ref)
        assert not bad.any(), (what, nm, int(bad.sum()), float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max() / eps))


def synth_forecast(p):
    from rapidnet_amd import synth
    return synth.forecast_at(p["forecast"], 0)


def check_a(what, rec, s, p, tree, kind, prevU=None):
    """the kernel against the restatement of its own inputs; returns the worst share of the bound used"""
    r, bound = held(s, p, tree, kind, prevU)
    check_hz(what, s, p, tree, kind)
    assert all(np.isfinite(rec[k]) for k in capi.CERT_COLUMNS), (what, rec)
    worst = 0.0
    for col in co.SUM_COLUMNS:
        err = abs(sum_of(rec, col) - r["sums"][col])
        assert err <= bound[col], (what, col, sum_of(rec, col), r["sums"][col], err / max(bound[col], 1e-300))
        worst = max(worst, err / bound[col] if bound[col] > 0 else 0.0)
    assert bits(rec["uExcess"]) == bits(r["uExcess"]) and bits(rec["xisPos"]) == bits(r["xisPos"]), (what, rec["uExcess"], r["uExcess"], rec["xisPos"], r["xisPos"])
    total = bound["cost"] + bound["inner"] + bound["support"] + gamma(4) * r["absTerms"]
    assert abs(rec["dual"] - r["dual"]) <= total and abs(rec["absTerms"] - r["absTerms"]) <= total, what
    return worst


def context(name, mode, kind, gran=None, tree=None, **kw):
    p, fc = problem(name)
    s = make(p, p["tree"] if tree is None else tree, mode, kind, **kw)
    s.initialiseSmpcController(*fc)
    if gran is not None:
        s.setBounds(gran, **table_for(p, gran, tree)[0])
    return s


def walk(what, s, p, tree, kind, want=None, counts=COUNTS, tol=TOL):
    """certificates after every count of `counts` (cumulative, from a reset): A always, B where `want` holds the oracle's records"""
    s.apgReset()
    done, wa, wb, out = 0, 0.0, 0.0, {}
    for c in counts:
        if c > done:
            s.apgIterate(c - done)
            done = c
        rec = s.solveCertificate()
        wa = max(wa, check_a("%s, %d iterations" % (what, c), rec, s, p, tree, kind))
        if want is not None:
            wb = max(wb, check_b("%s, %d iterations" % (what, c), rec, want[c], tol))
        out[c] = rec
    record("%s: A %.3f of the bound%s" % (what, wa, "; B %.2e of the tolerance" % wb if want is not None else ""))
    return out


# ---- 1. cold solves against the oracle and against what the context holds ------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "structured", "auto"])
@pytest.mark.parametrize("name", ["tiny", "small", "odd", "ragged"])
def test_record_after_a_cold_solve(name, mode):
    p, fc = problem(name)
    s = context(name, mode, "f64")
    out = walk("%s %s f64" % (name, mode), s, p, p["tree"], "f64", oracle_records(name))
    assert out[0]["inner"] == 0.0 and out[0]["support"] == 0.0 and out[0]["valid"] == 1.0 and out[0]["dual"] == out[0]["cost"]      # y = 0: the unconstrained minimum
    s.close()


@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name", ["medium", "barcelona31"])
def test_record_on_the_larger_trees(name, mode):
    p, fc = problem(name)
    s = context(name, mode, "f64")
    walk("%s %s f64" % (name, mode), s, p, p["tree"], "f64", oracle_records(name))
    s.close()


# ---- 2. the solve goes on as if nobody had asked --------------------------------------------------------------------------------------------
def snapshot(s):
    out = {bid: s.get(bid) for bid in ALL_BUFS if s.lib.rn_buffer_size(s.h, bid) > 0}
    out["last_solve"] = s.last_solve()
    return out


@pytest.mark.parametrize("name,mode,first,second,restart", [("odd", "dense", 17, 20, False), ("odd", "structured", 17, 20, False), ("ragged", "dense", 16, 23, False),
                                                            ("small", "structured", 40, 17, True)])
def test_a_call_between_two_batches_leaves_the_solve_untouched(name, mode, first, second, restart):
    p, fc = problem(name)
    a, b = context(name, mode, "f64"), context(name, mode, "f64")
    hist = []
    for s in (a, b):
        if restart:
            s.setRestart("gradient")
            n, h1 = s.apg_solve(first, 0.0, 10)
            assert n == first
        else:
            s.apgReset()
            h1 = s.apgIterate(first)
        hist.append([h1])
    r1 = a.solveCertificate()      # (no snapshot in front: in the structured mode this call meets the pending v product of the batch's last sweep)
    m2 = a.deviceMemoryInfo()["context_bytes"]
    r2 = a.solveCertificate()
    assert a.deviceMemoryInfo()["context_bytes"] == m2                      # the first call allocated, the second did not ...
    ptr = a.solveCertificateDevice()
    a.synchronize()
    assert a.deviceMemoryInfo()["context_bytes"] == m2                      # ... nor the third
    assert all(bits(r1[k]) == bits(r2[k]) for k in capi.CERT_COLUMNS)       # two calls, the same bits
    assert np.array_equal(bits(_d2h(ptr, capi.CERT_COLS, "f64")[:len(capi.CERT_COLUMNS)]), bits([r1[k] for k in capi.CERT_COLUMNS]))
    after, twin = snapshot(a), snapshot(b)
    assert set(after) == set(twin)
    for k in twin:
        same = after[k] == twin[k] if k == "last_solve" else np.array_equal(bits(after[k]), bits(twin[k]))
        assert same, (name, mode, "buffer %s changed under the certificate" % k)
    for s, h in zip((a, b), hist):
        h.append(s.apgIterate(second))                                      # (16 and more: an optimistic batch follows)
    assert np.array_equal(bits(np.concatenate(hist[0])), bits(np.concatenate(hist[1])))
    after, twin = snapshot(a), snapshot(b)
    for k in twin:
        same = after[k] == twin[k] if k == "last_solve" else np.array_equal(bits(after[k]), bits(twin[k]))
        assert same, (name, mode, "buffer %s differs %d iterations later" % (k, second))
    if restart:
        assert a.last_restarts() == b.last_restarts()
    a.close(); b.close()


# ---- 3. other data and precisions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,kind,gran", [("odd", "dense", "f64", "stage"), ("ragged", "structured", "f64", "node"), ("odd", "dense", "f64_store32", "node")])
def test_record_under_bounds_per_stage_and_per_node_and_fp32_stored_blocks(name, mode, kind, gran):
    p, fc = problem(name)
    s = context(name, mode, kind, gran)
    # fp32-stored blocks: the same fp64 bounds, against the oracle given the blocks AS THE CONTEXT STORES THEM (rounded to fp32; the sweep
    # accumulates them in fp64), as tests/test_gpu_operator_storage.py pins that storage -- the oracle's own blocks are another problem's
    blocks = blocks_of(s) if kind == "f64_store32" else None
    walk("%s %s %s, %s rows" % (name, mode, kind, gran), s, p, p["tree"], "f64", oracle_records(name, gran, tag=kind if blocks else None, blocks=blocks))
    s.close()


@pytest.mark.parametrize("mode", ["dense", "structured"])
def test_record_after_a_reweighting_and_refusal_while_a_probability_of_zero_is_in_force(mode):
    import torch

    name = "ragged"
    p, fc = problem(name)
    new = reweighted(p["tree"], fc, 7)
    s = context(name, mode, "f64")
    s.apgReset()
    s.apgIterate(3)
    s.updateTree(new)
    out = np.zeros(capi.CERT_COLS)
    assert s.lib.rn_solve_certificate(s.h, out.ctypes.data) == RN_E_STATE          # the affine terms are the old tree's
    s.updateStateControl()
    s.eliminateInputDistubanceCoupling(*fc)
    walk("%s %s f64 after rn_set_tree_data" % (name, mode), s, p, new, "f64", oracle_records(name, tree=new, tag="reweighted", counts=(1, 23)), counts=(1, 23))
    # a probability of 0 (the device form takes it): the affine terms are refused while it is in force, and so is the certificate -- the sweep
    # divides by p_i, there is no z(y)
    prob = np.asarray(new["probNode"], float).copy()
    prob[-1] = 0.0
    t = torch.from_numpy(prob).cuda()
    torch.cuda.synchronize()
    s.setTreeDataDevice("f64", prob=t.data_ptr())
    s.synchronize()
    assert s.lib.rn_solve_certificate(s.h, out.ctypes.data) == RN_E_STATE
    s.updateStateControl()
    assert s.lib.rn_eliminate_input_disturbance_coupling(s.h, np.ascontiguousarray(fc[0], float).ctypes.data, np.ascontiguousarray(fc[1], float).ctypes.data) == RN_E_ARG
    assert s.lib.rn_solve_certificate(s.h, out.ctypes.data) == RN_E_STATE
    s.close()
    del t


@pytest.mark.parametrize("name,mode", [("odd", "dense"), ("ragged", "structured"), ("barcelona31", "dense")])
def test_fp32_contexts(name, mode):
    p, fc = problem(name)
    s, d = context(name, mode, "f32"), context(name, mode, "f64")
    got = walk("%s %s f32" % (name, mode), s, p, p["tree"], "f32", counts=(0, 1, 23))
    d.apgReset()
    done, worst = 0, 0.0
    for c in (0, 1, 23):
        if c > done:
            d.apgIterate(c - done)
            done = c
        want = d.solveCertificate()
        want["gammaX"], want["gammaS"] = float(np.ravel(p["config"]["penaltyStateX"])[0]), float(np.ravel(p["config"]["penaltySafetyX"])[0])
        want["penalties"] = want["gammaX"] * want["distX"] + want["gammaS"] * want["distS"]
        for col in ("dual", "primal", "gap", "cost", "inner", "support"):
            err = abs(got[c][col] - want[col]) / derived_tol(want, col, FP32_TOL)
            worst = max(worst, err)
            assert err <= 1.0, (name, mode, c, col, got[c][col], want[col])
    record("%s %s f32 against the f64 context's record: worst %.2e of the tolerance (FP32_TOL %.0e of ABS_TERMS)" % (name, mode, worst, FP32_TOL))
    s.close(); d.close()


# ---- 4. shards: every rank the same bits, the one-GPU record within 1e-12 of sum|terms| ------------------------------------------------------------
def u_excess_of(u, lo, hi):
    return float(np.maximum(np.maximum(lo - u, u - hi), 0.0).max())


@pytest.mark.parametrize("world,structured", [(2, False), (3, True)])
def test_shards_hold_the_whole_trees_record(world, structured):
    """Two records per rank.  OWN: the certificate of the shards' own solve -- every rank the same bits; the maxima bit for bit the MAX over the
    ranks of what each rank's own u(y) and y+ give; the sums within 1e-12 of sum|terms| of the one-GPU context's (measured: 1.6e-15 after 24
    iterations summed in another order at the cut).  SAME: every shard is then given the one-GPU context's y+, so that all evaluate one multiplier -- the
    sums within 1e-12 of sum|terms| of the one-GPU record (another summation order); XIS_POS, a function of y+ alone, bit for bit; U_EXCESS bit
    for bit wherever the shards' u(y) rows are bitwise the one-GPU rows, and otherwise (the sweep sums in another order at the cut: 1 ulp of 462
    apart on 3 ranks) within 1e-12 of max |u(y)|."""
    name = "medium"
    p, fc = problem(name)
    nx = int(np.ravel(p["network"]["nx"])[0])
    one = context(name, "structured" if structured else "dense", "f64")
    one.apgReset()
    one.apgIterate(24)
    want = one.solveCertificate()
    r, _ = held(one, p, p["tree"], "f64")
    src = {bid: one.get(bid) for bid in (capi.BUF_UPD_XI, capi.BUF_UPD_PSI)}
    one_u = one.get(capi.BUF_CERT_U).reshape(one.nodes, -1)
    one.close()
    lo, hi = co.physical_ubox(p["network"], one_u.shape[0])
    rk = Ranks(p, world, 0, structured)
    try:
        def solve(s):
            s.initialiseSmpcController(*fc)
            s.apgReset()
            s.apgIterate(24)
            g = np.asarray(s.global_nodes, int)
            own = s.solveCertificate()
            own_u, own_xis = s.get(capi.BUF_CERT_U).reshape(len(g), -1), s.get(capi.BUF_UPD_XI).reshape(len(g), -1)[:, nx:]
            for bid, dim in ((capi.BUF_UPD_XI, 2 * s.nx), (capi.BUF_UPD_PSI, s.nu)):
                s.set(bid, src[bid].reshape(-1, dim)[g])
            a = s.solveCertificate()
            return dict(own=own, own_u=own_u, own_xis=own_xis, a=a, b=s.solveCertificate(), u=s.get(capi.BUF_CERT_U).reshape(len(g), -1), g=g, bad=s.guardCheck())

        out = rk.run(solve)
        worst = worst_own = 0.0
        own_uexc = max(u_excess_of(o["own_u"], lo[o["g"]], hi[o["g"]]) for o in out)
        own_xis = max(max(float(o["own_xis"].max()), 0.0) for o in out)
        same_u = all(np.array_equal(bits(o["u"]), bits(one_u[o["g"]])) for o in out)
        for rank, o in enumerate(out):
            assert o["bad"] == 0
            own, a = o["own"], o["a"]
            for k in capi.CERT_COLUMNS:
                assert bits(own[k]) == bits(out[0]["own"][k]), (rank, k)                               # every rank the same bits
                assert bits(a[k]) == bits(out[0]["a"][k]) == bits(o["b"][k]), (rank, k)                # ... and every call
            assert bits(own["uExcess"]) == bits(own_uexc) and bits(own["xisPos"]) == bits(own_xis), (rank, own["uExcess"], own_uexc, own["xisPos"], own_xis)
            for col in co.SUM_COLUMNS:
                if not is_dust(r, col, sum_of(own, col)):
                    e = abs(sum_of(own, col) - sum_of(want, col))
                    assert e <= 1e-12 * r["sumabs"][col], (rank, "own solve", col, e / max(r["sumabs"][col], 1e-300))
                    worst_own = max(worst_own, e / r["sumabs"][col] if r["sumabs"][col] > 0 else 0.0)
                err = abs(sum_of(a, col) - sum_of(want, col))
                assert err <= 1e-12 * r["sumabs"][col], (rank, col, err / max(r["sumabs"][col], 1e-300))
                worst = max(worst, err / r["sumabs"][col] if r["sumabs"][col] > 0 else 0.0)
            assert abs(a["dual"] - want["dual"]) <= 1e-12 * r["absTerms"] and abs(a["primal"] - want["primal"]) <= 1e-12 * (r["absTerms"] + r["penalties"])
            print("rank %d: U_EXCESS %r (one GPU %r), XIS_POS %r (one GPU %r), u(y) bitwise the one-GPU rows: %s" % (rank, a["uExcess"], want["uExcess"], a["xisPos"],
                                                                                                                 want["xisPos"], same_u))
            assert bits(a["xisPos"]) == bits(want["xisPos"])
            assert bits(a["uExcess"]) == bits(want["uExcess"]) if same_u else abs(a["uExcess"] - want["uExcess"]) <= 1e-12 * float(np.abs(one_u).max())
            assert a["valid"] == want["valid"] == own["valid"]
        record("medium on %d shards (%s): every rank the same bits; the same y+: sums worst %.2e of sum|terms| against the one-GPU record (u(y) bitwise equal: %s); "
               "the shards' own solve: %.2e" % (world, "structured" if structured else "dense", worst, same_u, worst_own))
    finally:
        rk.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_state():
    p, fc = problem("odd")
    s = make(p, p["tree"], "dense", "f64")
    lib, C = s.lib, capi.C
    out, ptr = np.zeros(capi.CERT_COLS), C.c_void_p()

    def both():
        return lib.rn_solve_certificate(s.h, out.ctypes.data), lib.rn_solve_certificate_device(s.h, C.byref(ptr))

    assert both() == (RN_E_STATE,) * 2                                                      # before the factor step
    s.factorStep()
    s.updateStateControl()
    assert both() == (RN_E_STATE,) * 2                                                      # before the affine terms
    s.eliminateInputDistubanceCoupling(*fc)
    m0 = s.deviceMemoryInfo()["context_bytes"]
    assert lib.rn_solve_certificate(s.h, None) == RN_E_ARG and lib.rn_solve_certificate_device(s.h, None) == RN_E_ARG
    assert lib.rn_buffer_size(s.h, capi.BUF_CERT_X) == 0 and lib.rn_buffer_size(s.h, capi.BUF_CERT_U) == 0
    hz = np.zeros(s.nodes * 2 * s.nx)
    assert lib.rn_debug_certificate_hz(s.h, hz.ctypes.data, hz.ctypes.data) == RN_E_STATE
    assert s.deviceMemoryInfo()["context_bytes"] == m0                                      # none of the refused calls allocated anything
    assert both() == (0, 0) and ptr.value                                                   # straight after the reset of rn_create: y = 0
    assert lib.rn_buffer_size(s.h, capi.BUF_CERT_X) == s.nodes * s.nx and lib.rn_buffer_size(s.h, capi.BUF_CERT_U) == s.nodes * s.nu
    x = s.get(capi.BUF_CERT_X)
    assert lib.rn_set(s.h, capi.BUF_CERT_X, x.ctypes.data, x.size) == RN_E_ARG and "read-only" in lib.rn_last_error(s.h).decode()
    assert lib.rn_set_range(s.h, capi.BUF_CERT_U, 0, s.nu, x.ctypes.data) == RN_E_ARG
    s.setAlgorithm("namaAlgorithm", 5)
    assert both() == (RN_E_STATE,) * 2 and "FBE" in lib.rn_last_error(s.h).decode()         # their multiplier is another buffer
    s.setAlgorithm("proximalAlgorithm")
    assert both() == (0, 0)
    s.close()


def test_a_shard_without_a_communicator_and_a_failed_batch_are_refused():
    p, fc = problem("medium")
    s = capi.Solver(p["network"], p["tree"], p["config"], rank=0, nranks=2)
    s.initialiseSmpcController(*fc)
    out = np.zeros(capi.CERT_COLS)
    assert s.lib.rn_solve_certificate(s.h, out.ctypes.data) == RN_E_STATE and "communicator" in s.lib.rn_last_error(s.h).decode()
    s.debugSetAllreduce(lambda *a: 0)
    s.apgReset(); s.apgIterate(2)
    assert s.lib.rn_solve_certificate(s.h, out.ctypes.data) == 0
    s.debugSetAllreduce(lambda *a: 7)
    with pytest.raises(capi.RapidNetError):
        s.apgIterate(2)
    s.debugSetAllreduce(lambda *a: 0)
    assert s.lib.rn_solve_certificate(s.h, out.ctypes.data) == RN_E_STATE and "half-way" in s.lib.rn_last_error(s.h).decode()
    s.apgReset()
    assert s.lib.rn_solve_certificate(s.h, out.ctypes.data) == 0
    s.close()


# ---- 6. guard mode -----------------------------------------------------------------------------------------------------------------------------------
def test_under_the_buffer_guard(monkeypatch):
    """RAPIDNET_GUARD=1 (read when a context is created): every buffer between red zones and NaN until written.  A value read outside a buffer,
    or before anybody wrote it, would bring a NaN into the record (check_a asserts finiteness), a write outside a buffer changes a red zone."""
    monkeypatch.setenv("RAPIDNET_GUARD", "1")
    gc.collect()
    before = capi.guard_report()
    for name, mode, kind, gran in (("odd", "dense", "f64", "node"), ("ragged", "structured", "f32", "stage")):
        p, fc = problem(name)
        s = context(name, mode, kind, gran)
        walk("guard: %s %s %s" % (name, mode, kind), s, p, p["tree"], kind, counts=(0, 5))
        assert s.guardCheck() == 0
        s.close()
    after = capi.guard_report()
    assert after[0] - before[0] == 2 and after[1] == before[1]      # both contexts were checked once more when they went away: 0 bytes
