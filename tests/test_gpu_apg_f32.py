"""The fp32 instantiations of the APG kernels against the fp64 oracle, ONE ITERATION (or one 16-iteration batch) AT A TIME.

The suite holds the fp32 APG path to FP32_TOL = 2e-4 on a whole-buffer relmax after tens of iterations: a kernel that is wrong at the
1e-5 level in the rows of one stage passes (test_old_check_would_pass_a_subtly_wrong_stage shows it without a GPU).  Here an fp64
oracle (the DRIVER) runs the APG loop; after STATES iterations its xi, psi, updXi, updPsi are rounded to fp32 and written into
  (a) an fp32 capi.Solver            (the code under test),
  (b) a second fp64 oracle           (the REFERENCE) and
  (c) an fp32 oracle                 (the YARDSTICK),
each after apg_reset / apgReset (which zero the primal and dual iterates as well: at form A's first step Z_s is max |acc| / lambda, nothing
left over from an earlier run): theta = {1, 1}, the first lambda is 0 and w_0 = y+ on all three.  On the library's side the `set` of
XI / UPD_* clears acc_ready, so a batch re-derives w with k_extrapolate: that path is under test too.

The metric (stage_metric) is per stage.  With lambda = stepSize and, over the reference's rows of stage s,
    Z_s = max(max |primalXi|, max |primalPsi|, max |accXi| / lambda, max |accPsi| / lambda),
the error of a buffer in stage s is max |got - ref| over the stage's rows divided by
    Z_s            for primalXi, primalPsi, dualXi, dualPsi, resXi, resPsi,
    lambda Z_s     for xi, psi, accXi, accPsi, updXi, updPsi,
    max |ref|      of the stage for x, u, v,
and a buffer's error is its worst stage; a stage whose scale is exactly 0 in the reference must be 0 in `got`.  The two halves and the
three roles are sums of one another (z = primal + acc / lambda, res = primal - z, y+ = w + lambda res): a stage's OWN maximum of resXi
or xi is rounding noise wherever no bound is active, and the fp32 oracle alone would show errors of 1e0 ... 1e9 against it.

The bound is derived, not a number: for every compared buffer
    e_gpu = metric(gpu fp32, ref fp64),   e_cpu = metric(oracle fp32, ref fp64),   required: e_gpu <= 4 e_cpu + 32 * 2^-24.
Factor and floor are those of test_gpu_fbe_nama_f32.py: the factor covers another summation order of the same fp32 sums, the floor the
steps where the CPU happens to be exact.  The bound only says more than the suite does while 4 e_cpu + 32 * 2^-24 <= FP32_TOL / 4:
test_cap_holds_on_the_cpu_oracles checks that on every (problem, state, form) of the named and soft-penalty problems; for the trees
built from the device's CU count the same check runs before the GPU result is looked at.

Scalars: each of the two prox distances by the same rule, relative to the reference's value.  The primal-infeasibility history is NOT
compared across precisions (the reference reads the signed entry at the first index of max |.|, which may flip between two near-equal
entries): it is recomputed on the host from the context's own fp32 resXi / resPsi with the reference's rule
(oracle_primal_infeasibility) and must be EQUAL; where |.| ties exactly with different signs either candidate is accepted.

Forms, each from every state of STATES:
  A  the step entry points dualExtrapolationStep(0), solveStep, proximalFunG (+ proxDistances), computeFixedPointResidual, dualUpdate,
     updatePrimalInfeasibity: after each call the buffers that call may touch
  B  apgIterate(1): the exact batch path
  C  apgIterate(16): the optimistic path (RN_OPT_LOCAL_MIN); both oracles run apg_continue(16, [1, 1]); the batch must have been
     optimistic, and on the soft-penalty problems replayed exactly once

Shapes: the named problems tiny (n = 228), small (1330 = 2 mod 4), odd (891 = 3 mod 4), ragged, medium (three W tiles), barcelona31
(ny = 240), dense and structured, forms A, B, C; small with penalties 20 / 5 and medium with 2 / 1 (both thresholds at once); launch
shapes on medium, form B (unscaled_walk = 0 under form C as well); the fused walk + dual update on medium and barcelona31, and its
fall-back on small, form C; the split last round on two trees built from the
device's CU count, form B; shards of medium (2 ranks, cut 2) and ragged (3 ranks, cut 1), forms B and C.  The driver states and both
oracles' results are built once per problem and shared (barcelona31: 111 oracle iterations, some seconds of CPU, once).

When RAPIDNET_F32_ERRORS names a file, every (case, form, step, buffer) whose error is not zero on both sides is appended to it with both
errors (the worst state) and the share of the bound used: profiles/apg_f32_step_errors.txt is such a file.
"""
import os

import numpy as np
import pytest

from oracle.oracle import Oracle
from rapidnet_amd import capi, synth
from test_gpu_parity import FP32_TOL

gpu = pytest.mark.gpu

EPS32 = 2.0 ** -24
FACTOR, FLOOR = 4.0, 32 * EPS32
CAP = FP32_TOL / 4
STATES = (1, 5, 9)          # driver iterations whose state is used
BATCH = 16                  # RN_OPT_LOCAL_MIN (csrc/rapidnet_capi.hip): the shortest batch that runs optimistically on one GPU
PERTURB = 2e-5              # the sharpness self-test's stand-in for a kernel that is subtly wrong in the rows of one stage

PAIRS = [(capi.BUF_X, "x"), (capi.BUF_U, "u"), (capi.BUF_V, "v"), (capi.BUF_XI, "xi"), (capi.BUF_PSI, "psi"),
         (capi.BUF_ACC_XI, "accXi"), (capi.BUF_ACC_PSI, "accPsi"), (capi.BUF_UPD_XI, "updXi"), (capi.BUF_UPD_PSI, "updPsi"),
         (capi.BUF_PRIMAL_XI, "primalXi"), (capi.BUF_PRIMAL_PSI, "primalPsi"), (capi.BUF_DUAL_XI, "dualXi"),
         (capi.BUF_DUAL_PSI, "dualPsi"), (capi.BUF_RES_XI, "resXi"), (capi.BUF_RES_PSI, "resPsi")]
BID = {nm: bid for bid, nm in PAIRS}
ALL = tuple(nm for _, nm in PAIRS)
INJECT = ("xi", "psi", "updXi", "updPsi")
Z_FAMILY = ("primalXi", "primalPsi", "dualXi", "dualPsi", "resXi", "resPsi")
Y_FAMILY = ("xi", "psi", "accXi", "accPsi", "updXi", "updPsi")
Z_SOURCES = ("primalXi", "primalPsi", "accXi", "accPsi")
# form A: (step, the oracle's method, the library's method, the buffers the call may touch)
STEPS_A = (("extrapolate", "extrapolate", "dualExtrapolationStep", ("accXi", "accPsi", "xi", "psi")),
           ("solveStep", "solve_step", "solveStep", ("x", "u", "v", "primalXi", "primalPsi")),
           ("prox", "prox", "proximalFunG", ("dualXi", "dualPsi")),
           ("residual", "residual", "computeFixedPointResidual", ("resXi", "resPsi")),
           ("dualUpdate", "dual_update", "dualUpdate", ("updXi", "updPsi")))
FORMS = ("A", "B", "C")
NAMED = ["tiny", "small", "odd", "ragged", "medium", "barcelona31"]
SOFT = {"small": {"penalty_x": 20.0, "penalty_xs": 5.0}, "medium": {"penalty_x": 2.0, "penalty_xs": 1.0}}


def round32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def dims_of(o):
    d = {"x": o.nx, "u": o.nu, "v": o.nv}
    return lambda nm: d.get(nm, o.nu if nm.endswith("Psi") or nm == "psi" else 2 * o.nx)


# ---------------------------------------------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------------------------------------------
def stage_metric(got, ref, names, stages, lam, dim):
    """{name: (error of the buffer = its worst stage, that stage)} for `names`; `ref` holds the reference's primalXi, primalPsi, accXi,
    accPsi (Z_s comes from them) besides the compared buffers, `stages` the stage of every node, dim(name) a buffer's values per node.
    inf: `got` is not 0 in a stage whose scale is exactly 0 in the reference."""
    stages = np.asarray(stages, int)
    nodes, n = stages.size, int(stages.max()) + 1

    def stage_max(a, nm):
        a = np.asarray(a, float)
        assert a.size == nodes * dim(nm), (nm, a.size, nodes, dim(nm))
        assert np.isfinite(a).all(), nm
        m = np.zeros(n)
        np.maximum.at(m, stages, np.abs(a.reshape(nodes, dim(nm))).max(axis=1))
        return m

    Z = np.maximum(np.maximum(stage_max(ref["primalXi"], "primalXi"), stage_max(ref["primalPsi"], "primalPsi")),
                   np.maximum(stage_max(ref["accXi"], "accXi"), stage_max(ref["accPsi"], "accPsi")) / lam)
    out = {}
    for nm in names:
        r = np.asarray(ref[nm], float)
        scale = Z if nm in Z_FAMILY else lam * Z if nm in Y_FAMILY else stage_max(r, nm)
        err = stage_max(np.asarray(got[nm], float) - r, nm)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
        out[nm] = (float(e.max()), int(e.argmax()))
    return out


def scalar_error(g, r):
    """the metric's rule for one number: relative to the reference's value; a reference of exactly 0 must be 0"""
    assert np.isfinite(g) and np.isfinite(r)
    return abs(g - r) / abs(r) if r != 0 else (0.0 if g == 0 else float("inf"))


def relmax(a, b):
    """the suite's whole-buffer measure (test_gpu_parity.relmax)"""
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def infeasibility_candidates(res_xi, res_psi):
    """oracle_primal_infeasibility on the given residuals: the signed entry at the first index of max |.| of each half, the larger of the
    two; where |.| ties exactly with different signs both entries are candidates.  Returns the set of acceptable values."""
    def cands(r):
        r = np.asarray(r, float)
        a = np.abs(r)
        return set(r[a == a.max()].tolist())
    return {a if a > b else b for a in cands(res_xi) for b in cands(res_psi)}


# ---------------------------------------------------------------------------------------------------------------
# the driver, the reference and the yardstick: once per problem
# ---------------------------------------------------------------------------------------------------------------
class Snap:
    """what the reference holds after one call of form A or one batch of form B / C, and the yardstick's errors against it"""

    def __init__(self, step, names, ref, e_cpu, dist, e_dist):
        self.step, self.names, self.ref, self.e_cpu, self.dist, self.e_dist = step, names, ref, e_cpu, dist, e_dist


def oracle_form(o, form, dists=None):
    """runs one form on an oracle that holds an injected state; yields (step, compared buffers, prox distances or None) after every call.
    dists: a list that receives the distances of every iteration of a batch, which is then run one iteration at a time (theta travels through
    apg_continue unchanged, so that is the batch bit for bit: test_a_batch_run_one_iteration_at_a_time_is_the_batch); otherwise the batch
    is one apg_continue(n, [1, 1])"""
    if form == "A":
        for step, fn, _, names in STEPS_A:
            getattr(o, fn)(*((0.0,) if step == "extrapolate" else ()))
            yield step, names, (o.dist() if step == "prox" else None)
    else:
        n, th = (1 if form == "B" else BATCH), [1.0, 1.0]
        if dists is None:
            o.apg_continue(n, th)
        else:
            for _ in range(n):
                th = o.apg_continue(1, th)
                dists.append(o.dist())
        yield "batch", ALL, o.dist()


def inject_oracle(o, st):
    o.apg_reset()
    for nm in INJECT:
        o.set(nm, st[nm])


class Case:
    """one problem: the driver's rounded states after STATES iterations and, for every (state, form), the reference's buffers and the
    yardstick's errors -- computed once and left unchanged"""

    def __init__(self, tag, p, fc, alias=True, states=STATES):
        self.tag, self.p, self.fc, self.states_used = tag, p, fc, tuple(states)
        self.lam = float(p["config"]["stepSize"][0])
        self.thr = (p["config"]["penaltyStateX"][0] / self.lam, p["config"]["penaltySafetyX"][0] / self.lam)
        self.stages = np.asarray(p["tree"]["stages"], int)[: int(p["tree"]["nodes"][0])]
        self.ref = Oracle(p["network"], p["tree"], p["config"], alias_operators=alias)
        self.cpu = Oracle(p["network"], p["tree"], p["config"], precision="f32", alias_operators=alias)
        self.ref.initialise(*fc); self.cpu.initialise(*fc)
        self.dim = dims_of(self.ref)
        # the driver: the reference oracle itself, before its first injection
        self.states, th = {}, [1.0, 1.0]
        self.ref.apg_reset()
        for it in range(1, max(states) + 1):
            th = self.ref.apg_continue(1, th)
            if it in states:
                self.states[it] = {nm: round32(self.ref.get(nm)) for nm in INJECT}
        self.snaps, self.tripped = {}, {}
        for it, st in self.states.items():
            dists = []
            for form, snaps in self.run_oracles(st, dists=dists).items():
                self.snaps[(it, form)] = snaps
            # in how many of form C's iterations the reference's distances exceed a threshold (the optimistic batch is then replayed)
            self.tripped[it] = sum(int(dx > self.thr[0] or ds > self.thr[1]) for dx, ds in dists)

    def metric(self, got, ref, names):
        return stage_metric(got, ref, names, self.stages, self.lam, self.dim)

    def run_oracles(self, st, st_cpu=None, forms=FORMS, dists=None):
        """{form: [Snap, ...]} of the state `st` on the reference and of `st_cpu` (default: the same) on the yardstick; dists receives the
        reference's distances of every iteration of form C"""
        out = {}
        for form in forms:
            inject_oracle(self.ref, st); inject_oracle(self.cpu, st if st_cpu is None else st_cpu)
            snaps = []
            for (step, names, dist), (_, _, cdist) in zip(oracle_form(self.ref, form, dists if form == "C" else None), oracle_form(self.cpu, form)):
                keep = tuple(dict.fromkeys(names + Z_SOURCES))
                ref = {nm: self.ref.get(nm) for nm in keep}
                for a in ref.values():
                    a.setflags(write=False)
                e_cpu = self.metric({nm: self.cpu.get(nm) for nm in names}, ref, names)
                e_dist = None if dist is None else tuple(scalar_error(c, r) for c, r in zip(cdist, dist))
                snaps.append(Snap(step, names, ref, e_cpu, dist, e_dist))
            out[form] = snaps
        return out

    def cap_violations(self):
        """every (state, form, step, buffer) whose bound 4 e_cpu + floor exceeds FP32_TOL / 4"""
        bad = []
        for (it, form), snaps in self.snaps.items():
            for sn in snaps:
                for nm in sn.names:
                    if not FACTOR * sn.e_cpu[nm][0] + FLOOR <= CAP:
                        bad.append((self.tag, it, form, sn.step, nm, sn.e_cpu[nm]))
                for k, e in enumerate(sn.e_dist or ()):
                    if not FACTOR * e + FLOOR <= CAP:
                        bad.append((self.tag, it, form, sn.step, "dist%d" % k, e))
        return bad


_CASES = {}


def named_case(name, soft=False):
    key = (name, soft)
    if key not in _CASES:
        p = synth.make_problem(name, **(SOFT[name] if soft else {}))
        _CASES[key] = Case(name + (" soft" if soft else ""), p, synth.forecast_at(p["forecast"], 0))
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------
# the bound and the table of errors
# ---------------------------------------------------------------------------------------------------------------
class Ledger:
    """both errors of every compared (form, step, buffer) of one case -- the state that uses most of the bound -- and the violations"""

    def __init__(self, case):
        self.case, self.rows, self.bad = case, {}, []

    def add(self, form, step, it, k, e_gpu, e_cpu, where=""):
        bound = FACTOR * e_cpu + FLOOR
        share = e_gpu / bound
        old = self.rows.get((form, step, k))
        if old is None or share > old[3]:
            self.rows[(form, step, k)] = (e_gpu, e_cpu, it, share)
        if not e_gpu <= bound:
            self.bad.append("form %s %s state %d %s%s: e_gpu %.3e > 4 * e_cpu (%.3e) + %.3e" % (form, step, it, k, where, e_gpu, e_cpu, FLOOR))

    def compare(self, case, form, it, snap, got, dist=None):
        e_gpu = case.metric(got, snap.ref, snap.names)
        for nm in snap.names:
            self.add(form, snap.step, it, nm, e_gpu[nm][0], snap.e_cpu[nm][0], " (stage %d; the fp32 oracle's worst: stage %d)" % (e_gpu[nm][1], snap.e_cpu[nm][1]))
        if snap.dist is not None:
            assert dist is not None
            for k, (g, r, ec) in enumerate(zip(dist, snap.dist, snap.e_dist)):
                self.add(form, snap.step, it, "dist%d" % k, scalar_error(g, r), ec, " (%r, reference %r)" % (g, r))

    def worst(self):
        return max([r[3] for r in self.rows.values()] or [0.0])

    def finish(self):
        path = os.environ.get("RAPIDNET_F32_ERRORS")
        if path:
            with open(path, "a") as f:
                for (form, step, k), (e_gpu, e_cpu, it, share) in sorted(self.rows.items()):
                    if e_gpu or e_cpu:
                        f.write("apg %-44s %-14s %-12s it %d  e_gpu %.3e  e_cpu %.3e  of the bound %.3f\n" % (self.case, "%s %s" % (form, step), k, it, e_gpu, e_cpu, share))
        assert not self.bad, "%s: %s" % (self.case, "; ".join(self.bad))


# ---------------------------------------------------------------------------------------------------------------
# the code under test
# ---------------------------------------------------------------------------------------------------------------
def check_infeasibility(value, res_xi, res_psi, what):
    want = infeasibility_candidates(res_xi, res_psi)
    assert value in want, "%s: primal infeasibility %r, recomputed from the context's own residuals %s" % (what, value, sorted(want))


def solver_form(s, st, form, soft=False, what=""):
    """one form on an fp32 context of the library from the state `st`; yields (step, {buffer: values}, prox distances or None) in
    oracle_form's order.  Asserts the batch's path from counters() and the primal infeasibility against the context's own residuals."""
    s.apgReset()
    for nm in INJECT:
        s.set(BID[nm], st[nm])
    if form == "A":
        for step, _, fn, names in STEPS_A:
            getattr(s, fn)(*((0.0,) if step == "extrapolate" else ()))
            yield step, {nm: s.get(BID[nm]) for nm in names}, (s.proxDistances() if step == "prox" else None)
        check_infeasibility(s.updatePrimalInfeasibity(), s.get(capi.BUF_RES_XI), s.get(capi.BUF_RES_PSI), what + " form A")
        return
    s.setExchangeMode(True)            # (clears the hold a replayed batch leaves: every batch of form C is offered the optimistic path)
    before = s.counters()
    hist = s.apgIterate(1 if form == "B" else BATCH)
    c = s.counters()
    delta = {k: c[k] - before[k] for k in ("optimistic", "exact", "replayed")}
    if form == "B":
        assert delta == {"optimistic": 0, "exact": 1, "replayed": 0}, (what, delta)
    else:
        assert delta["optimistic"] == 1 and delta["exact"] == 0 and delta["replayed"] == (1 if soft else 0), (what, delta, soft)
    got = {nm: s.get(BID[nm]) for nm in ALL}
    check_infeasibility(hist[-1], got["resXi"], got["resPsi"], what + " form " + form)
    yield "batch", got, s.proxDistances()


def run_case(case, s, led, forms=FORMS, states=None, soft=False):
    """every form from every state on the context `s`, into the ledger"""
    for it in states or case.states_used:
        for form in forms:
            snaps = case.snaps[(it, form)]
            if soft and form == "C":
                assert case.tripped[it] >= 1, "%s state %d: the reference never exceeds a soft-constraint threshold in the batch" % (case.tag, it)
            k = 0
            for step, got, dist in solver_form(s, case.states[it], form, soft, "%s state %d" % (led.case, it)):
                assert snaps[k].step == step
                led.compare(case, form, it, snaps[k], got, dist)
                k += 1
            assert k == len(snaps)


def make_solver(case, **kw):
    s = capi.Solver(case.p["network"], case.p["tree"], case.p["config"], precision="f32", **kw)
    s.initialiseSmpcController(*case.fc)
    return s


def run_named(name, soft=False, forms=FORMS, states=None, label="", record=True, **kw):
    case = named_case(name, soft)
    s = make_solver(case, **kw)
    led = Ledger("%s%s" % (case.tag, label))
    try:
        run_case(case, s, led, forms, states, soft)
    finally:
        s.close()
    compared = len(led.rows)
    if not record:
        led.rows.clear()
    led.finish()
    return compared


# ---------------------------------------------------------------------------------------------------------------
# CPU tests: the metric, the cap, the sharpness of the bound
# ---------------------------------------------------------------------------------------------------------------
def _toy_buffers(rng, nodes, nx, nu, nv):
    d = {"x": nx, "u": nu, "v": nv}
    dim = lambda nm: d.get(nm, nu if nm.endswith("Psi") or nm == "psi" else 2 * nx)
    return {nm: rng.standard_normal(nodes * dim(nm)) for nm in ALL}, dim


def test_metric_zero_scale_stage():
    """a stage whose scale is exactly 0 in the reference: 0 in `got` is no error, anything else is inf -- for the three kinds of scale"""
    rng = np.random.default_rng(1)
    stages, lam = np.array([0, 1, 1, 2, 2]), 0.25
    ref, dim = _toy_buffers(rng, 5, 2, 3, 2)
    for nm in ALL:
        ref[nm].reshape(5, -1)[1:3] = 0.0                       # stage 1: every buffer, hence every scale, exactly 0
    got = {nm: v.copy() for nm, v in ref.items()}
    e = stage_metric(got, ref, ALL, stages, lam, dim)
    assert all(v[0] == 0.0 for v in e.values()), e
    for nm in ("resXi", "updPsi", "u"):
        g = dict(got)
        g[nm] = got[nm].copy()
        g[nm].reshape(5, -1)[2, 0] = 1e-30
        e = stage_metric(g, ref, ALL, stages, lam, dim)
        assert e[nm] == (float("inf"), 1) and all(v[0] == 0.0 for k, v in e.items() if k != nm), (nm, e)
    with pytest.raises(AssertionError):
        g = dict(got)
        g["x"] = got["x"].copy()
        g["x"][0] = np.nan
        stage_metric(g, ref, ALL, stages, lam, dim)


def test_metric_error_in_one_stage_only():
    """an error in the rows of one stage is divided by THAT stage's scale, however large the other stages are, and is reported there"""
    rng = np.random.default_rng(2)
    stages, lam = np.array([0, 1, 1, 2, 2, 2]), 0.5
    ref, dim = _toy_buffers(rng, 6, 2, 3, 2)
    for nm in ALL:
        ref[nm].reshape(6, -1)[0] *= 1e6                        # the root dwarfs everything: a whole-buffer maximum sees only it
    got = {nm: v.copy() for nm, v in ref.items()}
    got["updXi"].reshape(6, -1)[3:] *= 1 + 1e-5                 # stage 2 of updXi
    got["v"].reshape(6, -1)[1:3] *= 1 + 1e-5                    # stage 1 of v
    e = stage_metric(got, ref, ALL, stages, lam, dim)
    rows = lambda nm, a, b: np.abs(ref[nm].reshape(6, -1)[a:b]).max()
    Z2 = max(rows("primalXi", 3, 6), rows("primalPsi", 3, 6), rows("accXi", 3, 6) / lam, rows("accPsi", 3, 6) / lam)
    assert e["updXi"][1] == 2 and e["updXi"][0] == pytest.approx(1e-5 * rows("updXi", 3, 6) / (lam * Z2), rel=1e-6)
    assert e["v"][1] == 1 and e["v"][0] == pytest.approx(1e-5, rel=1e-6)
    assert all(v[0] == 0.0 for k, v in e.items() if k not in ("updXi", "v"))
    assert relmax(got["updXi"], ref["updXi"]) < 1e-9           # ... which the whole-buffer measure does not see at all


def test_metric_xi_and_psi_share_the_stage_scale():
    """psi at rounding noise beside a large xi (no input bound active): the shared Z_s measures psi's error on the dual vector's scale, not
    on its own; Z_s is the largest of the four sources, and the y family carries the factor lambda"""
    stages, lam = np.array([0, 1, 1]), 0.125
    rng = np.random.default_rng(3)
    ref, dim = _toy_buffers(rng, 3, 2, 3, 2)
    for nm in ("psi", "accPsi", "updPsi", "resPsi"):
        ref[nm] *= 1e-21
    ref["primalXi"].reshape(3, -1)[1:] = [[3.0, -1.0, 0.5, 2.0], [1.0, 1.0, -2.5, 0.0]]
    ref["primalPsi"].reshape(3, -1)[1:] *= 0.1
    ref["accXi"].reshape(3, -1)[1:] = [[0.5, -0.25, 0.1, 0.2], [0.1, 0.1, -0.3, 0.0]]          # / lambda: up to 4 -> Z_1 = 4
    got = {nm: v.copy() for nm, v in ref.items()}
    got["resPsi"].reshape(3, -1)[1, 0] += 4e-6
    got["updPsi"].reshape(3, -1)[2, 1] += 4e-6
    got["xi"].reshape(3, -1)[1, 2] += 4e-6
    e = stage_metric(got, ref, ALL, stages, lam, dim)
    assert e["resPsi"] == (pytest.approx(1e-6), 1)
    assert e["updPsi"] == (pytest.approx(1e-6 / lam), 1) and e["xi"] == (pytest.approx(1e-6 / lam), 1)
    assert scalar_error(1.0 + 1e-6, 1.0) == pytest.approx(1e-6) and scalar_error(0.0, 0.0) == 0.0 and scalar_error(1e-30, 0.0) == float("inf")
    assert infeasibility_candidates([1.0, -3.0, 3.0], [0.5, -0.25]) == {3.0, 0.5}            # a tie of different signs: either candidate of xi
    assert infeasibility_candidates([1.0, -3.0, 2.0], [0.5, -0.25]) == {0.5}                # the reference's quirk: the signed entry


@pytest.mark.parametrize("name,soft", [(n, False) for n in NAMED] + [(n, True) for n in SOFT])
def test_cap_holds_on_the_cpu_oracles(name, soft):
    """4 e_cpu + 32 * 2^-24 <= FP32_TOL / 4 for every buffer and distance of every (state, form): above that the bound would say little
    more than the suite's FP32_TOL.  On the soft-penalty problems the states must reach what they are there for: form C's batch exceeds a
    threshold (the optimistic batch is replayed) from every state, and form B's single iteration takes the soft branch."""
    case = named_case(name, soft)
    assert sorted(case.snaps) == sorted((it, f) for it in STATES for f in FORMS)
    assert [sn.step for sn in case.snaps[(STATES[0], "A")]] == [s[0] for s in STEPS_A]
    bad = case.cap_violations()
    assert not bad, bad
    if soft:
        assert all(case.tripped[it] >= 1 for it in STATES), case.tripped
        hit = [it for it in STATES if any(d > t for d, t in zip(case.snaps[(it, "B")][0].dist, case.thr))]
        assert hit, "no state of %s takes the soft branch in form B" % case.tag
        if name == "medium":      # both thresholds at once, as in test_both_soft_constraint_thresholds_trip_at_once
            assert any(all(d > t for d, t in zip(case.snaps[(it, "B")][0].dist, case.thr)) for it in STATES)
    else:
        assert not any(case.tripped.values()), case.tripped


@pytest.mark.parametrize("name", NAMED)
def test_old_check_would_pass_a_subtly_wrong_stage(name):
    """The sharpness self-test, no GPU: the fp32 oracle stands in for a kernel that is wrong in a few rows -- the rows of the second-to-last
    stage of updXi are multiplied by 1 + 2e-5 before injection.  In form B, from every state, the per-stage bound refuses it, while the
    whole-buffer relmax of the same run stays below FP32_TOL on every buffer: the suite's check would have passed.  With lambda_0 = 0 the
    iteration's accXi IS the injected updXi, so the metric must report exactly the perturbed stage there."""
    case = named_case(name)
    stage = int(case.stages.max()) - 1
    rows = np.flatnonzero(case.stages == stage)
    for it in STATES:
        st = case.states[it]
        bent = dict(st, updXi=st["updXi"].copy())
        bent["updXi"].reshape(case.stages.size, -1)[rows] *= 1 + PERTURB
        bent["updXi"] = round32(bent["updXi"])
        clean = case.snaps[(it, "B")][0]
        snap = case.run_oracles(st, bent, forms=("B",))["B"][0]          # e_cpu of this snap: the perturbed fp32 run against the reference
        over = {nm: snap.e_cpu[nm][0] / (FACTOR * clean.e_cpu[nm][0] + FLOOR) for nm in ALL}
        assert max(over.values()) > 1.0, (name, it, over)
        assert snap.e_cpu["accXi"][1] == stage and over["accXi"] > 1.0, (name, it, snap.e_cpu["accXi"], over["accXi"])
        inject_oracle(case.cpu, bent)
        case.cpu.apg_continue(1, [1.0, 1.0])
        old = {nm: relmax(case.cpu.get(nm), clean.ref[nm]) for nm in ALL}
        assert max(old.values()) < FP32_TOL, (name, it, old)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_batch_run_one_iteration_at_a_time_is_the_batch(precision):
    """the reference's form C is run one iteration at a time to count the iterations that exceed a threshold: bit for bit apg_continue(16, [1, 1])"""
    case = named_case("small", soft=True)
    o = case.ref if precision == "f64" else case.cpu
    out = []
    for dists in (None, []):
        inject_oracle(o, case.states[5])
        list(oracle_form(o, "C", dists))
        out.append({nm: o.get(nm) for nm in ALL})
        assert dists is None or len(dists) == BATCH
    for nm in ALL:
        assert np.array_equal(out[0][nm], out[1][nm]), nm


def test_ledger_refuses_a_violated_bound(monkeypatch):
    monkeypatch.delenv("RAPIDNET_F32_ERRORS", raising=False)        # (finish() would append its rows to a table being recorded)
    led = Ledger("self-test")
    led.add("B", "batch", 1, "xi", 3e-7, 1e-7)
    led.add("B", "batch", 5, "xi", 1.5e-6, 1e-8)
    led.finish()
    assert led.rows[("B", "batch", "xi")][2] == 5 and led.worst() == pytest.approx(1.5e-6 / (4e-8 + FLOOR))
    led.add("B", "batch", 9, "xi", 1e-5, 1e-7)
    led.add("B", "batch", 9, "dist0", float("inf"), 0.0)
    assert len(led.bad) == 2
    with pytest.raises(AssertionError):
        led.finish()


# ---------------------------------------------------------------------------------------------------------------
# 1 + 2: the named and the soft-penalty problems, dense and structured
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name", NAMED)
def test_f32_apg_matches_the_f64_reference(name, mode):
    """forms A, B, C from every state.  tiny n = 228; small 1330 = 2 mod 4; odd 891 = 3 mod 4; ragged: non-uniform branching; medium:
    three W tiles; barcelona31: ny = 240, the headline network's kernels"""
    run_named(name, label=" " + mode, operator_mode=mode)


@gpu
@pytest.mark.parametrize("mode", ["dense", "structured"])
@pytest.mark.parametrize("name", list(SOFT))
def test_f32_apg_soft_branch_matches_the_f64_reference(name, mode):
    """penalties small enough that the soft-constraint branch trips: k_prox_soft behind proximalFunG, the exact batch's fix-up, and an
    optimistic batch that is replayed exactly once.  medium with penalties 2 / 1: both thresholds at once"""
    run_named(name, soft=True, label=" " + mode, operator_mode=mode)


# ---------------------------------------------------------------------------------------------------------------
# 3: launch shapes on medium, form B
# ---------------------------------------------------------------------------------------------------------------
# vlv_wide is read where the v / Lv products are two (launch_v_lv behind the composite operator's branch): dense, and structured with the
# linear form off -- under the structured default (k_gemm_comp) the knob would change nothing
DENSE_KNOBS = [{"dual_trips": 1, "dual_pipe": 1}, {"dual_trips": 3, "dual_pipe": 2}, {"dual_trips": 8, "dual_pipe": 1}, {"unscaled_walk": 0},
               {"stream_two_per_cu": 0}, {"stream_two_per_cu": 1}, {"vlv_wide": 2}, {"vlv_wide": 3}]
STRUCT_KNOBS = [{"struct_linear": 0}, {}, {"struct_linear": 0, "vlv_wide": 2}, {"struct_linear": 0, "vlv_wide": 3}, {"slab_pipe": 0}, {"slab_frag": 0}]


def knob_label(knobs):
    return " ".join("%s=%d" % kv for kv in sorted(knobs.items())) or "default"


@gpu
@pytest.mark.parametrize("mode,knobs", [("dense", k) for k in DENSE_KNOBS] + [("structured", k) for k in STRUCT_KNOBS], ids=lambda v: v if isinstance(v, str) else knob_label(v))
def test_f32_launch_shapes_on_medium(monkeypatch, mode, knobs):
    """k_dual_stage's tile / pipelining shapes, both instantiations of k_stream_gemv, k_gemm_vlv_wide with 2 and 3 slabs per workgroup
    (kernelInfo reports the choice once a sweep has made it); structured: the linear form off / by default, the lean MFMA loop, A operands
    from the column-major operators -- one exact iteration from every state.
    unscaled_walk = 0: form B as the issue of this test asked for, where the knob changes nothing -- an exact batch's walk applies the
    preconditioner itself whatever the knob says -- and form C with the fused walk + dual update off, where it does: the inner iterations
    of an optimistic batch then run k_down_chain<T, false> + k_dual_stage instead of the unscaled pair, which
    test_f32_fused_walk_and_dual_update[medium-0-None] runs."""
    case = named_case("medium")
    forms = ("B",)
    if "unscaled_walk" in knobs:
        monkeypatch.setenv("RAPIDNET_FUSE_DOWN_DUAL", "0")
        forms = ("B", "C")
    s = make_solver(case, operator_mode=mode, knobs=knobs)
    try:
        k = s.kernelInfo()
        if "dual_trips" in knobs:
            assert k["dual_stage"] == 1 and k["dual_trips"] == knobs["dual_trips"] and k["dual_pipe"] == knobs["dual_pipe"], k
        if "unscaled_walk" in knobs:
            assert k["dual_stage"] == 1 and 1 <= k["chain_stage"] <= 8, k       # what the unscaled pair needs besides an optimistic batch
        if "stream_two_per_cu" in knobs:
            assert s.streamInfo()["twoPerCU"] == knobs["stream_two_per_cu"]
        assert s.operatorMode()[1] == mode and k["vlv_slab"] == 1, k
        led = Ledger("medium %s %s" % (mode, knob_label(knobs)))
        run_case(case, s, led, forms=forms)
        assert s.kernelInfo()["vlv_slab"] == knobs.get("vlv_wide", 1), (s.kernelInfo(), knobs)
    finally:
        s.close()
    led.finish()


# ---------------------------------------------------------------------------------------------------------------
# 4: the fused walk + dual update, form C
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fused,split", [("0", None), ("1", 1), ("1", 2), ("1", 1000)])
@pytest.mark.parametrize("name", ["medium", "small", "barcelona31"])
def test_f32_fused_walk_and_dual_update(monkeypatch, name, fused, split):
    """k_down_chain_dual<float> with 1, 2 and chain-length workgroups per chain, and the two launches it replaces (k_down_chain's unscaled
    form + k_dual_stage): one optimistic batch from every state, on medium (ny = 80, 20 chains) and barcelona31 (ny = 240, 31 chains).
    Whether the one launch happened is the sweep's answer to the batch and is not reported; asserted is what it depends on besides the
    optimistic batch (run_case): forced on, the stage-tiled dual update, a crown the chain workgroups fold.
    small (ny = 19, no multiple of the four values of an fp32 vector) CANNOT fuse: its dual update is the flat k_dual_fused, asserted
    below, and the request falls back to the two launches -- the four cases pin that fall-back to the same iterates."""
    monkeypatch.setenv("RAPIDNET_FUSE_DOWN_DUAL", fused)
    case = named_case(name)
    s = make_solver(case, knobs=None if split is None else {"fuse_split": split})
    try:
        k = s.kernelInfo()
        if name == "small":
            assert k["dual_stage"] == 0 and s.ny % 4 != 0, k
        else:
            assert k["dual_stage"] == 1 and k["dual_pipe"] != 0 and 1 <= k["chain_stage"] <= 8 and s.ny % 4 == 0, k
        led = Ledger("%s fuse=%s split=%s" % (name, fused, split))
        run_case(case, s, led, forms=("C",))
    finally:
        s.close()
    led.finish()


# ---------------------------------------------------------------------------------------------------------------
# 5: k_stream_gemv<float>'s split last round, form B
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("net,pos", [("b240", "three"), ("b236", "last")])
def test_f32_split_last_round(net, pos):
    """fp32 dense contexts on trees built from the device's CU count (test_gpu_stream_split.problem): the split is asserted from
    streamInfo() before anything is compared, the stage of every node is the built tree's, and the cap is checked on the two oracles
    before the GPU result is looked at"""
    import test_gpu_stream_split as spl

    p, fc = spl.problem(net, pos)
    key = ("split", net, pos)
    if key not in _CASES:
        _CASES[key] = Case("split %s %s" % (net, pos), p, fc, alias=spl.aliasing(p))
    case = _CASES[key]
    assert case.stages.size == int(p["tree"]["nodes"][0]) == spl.num_cus() + spl.position(pos, spl.num_cus())[0]
    bad = case.cap_violations()
    assert not bad, bad
    s = make_solver(case, operator_mode="dense")
    try:
        spl.expect_split(s, spl.position(pos, spl.num_cus())[0], case.tag + " f32")
        led = Ledger(case.tag)
        run_case(case, s, led, forms=("B",))
    finally:
        s.close()
    led.finish()


# ---------------------------------------------------------------------------------------------------------------
# 6: shards in one process, forms B and C
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,world,cut", [("medium", 2, 2), ("ragged", 3, 1)])
def test_f32_sharded_batches(name, world, cut):
    """rank-local fp32 contexts joined to an in-process group: the state goes into every shard through its global node ids, every batch is
    optimistic (one collective per iteration, the closing all-reduce, the vote), the results are gathered before the metric is applied;
    the distances and the history are tree-global on every rank"""
    from test_gpu_sharded_batched import Ranks

    case = named_case(name)
    rk = Ranks(case.p, world, cut, precision="f32")
    led = Ledger("%s %d ranks cut %d" % (name, world, cut))
    try:
        rk.run(lambda s: s.initialiseSmpcController(*case.fc))
        for it in STATES:
            st = case.states[it]
            for form in ("B", "C"):
                def batch(s):
                    ids = np.asarray(s.global_nodes)
                    s.apgReset()
                    for nm in INJECT:
                        s.set(BID[nm], st[nm].reshape(rk.nodes, -1)[ids].ravel())
                    before = s.counters()
                    hist = s.apgIterate(1 if form == "B" else BATCH)
                    c = s.counters()
                    return {k: c[k] - before[k] for k in ("optimistic", "exact", "replayed")}, hist, s.proxDistances()

                res = rk.run(batch)
                got = {nm: rk.gathered(BID[nm], case.dim(nm)) for nm in ALL}
                snap = case.snaps[(it, form)][0]
                for r, (delta, hist, dist) in enumerate(res):
                    assert delta == {"optimistic": 1, "exact": 0, "replayed": 0}, (r, delta)
                    check_infeasibility(hist[-1], got["resXi"], got["resPsi"], "%s rank %d state %d form %s" % (led.case, r, it, form))
                    assert np.array_equal(hist, res[0][1]) and dist == res[0][2], (r, dist, res[0][2])
                led.compare(case, form, it, snap, got, res[0][2])
    finally:
        rk.close()
    led.finish()


# ---------------------------------------------------------------------------------------------------------------
# guard mode's body (tests/test_gpu_guard.py)
# ---------------------------------------------------------------------------------------------------------------
def guard_body():
    """forms B and C on `small` (n = 1330 = 2 mod 4), dense and structured; returns the number of contexts"""
    for mode in ("dense", "structured"):
        # (the table of errors lists these batches already: test_f32_apg_matches_the_f64_reference)
        assert run_named("small", forms=("B", "C"), label=" guard " + mode, record=False, operator_mode=mode) == 2 * (len(ALL) + 2)
    return 2
