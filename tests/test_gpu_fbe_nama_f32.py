"""The fp32 instantiations of the global-FBE / NAMA kernels against the fp64 oracle, ONE STEP AT A TIME.

Whole fp32 loops cannot be compared with the oracle: the line search and the L-BFGS skip rule branch on computed values, so after a
few iterations an fp32 run legitimately takes other branches than an fp64 run.  Single steps can.  An fp64 oracle (the DRIVER) runs
the loop; before a step under test its whole state -- every buffer of FBE_PAIRS, the current / previous Yvec, every column of
matS / matY, rho, (col, mem, H) -- is rounded to fp32 and written into
  (a) an fp32 capi.Solver            (the code under test),
  (b) a second fp64 oracle           (the REFERENCE) and
  (c) an fp32 oracle                 (the YARDSTICK);
the three run the one step from identical inputs and every buffer the step may touch is compared.

The bound is derived, not a number: with relmax = max |a - ref| / max |ref|,
    e_gpu = relmax(gpu fp32, ref fp64),   e_cpu = relmax(oracle fp32, ref fp64),   required: e_gpu <= 4 e_cpu + 32 * 2^-24.
The fp32 oracle rounds every operation and every sum in fp32; the HIP path rounds the same operations in fp32 and sums in fp64: an
error of the same kind, no larger in expectation.  The factor 4 covers the different summation order of the sweeps; the floor the steps
where the CPU happens to be exact (copies, a clamp that binds): an output of an element kernel is a handful of fp32 roundings of
operands on the buffer's scale.  The floor is a hundred times tighter than the suite's FP32_TOL = 2e-4.

Tested driver iterations (0-based, m = 3, so the column index has wrapped and columns c >= 1 with c n mod 4 != 0 are live): ITERS.
The fp32 context is not reset between them: its logical L-BFGS columns start at c n values and are exchanged with the 16-byte aligned
scratch pair as pairs are stored, so aligned and misaligned columns are both walked.

Shapes (n = nodes (2 nx + nu) values per column; the element kernels' vector holds four fp32 values):
  tiny   n = 19 * 12 = 228 = 0 mod 4      small  n = 70 * 19 = 1330 = 2 mod 4      odd  n = 33 * 27 = 891 = 3 mod 4
  _f32_n1 (nx 4, nu 9, 33 nodes)  n = 33 * 17 = 561 = 1 mod 4
  medium nu = 38 (three W tiles)           barcelona31 nu = 114 (eight tiles, W in registers)
  _f32_nu150 nu = 150: k_value_mfma's slab_mfma fallback (128 < nu <= 192)         tall nu = 300: the vector-ALU value kernels by default

When RAPIDNET_F32_ERRORS names a file, every (config, algorithm, step, buffer) whose error is not zero on both sides is appended to it
with both errors (the worst iteration), followed by the shares of skipped states: profiles/fbe_f32_step_errors.txt is such a file.
"""
import os
import threading

import numpy as np
import pytest

from oracle.oracle import Oracle
from rapidnet_amd import capi, partition, synth
from test_gpu_fbe_nama import ALGS, FBE_PAIRS, REL_TOL, compare_fbe, cur_names, relmax

gpu = pytest.mark.gpu

EPS32 = 2.0 ** -24
FACTOR, FLOOR = 4.0, 32 * EPS32
M = 3                       # L-BFGS buffer size of every step test
ITERS = (5, 6, 7, 8)        # driver iterations whose steps are tested: the first one has m + 2 finished iterations behind it
SKIP_MARGIN = 1e-3          # skip rule / slope: distance of the decision quantity from its threshold, relative to the sum it comes from
LS_MARGIN = 100.0           # a line-search state counts when its value margin exceeds this many fp32 value errors
YVEC = (capi.BUF_LBFGS_CUR_YVEC_XI, capi.BUF_LBFGS_CUR_YVEC_PSI, capi.BUF_LBFGS_PREV_YVEC_XI, capi.BUF_LBFGS_PREV_YVEC_PSI)
LOCAL = {"_f32_n1": (31, 4, 9, 5, 3, 7, [2, 3]), "_f32_nu150": (32, 8, 150, 40, 10, 4, [2])}
FBE = "globalFbeAlgorithm"


def round32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def make_problem(name, **kw):
    """a named config of synth, or one of LOCAL registered for the duration of the call"""
    if name not in LOCAL:
        return synth.make_problem(name, **kw)
    synth.CONFIGS[name] = LOCAL[name]
    try:
        return synth.make_problem(name, **kw)
    finally:
        del synth.CONFIGS[name]


# ---------------------------------------------------------------------------------------------------------------
# state capture and injection
# ---------------------------------------------------------------------------------------------------------------
def capture(o, alg):
    """the driver's full quasi-Newton state, rounded to fp32"""
    st = {nm: round32(o.get(nm)) for _, nm in FBE_PAIRS}
    for nm in cur_names(alg) + ("matS", "matY", "rho"):
        st[nm] = round32(o.get(nm))
    col, mem, H = o.lbfgs_state()
    st["lbfgs"] = (col, mem, float(np.float32(H)))
    return st


class OracleUnit:
    """one of the CPU oracles behind the interface the step runner uses"""

    def __init__(self, p, alg, precision, dh, ah):
        self.alg, self.fbe = alg, alg == FBE
        self.o = Oracle(p["network"], p["tree"], p["config"], precision=precision)
        self.o.set_algorithm(alg, M)
        self.o.initialise(dh, ah)
        self.o.fbe_reset()

    def inject(self, st):
        for k, v in st.items():
            if k != "lbfgs":
                self.o.set(k, v)
        self.o.lbfgs_state(*st["lbfgs"])

    def read(self, full=False):
        out = {nm: self.o.get(nm) for _, nm in FBE_PAIRS}
        for nm in cur_names(self.alg):
            out[nm] = self.o.get(nm)
        if full:
            out.update(matS=self.o.get("matS"), matY=self.o.get("matY"), rho=self.o.get("rho"))
            col, mem, H = self.o.lbfgs_state()
            out["H"], out["colmem"] = np.array([H]), (col, mem)
        return out

    def prox(self):
        self.o.prox(); self.o.residual()

    def grad(self):
        self.o.gradient_fbe() if self.fbe else self.o.nama_residual()

    def hess(self):
        self.o.hessian_oracle()

    def value(self):
        return self.o.value_fbe()

    def direction(self):
        self.o.lbfgs_direction()

    def dual(self):
        self.o.dual_update()
        return self.o.primal_infeasibility()

    def ls(self, value_y):
        return self.o.line_search_fbe(value_y) if self.fbe else self.o.line_search_ame(value_y)

    def dist(self):
        return self.o.dist()


class SolverUnit:
    """an fp32 context of the library behind the same interface; ids: the global node ids of a shard's local nodes"""

    def __init__(self, p, alg, dh, ah, knobs=None, ids=None, **kw):
        self.alg, self.fbe, self.ids = alg, alg == FBE, ids
        self.s = capi.Solver(p["network"], p["tree"], p["config"], precision="f32", knobs=knobs, **kw)
        if ids is None:
            self.s.initialiseSmpcController(dh, ah)
            self.s.setAlgorithm(alg, M)

    def local(self, v, dim):
        return v if self.ids is None else v.reshape(-1, dim)[self.ids].ravel()

    def column(self, v):
        """one L-BFGS column (all xi | all psi) of the whole tree -> this context's nodes"""
        if self.ids is None:
            return v
        s = self.s
        nxi = s.full_nodes * 2 * s.nx
        return np.concatenate([self.local(v[:nxi], 2 * s.nx), self.local(v[nxi:], s.nu)])

    def dims(self):
        s = self.s
        d = {"x": s.nx, "u": s.nu, "xdir": s.nx, "udir": s.nu}
        return lambda nm: d.get(nm, s.nu if "Psi" in nm or nm == "psi" else 2 * s.nx)

    def inject(self, st):
        s, dim = self.s, self.dims()
        for bid, nm in FBE_PAIRS:
            s.set(bid, self.local(st[nm], dim(nm)))
        for bid, nm in zip(YVEC, cur_names(self.alg)):
            s.set(bid, self.local(st[nm], dim(nm)))
        n = st["matS"].size // (M + 1)
        for c in range(M + 1):
            s.lbfgsColumn(0, c, self.column(st["matS"][c * n:(c + 1) * n]))
            s.lbfgsColumn(1, c, self.column(st["matY"][c * n:(c + 1) * n]))
        col, mem, H = st["lbfgs"]
        s.lbfgsState(col, mem, H, st["rho"])

    def read(self, full=False):
        s = self.s
        out = {nm: s.get(bid) for bid, nm in FBE_PAIRS}
        for bid, nm in zip(YVEC, cur_names(self.alg)):
            out[nm] = s.get(bid)
        if full:
            out["matS"] = np.concatenate([s.lbfgsColumn(0, c) for c in range(M + 1)])
            out["matY"] = np.concatenate([s.lbfgsColumn(1, c) for c in range(M + 1)])
            col, mem, H, rho = s.lbfgsState()
            out["rho"], out["H"], out["colmem"] = rho, np.array([H]), (col, mem)
        return out

    def prox(self):
        self.s.proximalFunG(); self.s.computeFixedPointResidual()

    def grad(self):
        self.s.computeGradientFbe() if self.fbe else self.s.updateFixedPointResidualNamaAlgorithm()

    def hess(self):
        self.s.computeHessianOracalGlobalFbe()

    def value(self):
        return self.s.computeValueFbe()

    def direction(self):
        self.s.computeLbfgsDirection()

    def dual(self):
        self.s.dualUpdate()
        return self.s.updatePrimalInfeasibity()

    def ls(self, value_y):
        return self.s.computeLineSearchLbfgsUpdate(value_y) if self.fbe else self.s.computeLineSearchAmeLbfgsUpdate(value_y)

    def dist(self):
        return self.s.proxDistances()


# ---------------------------------------------------------------------------------------------------------------
# the bound, the table of errors, the cap on skipped states
# ---------------------------------------------------------------------------------------------------------------
class Ledger:
    """both errors of every compared (step, buffer), the violations of the bound, and the skipped / tried states of one case"""

    def __init__(self, case):
        self.case, self.rows, self.bad, self.tried, self.skipped = case, {}, [], {}, {}

    def compare(self, step, it, got, cpu, ref):
        for k, r in ref.items():
            if k == "colmem":
                if got[k] != r:
                    self.bad.append("%s it %d: (col, mem) %s, reference %s" % (step, it, got[k], r))
                continue
            self.scalar_or_vector(step, it, k, got[k], cpu[k], r)

    def scalar_or_vector(self, step, it, k, g, c, r):
        e_gpu, e_cpu = relmax(g, r), relmax(c, r)
        old = self.rows.get((step, k))
        if old is None or e_gpu - FACTOR * e_cpu > old[0] - FACTOR * old[1]:
            self.rows[(step, k)] = (e_gpu, e_cpu, it)
        if not e_gpu <= FACTOR * e_cpu + FLOOR:
            self.bad.append("%s it %d %s: e_gpu %.3e > 4 * e_cpu (%.3e) + %.3e" % (step, it, k, e_gpu, e_cpu, FLOOR))
        return e_gpu, e_cpu

    def state(self, kind, counted):
        self.tried[kind] = self.tried.get(kind, 0) + 1
        self.skipped[kind] = self.skipped.get(kind, 0) + (0 if counted else 1)

    def finish(self):
        """writes the table when asked to, then asserts the bound and the cap: at most one state in four skipped"""
        path = os.environ.get("RAPIDNET_F32_ERRORS")
        if path:
            with open(path, "a") as f:
                for (step, k), (e_gpu, e_cpu, it) in sorted(self.rows.items()):
                    if e_gpu or e_cpu:
                        f.write("%-40s %-10s %-12s it %d  e_gpu %.3e  e_cpu %.3e\n" % (self.case, step, k, it, e_gpu, e_cpu))
                for kind, n in sorted(self.tried.items()):
                    f.write("%-40s skipped %s states: %d of %d\n" % (self.case, kind, self.skipped[kind], n))
        assert not self.bad, "%s: %s" % (self.case, "; ".join(self.bad))
        for kind, n in self.tried.items():
            assert 4 * self.skipped[kind] <= n, "%s: %d of %d %s states skipped (at most one in four may be)" % (self.case, self.skipped[kind], n, kind)


def skip_rule_margin(st, alg):
    """distance of updateLbfgsBuffer's decision quantity <S,Y> / |S|^2 from its threshold 1e-6 |grad| (cubed below 1), relative to |<S,Y>|,
    on the injected state in fp64"""
    cx, cp, px, pp = cur_names(alg)
    S = np.concatenate([st["xi"] - st["prevXi"], st["psi"] - st["prevPsi"]])
    Y = np.concatenate([st[cx] - st[px], st[cp] - st[pp]])
    ng = float(np.sqrt(np.dot(st[cx], st[cx]) + np.dot(st[cp], st[cp])))
    if ng < 1:
        ng = ng ** 3
    sy, ss = float(np.dot(S, Y)), float(np.dot(S, S))
    return abs(sy - 1e-6 * ng * ss) / max(abs(sy), 1e-300)


def value_terms(o):
    """the FBE value's terms on an oracle that holds the state after prox and residual: <w, res>, step/2 |res|^2 and the rest (the g
    terms and the two primal terms, which the oracle does not expose one by one)"""
    step = float(o.config["stepSize"][0])
    t1 = float(np.dot(o.get("accXi"), o.get("resXi")) + np.dot(o.get("accPsi"), o.get("resPsi")))
    t2 = 0.5 * step * float(np.dot(o.get("resXi"), o.get("resXi")) + np.dot(o.get("resPsi"), o.get("resPsi")))
    v = o.value_fbe()
    return v, (t1, t2, v - t1 - t2)


def ls_candidates(o, alg, value_y):
    """The line search of `alg` on the fp64 oracle `o` (which holds the injected state and is left in the accepted state), candidate by
    candidate through the exposed steps: returns (slope, slope margin, [value of every evaluated candidate], tau).  The cumulative
    positions are 1, 1/2, 1/4, ...: the increments are +1, -1/2, -1/4, ... (oracle/apg_oracle.c, line_search_loop)."""
    step = float(o.config["stepSize"][0])
    b = o.buf
    dxi, dpsi = o.get("dirXi"), o.get("dirPsi")

    def oracle_on(xi_name, psi_name, vxi, vpsi):   # the Hessian oracle reads grad (FBE) / res (NAMA): lend it another input
        kx, kp = o.get(xi_name), o.get(psi_name)
        o.set(xi_name, vxi); o.set(psi_name, vpsi)
        o.hessian_oracle()
        o.set(xi_name, kx); o.set(psi_name, kp)

    def move(t):
        b("x")[:] += t * b("xdir"); b("u")[:] += t * b("udir")
        b("primalXi")[:] += t * b("primalXiDir"); b("primalPsi")[:] += t * b("primalPsiDir")

    if alg == FBE:
        terms = np.concatenate([o.get("gradXi") * dxi, o.get("gradPsi") * dpsi])
        slope = float(terms.sum())
        oracle_on("gradXi", "gradPsi", dxi, dpsi)
    else:
        rxi, rpsi = o.get("resXi"), o.get("resPsi")
        terms = -np.concatenate([rxi * dxi, rpsi * dpsi])
        slope = float(terms.sum())
        o.hessian_oracle()
        b("accXi")[:] += step * rxi; b("accPsi")[:] += step * rpsi
        move(step)
        b("dirXi")[:] -= step * rxi; b("dirPsi")[:] -= step * rpsi
        dxi, dpsi = o.get("dirXi"), o.get("dirPsi")
        oracle_on("resXi", "resPsi", dxi, dpsi)
    slope_margin = min(abs(slope), abs(slope + 1e-4)) / max(float(np.abs(terms).sum()), 1e-300)
    if slope > 0:
        return slope, slope_margin, [], 1.0
    if abs(slope) < 1e-4:
        return slope, slope_margin, [], 0.0
    vals, tau, i_step = [], 1.0, 0
    while i_step < 11:
        b("accXi")[:] += tau * dxi; b("accPsi")[:] += tau * dpsi
        move(tau)
        o.prox(); o.residual()
        vals.append(o.value_fbe())
        if vals[-1] <= value_y:
            i_step += 1
            if i_step < 10:
                tau = (-1.0 if i_step == 1 else tau) + 0.5 ** i_step
        else:
            i_step = 11
    return slope, slope_margin, vals, abs(tau)


def ls_margin(vals, value_y):
    return min(abs(v - value_y) for v in vals) / max(abs(value_y), 1.0)


# ---------------------------------------------------------------------------------------------------------------
# the step runner
# ---------------------------------------------------------------------------------------------------------------
def run_steps(name, alg, make_gpu, steps=("prox", "grad", "hess", "direction", "ls", "exits", "dual"), iters=ITERS, ls_knobs=((1, 0), (0, 0), (1, 1), (0, 1)),
              value_knobs=(1, 0), soft=False):
    """drives the fp64 loop and tests `steps` at `iters`; make_gpu(p, alg, dh, ah, knobs) builds the unit under test -- the library's
    fp32 context on the GPU, an fp32 oracle where the helpers are exercised on the CPU alone.  Returns the ledger."""
    kw = {"penalty_x": 2.0, "penalty_xs": 1.0} if soft else {}
    p = make_problem(name, **kw)
    dh, ah = synth.forecast_at(p["forecast"], 0)
    fbe = alg == FBE
    drv, ref, cpu = OracleUnit(p, alg, "f64", dh, ah), OracleUnit(p, alg, "f64", dh, ah), OracleUnit(p, alg, "f32", dh, ah)
    units = {}

    def unit(mfma, seq):
        if (mfma, seq) not in units:
            units[(mfma, seq)] = make_gpu(p, alg, dh, ah, {"value_mfma": mfma, "ls_sequential": seq})
        return units[(mfma, seq)]

    main = (value_knobs[0], ls_knobs[0][1])
    led = Ledger("%s%s %s" % (name, " soft" if soft else "", alg))
    searches = {k: 0 for k in ls_knobs}
    e_value = EPS32                       # the fp32 value error of this config: the largest e_gpu of the value step so far
    tripped = False
    thr = (p["config"]["penaltyStateX"][0] / p["config"]["stepSize"][0], p["config"]["penaltySafetyX"][0] / p["config"]["stepSize"][0])

    def three(st, g, fn):
        out = []
        for u in (g, cpu, ref):
            u.inject(st)
            out.append(fn(u))
        return out

    for it in range(max(iters) + 1):
        test = it in iters
        drv.o.solve_step()
        if test and "prox" in steps:
            st = capture(drv.o, alg)
            for mfma in value_knobs:
                g = unit(mfma, main[1])
                vg, vc, vr = three(st, g, lambda u: (u.prox(), u.value())[1])
                if mfma == value_knobs[0]:
                    led.compare("prox", it, g.read(), cpu.read(), ref.read())
                    # the value must not be a cancellation: checked on the reference against the largest term of its sum
                    v, terms = value_terms(ref.o)
                    assert abs(v) >= 0.1 * max(abs(t) for t in terms), "it %d: the FBE value %g cancels from terms %s" % (it, v, terms)
                    dx, ds = ref.dist()
                    if dx > thr[0] or ds > thr[1]:
                        tripped = True
                        gx, gs = g.dist()
                        assert (gx > thr[0]) == (dx > thr[0]) and (gs > thr[1]) == (ds > thr[1]), "soft branch taken differently: %s, reference %s" % ((gx, gs), (dx, ds))
                e_gpu, _ = led.scalar_or_vector("value mfma=%d" % mfma, it, "value", [vg], [vc], [vr])
                e_value = max(e_value, e_gpu)
        drv.prox()
        for step in ("grad", "hess"):
            if test and step in steps:
                st = capture(drv.o, alg)
                g = unit(*main)
                three(st, g, lambda u: getattr(u, step)())
                led.compare(step, it, g.read(), cpu.read(), ref.read())
        drv.grad()
        if it == 0:
            drv.dual()
            continue
        vo = drv.value()
        if test and "direction" in steps:
            st = capture(drv.o, alg)
            counted = skip_rule_margin(st, alg) >= SKIP_MARGIN
            led.state("direction", counted)
            if counted:
                g = unit(*main)
                three(st, g, lambda u: u.direction())
                led.compare("direction", it, g.read(True), cpu.read(True), ref.read(True))
        drv.direction()
        value_y = float(np.float32(vo))
        if test and "exits" in steps and it == iters[0]:
            # the two early exits (positive slope: tau = 1, nothing applied; |slope| < 1e-4: tau = 0) on a constructed direction
            st = capture(drv.o, alg)
            yx, yp = (st[cur_names(alg)[0]], st[cur_names(alg)[1]]) if fbe else (-st["resXi"], -st["resPsi"])
            for kind, scale in (("positive", 1.0), ("tiny", -1e-7 / max(float(np.dot(yx, yx) + np.dot(yp, yp)), 1e-300))):
                st2 = dict(st, dirXi=round32(scale * yx), dirPsi=round32(scale * yp))
                for k in ls_knobs[::2]:
                    g = unit(*k)
                    before = g.s.fbeCounters()["searches"] if hasattr(g, "s") else 0
                    tg, tc, tr = three(st2, g, lambda u: u.ls(value_y))
                    want = 1.0 if kind == "positive" else 0.0
                    if not (tg == want and tr == want and tc == want):
                        led.bad.append("exit %s it %d knobs %s: tau %s, reference %s, fp32 oracle %s" % (kind, it, k, tg, tr, tc))
                    led.compare("exit " + kind, it, g.read(), cpu.read(), ref.read())
                    assert not hasattr(g, "s") or g.s.fbeCounters()["searches"] == before
        if test and "ls" in steps:
            st = capture(drv.o, alg)
            ref.inject(st)
            slope, slope_margin, vals, tau_steps = ls_candidates(ref.o, alg, value_y)
            ref.inject(st)
            tau_ref = ref.ls(value_y)
            assert tau_ref == tau_steps, "the candidate walk (%s) is not the oracle's search (%s)" % (tau_steps, tau_ref)
            cpu.inject(st)
            tau_cpu = cpu.ls(value_y)
            counted = bool(vals) and slope_margin >= SKIP_MARGIN and ls_margin(vals, value_y) > LS_MARGIN * e_value and tau_cpu == tau_ref
            led.state("line-search", counted)
            if counted:
                for k in ls_knobs:
                    g = unit(*k)
                    g.inject(st)
                    tau = g.ls(value_y)
                    searches[k] += 1
                    if tau != tau_ref:
                        led.bad.append("ls it %d knobs %s: tau %s, reference %s (margin %.2e, value error %.2e)" % (it, k, tau, tau_ref, ls_margin(vals, value_y), e_value))
                    led.compare("ls mfma=%d seq=%d" % k, it, g.read(), cpu.read(), ref.read())
                    if soft:
                        dx, ds = ref.dist()
                        gx, gs = g.dist()
                        assert dx > thr[0] or ds > thr[1], "the accepted candidate's prox did not take the soft branch"
                        assert (gx > thr[0]) == (dx > thr[0]) and (gs > thr[1]) == (ds > thr[1])
        drv.ls(vo)
        if test and "dual" in steps:
            st = capture(drv.o, alg)
            g = unit(*main)
            ig, ic, ir = three(st, g, lambda u: u.dual())
            led.compare("dual", it, g.read(), cpu.read(), ref.read())
            # a signed arg-max entry: entries of equal magnitude within rounding may resolve to either sign -- the magnitude is compared
            led.scalar_or_vector("dual", it, "primalInf", [abs(ig)], [abs(ic)], [abs(ir)])
        drv.dual()
    if soft:
        assert tripped, "soft branch not exercised"
    for k, n in searches.items():       # the intended path: batched searches never trial by trial, sequential ones always
        g = units.get(k)
        if g is not None and hasattr(g, "s") and "ls" in steps:
            c = g.s.fbeCounters()
            assert c["searches"] == n and c["sequential"] == (n if k[1] or soft else 0), (k, n, c)
    for g in units.values():
        if hasattr(g, "s"):
            g.s.close()
    led.contexts = len(units)
    return led


def gpu_unit(p, alg, dh, ah, knobs):
    return SolverUnit(p, alg, dh, ah, knobs)


def cpu_unit(p, alg, dh, ah, knobs):
    return OracleUnit(p, alg, "f32", dh, ah)


STEP_CONFIGS = ["tiny", "small", "odd", "_f32_n1", "medium", "_f32_nu150", "tall"]


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", ["small", "odd", "_f32_n1"])
def test_helpers_on_the_cpu_oracles(name, alg):
    """No GPU: the fp32 oracle stands in for the context under test, so e_gpu = e_cpu and the bound holds by construction -- what runs is
    the injection into the oracles, the candidate walk of the line search (it must find the oracle's own tau), the margins and the
    accounting of skipped states: the fp64 and fp32 oracles alone stay inside the cap at ITERS."""
    led = run_steps(name, alg, cpu_unit, ls_knobs=((1, 0),), value_knobs=(1,))
    assert led.tried == {"direction": len(ITERS), "line-search": len(ITERS)}
    assert ("direction", "dirXi") in led.rows and ("ls mfma=1 seq=0", "accXi") in led.rows and ("value mfma=1", "value") in led.rows
    led.finish()


def test_ledger_refuses_a_violated_bound_and_too_many_skips():
    led = Ledger("self-test")
    ref = {"a": np.array([1.0, -2.0]), "colmem": (1, 2)}
    led.compare("s", 0, {"a": ref["a"] * (1 + 1e-7), "colmem": (1, 2)}, {"a": ref["a"] * (1 + 1e-7)}, ref)
    led.finish()
    led.compare("s", 1, {"a": ref["a"] * (1 + 1e-5), "colmem": (1, 3)}, {"a": ref["a"] * (1 + 1e-7)}, ref)
    assert len(led.bad) == 2
    with pytest.raises(AssertionError):
        led.finish()
    led = Ledger("self-test")
    for counted in (True, True, False, False):
        led.state("line-search", counted)
    with pytest.raises(AssertionError):
        led.finish()
    assert ls_margin([3.0, 2.5, 2.1], 2.0) == pytest.approx(0.05)


# ---------------------------------------------------------------------------------------------------------------
# 1 + 2: every step, the line search included, on the GPU
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", STEP_CONFIGS)
def test_f32_steps_match_the_f64_reference(name, alg):
    """prox + residual (+ value, on the matrix cores and on the vector ALUs), gradient / NAMA residual, Hessian oracle, L-BFGS direction
    (direction, S / Y columns, H, rho, (col, mem)), the line search (batched and sequential, value on the matrix cores and on the vector
    ALUs: the reference's tau exactly for every counted state, every buffer afterwards; the two early exits) and the dual update with the
    primal infeasibility, at ITERS, each from the driver's rounded state.  _f32_n1: n = 561 = 1 mod 4."""
    run_steps(name, alg, gpu_unit).finish()


@gpu
@pytest.mark.parametrize("alg", ALGS)
def test_f32_soft_branch_steps_match_the_f64_reference(alg):
    """penalties small enough that the soft-constraint branch trips (asserted on the distances): proximalFunG runs k_prox_soft, and the
    sequential line search -- the path such a search takes -- k_prox_soft_res on every trial.  The values of this problem's candidates
    lie closer to the reference value than those of the default one (margins of 2e-5 ... 2e-3 against fp32 value errors of 1e-7), so the
    iterations are chosen per algorithm where the fp64 and fp32 oracles alone count every state: NAMA's 7 and 8 have margins of 3e-6."""
    iters = ITERS if alg == FBE else (5, 6, 9, 10)
    run_steps("small", alg, gpu_unit, steps=("prox", "ls"), iters=iters, ls_knobs=((1, 1), (0, 1)), soft=True).finish()


@gpu
@pytest.mark.parametrize("alg", ALGS)
def test_f32_value_and_line_search_at_the_headline_dimensions(alg):
    """barcelona31 (nu = 114: k_value_mfma's eight-tile, 32-k-step form with W in registers): the value step and one line search"""
    run_steps("barcelona31", alg, gpu_unit, steps=("prox", "ls"), iters=(5,), ls_knobs=((1, 0), (1, 1))).finish()


# ---------------------------------------------------------------------------------------------------------------
# the value paths no quasi-Newton test reached in either precision: whole fp64 loops
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", ["_f32_nu150", "tall"])
def test_f64_loop_matches_oracle_on_the_untested_value_paths(name, alg):
    """test_gpu_fbe_nama.test_loop_matches_oracle, at its tolerances, for nu = 150 (k_value_mfma without W in registers: the slab_mfma
    fallback) and nu = 300 (the vector-ALU value kernels by default).  The nu = 300 case is a regression test as well: its candidates' tile
    (115 KB of LDS in fp64) needs the function attribute, which rn_set_algorithm used to request for all 160 KB of the CU -- refused, because
    k_ls_value's static arrays share them -- so every search silently ran trial by trial (sequential == searches)."""
    p = make_problem(name)
    dh, ah = synth.forecast_at(p["forecast"], 0)
    o = Oracle(p["network"], p["tree"], p["config"])
    o.set_algorithm(alg, 5); o.initialise(dh, ah); o.fbe_reset()
    s = capi.Solver(p["network"], p["tree"], p["config"])
    s.initialiseSmpcController(dh, ah)
    s.setAlgorithm(alg, 5)
    iters = 8
    ho, vo, to = o.fbe_nama(iters)
    hs, vs, ts = (s.algorithmGlobalFbe if alg == FBE else s.algorithmNama)(iters)
    assert np.array_equal(ts, to), (ts, to)
    assert relmax(vs, vo) < REL_TOL
    assert relmax(hs, ho) < 1e-7
    compare_fbe(s, o, alg, 1e-8, "%s %s after %d iterations" % (alg, name, iters))
    assert s.lbfgsState()[:2] == o.lbfgs_state()[:2]
    c = s.fbeCounters()
    assert c["searches"] >= 1 and c["sequential"] == 0 and c["searches"] <= c["batches"] <= 3 * c["searches"], c
    s.close()


# ---------------------------------------------------------------------------------------------------------------
# 3: shards -- the crown's cut-off `first` inside a vector
# ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("alg", ALGS)
def test_f32_sharded_direction_and_value(alg):
    """two rank-local fp32 contexts of `small` (in-process group, one thread per rank): ranks other than 0 start counting at
    first = crown * 19 values, which is no multiple of 4.  The driver's rounded state goes into each rank by its global nodes; the
    reassembled direction, S / Y columns, H, rho and the value on every rank against the fp64 reference of the whole tree, the fp32
    oracle of the whole tree as the yardstick.  A crown element counted twice or not at all changes the value, H and rho at first order."""
    world = 2
    p = make_problem("small")
    dh, ah = synth.forecast_at(p["forecast"], 0)
    drv, ref, cpu = OracleUnit(p, alg, "f64", dh, ah), OracleUnit(p, alg, "f64", dh, ah), OracleUnit(p, alg, "f32", dh, ah)
    group = capi.local_group_create(world)
    shards = []
    for r in range(world):
        u = SolverUnit(p, alg, dh, ah, ids=(), rank=r, nranks=world, cut_stage=0)
        u.s.joinLocalGroup(group, r)
        u.ids = np.asarray(u.s.global_nodes)
        shards.append(u)
    s0 = shards[0].s
    ny = 2 * s0.nx + s0.nu
    cum = np.asarray(p["tree"]["nodesPerStageCumul"], int)
    crown = int(cum[s0.shardInfo()["cut_stage"]])
    assert np.array_equal(shards[1].ids[:crown], np.arange(crown)) and shards[1].ids[crown] > crown - 1 and not set(shards[0].ids[crown:]) & set(shards[1].ids[crown:])
    assert (crown * ny) % 4 != 0, "first = %d * %d is a multiple of 4" % (crown, ny)
    led = Ledger("small 2 ranks %s" % alg)
    states = []
    for it in range(max(ITERS) + 1):
        drv.o.solve_step()
        st_prox = capture(drv.o, alg)
        drv.prox(); drv.grad()
        if it:
            vo = drv.value()
            st = capture(drv.o, alg)
            if it in ITERS:
                counted = skip_rule_margin(st, alg) >= SKIP_MARGIN
                led.state("direction", counted)
                states.append((it, st_prox, st if counted else None))
            drv.direction()
            drv.ls(vo)
        drv.dual()
    out, errs = [[] for _ in range(world)], []

    def work(i):
        try:
            u = shards[i]
            u.s.initialiseSmpcController(dh, ah)
            u.s.setAlgorithm(alg, M)
            for it, st_prox, st in states:
                u.inject(st_prox)
                u.prox()
                v = u.value()
                res = None
                if st is not None:
                    u.inject(st)
                    u.direction()
                    res = u.read(True)
                out[i].append((v, res))
        except Exception as e:   # noqa: BLE001
            errs.append((i, e))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    dim = shards[0].dims()
    nodes = s0.full_nodes
    for j, (it, st_prox, st) in enumerate(states):
        vc, vr = [(u.inject(st_prox), u.prox(), u.value())[2] for u in (cpu, ref)]
        for r in range(world):
            led.scalar_or_vector("value rank %d" % r, it, "value", [out[r][j][0]], [vc], [vr])
        if st is None:
            continue
        for u in (cpu, ref):
            u.inject(st)
            u.direction()
        rc, rr = cpu.read(True), ref.read(True)
        got = {}
        for nm in ("dirXi", "dirPsi"):
            got[nm] = partition.scatter_to_global([out[r][j][1][nm] for r in range(world)], [u.ids for u in shards], nodes, dim(nm))
        n = nodes * ny
        nxi = nodes * 2 * s0.nx
        for nm in ("matS", "matY"):
            cols = []
            for c in range(M + 1):
                parts = [out[r][j][1][nm].reshape(M + 1, -1)[c] for r in range(world)]
                lx = [len(u.ids) * 2 * s0.nx for u in shards]
                cols.append(partition.scatter_to_global([q[:k] for q, k in zip(parts, lx)], [u.ids for u in shards], nodes, 2 * s0.nx))
                cols.append(partition.scatter_to_global([q[k:] for q, k in zip(parts, lx)], [u.ids for u in shards], nodes, s0.nu))
            got[nm] = np.concatenate(cols)
            assert got[nm].size == (M + 1) * n and nxi < n
        for r in range(world):
            mine = dict(got, rho=out[r][j][1]["rho"], H=out[r][j][1]["H"], colmem=out[r][j][1]["colmem"])
            led.compare("direction rank %d" % r, it, mine, rc, {k: rr[k] for k in mine})
    for u in shards:
        u.s.close()
    capi.local_group_destroy(group)
    led.finish()


# ---------------------------------------------------------------------------------------------------------------
# 4: guard mode's body, rn_get_range / rn_set_range
# ---------------------------------------------------------------------------------------------------------------
def guard_body(alg):
    """the `odd` fp32 direction + line-search steps (n = 891 = 3 mod 4: scalar walks of misaligned columns, tails) for tests/test_gpu_guard.py"""
    led = run_steps("odd", alg, gpu_unit, steps=("prox", "direction", "ls"), ls_knobs=((1, 0), (0, 0), (0, 1)))
    led.rows.clear(); led.tried.clear()       # (the table of errors lists these steps already: test_f32_steps_match_the_f64_reference)
    led.finish()
    return led.contexts


@gpu
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_get_range_set_range_round_trip(precision):
    """rn_get_range / rn_set_range: a range whose start and length are no multiples of 4 in a plain buffer (x) and whole nodes of a
    dual-shaped one (xi), the neighbours untouched, ranges outside the buffer and split nodes refused"""
    p = make_problem("odd")
    s = capi.Solver(p["network"], p["tree"], p["config"], precision=precision)
    s.initialiseSmpcController(*synth.forecast_at(p["forecast"], 0))
    s.algorithmApg(5)
    rng = np.random.default_rng(5)
    rnd = round32 if precision == "f32" else (lambda v: v)
    for bid, first, n in ((capi.BUF_X, 13, 31), (capi.BUF_U, 27, 101), (capi.BUF_XI, 3 * 14, 5 * 14), (capi.BUF_PSI, 7 * 13, 9 * 13)):
        assert first % 4 and n % 4
        full = s.get(bid)
        assert np.array_equal(s.getRange(bid, first, n), full[first:first + n])
        v = rnd(rng.standard_normal(n))
        s.setRange(bid, first, v)
        want = full.copy()
        want[first:first + n] = v
        assert np.array_equal(s.get(bid), want)                       # the range as written, the neighbours untouched
        assert np.array_equal(s.getRange(bid, first, n), v)
        for f, m in ((full.size - 3, 4), (full.size, 1)):
            with pytest.raises(capi.RapidNetError):
                s.getRange(bid, f, m)
            with pytest.raises(capi.RapidNetError):
                s.setRange(bid, f, np.zeros(m))
    for f, m in ((3, 14), (14, 15)):                                 # dual-shaped buffers are addressed in whole nodes
        with pytest.raises(capi.RapidNetError):
            s.getRange(capi.BUF_XI, f, m)
        with pytest.raises(capi.RapidNetError):
            s.setRange(capi.BUF_XI, f, np.zeros(m))
    with pytest.raises(capi.RapidNetError):
        s.getRange(10 ** 6, 0, 1)
    s.close()
