"""The dual update of ONE iteration alone (rn_debug_dual_update: k_dual_stage, k_dual_fused, the fix-up pass, the bookkeeping kernels) against an exactly
rounded restatement (dual_update_ref.py).  No case is a solve: each is one or a few hook calls on buffers made for it.

 (a) normal data: every form gives the restatement's numbers, element for element (np.array_equal): the main pass stage-tiled and flat, materialised and
     not, behind a scaled and an unscaled walk; the exact form, the exact sharded form, the optimistic close.  lo / hi of the context equal the bounds
     rebuilt from its tables.  The dist^2 sums are within n 2^-53 (relative to the exact sum; n the terms; every term is nonnegative, so this is the
     bound of any summation order in fp64) of the exact sum of the restated squares.  The decision, the scales and the fixed-up outputs are restated
     from the kernel's OWN sums and must then be equal.  Thresholds: neither half trips, each alone, both.
 (b) integer data (zero bounds, lambda a power of two, iteration 0 whose extrapolation parameter is 0): everything bit for bit, the sums included, at
     thr = D (not tripped: the test is strict), the double just below D (tripped) and D / 2 (scale exactly 1/2).
 (c) ties: the largest |res| twice with opposite signs, the negative one first: in one vector, two trips of a thread, two lanes, two waves, two
     workgroups of a stage, a crown and a regular workgroup, two stages, one grid stride apart in the flat kernel, its vector body against its tail,
     the same magnitude in xi and psi, an all-zero residual, a workgroup without an xi element (the -1 sentinel).  (A workgroup without a PSI element
     cannot occur: every tile of either kernel ends at the end of a node or holds 256 consecutive vectors, and a node's last vector is psi.)
 (d) the cells of k_dual_stage, (e) of the flat kernel, each asserted from the hook's record (dual_update_ref.stage_cells / coordinates).
 (f) shards: the ranks' sums add up to the one-GPU context's, the crown counted once.
 (g) the step-wise entry points give the exact form's numbers.
 (h) the hook's refusals, and that it disturbs nothing.
$DUAL_UPDATE_ERRORS names a file every case appends its cells and its worst fraction of the d^2 bound to (profiles/dual_update_errors.txt)."""
import math
import os

import numpy as np
import pytest

import dual_update_ref as ref
from rapidnet_amd import capi, synth

pytestmark = pytest.mark.gpu

# (seed index, nx, nu, nd, ne, N, branching)
EXTRA = {
    "du_k128": (60, 3, 6, 4, 2, 3, [128]),        # ny 12: a stage of 128 nodes is 768 fp64 vectors: three tiles of one trip, one tile of three
    "du_k43": (63, 3, 6, 4, 2, 3, [43]),          # 258 vectors: a last tile of two (both psi: no xi element in that workgroup)
    "du_k43x3": (64, 3, 6, 4, 2, 4, [43, 3]),     # node0 = 44: 264 crown vectors, two crown workgroups of one trip, one of two
    "du_big": (61, 3, 6, 4, 2, 3, [22100]),       # 530 412 fp64 elements: 1 037 workgroups of one trip (fold_partials' second round)
    "du_flatbig": (62, 5, 9, 6, 3, 3, [1800]),    # ny 19: 68 419 elements: the fix-up launch has fewer workgroups than the flat main pass
    "du_tail1": (65, 5, 9, 6, 3, 4, [2]),         # 7 nodes of ny 19: 133 elements: a tail of 1 in fp32 and in fp64
    "du_k256": (66, 3, 6, 4, 2, 3, [256]),        # 768 fp32 vectors per stage: three live trips of one thread in either type
    "du_k100x2": (67, 3, 6, 4, 2, 4, [100, 2]),   # node0 = 101: 303 fp32 crown vectors: two crown workgroups of one trip in either type
}
for _k, _v in EXTRA.items():
    synth.CONFIGS.setdefault(_k, _v)
FORMS = ["f64", "f32"]
FILL = 7777.0
_PROBLEMS = {}


def problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = synth.make_problem(name)
    return _PROBLEMS[name]


def record(tag, what):
    print("%s: %s" % (tag, what))
    path = os.environ.get("DUAL_UPDATE_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write("%s: %s\n" % (tag, what))


def context(name, form, knobs=None, lam=None, zero_bounds=False, **kw):
    p = problem(name)
    cfg = dict(p["config"])
    if lam is not None:
        cfg["stepSize"] = [lam]
    s = capi.Solver(p["network"], p["tree"], cfg, precision=form, knobs=knobs, **kw)
    s.factorStep()
    s.apgReset()
    if zero_bounds:
        s.setBounds("shared", np.zeros(s.nx), np.zeros(s.nx), np.zeros(s.nx), np.zeros(s.nu), np.zeros(s.nu))
    return s


def set_thresholds(s, thr_x, thr_s):
    """penalties such that gamma / lambda are the wanted thresholds (exactly, where lambda is a power of two); returns what the context then uses"""
    _, info = s.debugDualUpdate("info")
    lam = info["lambda"]
    step = float(np.ravel(s.config["stepSize"])[0])
    s._check(s.lib.rn_set_parameters(s.h, step, thr_x * step, thr_s * step))
    _, info = s.debugDualUpdate("info")
    assert info["lambda"] == lam
    assert info["thrX"] == (thr_x * step) / step and info["thrS"] == (thr_s * step) / step
    return info["thrX"], info["thrS"]


def load(s, case):
    """the case's Hx, w, y into the context's buffers; read back and asserted"""
    nx2 = 2 * s.nx
    for xi, psi, key in ((capi.BUF_PRIMAL_XI, capi.BUF_PRIMAL_PSI, "hx"), (capi.BUF_ACC_XI, capi.BUF_ACC_PSI, "w"), (capi.BUF_UPD_XI, capi.BUF_UPD_PSI, "yp")):
        v = np.asarray(case[key], dtype=np.float64)
        s.set(xi, np.ascontiguousarray(v[:, :nx2]).ravel())
        s.set(psi, np.ascontiguousarray(v[:, nx2:]).ravel())
        back = np.concatenate([s.get(xi).reshape(s.nodes, nx2), s.get(psi).reshape(s.nodes, s.nu)], axis=1)
        assert np.array_equal(back, v), key


def tables(s, form, **kw):
    """the context's tables through the hook, and the bounds rebuilt from them; asserts that the materialised bounds are those"""
    dt = ref.DTYPES[form]
    out, info = s.debugDualUpdate("info", tables=True, **kw)
    lo, hi, k = ref.bounds_from_tables(out["sqrtp"], out["dy"], out["blo"], out["bhi"], out["stageOf"], int(info["bStrideStage"]), int(info["bStrideNode"]), s.nx, dt)
    assert np.array_equal(out["lo"], lo.astype(np.float64)) and np.array_equal(out["hi"], hi.astype(np.float64)), "the context's lo / hi are not the bounds rebuilt from its tables"
    return lo, hi, k, info


def inputs(case, lo, hi, info, k=None):
    """the restatement's inputs; k: the walk left Hx unscaled (hx = k * value, one product in the type)"""
    hx = case["hx"] if k is None else (k * case["hx"].astype(k.dtype)).astype(k.dtype)
    return dict(hx=hx, w=case["w"], yp=case["yp"], lo=lo, hi=hi, lam=info["lambda"], inv_lam=info["invLambda"], ln=info["ln"], nx=case["nx"])


def lam_table(n):
    th0, th1, out = 1.0, 1.0, []
    for _ in range(n):
        out.append(th1 * (1.0 / th0 - 1.0))
        th0, th1 = th1, 0.5 * (math.sqrt(th1 ** 4 + 4 * th1 ** 2) - th1 ** 2)
    return out


def same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want).astype(np.float64)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    return np.array_equal(got, want)


def fold(partials):
    """the lowest-index fold of raw partials: ((abs, val, idx) xi, (abs, val, idx) psi)"""
    out = []
    for a, v, i in ((2, 3, 6), (4, 5, 7)):
        live = partials[partials[:, i] >= 0]
        if live.shape[0] == 0:
            out.append((-1.0, 0.0, -1))
            continue
        m = live[:, a].max()
        t = live[live[:, a] == m]
        j = t[:, i].argmin()
        out.append((float(m), float(t[j, v]), int(t[j, i])))
    return out


def check_d2(tag, info, r, worst):
    """the kernel's sums against the exact sums of the restated squares: n 2^-53 of the sum (any order of n nonnegative terms in fp64)"""
    for key, n in (("d2x", r["nX"]), ("d2s", r["nS"])):
        bound = n * 2.0 ** -53 * r[key]
        err = abs(info[key] - r[key])
        assert err <= bound, (tag, key, info[key], r[key], err, bound)
        if bound > 0:
            worst[0] = max(worst[0], err / bound)


def check_main(tag, out, info, r, materialize):
    yn, wn, z, res, _ = r["main"]
    assert same(out["ynew"], yn) and same(out["wnext"], wn), (tag, "y+ / w_next of the main pass")
    if materialize:
        assert same(out["z"], z) and same(out["res"], res), (tag, "z / res of the main pass")
    else:
        assert (out["z"] == FILL).all() and (out["res"] == FILL).all(), (tag, "a pass that does not materialise wrote z / res")
    assert fold(out["partials"]) == [r["main_argmax"][0], r["main_argmax"][1]], (tag, fold(out["partials"]), r["main_argmax"])


def check_closed(tag, form_name, out, info, inp, dt, thr, materialize, cache, counted=None):
    """a form with bookkeeping: the decision and the fixed-up outputs restated from the kernel's own sums"""
    key = (info["d2x"], info["d2s"], thr)
    if key not in cache:
        cache[key] = ref.restate(inp, dt, thr[0], thr[1], d2=(info["d2x"], info["d2s"]), counted=counted)
    r = cache[key]
    assert info["distX"] == r["distX"] and info["distS"] == r["distS"], (tag, "distances")
    if form_name == "optimistic_close":
        assert info["violated"] == r["tripped"], (tag, "verdict", info["violated"], r["tripped"])
        want, am, hist = r["main"][:4], r["main_argmax"], r["main_hist"]
    else:
        assert (info["tripped"], info["scaleX"], info["scaleS"]) == (r["tripped"], r["scaleX"], r["scaleS"]), (tag, "decision", info, r["tripped"], r["scaleX"], r["scaleS"])
        want, am, hist = r["out"], r["argmax"], r["hist"]
    assert same(out["ynew"], want[0]) and same(out["wnext"], want[1]), (tag, "y+ / w_next")
    if materialize:
        assert same(out["z"], want[2]) and same(out["res"], want[3]), (tag, "z / res")
    else:
        assert (out["z"] == FILL).all() and (out["res"] == FILL).all(), tag
    got = ((info["absXi"], info["valXi"], int(info["idxXi"])), (info["absPsi"], info["valPsi"], int(info["idxPsi"])))
    assert got == (am[0], am[1]), (tag, "arg-max", got, am)
    assert info["hist"] == hist, (tag, "history entry", info["hist"], hist)
    assert info["itAfter"] == info["_t"] + 1, (tag, "iteration counter of the scratch state")
    return r


def run(s, form_name, t=0, **kw):
    out, info = s.debugDualUpdate(form_name, iteration=t, fill=FILL, **kw)
    info["_t"] = t
    return out, info


class _Ctx:
    """a context with the bookkeeping the cases share"""

    def __init__(self, name, form, knobs=None, lam=None, zero_bounds=False, **kw):
        self.s = context(name, form, knobs, lam, zero_bounds, **kw)
        self.form, self.dt = form, ref.DTYPES[form]

    def close(self):
        self.s.close()


# ---- (a) normal data ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["tiny", "fan", "small", "odd", "medium"])
def test_every_form_restates_on_normal_data(name, form):
    c = _Ctx(name, form)
    s, dt = c.s, c.dt
    try:
        t = 3
        lo, hi, k, info0 = tables(s, form, iteration=t)
        assert abs(info0["ln"] - lam_table(t + 2)[t + 1]) <= 1e-6 * abs(info0["ln"]) and info0["ln"] != 0
        case = ref.normal_case(lo, hi, info0["lambda"], s.nx, 100 + len(name), dt)
        load(s, case)
        inp = inputs(case, lo, hi, info0)
        inp_u = inputs(case, lo, hi, info0, k)
        stage = info0["kernel"] == "k_dual_stage"
        r0 = ref.restate(inp, dt, math.inf, math.inf)
        r0u = ref.restate(inp_u, dt, math.inf, math.inf)
        ref.assert_mix(ref.fma_array(dt(info0["invLambda"]), case["w"], case["hx"], dt), lo, hi, s.nx)
        worst, cells = [0.0], []
        for mat, flat, unsc in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)):
            out, info = run(s, "main", t, materialize=mat, flat=flat, unscaled=unsc)
            tag = "%s %s main mat %d flat %d unscaled %d" % (name, form, mat, flat, unsc)
            assert info["kernel"] == ("k_dual_stage" if stage and not flat else "k_dual_fused"), (tag, info["kernel"])
            assert info["scale"] == (1 if unsc and not flat and stage else 0) and info["preScale"] == (1 if unsc and (flat or not stage) else 0), tag
            r = r0u if unsc else r0
            check_main(tag, out, info, r, mat)
            check_d2(tag, info, r, worst)
            cells.append("%s grid %d" % (info["kernel"], info["grid"]))
        Dx, Ds = r0["distX"], r0["distS"]
        assert Dx > 0 and Ds > 0
        cache = {}
        for thr in ((4 * Dx, 4 * Ds), (Dx / 3, 4 * Ds), (4 * Dx, Ds / 3), (Dx / 3, Ds / 3)):
            thr = set_thresholds(s, *thr)
            for form_name, kw in (("exact", dict(materialize=1)), ("exact", dict(materialize=0)), ("exact_sharded", dict(materialize=1)), ("optimistic_close", dict(materialize=0)),
                                  ("exact", dict(materialize=1, flat=1))):
                out, info = run(s, form_name, t, **kw)
                tag = "%s %s %s %s thr %s" % (name, form, form_name, kw, thr)
                r = check_closed(tag, form_name, out, info, inp, dt, thr, kw.get("materialize"), cache)
                check_d2(tag, info, r0, worst)
                if form_name != "optimistic_close":
                    assert r["tripped"] == (1 if (thr[0] < Dx or thr[1] < Ds) else 0), tag
        record("normal %s %s" % (name, form), "worst d2 error / bound %.3f; %s; thresholds none / box / safety / both tripped" % (worst[0], sorted(set(cells))))
    finally:
        c.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("gran, stride", [("stage", "bStrideStage"), ("node", "bStrideNode")])
def test_bounds_per_stage_and_per_node(gran, stride, form):
    """both strides of the bounds tables, stage-tiled and flat; rows with lo == hi planted"""
    c = _Ctx("tiny", form)
    s, dt = c.s, c.dt
    try:
        rows = s.N if gran == "stage" else s.nodes
        rng = np.random.default_rng(7)
        b = s.getBounds()
        mk = lambda v, d: np.repeat(np.asarray(v).reshape(1, -1), rows, axis=0) * rng.uniform(0.5, 1.5, (rows, d))
        xmin, xmax, xs, umin, umax = mk(b["xmin"], s.nx), mk(b["xmax"], s.nx), mk(b["xsafe"], s.nx), mk(b["umin"], s.nu), mk(b["umax"], s.nu)
        xmax, umax = np.maximum(xmax, xmin), np.maximum(umax, umin)
        xmax[rows // 2] = xmin[rows // 2]      # lo == hi
        umax[rows - 1] = umin[rows - 1]
        s.setBounds(gran, xmin, xmax, xs, umin, umax)
        lo, hi, k, info0 = tables(s, form, iteration=2)
        assert info0[stride] == s.ny and info0["bRows"] == rows and info0["bStrideStage"] + info0["bStrideNode"] == s.ny, info0
        assert (lo == hi).any()
        case = ref.normal_case(lo, hi, info0["lambda"], s.nx, 11, dt)
        load(s, case)
        inp = inputs(case, lo, hi, info0)
        r0 = ref.restate(inp, dt, math.inf, math.inf)
        worst = [0.0]
        for flat in (0, 1):
            out, info = run(s, "main", 2, materialize=1, flat=flat)
            assert info["kernel"] == ("k_dual_fused" if flat else "k_dual_stage")
            check_main("bounds per %s flat %d" % (gran, flat), out, info, r0, 1)
            check_d2("bounds per %s" % gran, info, r0, worst)
        thr = set_thresholds(s, r0["distX"] / 2, r0["distS"] / 2)
        out, info = run(s, "exact", 2, materialize=1)
        check_closed("bounds per %s exact" % gran, "exact", out, info, inp, dt, thr, 1, {})
        record("bounds per %s %s" % (gran, form), "strides %d / %d, rows %d, worst d2 error / bound %.3f" % (info0["bStrideStage"], info0["bStrideNode"], rows, worst[0]))
    finally:
        c.close()


# ---- (b) integer data ----------------------------------------------------------------------------------------------------------------------------------------
def integer_setup(c, seed=3, reserve=48):
    s = c.s
    lo, hi, k, info0 = tables(s, c.form)
    box, safe, psi = ref.column_groups(s.nodes, s.nx, s.ny)
    assert not lo.any() and not hi[box | psi].any() and (hi[safe] >= 1e6).all(), "zero physical bounds: lo = hi = 0, the safety half open above"
    assert info0["ln"] == 0.0 and info0["lambda"] == 0.125
    case = ref.integer_case(s.nodes, s.nx, s.ny, seed, lam_log2=-3, dtype=c.dt, reserve=reserve)
    return case, lo, hi, info0


def integer_ref(case, nx, scX=0.0, scS=0.0):
    """plain numpy on exact values: the outputs with scales that are 0 or 1/2"""
    yn, wn, z, res, d2x, d2s = ref.integer_main_ref(case, nx)
    if scX or scS:
        t = case["tint"].astype(np.float64)
        nodes, ny = t.shape
        box, safe, _ = ref.column_groups(nodes, nx, ny)
        z = z + np.where(box, scX * t, np.where(safe, scS * np.minimum(t, 0), 0.0))
        res = case["hx"].astype(np.float64) - z
        yn = case["w"].astype(np.float64) + case["lam"] * res
        wn = yn.copy()
    return yn, wn, z, res, d2x, d2s


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["tiny", "odd", "medium"])
def test_integer_data_bit_for_bit(name, form):
    c = _Ctx(name, form, lam=0.125, zero_bounds=True)
    s, dt = c.s, c.dt
    try:
        case, lo, hi, info0 = integer_setup(c)
        load(s, case)
        inp = inputs(case, lo, hi, info0)
        DX, DS = float(case["DX"]), float(case["DS"])
        below = lambda d: float(np.nextafter(np.float64(d), 0.0))
        for what, thr in (("thr = D", (DX, DS)), ("thr just below D", (below(DX), below(DS))), ("thr = D / 2", (DX / 2, DS / 2))):
            thr = set_thresholds(s, *thr)
            assert thr == ((DX, DS) if what == "thr = D" else (below(DX), below(DS)) if "below" in what else (DX / 2, DS / 2))
            cache = {}
            for form_name in ("exact", "exact_sharded", "optimistic_close"):
                out, info = run(s, form_name, 0, materialize=1)
                tag = "%s %s %s %s" % (name, form, form_name, what)
                assert info["d2x"] == DX * DX and info["d2s"] == DS * DS and info["distX"] == DX and info["distS"] == DS, (tag, info["d2x"], DX * DX, info["d2s"], DS * DS)
                r = check_closed(tag, form_name, out, info, inp, dt, thr, 1, cache)
                tripped = what != "thr = D"
                if form_name == "optimistic_close":
                    assert info["violated"] == int(tripped), tag
                    want = integer_ref(case, s.nx)
                else:
                    assert info["tripped"] == int(tripped), tag
                    if what == "thr = D / 2":
                        assert info["scaleX"] == 0.5 and info["scaleS"] == 0.5, tag
                    if what == "thr just below D":
                        assert 0 < info["scaleX"] < 1e-15 and 0 < info["scaleS"] < 1e-15, tag
                        continue      # (outputs: the restatement's, checked above)
                    want = integer_ref(case, s.nx, *((0.5, 0.5) if tripped else (0.0, 0.0)))
                for got, w, nm in zip((out["ynew"], out["wnext"], out["z"], out["res"]), want, ("y+", "w_next", "z", "res")):
                    assert np.array_equal(got, w), (tag, nm)
        record("integer %s %s" % (name, form), "D = %d, %d; %s grid %d; thresholds D, below D, D / 2 in exact, exact_sharded, optimistic_close" % (DX, DS, info["kernel"], info["grid"]))
    finally:
        c.close()


# ---- (c) ties ------------------------------------------------------------------------------------------------------------------------------------------------
def _eq(*keys):
    return lambda co, a, js: np.logical_and.reduce([co[k][js] == co[k][a] for k in keys])


PLACEMENTS = {
    # name -> (tree, knobs, flat, half ("box" | "psi"), predicate over the coordinates of the two elements)
    # (a thread's trips are 256 vectors apart: with 6 or 3 vectors per node only psi vectors meet psi vectors there)
    "one vector": ("tiny", None, 0, "box", _eq("vec")),
    "two trips of a thread": ("du_k256", {"dual_trips": 3}, 0, "psi", lambda co, a, js: _eq("block", "tid")(co, a, js) & (co["trip"][js] != co["trip"][a])),
    "two trips of a thread, double-buffered": ("du_k256", {"dual_trips": 3, "dual_pipe": 2}, 0, "psi", lambda co, a, js: _eq("block", "tid")(co, a, js) & (co["trip"][js] == co["trip"][a] + 2)),
    "two lanes of a wave": ("du_k128", {"dual_trips": 1}, 0, "box", lambda co, a, js: _eq("block", "wave", "trip")(co, a, js) & (co["tid"][js] != co["tid"][a])),
    "two waves of a workgroup": ("du_k128", {"dual_trips": 1}, 0, "psi", lambda co, a, js: _eq("block")(co, a, js) & (co["wave"][js] != co["wave"][a])),
    "two workgroups of a stage": ("du_k128", {"dual_trips": 1}, 0, "box", lambda co, a, js: _eq("stage_block")(co, a, js) & (co["block"][js] != co["block"][a]) & (co["crown"][a] == 0)),
    "a crown and a regular workgroup": ("du_k43x3", {"dual_trips": 1}, 0, "box", lambda co, a, js: (co["crown"][a] == 1) & (co["crown"][js] == 0)),
    "two crown workgroups": ("du_k100x2", {"dual_trips": 1}, 0, "psi", lambda co, a, js: (co["crown"][a] == 1) & (co["crown"][js] == 1) & (co["block"][js] != co["block"][a])),
    "two stages": ("du_k128", {"dual_trips": 3}, 0, "psi", lambda co, a, js: (co["crown"][a] == 0) & (co["crown"][js] == 0) & (co["stage_block"][js] != co["stage_block"][a])),
    "flat, one grid stride apart": ("small", None, 1, "box", lambda co, a, js: _eq("block", "tid")(co, a, js) & (co["trip"][js] == co["trip"][a] + 1) & (co["tail"][js] == 0)),
    "flat, two workgroups": ("small", None, 1, "psi", lambda co, a, js: (co["block"][js] != co["block"][a]) & (co["trip"][js] == co["trip"][a])),
    "flat, vector body against scalar tail": ("odd", None, 1, "psi", lambda co, a, js: (co["tail"][a] == 0) & (co["tail"][js] == 1)),
}


def _check_tie(tag, s, case, lo, hi, info0, a, b, dt, flat, other=None):
    """every form on a case with the tie planted at elements a < b (and, other: a second tie in the other half)"""
    load(s, case)
    inp = inputs(case, lo, hi, info0)
    r0 = ref.restate(inp, dt, math.inf, math.inf)
    half = 0 if (a % s.ny) < 2 * s.nx else 1
    M = float(abs(case["hx"].ravel()[a]))
    assert r0["main_argmax"][half] == (M, -M, a), (tag, r0["main_argmax"], a, b)
    assert ref.argmax_ref(r0["main"][3], s.nx, mistake="last")[half][1] == M, tag      # a wrong rule WOULD change the sign here
    out, info = run(s, "main", 0, materialize=1, flat=flat)
    check_main(tag + " main", out, info, r0, 1)
    got = fold(out["partials"])[half]
    assert got == (M, -M, a), (tag, "main partials", got, (M, -M, a))
    # tripped: the safety half alone -- the box and psi residuals keep their values, and the arg-max is then the FIX-UP pass's (its own partials, folded by
    # its last arriver or by k_finalize)
    for thr, what in (((1e30, 1e30), "untripped"), ((1e30, r0["distS"] / 2), "tripped")):
        thr = set_thresholds(s, *thr)
        cache = {}
        for form_name in ("exact", "exact_sharded", "optimistic_close"):
            if flat == 0 and form_name == "exact_sharded":
                continue      # (that form always runs the flat kernel: the flat placements cover it)
            out, info = run(s, form_name, 0, materialize=1, flat=flat)
            r = check_closed("%s %s %s" % (tag, form_name, what), form_name, out, info, inp, dt, thr, 1, cache)
            am = r["main_argmax"] if form_name == "optimistic_close" else r["argmax"]
            assert form_name == "optimistic_close" or r["tripped"] == (what == "tripped"), (tag, form_name, what)
            assert am[half][2] == a and am[half][1] < 0, (tag, form_name, what, am)      # the planted pair is still the arg-max, the negative one first
            assert (info["idxXi"], info["valXi"]) == (am[0][2], am[0][1]) and (info["idxPsi"], info["valPsi"]) == (am[1][2], am[1][1]), (tag, form_name, what)
    return r0


# (the flat main pass strides a second time only in fp64: it has ceil(n / 1024) workgroups of 256 threads, and an fp32 thread takes four elements)
@pytest.mark.parametrize("where, form", [(w, f) for w in sorted(PLACEMENTS) for f in FORMS if (w, f) != ("flat, one grid stride apart", "f32")])
def test_ties_keep_the_lowest_index(where, form):
    name, knobs, flat, half, pred = PLACEMENTS[where]
    c = _Ctx(name, form, knobs=knobs, lam=0.125, zero_bounds=True)
    s, dt = c.s, c.dt
    try:
        case, lo, hi, info0 = integer_setup(c)
        _, info = s.debugDualUpdate("info", flat=flat)
        for kname, kv in (knobs or {}).items():
            assert info[{"dual_trips": "trips", "dual_pipe": "pipe"}[kname]] == kv, (where, "the knob did not take", info)
        assert info["kernel"] == ("k_dual_fused" if flat else "k_dual_stage"), (where, info["kernel"])
        co = ref.coordinates(info, s.nodes, s.ny, dt)
        box, safe, psi = ref.column_groups(s.nodes, s.nx, s.ny)
        pair = ref.pick_pair(co, (box if half == "box" else psi).ravel(), pred)
        assert pair is not None, (where, form, "this launch has no such pair of elements", ref.stage_cells(info, s.N, dt) if not flat else info["grid"])
        a, b = pair
        tied = ref.plant_tie(case, a, b, s.nx)
        _check_tie("tie %s %s" % (where, form), s, tied, lo, hi, info0, a, b, dt, flat)
        record("tie %s %s" % (where, form), "elements %d (-) and %d (+): %s" % (a, b, {k: (int(co[k][a]), int(co[k][b])) for k in ("block", "wave", "tid", "trip", "crown", "stage_block", "tail")}))
    finally:
        c.close()


@pytest.mark.parametrize("form", FORMS)
def test_ties_across_the_halves_zero_residual_and_the_sentinel(form):
    c = _Ctx("du_k43", form, knobs={"dual_trips": 1}, lam=0.125, zero_bounds=True)
    s, dt = c.s, c.dt
    try:
        case, lo, hi, info0 = integer_setup(c)
        box, safe, psi = ref.column_groups(s.nodes, s.nx, s.ny)
        # the same magnitude in both halves: xi holds -M first, psi holds +M first and -M later: the entry is max(-M, +M) = +M only by the rule
        bi, pi = np.flatnonzero(box.ravel()), np.flatnonzero(psi.ravel())
        M = float(np.abs(case["hx"]).max() + 1)
        both = ref.plant_tie(ref.plant_tie(case, int(bi[5]), int(bi[-7]), s.nx, M), int(pi[3]), int(pi[-4]), s.nx, M)
        both["hx"].ravel()[pi[3]], both["hx"].ravel()[pi[-4]] = M, -M
        both["tint"].ravel()[pi[3]], both["tint"].ravel()[pi[-4]] = int(M), -int(M)
        load(s, both)
        inp = inputs(both, lo, hi, info0)
        r0 = ref.restate(inp, dt, math.inf, math.inf)
        assert r0["main_argmax"][0] == (M, -M, int(bi[5])) and r0["main_argmax"][1] == (M, M, int(pi[3])) and r0["main_hist"] == M
        thr = set_thresholds(s, 1e30, 1e30)
        for form_name, flat in (("exact", 0), ("exact", 1), ("exact_sharded", 1), ("optimistic_close", 0)):
            out, info = run(s, form_name, 0, materialize=1, flat=flat)
            check_closed("both halves %s %s flat %d" % (form, form_name, flat), form_name, out, info, inp, dt, thr, 1, {})
            assert info["hist"] == M and info["idxXi"] == bi[5] and info["idxPsi"] == pi[3]
            if form_name == "exact" and flat == 0:
                # the last tile of a stage holds two vectors, both psi: that workgroup met no xi element and says so with the sentinel
                cells = ref.stage_cells(info, s.N, dt)
                if form == "f64":
                    assert cells["last_tile_vectors"] == 2 and cells["tiles"] == 2, cells
                    assert (out["partials"][:, 6] == -1).sum() == cells["stages"] and (out["partials"][out["partials"][:, 6] == -1, 2] == -1).all(), out["partials"][:, 6]
                assert not (out["partials"][:, 7] == -1).any()
        # an all-zero residual: indices 0 and 2 nx, entries +0
        zero = {k: (np.zeros_like(v) if isinstance(v, np.ndarray) else v) for k, v in case.items()}
        load(s, zero)
        for form_name, flat in (("exact", 0), ("exact", 1), ("exact_sharded", 1), ("optimistic_close", 0)):
            out, info = run(s, form_name, 0, materialize=1, flat=flat)
            assert (info["idxXi"], info["idxPsi"]) == (0, 2 * s.nx) and info["absXi"] == 0 and info["absPsi"] == 0 and info["hist"] == 0, (form_name, flat, info)
            assert not out["res"].any() and not out["ynew"].any()
        record("tie across the halves / zero residual / sentinel %s" % form, "K 43 trips 1: workgroups without an xi element %d" % int((out["partials"][:, 6] == -1).sum()))
    finally:
        c.close()


# ---- (d) the cells of k_dual_stage ---------------------------------------------------------------------------------------------------------------------------
def _integer_forms(tag, c, want_kernel, flat=0, reserve=48, forms=("main", "exact"), half_scale=True):
    """integer data through the main pass and the exact form (thr = D: untripped; thr = D / 2: every fix-up workgroup redoes its share), int64 reference"""
    s = c.s
    case, lo, hi, info0 = integer_setup(c, reserve=reserve)
    load(s, case)
    DX, DS = float(case["DX"]), float(case["DS"])
    info = None
    for thr, sc in (((DX, DS), 0.0),) + ((((DX / 2, DS / 2), 0.5),) if half_scale else ()):
        set_thresholds(s, *thr)
        want = integer_ref(case, s.nx, sc, sc)
        for form_name in forms:
            if form_name == "main" and sc:
                continue
            out, info = run(s, form_name, 0, materialize=1, flat=flat)
            assert info["kernel"] == want_kernel, (tag, info["kernel"])
            assert info["d2x"] == DX * DX and info["d2s"] == DS * DS, (tag, form_name, info["d2x"], DX * DX, info["d2s"], DS * DS)
            assert out["partials"][:, 0].sum() == DX * DX and out["partials"][:, 1].sum() == DS * DS, tag
            w = integer_ref(case, s.nx) if form_name == "main" else want
            for got, ww, nm in zip((out["ynew"], out["wnext"], out["z"], out["res"]), w, ("y+", "w_next", "z", "res")):
                assert np.array_equal(got, ww), (tag, form_name, thr, nm)
            if form_name != "main":
                assert info["tripped"] == (1 if sc else 0) and info["scaleX"] == sc and info["scaleS"] == sc, (tag, info)
                am = ref.argmax_ref(w[3], s.nx)
                assert (info["idxXi"], info["valXi"], info["idxPsi"], info["valPsi"], info["hist"]) == (am[0][2], am[0][1], am[1][2], am[1][1], am[2]), (tag, info, am)
    return info


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pipe", [1, 2])
@pytest.mark.parametrize("trips", [1, 2, 3, 4, 5, 6, 8])
def test_stage_tiles_by_trips_and_pipe(trips, pipe, form):
    """K = 128 on ny 12: 768 fp64 vectors per stage (384 in fp32): exactly three tiles of one trip, exactly one of three, wholly idle trips from four on"""
    c = _Ctx("du_k128", form, knobs={"dual_trips": trips, "dual_pipe": pipe}, lam=0.125, zero_bounds=True)
    try:
        info = _integer_forms("trips %d pipe %d %s" % (trips, pipe, form), c, "k_dual_stage")
        assert info["trips"] == trips and info["pipe"] == pipe, ("the knobs did not take", info)
        cells = ref.stage_cells(info, c.s.N, c.dt)
        per_stage = 768 if form == "f64" else 384
        assert cells["stage_vectors"] == per_stage and cells["tiles"] == -(-per_stage // (256 * trips)) and cells["crown_blocks"] == 1 and cells["stages"] == 2, cells
        assert cells["idle_trips"] == trips - -(-(per_stage - (cells["tiles"] - 1) * 256 * trips) // 256), cells
        if form == "f64":
            assert cells["idle_trips"] == {1: 0, 2: 1, 3: 0, 4: 1, 5: 2, 6: 3, 8: 5}[trips] and cells["partial_tile"] == (trips not in (1, 3)), cells
        assert cells["odd_trips_pipe2"] == (pipe == 2 and trips % 2 == 1) and cells["crown_idle_trips"] == trips - 1
        record("stage trips %d pipe %d %s" % (trips, pipe, form), cells)
    finally:
        c.close()


@pytest.mark.parametrize("name, form, knobs, expect", [
    ("du_k43", "f64", {"dual_trips": 1}, dict(last_tile_vectors=2, tiles=2, vpn=6, crown_blocks=1)),
    ("du_k43x3", "f64", {"dual_trips": 1}, dict(crown_blocks=2, crown_vectors=264, vpn=6)),              # a crown of two workgroups
    ("du_k43x3", "f64", {"dual_trips": 2}, dict(crown_blocks=1, crown_vectors=264, vpn=6)),              # one crown workgroup, nodes of two stages
    ("toy", "f64", None, dict(crown_blocks=0, crown_vectors=0, vpn=6)),                                   # no crown at all
    ("tiny", "f32", None, dict(vpn=3)), ("fan", "f32", None, dict(vpn=4)), ("fan", "f64", None, dict(vpn=8)),
    ("medium", "f32", None, dict(vpn=20)), ("medium", "f64", {"dual_trips": 2, "dual_pipe": 2}, dict(vpn=40, trips=2, pipe=2)),
])
def test_stage_cells_by_shape(name, form, knobs, expect):
    c = _Ctx(name, form, knobs=knobs, lam=0.125, zero_bounds=True)
    try:
        info = _integer_forms("%s %s %s" % (name, form, knobs), c, "k_dual_stage")
        cells = ref.stage_cells(info, c.s.N, c.dt)
        assert {k: cells[k] for k in expect} == expect, (cells, expect)
        if expect.get("crown_blocks") == 1 and name == "du_k43x3":
            stage_of = np.asarray(problem(name)["tree"]["stages"])[:int(info["node0"])]
            assert len(set(stage_of)) == 2      # that one crown workgroup looks up two stages
        record("stage cells %s %s %s" % (name, form, knobs), cells)
    finally:
        c.close()


def test_more_than_1024_partials_are_folded():
    """trips 1 on 530 412 fp64 elements: 1 037 main partials, so fold_partials takes a second round of its four-at-a-time loop -- in k_reduce_dist (the
    record's sums), and under the exact form in every fix-up workgroup and in the workgroup that folds the arg-max"""
    c = _Ctx("du_big", "f64", knobs={"dual_trips": 1}, lam=0.125, zero_bounds=True)
    try:
        info = _integer_forms("1037 partials", c, "k_dual_stage", reserve=400)
        assert info["grid"] > 1024 and info["trips"] == 1, info
        record("more than 1024 partials f64", "grid %d, eltBlocks %d, fix-up workgroups %d" % (info["grid"], info["eltBlocks"], info["fixBlocks"]))
    finally:
        c.close()


# ---- (e) the cells of the flat kernel ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, form, tail, blocks", [("odd", "f64", 1, 1), ("odd", "f32", 3, 1), ("small", "f32", 2, 2), ("du_tail1", "f32", 1, 1), ("du_tail1", "f64", 1, 1),
                                                      ("small", "f64", 0, 2)])
def test_flat_kernel_tails_and_workgroups(name, form, tail, blocks):
    """(synth admits ny = 2 mod 4 -- small2 has ny 20, a multiple of four -- but a tail of two only needs an element count of 2 mod 4: small, 70 nodes of ny 19)"""
    c = _Ctx(name, form, lam=0.125, zero_bounds=True)
    try:
        info = _integer_forms("flat %s %s" % (name, form), c, "k_dual_fused", forms=("main", "exact", "exact_sharded"))
        co = ref.coordinates(info, c.s.nodes, c.s.ny, c.dt)
        assert int(co["tail"].sum()) == tail and info["grid"] == blocks and c.s.ny % 2 == 1, (int(co["tail"].sum()), info["grid"])
        record("flat %s %s" % (name, form), "tail %d, workgroups %d, ny %d (vectors straddle two nodes)" % (tail, blocks, c.s.ny))
    finally:
        c.close()


def test_flat_fixup_strides_with_fewer_workgroups():
    c = _Ctx("du_flatbig", "f64", lam=0.125, zero_bounds=True)
    try:
        info = _integer_forms("flat big", c, "k_dual_fused", reserve=200, forms=("main", "exact", "exact_sharded"))
        assert c.s.nodes * c.s.ny > 65536 and info["fixBlocks"] == 64 and info["eltBlocks"] > 64, info
        record("flat fix-up f64", "elements %d, main workgroups %d, fix-up workgroups %d" % (c.s.nodes * c.s.ny, info["eltBlocks"], info["fixBlocks"]))
    finally:
        c.close()


# ---- (g) the step-wise entry points ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_step_wise_entry_points_give_the_exact_forms_numbers(name, form):
    """rn_proximal_fun_g, rn_compute_fixed_point_residual, rn_dual_update, rn_update_primal_infeasibility, rn_get_prox_distances,
    rn_dual_extrapolation_step on the inputs of an exact hook call: z, res, y+, the history value and w as numbers.  The distances: the step-wise
    prox sums the same squares in another order, so they are held to the n 2^-53 bound of check_d2, and to equality on integer data
    (test_step_wise_distances_on_integer_data)."""
    c = _Ctx(name, form)
    s, dt = c.s, c.dt
    try:
        t = 3
        lo, hi, k, info0 = tables(s, form, iteration=t)
        case = ref.normal_case(lo, hi, info0["lambda"], s.nx, 31, dt)
        inp = inputs(case, lo, hi, info0)
        r0 = ref.restate(inp, dt, math.inf, math.inf)
        differ = {}
        for what, thr in (("untripped", (4 * r0["distX"], 4 * r0["distS"])), ("tripped", (r0["distX"] / 3, r0["distS"] / 3))):
            thr = set_thresholds(s, *thr)
            load(s, case)
            out, info = run(s, "exact", t, materialize=1)
            r = check_closed("step-wise %s" % what, "exact", out, info, inp, dt, thr, 1, {})
            s.proximalFunG()
            s.computeFixedPointResidual()
            s.dualUpdate()
            hist = s.updatePrimalInfeasibity()
            dX, dS = s.proxDistances()
            got = {nm: np.concatenate([s.get(xi).reshape(s.nodes, 2 * s.nx), s.get(psi).reshape(s.nodes, s.nu)], axis=1)
                   for nm, xi, psi in (("z", capi.BUF_DUAL_XI, capi.BUF_DUAL_PSI), ("res", capi.BUF_RES_XI, capi.BUF_RES_PSI), ("ynew", capi.BUF_UPD_XI, capi.BUF_UPD_PSI))}
            assert info["tripped"] == (what == "tripped")
            for key, n in (("distX", r0["nX"]), ("distS", r0["nS"])):
                g = dX if key == "distX" else dS
                assert abs(g * g - info[key] ** 2) <= 4 * n * 2.0 ** -53 * info[key] ** 2, (what, key, g, info[key])
            # the step-wise prox decides from ITS sums: where they differ from the fused kernels' in the last bits, so may its scales -- the outputs
            # are therefore compared under the step-wise prox's own decision, restated
            rs = ref.restate(inp, dt, thr[0], thr[1], d2=(dX * dX, dS * dS))
            same_decision = (dX, dS) == (info["distX"], info["distS"])
            want = r["out"] if same_decision else rs["out"]
            for nm, idx in (("z", 2), ("res", 3), ("ynew", 0)):
                n_diff = int((got[nm] != np.asarray(want[idx]).astype(np.float64)).sum())
                differ[(what, nm)] = n_diff
            assert hist == (r["hist"] if same_decision else rs["hist"]), (what, hist, r["hist"])
            # w of the next iteration from (y+, y) by the extrapolation step: y must be the y the fused update read
            s.set(capi.BUF_XI, np.ascontiguousarray(case["yp"][:, :2 * s.nx].astype(np.float64)).ravel())
            s.set(capi.BUF_PSI, np.ascontiguousarray(case["yp"][:, 2 * s.nx:].astype(np.float64)).ravel())
            s.dualExtrapolationStep(info["ln"])
            w = np.concatenate([s.get(capi.BUF_ACC_XI).reshape(s.nodes, 2 * s.nx), s.get(capi.BUF_ACC_PSI).reshape(s.nodes, s.nu)], axis=1)
            differ[(what, "w_next")] = int((w != np.asarray(want[1]).astype(np.float64)).sum())
            record("step-wise %s %s %s" % (name, form, what), "elements that differ from the exact form: %s; same distances bit for bit: %s" % ({k[1]: v for k, v in differ.items() if k[0] == what}, same_decision))
        assert not any(differ.values()), differ
    finally:
        c.close()


@pytest.mark.parametrize("form", FORMS)
def test_step_wise_distances_on_integer_data(form):
    c = _Ctx("small", form, lam=0.125, zero_bounds=True)
    s = c.s
    try:
        case, lo, hi, info0 = integer_setup(c)
        load(s, case)
        set_thresholds(s, case["DX"] / 2, case["DS"] / 2)
        out, info = run(s, "exact", 0, materialize=1)
        s.proximalFunG()
        s.computeFixedPointResidual()
        s.dualUpdate()
        assert s.proxDistances() == (info["distX"], info["distS"]) == (float(case["DX"]), float(case["DS"]))
        assert s.updatePrimalInfeasibity() == info["hist"]
        for nm, xi, psi in (("z", capi.BUF_DUAL_XI, capi.BUF_DUAL_PSI), ("res", capi.BUF_RES_XI, capi.BUF_RES_PSI), ("ynew", capi.BUF_UPD_XI, capi.BUF_UPD_PSI)):
            got = np.concatenate([s.get(xi).reshape(s.nodes, 2 * s.nx), s.get(psi).reshape(s.nodes, s.nu)], axis=1)
            assert np.array_equal(got, out[nm]), nm
    finally:
        c.close()


# ---- (f) shards --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world, cut", [(2, 1), (3, 1)])
def test_shards_count_the_crown_once(world, cut):
    from test_gpu_sharded_batched import Ranks

    p = dict(problem("medium"))
    p["config"] = dict(p["config"], stepSize=[0.125])
    one = capi.Solver(p["network"], p["tree"], p["config"])
    rk = Ranks(p, world, cut)
    try:
        one.factorStep()
        one.apgReset()
        zb = lambda s: s.setBounds("shared", np.zeros(s.nx), np.zeros(s.nx), np.zeros(s.nx), np.zeros(s.nu), np.zeros(s.nu))
        zb(one)
        case = ref.integer_case(one.nodes, one.nx, one.ny, 5, lam_log2=-3)
        load(one, case)
        set_thresholds(one, 1e30, 1e30)
        _, full = run(one, "main", 0, flat=1)
        assert full["d2x"] == case["DX"] ** 2 and full["d2s"] == case["DS"] ** 2 and full["countCrown"] == 1 and full["crownElems"] == 0

        def on_rank(s):
            s.factorStep()
            s.apgReset()
            zb(s)
            local = {k: (v[s.global_nodes] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
            load(s, local)
            out, info = run(s, "main", 0, flat=1)
            want = ref.integer_main_ref(local, s.nx)
            assert np.array_equal(out["ynew"], want[0])
            return info

        infos = rk.run(on_rank)
        assert [i["countCrown"] for i in infos] == [1] + [0] * (world - 1), [i["countCrown"] for i in infos]
        assert all(i["crownElems"] > 0 and i["crownElems"] == infos[0]["crownElems"] for i in infos)
        assert sum(i["d2x"] for i in infos) == full["d2x"] and sum(i["d2s"] for i in infos) == full["d2s"], ([(i["d2x"], i["d2s"]) for i in infos], full["d2x"], full["d2s"])
        record("shards %d ranks" % world, "crown elements %d; d2x %s = %d, d2s %s = %d" % (infos[0]["crownElems"], [int(i["d2x"]) for i in infos], full["d2x"], [int(i["d2s"]) for i in infos], full["d2s"]))
    finally:
        rk.close()
        one.close()


# ---- (h) refusals; the hook disturbs nothing -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    p = problem("tiny")
    s = capi.Solver(p["network"], p["tree"], p["config"])
    try:
        info = np.zeros(40)
        import ctypes as C

        class A(C.Structure):
            _fields_ = [(n, C.c_int) for n in ("form", "materialize", "flat", "unscaled", "iteration")] + [(n, C.c_void_p) for n in "abcdefghijkl"] + [("n", C.c_size_t)]
        a = A(4, 0, 0, 0, 0)
        assert s.lib.rn_debug_dual_update(s.h, C.addressof(a), info.ctypes.data) == -3          # RN_E_STATE before the factor step
        s.factorStep()
        s.apgReset()
        assert s.lib.rn_debug_dual_update(s.h, None, info.ctypes.data) == -1 and s.lib.rn_debug_dual_update(s.h, C.addressof(a), None) == -1
        for bad in (A(9, 0, 0, 0, 0), A(0, 0, 0, 0, -1), A(0, 1, 0, 1, 0), A(1, 0, 0, 1, 0), A(2, 0, 0, 1, 0), A(0, 0, 0, 0, 0)):      # unknown form; iteration; SCALE with
            assert s.lib.rn_debug_dual_update(s.h, C.addressof(bad), info.ctypes.data) == -1, (bad.form, bad.materialize, bad.unscaled)   # MATERIALIZE; unscaled exact; no outputs
        with pytest.raises(capi.RapidNetError):
            s.debugDualUpdate("main", materialize=1, unscaled=1)
        s.debugDualUpdate("main", materialize=1, unscaled=1, flat=1)      # the flat kernel behind k_hx_scale: a launch the library has
        s._check(s.lib.rn_set_algorithm(s.h, 2, 5))
        assert s.lib.rn_debug_dual_update(s.h, C.addressof(a), info.ctypes.data) == -3          # under NAMA
    finally:
        s.close()


@pytest.mark.parametrize("form", FORMS)
def test_hook_calls_between_batches_disturb_nothing(form):
    p = problem("medium")
    dh, ah = synth.forecast_at(p["forecast"], 0)
    ctxs = []
    try:
        for _ in range(2):
            s = capi.Solver(p["network"], p["tree"], p["config"], precision=form)
            s.initialiseSmpcController(dh, ah)
            s.apgReset()
            ctxs.append(s)
        a, b = ctxs
        hists = [[], []]
        for n in (3, 20, 5):
            hists[0].append(a.apgIterate(n))
            hists[1].append(b.apgIterate(n))
            for form_name, kw in (("main", dict(materialize=1)), ("main", dict(unscaled=1)), ("exact", dict(materialize=1)), ("exact_sharded", {}), ("optimistic_close", {}),
                                  ("main", dict(flat=1, unscaled=1, materialize=1))):
                a.debugDualUpdate(form_name, iteration=7, **kw)
            a.debugDualUpdate("next_w")
        assert np.array_equal(np.concatenate(hists[0]), np.concatenate(hists[1]))
        for bid in range(capi.BUF_X, capi.BUF_UMAX + 1):
            assert np.array_equal(a.get(bid), b.get(bid)), bid
        wa, wb = a.debugDualUpdate("next_w")[0]["wnext"], b.debugDualUpdate("next_w")[0]["wnext"]
        assert np.array_equal(wa, wb)
    finally:
        for s in ctxs:
            s.close()


# ---- the fused walk + dual update (k_down_chain_dual), pinned by its closing identity -----------------------------------------------------------------------
# k_down_chain_dual takes Hx from LDS and cannot be handed one; but the LAST iteration of a batch materialises it.  Behind rn_apg_iterate(n) the context
# shows that iteration's inputs -- Hx (BUF_PRIMAL_*), w (BUF_ACC_*), y (BUF_XI / BUF_PSI: the buffers have rotated) -- and its outputs: y+ (BUF_UPD_*), z
# (BUF_DUAL_*), res (BUF_RES_*), the next w (the hook's NEXT_W) and the last history entry.  The outputs must be the restatement of the inputs, whichever
# kernel computed them.  (Default penalties: the distances stay far below the thresholds, which is asserted, so the outputs are the main pass's.)
def _rows(s, xi, psi):
    return np.concatenate([s.get(xi).reshape(s.nodes, 2 * s.nx), s.get(psi).reshape(s.nodes, s.nu)], axis=1)


def closing_identity(tag, s, form, t, last_hist=None):
    dt = ref.DTYPES[form]
    lo, hi, k, info = tables(s, form, iteration=t)
    case = dict(hx=_rows(s, capi.BUF_PRIMAL_XI, capi.BUF_PRIMAL_PSI).astype(dt), w=_rows(s, capi.BUF_ACC_XI, capi.BUF_ACC_PSI).astype(dt),
                yp=_rows(s, capi.BUF_XI, capi.BUF_PSI).astype(dt), nx=s.nx)
    r = ref.restate(inputs(case, lo, hi, info), dt, info["thrX"], info["thrS"])
    assert r["tripped"] == 0 and r["distX"] < 0.5 * info["thrX"] and r["distS"] < 0.5 * info["thrS"], (tag, r["distX"], info["thrX"], r["distS"], info["thrS"])
    yn, wn, z, res = r["out"]
    got = dict(ynew=_rows(s, capi.BUF_UPD_XI, capi.BUF_UPD_PSI), z=_rows(s, capi.BUF_DUAL_XI, capi.BUF_DUAL_PSI), res=_rows(s, capi.BUF_RES_XI, capi.BUF_RES_PSI),
               wnext=s.debugDualUpdate("next_w")[0]["wnext"])
    for nm, want in (("ynew", yn), ("wnext", wn), ("z", z), ("res", res)):
        bad = np.flatnonzero(got[nm].ravel() != np.asarray(want).astype(np.float64).ravel())
        assert bad.size == 0, (tag, nm, "elements that differ", bad.size, "first", int(bad[0]), got[nm].ravel()[bad[0]], float(np.asarray(want).ravel()[bad[0]]))
    if last_hist is not None:
        assert last_hist == r["hist"], (tag, "history entry", last_hist, r["hist"], r["argmax"])
    return r


@pytest.mark.parametrize("name, structured, form, knobs", [
    ("medium", False, "f64", None), ("medium", True, "f64", None), ("ragged", False, "f64", None), ("ragged", True, "f64", None), ("barcelona31", False, "f64", None),
    ("barcelona31", True, "f64", None), ("medium", False, "f32", None), ("medium", False, "f64", {"fuse_split": 1}), ("medium", False, "f64", {"fuse_split": 2}),
    ("medium", False, "f64", {"fuse_split": 3}), ("medium", False, "f64", {"fuse_split": 1000})])
def test_closing_identity_of_the_fused_walk_and_dual_update(name, structured, form, knobs):
    p = problem(name)
    s = capi.Solver(p["network"], p["tree"], p["config"], structured=structured, precision=form, knobs=knobs)
    try:
        s.initialiseSmpcController(*synth.forecast_at(p["forecast"], 0))
        for fused, n in ((1, 20), (0, 17), (1, 5)):      # an optimistic batch with the fusion, one without it, an exact batch
            s.setFusedWalkDual(fused)
            s.apgReset()
            hist = s.apgIterate(n)
            closing_identity("%s %s %s %s fused %d n %d" % (name, "structured" if structured else "dense", form, knobs, fused, n), s, form, n - 1, float(hist[-1]))
        record("closing identity %s %s %s %s" % (name, "structured" if structured else "dense", form, knobs), "fused n 20, unfused n 17, exact n 5: y+, w next, z, res, history entry equal")
    finally:
        s.close()


@pytest.mark.parametrize("world", [2, 3])
def test_closing_identity_on_shards(world):
    """crown nodes are written by workgroups of their own there; every rank's rows are the restatement of that rank's inputs (the history entry of a
    sharded batch is made tree-global by a MAX all-reduce with a tie rule of its own, k_batch_close_pack: not part of this identity)"""
    from test_gpu_sharded_batched import Ranks

    p = problem("medium")
    dh, ah = synth.forecast_at(p["forecast"], 0)
    rk = Ranks(p, world, 0)
    try:
        def solve(s):
            s.initialiseSmpcController(dh, ah)
            s.setFusedWalkDual(1)
            s.apgReset()
            s.apgIterate(20)
            return s.counters()

        rk.run(solve)
        for i, s in enumerate(rk.shards):      # (reads only: no collective)
            closing_identity("medium %d ranks, rank %d" % (world, i), s, "f64", 19)
    finally:
        rk.close()


def guard_body():
    """a few hook cases for tests/test_gpu_guard.py: the scratch outputs, partials and state between red zones; returns the contexts it made"""
    test_every_form_restates_on_normal_data("tiny", "f64")
    test_every_form_restates_on_normal_data("odd", "f32")
    test_stage_tiles_by_trips_and_pipe(3, 2, "f64")
    test_stage_cells_by_shape("du_k43", "f64", {"dual_trips": 1}, dict(last_tile_vectors=2, tiles=2, vpn=6, crown_blocks=1))
    test_flat_kernel_tails_and_workgroups("du_tail1", "f32", 1, 1)
    return 5
