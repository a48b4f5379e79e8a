"""The numpy side of tests/test_gpu_dual_update.py (dual_update_ref.py) is checked here, without a GPU: a restatement that is wrong, or a builder that
stopped producing the case it is named for, would otherwise make a GPU assertion pass for nothing.  The exactly rounded FMAs against rationals (normal
triples and triples built to sit on rounding ties), the restatement against the CPU oracle's step-wise prox / residual / dual update / primal
infeasibility / distances, the builders on hand-made inputs, and the deliberate mistakes -- each must change its named case."""
import math
from fractions import Fraction

import numpy as np
import pytest

import dual_update_ref as ref
from oracle.oracle import Oracle
from rapidnet_amd import synth


# ---- the FMAs ----------------------------------------------------------------------------------------------------------------------------------------------
def _nearest(q, dt):
    """the two neighbours of the rational q in dt and which one is nearest (ties: even significand), by search -- not by round_fraction's arithmetic"""
    x = dt(float(q))                      # some value of the type near q (possibly doubly rounded)
    cands = sorted({float(x), float(np.nextafter(x, dt(np.inf))), float(np.nextafter(x, dt(-np.inf)))})
    best = min(cands, key=lambda v: abs(Fraction(v) - q))
    tied = [v for v in cands if abs(Fraction(v) - q) == abs(Fraction(best) - q)]
    if len(tied) == 2:                    # the even one: its successor in the type is an odd multiple of the spacing
        sp = Fraction(tied[1]) - Fraction(tied[0])
        best = [v for v in tied if (Fraction(v) / sp).numerator % 2 == 0][0]
    return best


@pytest.mark.parametrize("form", ["f64", "f32"])
def test_fma_is_exactly_rounded_on_normal_triples(form):
    dt = ref.DTYPES[form]
    rng = np.random.default_rng(5)
    a, b, c = (rng.standard_normal(3000).astype(dt) for _ in range(3))
    got = ref.fma_array(a, b, c, dt)
    two = ref.fma_two_roundings(a, b, c, dt)
    for i in range(0, 3000, 7):
        q = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert float(got[i]) == _nearest(q, dt), (i, a[i], b[i], c[i])
    differ = int((got != two).sum())
    print("%s: a*b+c in two roundings differs from the fused result in %d of 3000 triples" % (form, differ))
    assert 300 < differ < 1500      # about a quarter: a test that holds the bits sees an unfused build


def test_fma32_rounds_once_on_ties_that_fool_a_double():
    one_ulp = np.float32(1 + 2.0 ** -23)
    # exact ties go to the even neighbour, in fp32 and in fp64
    assert ref.fma32(1, 2.0 ** -24, 1) == np.float32(1.0)                           # 1 + 2^-24: between 1 (even) and 1 + 2^-23
    assert ref.fma32(3, 2.0 ** -24, 1) == np.float32(1 + 2.0 ** -22)                # 1 + 3 * 2^-24: between 1 + 2^-23 (odd) and 1 + 2^-22
    assert ref.fma64(1.0, 2.0 ** -53, 1.0) == 1.0 and ref.fma64(3.0, 2.0 ** -53, 1.0) == 1 + 2.0 ** -51
    a = np.float32(1 + 2.0 ** -12)                                                  # a a = 1 + 2^-11 + 2^-24
    assert Fraction(float(a)) ** 2 + Fraction(-(2.0 ** -11)) == 1 + Fraction(1, 2 ** 24) and ref.fma32(a, a, -(2.0 ** -11)) == np.float32(1.0)
    # just above the tie by less than a double can hold: q = 1 + 2^-24 + 2^-54.  float(q) is 1 + 2^-24, the tie, and np.float32 of THAT goes to even: 1.0.
    # Rounded once, q goes up.
    q = 1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 54)
    assert np.float32(float(q)) == np.float32(1.0) and ref.round_fraction(q, 24, -126, 127) == float(one_ulp)
    # a result strictly inside an interval: the scalar form, the array form (its double fast path) and the search over the neighbours agree
    b = np.float32(1 + 2.0 ** -12 + 2.0 ** -23)
    c = np.float32(-(2.0 ** -11))
    q3 = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    assert float(ref.fma32(a, b, c)) == _nearest(q3, np.float32) == float(ref.fma_array([a], [b], [c], np.float32)[0])
    # a product too small for the double sum to hold (2^-60 beside 1 + 2^-23): the array form's fast path must notice and go through the rational
    tiny = np.float32(2.0 ** -30)
    assert ref.fma32(tiny, tiny, one_ulp) == one_ulp and ref.fma_array([tiny], [tiny], [one_ulp], np.float32)[0] == one_ulp
    # the product is the half ulp itself: 2^-12 * 2^-12 = 2^-24 onto 1 (tie: down to even) and onto 1 + 2^-23 (tie: up to even)
    h = np.float32(2.0 ** -12)
    assert ref.fma_array([h, h], [h, h], [np.float32(1), one_ulp], np.float32).tolist() == [1.0, float(np.float32(1 + 2.0 ** -22))]


def test_round_fraction_subnormals_and_overflow():
    assert ref.round_fraction(Fraction(1, 2 ** 150), 24, -126, 127) == 0.0                       # half the smallest subnormal: tie to even (0)
    assert ref.round_fraction(Fraction(3, 2 ** 150), 24, -126, 127) == 2.0 ** -148                 # 1.5 subnormals: tie to even (2)
    assert ref.round_fraction(Fraction(2) ** 128, 24, -126, 127) == math.inf
    assert ref.round_fraction(-Fraction(5, 2 ** 1075), 53, -1022, 1023) == -2 * 2.0 ** -1074       # 2.5 -> 2


# ---- against the CPU oracle ----------------------------------------------------------------------------------------------------------------------------------
def _interleave(o, xi, psi):
    return np.concatenate([o.get(xi).reshape(o.nodes, 2 * o.nx), o.get(psi).reshape(o.nodes, o.nu)], axis=1)


def _oracle_bounds(o):
    nx = o.nx
    lo = np.concatenate([o.get("xmin").reshape(-1, nx), o.get("xs").reshape(-1, nx), o.get("umin").reshape(o.nodes, o.nu)], axis=1)
    hi = np.concatenate([o.get("xmax").reshape(-1, nx), np.full((o.nodes, nx), np.inf), o.get("umax").reshape(o.nodes, o.nu)], axis=1)
    return lo, hi


# penalties 20 / 5: `small` trips its box half from iteration 8 on; `medium` stays under both thresholds through iteration 9 (its distances reach 6.5e5 and
# 8.3e4 against 8.5e5 and 2.1e5), so it runs once more with 5 / 1, where both halves trip from iteration 3 on
@pytest.mark.parametrize("name, penX, penS, trips", [("small", 20.0, 5.0, True), ("medium", 20.0, 5.0, False), ("medium", 5.0, 1.0, True)])
def test_restatement_against_the_oracle_step_by_step(name, penX, penS, trips):
    p = synth.make_problem(name)
    cfg = dict(p["config"], penaltyStateX=[penX], penaltySafetyX=[penS])
    dh, ah = synth.forecast_at(p["forecast"], 0)
    o = Oracle(p["network"], p["tree"], cfg)
    o.initialise(dh, ah)
    o.apg_reset()
    lo, hi = _oracle_bounds(o)
    step = float(np.ravel(cfg["stepSize"])[0])
    theta = [1.0, 1.0]
    seen_trip = 0
    for it in range(1, 10):
        lam_t = theta[1] * (1 / theta[0] - 1)
        o.extrapolate(lam_t)
        o.solve_step()
        theta = [theta[1], 0.5 * (math.sqrt(theta[1] ** 4 + 4 * theta[1] ** 2) - theta[1] ** 2)]
        ln = theta[1] * (1 / theta[0] - 1)
        inp = dict(hx=_interleave(o, "primalXi", "primalPsi"), w=_interleave(o, "accXi", "accPsi"), yp=_interleave(o, "updXi", "updPsi"), lo=lo, hi=hi,
                   lam=step, inv_lam=1.0 / step, ln=ln, nx=o.nx)
        o.prox()
        o.residual()
        o.dual_update()
        hist = o.primal_infeasibility()
        if it not in (1, 5, 9):
            continue
        r = ref.restate(inp, np.float64, penX / step, penS / step)
        seen_trip += r["tripped"]
        yn, wn, z, res = r["out"]
        for got, want, what in ((z, _interleave(o, "dualXi", "dualPsi"), "z"), (res, _interleave(o, "resXi", "resPsi"), "res"), (yn, _interleave(o, "updXi", "updPsi"), "y+")):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (it, what)
        dX, dS = o.dist()
        assert abs(r["distX"] - dX) <= 1e-12 * dX and abs(r["distS"] - dS) <= 1e-12 * max(dS, 1e-300), (it, r["distX"], dX, r["distS"], dS)
        assert abs(r["hist"] - hist) <= 1e-12 * np.abs(res).max(), (it, r["hist"], hist)
        # w of the next iteration: the oracle's extrapolation of (y+, y) with ln
        chk = Oracle(p["network"], p["tree"], cfg)
        for nm in ("xi", "psi", "updXi", "updPsi"):
            chk.set(nm, o.get(nm))
        chk.set("xi", inp["yp"][:, :2 * o.nx].ravel())
        chk.set("psi", inp["yp"][:, 2 * o.nx:].ravel())
        chk.extrapolate(ln)
        want = _interleave(chk, "accXi", "accPsi")
        assert np.abs(wn - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (it, "w next")
    assert (seen_trip >= 1) == trips, (name, penX, penS, seen_trip)


# ---- the builders ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f64", "f32"])
def test_integer_case_is_exact_and_its_sums_are_perfect_squares(form):
    dt = ref.DTYPES[form]
    nx, nu, nodes = 3, 6, 43
    c = ref.integer_case(nodes, nx, 2 * nx + nu, 3, dtype=dt)
    yn, wn, z, res, d2x, d2s = ref.integer_main_ref(c, nx)
    assert d2x == c["DX"] ** 2 and d2s == c["DS"] ** 2 and c["DX"] > 0 and c["DS"] > 0
    inp = dict(c, lo=np.zeros_like(c["hx"]), hi=np.where(ref.column_groups(nodes, nx, 2 * nx + nu)[1], 1e30, 0).astype(dt), inv_lam=1 / c["lam"], ln=0.0)
    r = ref.restate(inp, dt, c["DX"], c["DS"])
    assert r["tripped"] == 0 and r["d2x"] == d2x and r["d2s"] == d2s                     # thr = D exactly: the test is strict
    for got, want in zip(r["out"], (yn, wn, z, res)):
        assert np.array_equal(got.astype(np.float64), want)
    below = float(np.nextafter(np.float64(c["DX"]), 0.0))
    r2 = ref.restate(inp, dt, below, c["DS"])
    assert r2["tripped"] == 1 and r2["scaleX"] > 0 and r2["scaleS"] == 0.0
    r3 = ref.restate(inp, dt, c["DX"] / 2, c["DS"] / 2)
    assert r3["scaleX"] == 0.5 and r3["scaleS"] == 0.5
    box = ref.column_groups(nodes, nx, 2 * nx + nu)[0]
    assert np.array_equal(r3["out"][2][box].astype(np.float64), c["tint"][box] / 2.0)   # z = 0 + (t - 0) / 2


def test_coordinates_by_hand():
    # fp64, ny 12: vpn 6; K 2 nodes per stage, node0 3, trips 1: a regular stage has 12 vectors in one workgroup, the crown 18 vectors in one
    info = dict(kernel="k_dual_stage", vpn=6, trips=1, node0=3, K=2, crownBlocks=1, bps=1, grid=3, pipe=1)
    co = ref.coordinates(info, 7, 12, np.float64)
    assert co["block"][0] == 0 and co["crown"][35] == 1 and co["block"][36] == 1 and co["crown"][36] == 0          # element 36 = node 3, the first regular node
    assert co["tid"][36] == 0 and co["tid"][38] == 1 and co["block"][36 + 24] == 2 and co["stage_block"][36 + 24] == 1
    cells = ref.stage_cells(info, 4, np.float64)
    assert cells["last_tile_vectors"] == 12 and cells["partial_tile"] and cells["idle_trips"] == 0 and cells["stages"] == 2
    cells = ref.stage_cells(dict(info, trips=3), 4, np.float64)
    assert cells["idle_trips"] == 2 and cells["odd_trips_pipe2"] is False
    # the flat kernel, fp32, 27 elements: 6 vectors and a tail of 3
    co = ref.coordinates(dict(kernel="k_dual_fused", grid=1), 1, 27, np.float32)
    assert co["tail"].sum() == 3 and co["tid"][24] == 0 and co["tid"][26] == 2 and co["tid"][23] == 5 and co["trip"][23] == 0
    pair = ref.pick_pair(co, np.ones(27, bool), lambda c, a, js: (c["tail"][js] == 1) & (c["tail"][a] == 0))
    assert pair == (0, 24)


def test_bounds_from_tables_by_hand():
    sp, dy = np.array([1.0, 0.5]), np.array([[2.0, 2.0, 2.0, 4.0], [1.0, 1.0, 1.0, 1.0]])
    blo, bhi = np.array([[-1.0, -2.0, 0.0, -3.0]]), np.array([[1.0, 2.0, 9.0, 3.0]])
    lo, hi, k = ref.bounds_from_tables(sp, dy, blo, bhi, [0, 1], 0, 0, 1, np.float64)         # nx = 1: column 1 is the safety half
    assert np.array_equal(lo, [[-2.0, -4.0, 0.0, -12.0], [-0.5, -1.0, 0.0, -1.5]]) and np.array_equal(hi, [[2.0, 2.0, 18.0, 12.0], [0.5, 2.0, 4.5, 1.5]])
    blo2 = np.array([[-1.0, -2.0, 0.0, -3.0], [-10.0, -20.0, 0.0, -30.0]])
    lo2, _, _ = ref.bounds_from_tables(sp, dy, blo2, np.vstack([bhi, bhi]), [0, 1], 4, 0, 1, np.float64)      # a row per stage
    assert np.array_equal(lo2[1], [-5.0, -10.0, 0.0, -15.0])
    lo3, _, _ = ref.bounds_from_tables(sp, dy, blo2, np.vstack([bhi, bhi]), [0, 0], 0, 4, 1, np.float64)      # a row per node
    assert np.array_equal(lo3[1], [-10.0, -20.0, 0.0, -60.0])


# ---- the deliberate mistakes: each changes its hand-made case -----------------------------------------------------------------------------------------------------
def _hand_case(dt=np.float32):
    """one node, nx = 1, nu = 1 (columns: box, safety, psi), values whose every FMA lands between two neighbours"""
    third = dt(1) / dt(3)
    hx = np.array([[third, -third, dt(0.7)]], dtype=dt)
    w = np.array([[dt(0.1), dt(0.3), dt(-0.9)]], dtype=dt)
    yp = np.array([[dt(1) / dt(7), dt(1) / dt(9), dt(1) / dt(11)]], dtype=dt)
    lo = np.array([[-0.1, 0.2, -0.05]], dtype=dt)
    hi = np.array([[0.1, np.inf, 0.05]], dtype=dt)
    return dict(hx=hx, w=w, yp=yp, lo=lo, hi=hi, lam=dt(0.3), inv_lam=dt(1) / dt(0.3), ln=dt(0.28), nx=1)


@pytest.mark.parametrize("which, out", [("unfuse_t", 4), ("unfuse_yn", 0), ("unfuse_wn", 1)])
def test_mistake_one_fma_unfused(which, out):
    changed = 0
    for seed in range(40):      # (one triple in four shows an unfused FMA: forty hand-made variations, and the count is asserted)
        c = _hand_case()
        rng = np.random.default_rng(seed)
        c["hx"] = (c["hx"] * rng.uniform(0.5, 1.5, 3)).astype(np.float32)
        c["w"] = (c["w"] * rng.uniform(0.5, 1.5, 3)).astype(np.float32)
        good = ref.dual_elem_ref(c["hx"], c["w"], c["lo"], c["hi"], c["yp"], c["lam"], c["inv_lam"], c["ln"], None, np.float32)
        bad = ref.dual_elem_ref(c["hx"], c["w"], c["lo"], c["hi"], c["yp"], c["lam"], c["inv_lam"], c["ln"], None, np.float32, mistake=which)
        changed += int(not np.array_equal(good[out], bad[out]))
    assert changed >= 10, (which, changed)


def test_mistake_trip_test_not_strict():
    c = _hand_case(np.float64)
    r = ref.restate(c, np.float64, 1e9, 1e9)
    dX = r["distX"]
    assert dX > 0
    assert ref.restate(c, np.float64, dX, 1e9)["tripped"] == 0 and ref.restate(c, np.float64, dX, 1e9, mistake="ge")["tripped"] == 1


def test_mistakes_in_the_tie_rule():
    res = np.array([[0.0, 1.0, -3.0], [2.0, 0.5, 3.0]])      # nx = 1: xi columns 0, 1; psi column 2: -3 at element 2, +3 at element 5
    (_, _, _), (aP, vP, iP), hist = ref.argmax_ref(res, 1)
    assert (aP, vP, iP) == (3.0, -3.0, 2) and hist == 2.0     # the larger of the signed entries: xi's 2.0 against psi's -3.0
    assert ref.argmax_ref(res, 1, mistake="last")[1] == (3.0, 3.0, 5) and ref.argmax_ref(res, 1, mistake="last")[2] == 3.0
    assert ref.argmax_ref(res, 1, mistake="positive")[1] == (3.0, 3.0, 5) and ref.argmax_ref(res, 1, mistake="positive")[2] == 3.0
    zero = np.zeros((2, 3))
    assert ref.argmax_ref(zero, 1)[0][2] == 0 and ref.argmax_ref(zero, 1)[1][2] == 2          # an all-zero residual: indices 0 and 2 nx


def test_mistake_scale_on_psi():
    c = _hand_case(np.float64)
    r0 = ref.restate(c, np.float64, 1e9, 1e9)
    good = ref.restate(c, np.float64, r0["distX"] / 2, 1e9)
    bad = ref.restate(c, np.float64, r0["distX"] / 2, 1e9, mistake="scale_psi")
    assert good["tripped"] == 1 and np.array_equal(good["out"][2][:, :2], bad["out"][2][:, :2]) and not np.array_equal(good["out"][2][:, 2], bad["out"][2][:, 2])
    assert np.array_equal(good["out"][2][:, 2], r0["out"][2][:, 2])      # psi is a pure projection


def test_mistake_crown_counted_on_every_rank():
    c = _hand_case(np.float64)
    c = {k: (np.vstack([v, v]) if isinstance(v, np.ndarray) else v) for k, v in c.items()}      # two nodes; the first is a crown node
    r0 = ref.restate(c, np.float64, 1e9, 1e9)
    other_rank = ref.restate(c, np.float64, 1e9, 1e9, counted=[False, True])
    assert other_rank["d2x"] * 2 == r0["d2x"] and other_rank["nX"] == 1
    assert ref.restate(c, np.float64, 1e9, 1e9, counted=[False, True], mistake="crown_every_rank")["d2x"] == r0["d2x"]
