"""The numpy restatement of the solve certificate (tests/certificate_oracle.py) against the problem's definition, without a GPU.

(a) The restatement against a brute-force evaluation on `tiny`, `small`, `odd`, `ragged`: DUAL of the restatement at the CPU oracle's solve
    step at y+ equals first_principles.Model's Lagrangian value at ITS dense argmin at y+ minus SUPPORT, within 1e-12 ABS_TERMS (the oracle's
    solve step is the dense argmin to 1e-9 per stage, tests/test_first_principles.py, and the Lagrangian is stationary there).
(b) Weak duality on the oracle, `tiny` and `small` made feasible: DUAL after 1, 5, 20, 50 and 100 iterations is <= DUAL after 600 iterations +
    1e-9 ABS_TERMS (every dual value is a lower bound of the one optimal value, and 600 iterations are nearest to it); PRIMAL >= DUAL - 1e-9
    ABS_TERMS at every checked count at which u(y) is inside its box (U_EXCESS = 0), and at least one such count exists on `tiny`.
(c) A hand-made dual with one xi_s entry > 0, and one with |xi_s| > gamma_s, give VALID = 0 and finite columns.
(d) Five deliberate mistakes must each move the restatement on a hand-made case by more than 1e-6 ABS_TERMS: the xmax row dropped from the
    support term, the safety half given an upper bound, p_i instead of sqrt(p_i) in F, the root's du without prevU (all four: DUAL), and the
    distances taken per node instead of tree-global (PRIMAL: DUAL holds no distance, the mistake cannot show there)."""
import numpy as np
import pytest

import certificate_oracle as co
import first_principles as fp
from oracle.oracle import Oracle
from rapidnet_amd import synth

_PROBLEMS = {}


def problem(name, feasible=None):
    key = (name, feasible)
    if key not in _PROBLEMS:
        p = synth.make_problem(name, feasible=feasible)
        _PROBLEMS[key] = (p, synth.forecast_at(p["forecast"], 0))
    return _PROBLEMS[key]


def oracle(p, fc):
    o = Oracle(p["network"], p["tree"], p["config"])
    o.initialise(*fc)
    return o


def finite(r):
    return all(np.isfinite(r[k]) for k in co.COLUMNS)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "small", "odd", "ragged"])
def test_dual_is_the_lagrangian_at_the_dense_argmin_minus_the_support(name):
    p, fc = problem(name)
    o, m = oracle(p, fc), fp.Model(p["network"], p["tree"], p["config"], fc)
    ubox = co.physical_ubox(p["network"], m.nodes)
    o.apg_reset()
    theta, done = [1.0, 1.0], 0
    for iters in (0, 1, 9):
        if iters > done:
            theta = list(o.apg_continue(iters - done, theta))
            done = iters
        r = co.oracle_certificate(o, m, ubox)
        xi, psi = o.get("updXi"), o.get("updPsi")
        ref = m.argmin(xi, psi)
        assert ref["correction"] <= 1e-12
        want = co.lagrangian(m, ref["x"], ref["u"], xi, psi) - r["support"]
        print("%s after %d iterations: DUAL %.12g, brute force %.12g, difference / ABS_TERMS %.1e" % (name, iters, r["dual"], want, abs(r["dual"] - want) / r["absTerms"]))
        assert finite(r) and r["absTerms"] > 0
        assert abs(r["dual"] - want) <= 1e-12 * r["absTerms"]
        if iters == 0:      # y = 0: the unconstrained minimum, nothing but COST
            assert r["inner"] == 0.0 and r["support"] == 0.0 and r["valid"] == 1.0 and r["dual"] == r["cost"]


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,extra", [("tiny", (300, 500)), ("small", ())])
def test_weak_duality_on_the_oracle(name, extra):
    p, fc = problem(name, feasible=True)
    o, m = oracle(p, fc), fp.Model(p["network"], p["tree"], p["config"], fc)
    ubox = co.physical_ubox(p["network"], m.nodes)
    counts = sorted(set((1, 5, 20, 50, 100, 600) + tuple(extra)))
    o.apg_reset()
    theta, done, rec = [1.0, 1.0], 0, {}
    for c in counts:
        theta = list(o.apg_continue(c - done, theta))
        done = c
        rec[c] = co.oracle_certificate(o, m, ubox)
        print("%s after %4d iterations: DUAL %.9g PRIMAL %.9g U_EXCESS %.3g VALID %d" % (name, c, rec[c]["dual"], rec[c]["primal"], rec[c]["uExcess"], rec[c]["valid"]))
    last = rec[600]
    inside = 0
    for c in counts:
        r = rec[c]
        assert finite(r) and r["valid"] == 1.0, (name, c)
        if c in (1, 5, 20, 50, 100):
            assert r["dual"] <= last["dual"] + 1e-9 * r["absTerms"], (name, c, r["dual"], last["dual"])
        if r["uExcess"] == 0.0:
            inside += 1
            assert r["primal"] >= r["dual"] - 1e-9 * r["absTerms"], (name, c, r["primal"], r["dual"])
    if name == "tiny":
        assert inside >= 1, "no checked count with U_EXCESS = 0: the gap was never a gap"
        assert rec[300]["uExcess"] == 0.0 and rec[500]["uExcess"] == 0.0


# ---- (c), (d): a hand-made dual ---------------------------------------------------------------------------------------------------------
def hand_made(name="tiny", seed=11, perturb=()):
    """(model, ubox, x, u, xi, psi): random normal duals of the size of the oracle's own after 20 iterations, and the oracle's solve step there"""
    p, fc = problem(name)
    o = oracle(p, fc)
    o.apg(20)
    rng = np.random.default_rng(seed)
    sx, sp = np.abs(o.get("updXi")).max(), np.abs(o.get("updPsi")).max()
    xi = (sx if sx > 0 else 1.0) * rng.standard_normal(o.nodes * 2 * o.nx)
    psi = (sp if sp > 0 else 1.0) * rng.standard_normal(o.nodes * o.nu)
    x, u, xi, psi = co.oracle_point(o, (xi, psi))
    m = fp.Model(p["network"], p["tree"], p["config"], fc, perturb=perturb)
    return m, co.physical_ubox(p["network"], m.nodes), x, u, xi, psi


def test_a_dual_outside_the_domain_is_reported_and_stays_finite():
    m, ubox, x, u, xi, psi = hand_made()
    xi = xi.reshape(m.nodes, 2 * m.nx).copy()
    inside = xi.copy()
    inside[:, m.nx:] = -np.abs(inside[:, m.nx:])
    scale = 0.5 * min(m.gammaX / np.linalg.norm(inside[:, :m.nx]), m.gammaS / np.linalg.norm(inside[:, m.nx:]), 1.0)
    inside *= scale
    r = co.certificate(x, u, inside, psi, m, ubox)
    assert r["valid"] == 1.0 and finite(r)
    pos = inside.copy()
    pos[m.nodes // 2, m.nx + 1] = 1e-3 * np.abs(inside[:, m.nx:]).max()            # one xi_s entry > 0
    r = co.certificate(x, u, pos, psi, m, ubox)
    assert r["valid"] == 0.0 and r["xisPos"] == pos[m.nodes // 2, m.nx + 1] and finite(r)
    big = inside.copy()
    big[:, m.nx:] *= 1.01 * m.gammaS / np.linalg.norm(inside[:, m.nx:])            # |xi_s| > gamma_s
    r = co.certificate(x, u, big, psi, m, ubox)
    assert r["valid"] == 0.0 and r["normS"] > m.gammaS and r["xisPos"] == 0.0 and finite(r)
    dust = inside.copy()
    dust[0, m.nx] = 3e-20                                                          # rounding dust of the prox: outside the domain, reported as such
    r = co.certificate(x, u, dust, psi, m, ubox)
    assert r["xisPos"] == 3e-20 and finite(r) and r["valid"] == (1.0 if 3e-20 <= co.U * r["normS"] else 0.0)


@pytest.mark.parametrize("mistake", ["drop_xmax_support", "safety_upper_bound", "p_in_F", "drop_root_prev", "per_node_distance"])
def test_a_mistake_in_the_restatement_shows(mistake):
    m, ubox, x, u, xi, psi = hand_made()
    right = co.certificate(x, u, xi, psi, m, ubox)
    if mistake in co.MISTAKES:
        wrong = co.certificate(x, u, xi, psi, m, ubox, mistakes=(mistake,))
    else:
        wrong = co.certificate(x, u, xi, psi, hand_made(perturb=(mistake,))[0], ubox)
    col = "primal" if mistake == "per_node_distance" else "dual"
    moved = abs(wrong[col] - right[col]) / right["absTerms"]
    print("%s: %s moves by %.2e of ABS_TERMS" % (mistake, col.upper(), moved))
    assert moved > 1e-6
    if mistake == "per_node_distance":
        assert wrong["dual"] == right["dual"]
