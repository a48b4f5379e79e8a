"""The solve certificate (rn_solve_certificate) restated in numpy (test infrastructure, like plan_oracle.py): np.longdouble sums, the
formulas of DESIGN.md "the solve certificate", nothing imported from the library.

In the notation of tests/first_principles.py, with y = (xi_b, xi_s, psi) a multiplier and z = (x, u) a point on the dynamics:

    COST    = sum_i p_i (du_i' W du_i + alpha_i' u_i),        du_i = u_i - u_anc(i), the root against prevU
    Hz      = (F_i x_i, G_i u_i) = (fx_i x_i, fs_i x_i, g_i u_i)
    INNER   = <xi_b, fx x> + <xi_s, fs x> + <psi, g u>
    SUPPORT = sum max(xi_b xmin, xi_b xmax) + sum xi_s xs + sum max(psi umin, psi umax)            (the scaled bounds of the model)
    DUAL    = COST + INNER - SUPPORT                       <= the optimal value for y in the domain of g* and z the Lagrangian's minimiser at y
    NORM_X  = |xi_b|_2,  NORM_S = |xi_s|_2,  XIS_POS = max(xi_s, 0);  VALID = NORM_X <= gamma_x (1 + 4 u sqrt(n)), the same for NORM_S, and
              XIS_POS <= u NORM_S, u = 2^-53, n = nodes * nx
    DIST_X  = |fx x - clip(fx x, xmin, xmax)|_2,  DIST_S = |max(xs - fs x, 0)|_2                   (tree-global)
    PRIMAL  = COST + gamma_x DIST_X + gamma_s DIST_S;  GAP = PRIMAL - DUAL
    U_EXCESS = max over nodes and inputs of max(umin - u, u - umax, 0) in PHYSICAL units
    ABS_TERMS = sum|terms| of COST (per node: p_i |alpha_i' u_i| and p_i |du_i' W du_i|), of INNER and of SUPPORT (per entry)

`model` is a first_principles.Model, or anything with its attributes nodes, nx, nu, p, W, alpha, anc, u_root, fx, fs, g, xmin, xmax, xs, umin,
umax (scaled), gammaX, gammaS.  MISTAKES are deliberate mistakes for the negative controls of tests/test_certificate_oracle.py; two more
(p_in_F, drop_root_prev) are first_principles.Model's own."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
COLUMNS = ("dual", "primal", "gap", "cost", "inner", "support", "distX", "distS", "uExcess", "normX", "normS", "xisPos", "absTerms", "valid")
SUM_COLUMNS = ("cost", "inner", "support", "dist2X", "dist2S", "norm2X", "norm2S")
MISTAKES = ("drop_xmax_support", "safety_upper_bound", "per_node_distance")


def physical_ubox(network, nodes):
    """the network's own u box as per-node physical rows"""
    lo, hi = (np.asarray(network[k], float).ravel() for k in ("vecUmin", "vecUmax"))
    return np.repeat(lo[None, :], nodes, 0), np.repeat(hi[None, :], nodes, 0)


def certificate(x, u, xi, psi, model, ubox, hz=None, mistakes=()):
    """every column of the record (floats), plus "sums" / "sumabs" / "terms": value, sum of |terms| and number of terms of every sum column
    (SUM_COLUMNS; longdouble sums rounded once).  ubox: (umin, umax) physical, [nodes][nu].  hz: (Hz_xi [nodes][2 nx], Hz_psi [nodes][nu]) to
    use in place of (F x, G u) -- a context's own Hz(y)."""
    assert set(mistakes) <= set(MISTAKES), mistakes
    m = model
    n, nx, nu = m.nodes, m.nx, m.nu
    x, u = np.asarray(x, float).reshape(n, nx).astype(LD), np.asarray(u, float).reshape(n, nu).astype(LD)
    xi, psi = np.asarray(xi, float).reshape(n, 2 * nx).astype(LD), np.asarray(psi, float).reshape(n, nu).astype(LD)
    xib, xis = xi[:, :nx], xi[:, nx:]
    p = np.asarray(m.p, float).astype(LD)
    # COST: per node, as the record's ABS_TERMS counts it
    du = u.copy()
    du[1:] -= u[np.asarray(m.anc)[1:]]
    du[0] -= np.asarray(m.u_root, float).astype(LD)
    smooth = p * ((du @ np.asarray(m.W, float).astype(LD).T) * du).sum(axis=1)
    econ = p * (np.asarray(m.alpha, float).astype(LD) * u).sum(axis=1)
    if hz is None:
        hb, hs, hp = np.asarray(m.fx, float).astype(LD) * x, np.asarray(m.fs, float).astype(LD) * x, np.asarray(m.g, float).astype(LD) * u
    else:
        hxi, hp = np.asarray(hz[0], float).reshape(n, 2 * nx).astype(LD), np.asarray(hz[1], float).reshape(n, nu).astype(LD)
        hb, hs = hxi[:, :nx], hxi[:, nx:]
    xmin, xmax, xs, umin, umax = (np.asarray(getattr(m, k), float).astype(LD) for k in ("xmin", "xmax", "xs", "umin", "umax"))
    t_inner = np.concatenate([(xib * hb).ravel(), (xis * hs).ravel(), (psi * hp).ravel()])
    sb = xib * xmin if "drop_xmax_support" in mistakes else np.maximum(xib * xmin, xib * xmax)
    ss = xis * xs
    xs_hi = xs + np.abs(xs) + 1.0
    if "safety_upper_bound" in mistakes:
        ss = np.maximum(xis * xs, xis * xs_hi)
    t_support = np.concatenate([sb.ravel(), ss.ravel(), np.maximum(psi * umin, psi * umax).ravel()])
    db = hb - np.clip(hb, xmin, xmax)
    ds = np.maximum(xs - hs, 0) if "safety_upper_bound" not in mistakes else hs - np.clip(hs, xs, xs_hi)
    sums = {"cost": econ.sum() + smooth.sum(), "inner": t_inner.sum(), "support": t_support.sum(), "dist2X": (db * db).sum(), "dist2S": (ds * ds).sum(),
            "norm2X": (xib * xib).sum(), "norm2S": (xis * xis).sum()}
    sumabs = {"cost": np.abs(econ).sum() + np.abs(smooth).sum(), "inner": np.abs(t_inner).sum(), "support": np.abs(t_support).sum(),
              "dist2X": sums["dist2X"], "dist2S": sums["dist2S"], "norm2X": sums["norm2X"], "norm2S": sums["norm2S"]}
    terms = {"cost": 2 * n, "inner": n * (2 * nx + nu), "support": n * (2 * nx + nu), "dist2X": n * nx, "dist2S": n * nx, "norm2X": n * nx, "norm2S": n * nx}
    if "per_node_distance" in mistakes:
        dist_x, dist_s = np.sqrt((db * db).sum(axis=1)).sum(), np.sqrt((ds * ds).sum(axis=1)).sum()
    else:
        dist_x, dist_s = np.sqrt(sums["dist2X"]), np.sqrt(sums["dist2S"])
    gx, gs = LD(m.gammaX), LD(m.gammaS)
    dual = sums["cost"] + sums["inner"] - sums["support"]
    primal = sums["cost"] + gx * dist_x + gs * dist_s
    norm_x, norm_s = np.sqrt(sums["norm2X"]), np.sqrt(sums["norm2S"])
    xis_pos = max(float(xis.max()), 0.0)
    uf = np.asarray(u, float)
    lo, hi = np.asarray(ubox[0], float).reshape(n, nu), np.asarray(ubox[1], float).reshape(n, nu)
    u_excess = float(np.maximum(np.maximum(lo - uf, uf - hi), 0.0).max())      # (one IEEE subtraction and comparisons: exact, as the kernel's)
    slack = 1.0 + 4.0 * U * np.sqrt(float(n * nx))
    valid = bool(norm_x <= gx * slack and norm_s <= gs * slack and xis_pos <= U * float(norm_s))
    out = {"dual": dual, "primal": primal, "gap": primal - dual, "cost": sums["cost"], "inner": sums["inner"], "support": sums["support"],
           "distX": dist_x, "distS": dist_s, "uExcess": u_excess, "normX": norm_x, "normS": norm_s, "xisPos": xis_pos,
           "absTerms": sumabs["cost"] + sumabs["inner"] + sumabs["support"], "valid": 1.0 if valid else 0.0}
    out = {k: float(v) for k, v in out.items()}
    out["sums"] = {k: float(v) for k, v in sums.items()}
    out["sumabs"] = {k: float(v) for k, v in sumabs.items()}
    out["terms"] = terms
    # the largest |.| of the two vectors whose entries the squared columns are made of: y (NORM) and Hz (DIST)
    out["penalties"] = float(gx * dist_x + gs * dist_s)      # the two terms PRIMAL and GAP hold beside COST, INNER and SUPPORT
    out["gammaX"], out["gammaS"] = float(gx), float(gs)
    out["maxY"] = float(max(np.abs(xi).max(), np.abs(psi).max()))
    out["maxHz"] = float(max(np.abs(hb).max(), np.abs(hs).max(), np.abs(hp).max()))
    return out


def lagrangian(model, x, u, xi, psi):
    """Phi at (x, u) and the dual (xi, psi) by first_principles.Model's own methods alone (fp64): primal_value + <xi, F x> + <psi, G u>"""
    m = model
    psi = np.asarray(psi, float).reshape(m.nodes, m.nu)
    return m.primal_value(u) + float(np.dot(np.asarray(xi, float).ravel(), m.Fx(x).ravel())) + float((psi * m.g * np.asarray(u, float).reshape(m.nodes, m.nu)).sum())


SAVED = ("accXi", "accPsi", "x", "u", "v", "primalXi", "primalPsi")


def oracle_point(o, y=None):
    """(x, u, xi, psi): the CPU oracle's solve step at y = (xi, psi) -- default: its y+ (updXi, updPsi), the multiplier a warm start would keep --
    with the oracle's own iterates put back afterwards, so that an APG loop driven through apg_continue goes on undisturbed"""
    keep = {k: o.get(k) for k in SAVED}
    xi, psi = (o.get("updXi"), o.get("updPsi")) if y is None else (np.asarray(y[0], float).ravel(), np.asarray(y[1], float).ravel())
    o.set("accXi", xi)
    o.set("accPsi", psi)
    o.solve_step()
    x, u = o.get("x"), o.get("u")
    for k, v in keep.items():
        o.set(k, v)
    return x, u, xi, psi


def oracle_certificate(o, model, ubox, y=None, **kw):
    x, u, xi, psi = oracle_point(o, y)
    return certificate(x, u, xi, psi, model, ubox, **kw)
