"""The plan report (rn_plan_report, rn_plan_report_scenarios) restated in numpy from plain arrays.  It imports neither the library nor the
CPU oracle: the tests hand it what they read from either.

Per node i with parent a(i): du_i = u_i - u_a(i) (the root against prevU), bounds row brow[i] of the tables given, all values physical.

    ECON      p_i alpha_i' u_i                  SMOOTH    p_i du_i' W du_i             STORED    p_i sum_j x_ij
    SHORT_EXP p_i sum_j max(xs_j - x_ij, 0)     XBOX_EXP  p_i sum_j [max(xmin_j - x_ij, 0) + max(x_ij - xmax_j, 0)]      UBOX_EXP  the same for u
    SHORT_MAX, XBOX_MAX, UBOX_MAX: the largest single entry of the same three violations, not weighted

Per stage: the sum columns summed over the nodes of the stage (each node `mult[i]` times: 1, or the number of ranks that would count it),
the maxima over the same nodes.  Per leaf: the terms NOT weighted, summed (maxima: taken) along the path leaf -> root; STORED the leaf's own.
Next to every sum: the sum of the absolute values of its terms and their number m -- a term is one product p * a * b (ECON, STORED, the
violations: one entry; SMOOTH: one p du_j W_jk du_k) -- which is what a bound on the difference of two summation orders needs.
A violation is written max(a - b, 0) = where(a - b > 0, a - b, 0): one IEEE subtraction and a comparison, so the maxima are exact."""
import numpy as np

COLUMNS = ("econ", "smooth", "stored", "shortExp", "xboxExp", "uboxExp", "shortMax", "xboxMax", "uboxMax")
SUMS = 6
ECON, SMOOTH, STORED, SHORT_EXP, XBOX_EXP, UBOX_EXP, SHORT_MAX, XBOX_MAX, UBOX_MAX = range(9)


def excess(a, b):
    d = a - b
    return np.where(d > 0, d, 0.0)


def node_terms(x, u, alpha, prevU, W, parent, xmin, xmax, xs, umin, umax, brow):
    """unweighted per-node columns [nodes][9], the sums of absolute terms [nodes][6] and the term counts [6]"""
    x, u, alpha = (np.asarray(a, np.float64) for a in (x, u, alpha))
    nodes, nx = x.shape
    nu = u.shape[1]
    W = np.asarray(W, np.float64).reshape(nu, nu)
    parent = np.asarray(parent, int)
    brow = np.asarray(brow, int)
    up = np.where((parent >= 0)[:, None], u[np.maximum(parent, 0)], np.asarray(prevU, np.float64)[None, :])
    du = u - up
    val, ab = np.zeros((nodes, 9)), np.zeros((nodes, SUMS))
    val[:, ECON] = (alpha * u).sum(1)
    ab[:, ECON] = np.abs(alpha * u).sum(1)
    val[:, SMOOTH] = ((du @ W.T) * du).sum(1)
    ab[:, SMOOTH] = ((np.abs(du) @ np.abs(W).T) * np.abs(du)).sum(1)
    val[:, STORED] = x.sum(1)
    ab[:, STORED] = np.abs(x).sum(1)
    sh = excess(np.asarray(xs, np.float64)[brow], x)
    x1, x2 = excess(np.asarray(xmin, np.float64)[brow], x), excess(x, np.asarray(xmax, np.float64)[brow])
    u1, u2 = excess(np.asarray(umin, np.float64)[brow], u), excess(u, np.asarray(umax, np.float64)[brow])
    val[:, SHORT_EXP] = ab[:, SHORT_EXP] = sh.sum(1)
    val[:, XBOX_EXP] = ab[:, XBOX_EXP] = (x1 + x2).sum(1)
    val[:, UBOX_EXP] = ab[:, UBOX_EXP] = (u1 + u2).sum(1)
    val[:, SHORT_MAX] = sh.max(1)
    val[:, XBOX_MAX] = np.maximum(x1, x2).max(1)
    val[:, UBOX_MAX] = np.maximum(u1, u2).max(1)
    m = np.array([nu, nu * nu, nx, nx, 2 * nx, 2 * nu])
    return val, ab, m


def evaluate(x, u, alpha, prevU, p, W, parent, stage, xmin, xmax, xs, umin, umax, brow, mult=None, variant=None):
    """{"stage": [N][9], "stage_abs": [N][6], "stage_m": [N][6], "leaf": [leaves][9], "leaf_abs": [leaves][6], "leaf_m": [leaves][6],
    "leafNode": [leaves], "stage_absmax_x": [N], "stage_absmax_u": [N], "node": [nodes][9], "node_abs": [nodes][6] (not weighted)}.
    variant (negative controls of the tests): "smooth_unweighted" drops p from SMOOTH, "short_max_weighted" weights SHORT_MAX by p."""
    val, ab, m = node_terms(x, u, alpha, prevU, W, parent, xmin, xmax, xs, umin, umax, brow)
    p = np.asarray(p, np.float64)
    stage = np.asarray(stage, int)
    parent = np.asarray(parent, int)
    N = int(stage.max()) + 1
    mult = np.ones(len(p)) if mult is None else np.asarray(mult, np.float64)
    out = {k: np.zeros((N, 9 if k == "stage" else SUMS)) for k in ("stage", "stage_abs", "stage_m")}
    out["stage_absmax_x"], out["stage_absmax_u"] = np.zeros(N), np.zeros(N)
    out["node"], out["node_abs"] = val, ab          # the per-node terms, not weighted
    for k in range(N):
        idx = np.flatnonzero(stage == k)
        w = (p[idx] * mult[idx])[:, None]
        ws = np.repeat(w, SUMS, axis=1)
        if variant == "smooth_unweighted":
            ws[:, SMOOTH] = mult[idx]
        out["stage"][k, :SUMS] = (ws * val[idx, :SUMS]).sum(0)
        out["stage_abs"][k] = (ws * ab[idx]).sum(0)
        out["stage_m"][k] = m * mult[idx].sum()
        mx = val[idx, SUMS:].copy()
        if variant == "short_max_weighted":
            mx[:, 0] *= p[idx]
        out["stage"][k, SUMS:] = mx.max(0)
        out["stage_absmax_x"][k] = np.abs(np.asarray(x, np.float64)[idx]).max()
        out["stage_absmax_u"][k] = np.abs(np.asarray(u, np.float64)[idx]).max()
    leaves = np.flatnonzero(stage == N - 1)
    out["leafNode"] = leaves
    out["leaf"], out["leaf_abs"], out["leaf_m"] = np.zeros((len(leaves), 9)), np.zeros((len(leaves), SUMS)), np.zeros((len(leaves), SUMS))
    for r, leaf in enumerate(leaves):
        path, i = [], leaf
        while i >= 0 and len(path) <= N:
            path.append(i)
            i = parent[i]
        out["leaf"][r, :SUMS] = val[path, :SUMS].sum(0)
        out["leaf_abs"][r] = ab[path].sum(0)
        out["leaf_m"][r] = m * len(path)
        out["leaf"][r, SUMS:] = val[path, SUMS:].max(0)
        out["leaf"][r, STORED], out["leaf_abs"][r, STORED], out["leaf_m"][r, STORED] = val[leaf, STORED], ab[leaf, STORED], m[STORED]
    return out


def alive(table):
    """per column: the fraction of the rows in which it is not zero"""
    return (np.asarray(table) != 0).mean(0)
