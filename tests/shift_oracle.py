"""numpy restatement of the shifted warm start (rn_shift_warm_start, rn_get_shift_map; k_shift_duals, rapidnet_amd/csrc/k_dual.hpp and
rapidnet_amd/csrc/shift_map.hpp), written from the definition in include/rapidnet.h and from nothing of the library.  No library import.

The correspondence m: m(root) = child number root_child of the root (a lone root: itself); for the r-th child j of i: child number
min(r, nc - 1) of m(i) when m(i) has nc > 0 children, else m(i).  The values, all in fp64 and in this order:
    f = sqrt(p_i / p_m) * (d[stage(m)][c] / d[stage(i)][c]),  0 where p_i == 0, p_m == 0 or d[stage(i)][c] == 0
    y_new[i][c] = f * (y+[m][c] + 0)            (the + 0: a zero enters as +0), rounded once to the context's type by the caller
written to both y and y+; a map entry of -1 starts the row from zero.

`mistake` names one deliberate error (tests/test_shift_oracle.py shows that each of them changes a hand-made case):
    "d_inverted"  d[stage(i)] / d[stage(m)]          "p_not_sqrt"  p_i / p_m in place of its root
    "y_for_yp"    y taken for y+                     "in_place"    the gather row by row inside y+ itself
    "no_clamp"    child number r of m(i) taken modulo nc instead of clamped at nc - 1"""
import numpy as np

MISTAKES = ("d_inverted", "p_not_sqrt", "y_for_yp", "in_place", "no_clamp")


def tree_arrays(tree):
    """(parent [nodes], -1 for the root; stage [nodes]) from the JSON arrays: `ancestor` is 1-based with 0 for the root"""
    nodes = int(np.asarray(tree["nodes"]).ravel()[0])
    return np.asarray(tree["ancestor"], int).ravel()[:nodes] - 1, np.asarray(tree["stages"], int).ravel()[:nodes]


def children(parent):
    """the list of children of every node, in node order"""
    kids = [[] for _ in parent]
    for j, par in enumerate(parent):
        if par >= 0:
            kids[par].append(j)
    return kids


def shift_map(parent, root_child, mistake=None):
    parent = np.asarray(parent, int)
    kids = children(parent)
    m = np.zeros(len(parent), dtype=np.int64)
    m[0] = kids[0][root_child] if kids[0] else 0
    for i in range(len(parent)):                       # parents are numbered before their children
        src = kids[m[i]]
        for r, j in enumerate(kids[i]):
            if not src:
                m[j] = m[i]
            else:
                m[j] = src[r % len(src)] if mistake == "no_clamp" else src[min(r, len(src) - 1)]
    return m


def most_probable_child(parent, prob):
    kids = children(np.asarray(parent, int))[0]
    return int(np.argmax(np.asarray(prob, float)[kids])) if kids else 0      # argmax: the first of equal maxima


def factors(prob, d, stage, m):
    """f [nodes][ny] in fp64: one quotient, one root, one quotient, one product"""
    prob, d, stage, m = np.asarray(prob, np.float64), np.asarray(d, np.float64), np.asarray(stage, int), np.asarray(m, int)
    src = np.where(m >= 0, m, 0)
    pi, pm = prob[:, None], prob[src][:, None]
    di, dm = d[stage], d[stage[src]]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.sqrt(pi / pm) * (dm / di)
    return np.where((pi == 0) | (pm == 0) | (di == 0), 0.0, f)


def shift_duals(yp, prob, d, stage, m, y=None, mistake=None):
    """the shifted duals [nodes][ny] in fp64 (what both y and y+ become, before the rounding to the context's type).
    yp: y+ [nodes][ny]; prob [nodes]; d: the stage diagonal [N][ny] in y order; stage [nodes]; m: the correspondence (-1: from zero)"""
    yp, m = np.array(yp, np.float64), np.asarray(m, int)
    prob, d = np.asarray(prob, np.float64), np.asarray(d, np.float64)
    if mistake == "y_for_yp":
        yp = np.array(y, np.float64)
    if mistake == "d_inverted":
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(d == 0, 0.0, 1.0 / d)
    f = factors(prob * prob if mistake == "p_not_sqrt" else prob, d, stage, m)
    src = np.where(m >= 0, m, 0)
    if mistake == "in_place":
        out = yp
        for i in range(len(m)):                        # a row is read after another may have been written
            out[i] = f[i] * (out[src[i]] + 0.0)
    else:
        out = f * (yp[src] + 0.0)
    out[m < 0] = 0.0
    return out


def y_rows(xi, psi, nx, nu):
    """[node][2 nx + nu] from the flat RN_BUF_*_XI ([node][2 nx]) and RN_BUF_*_PSI ([node][nu]) arrays"""
    return np.hstack([np.asarray(xi, float).reshape(-1, 2 * nx), np.asarray(psi, float).reshape(-1, nu)])


def split_rows(y, nx):
    """the flat (xi, psi) arrays of [node][2 nx + nu] rows"""
    y = np.asarray(y)
    return y[:, : 2 * nx].ravel().copy(), y[:, 2 * nx:].ravel().copy()


def diag_y_order(mat_diag_precnd, N, nx, nu):
    """the stage diagonal in the y order of the context's rows.  matDiagPrecnd holds per stage [nu | nx | nx] (the psi part first, then the
    two halves of xi); a row of the context is [xi (2 nx) | psi (nu)]"""
    dg = np.asarray(mat_diag_precnd, float).reshape(N, 2 * nx + nu)
    return np.hstack([dg[:, nu:], dg[:, :nu]])
