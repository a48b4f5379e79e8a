"""numpy restatement of the plan bands (rn_plan_quantiles, rn_plan_paths; k_plan_bands, rapidnet_amd/csrc/k_plan.hpp), written from the
definition in include/rapidnet.h and from nothing of the kernel.

Quantile of stage k, component c, level q: the nodes i of the stage with p_i > 0, ordered by (value ascending, node index ascending); their p
added in that order in fp64, strictly one after the other (c_1 = p_(1), c_j = c_(j-1) + p_(j)); the result is the value of the first j with
c_j >= q * c_m, c_m the last sum.  Path of leaf l at stage k: the row of l's ancestor at stage k.

`mistake` names one deliberate error (tests/test_bands_oracle.py shows that each of them changes a result):
    "gt"          > for >=                        "desc_index"   ties in value broken by DESCENDING index
    "keep_zero"   nodes with p = 0 kept           "pairwise"     the sums by pairwise (tree) summation instead of one after the other
    "next_stage"  the rows of stage k + 1 taken for stage k (the last stage: its own)"""
import numpy as np

MISTAKES = ("gt", "desc_index", "keep_zero", "pairwise", "next_stage")


def tree_arrays(tree):
    """(parent [nodes], -1 for the root; stage [nodes]) from the JSON arrays: `ancestor` is 1-based with 0 for the root"""
    return np.asarray(tree["ancestor"], int) - 1, np.asarray(tree["stages"], int)


def _pairwise(p):
    if len(p) == 1:
        return float(p[0])
    h = len(p) // 2
    return _pairwise(p[:h]) + _pairwise(p[h:])


def ordered_sums(p, mistake=None):
    """c_1 ... c_m, each the sum of the first j entries added one after the other"""
    p = np.asarray(p, np.float64)
    if mistake == "pairwise":
        return np.array([_pairwise(p[: j + 1]) for j in range(len(p))])
    c = np.empty(len(p))
    run = 0.0
    for j, v in enumerate(p):      # (a Python loop: the order of the additions IS the definition)
        run = v if j == 0 else run + v
        c[j] = run
    return c


def quantile(values, prob, index, q, mistake=None):
    """the levels q of one (stage, component): values, prob, index [m] of the stage's nodes; returns [len(q)]"""
    values, prob, index = np.asarray(values, np.float64), np.asarray(prob, np.float64), np.asarray(index, int)
    keep = np.ones(len(prob), bool) if mistake == "keep_zero" else prob > 0
    v, p, i = values[keep], prob[keep], index[keep]
    order = np.lexsort((-i if mistake == "desc_index" else i, v))      # (the last key is the primary one)
    v, p = v[order], p[order]
    c = ordered_sums(p, mistake)
    out = np.empty(len(q))
    for l, ql in enumerate(np.asarray(q, np.float64)):
        thr = np.float64(ql) * c[-1]
        hit = np.flatnonzero(c > thr if mistake == "gt" else c >= thr)
        out[l] = v[hit[0]] if len(hit) else v[-1]
    return out


def quantiles(values, prob, stage, q, mistake=None):
    """values [nodes][dim], prob [nodes], stage [nodes] -> [N][dim][len(q)]"""
    values = np.asarray(values, np.float64)
    stage = np.asarray(stage, int)
    N, dim = int(stage.max()) + 1, values.shape[1]
    out = np.empty((N, dim, len(q)))
    for k in range(N):
        idx = np.flatnonzero(stage == (min(k + 1, N - 1) if mistake == "next_stage" else k))
        for c in range(dim):
            out[k, c] = quantile(values[idx, c], np.asarray(prob, np.float64)[idx], idx, q, mistake)
    return out


def paths(values, parent, stage):
    """values [nodes][dim] -> ([leaves][N][dim], leafNode [leaves]): leaf l is the l-th node of the last stage, row k its ancestor at stage k"""
    values = np.asarray(values, np.float64)
    stage = np.asarray(stage, int)
    N = int(stage.max()) + 1
    leaves = np.flatnonzero(stage == N - 1)
    out = np.empty((len(leaves), N, values.shape[1]))
    for l, leaf in enumerate(leaves):
        i = leaf
        for k in range(N - 1, -1, -1):
            assert stage[i] == k
            out[l, k] = values[i]
            i = parent[i]
        assert i == -1
    return out, leaves.astype(np.int32)
