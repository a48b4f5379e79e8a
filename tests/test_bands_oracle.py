"""The numpy restatement of the plan bands (tests/bands_oracle.py) on hand-made cases, without a GPU: each result is written down by hand,
and each of five deliberate mistakes changes the result of at least one case -- a restatement on which a mistake does not show would prove
nothing about the kernel that is compared with it bit for bit (tests/test_gpu_plan_bands.py)."""
import numpy as np
import pytest

import bands_oracle as bo

Q_ABOVE = 0.6000000000000001      # the double right above 0.6: (0.1 + 0.2) + 0.3 in fp64, while 0.1 + (0.2 + 0.3) and (0.3 + 0.2) + 0.1 are 0.6


def one(values, prob, q, mistake=None, index=None):
    index = np.arange(len(values)) if index is None else index
    return bo.quantile(values, prob, index, q, mistake)


# name -> (values, prob, levels, expected)
CASES = {
    # c = .25 .5 .75 1: the sum meets q c_m = 0.5 exactly at the second node, and >= takes it
    "even count, equal p, q = 0.5": ([4.0, 1.0, 3.0, 2.0], [0.25, 0.25, 0.25, 0.25], [0.5], [2.0]),
    # three nodes tied at 1.0 with p = .1 .2 .3 by ascending index: c_3 = 0.6000000000000001 >= q c_m (c_m = 1.0), the tied value;
    # by descending index c_3 = (.3 + .2) + .1 = 0.6 < q c_m and the walk goes on to 2.0
    "ties in value": ([1.0, 1.0, 1.0, 2.0], [0.1, 0.2, 0.3, 0.4], [Q_ABOVE], [1.0]),
    # the same sums on distinct values: one after the other c_3 = 0.6000000000000001, by halves c_3 = .1 + (.2 + .3) = 0.6
    "ordered summation": ([1.0, 2.0, 3.0, 4.0], [0.1, 0.2, 0.3, 0.4], [Q_ABOVE], [3.0]),
    "zero-probability node holds the maximum": ([1.0, 9.0, 2.0, 3.0], [0.5, 0.0, 0.25, 0.25], [0.0, 1.0], [1.0, 3.0]),
    "zero-probability node holds the minimum": ([1.0, -9.0, 2.0, 3.0], [0.5, 0.0, 0.25, 0.25], [0.0, 1.0], [1.0, 3.0]),
    "q = 0 and q = 1, levels unsorted": ([3.0, 1.0, 2.0], [0.2, 0.3, 0.5], [1.0, 0.0, 0.4], [3.0, 1.0, 2.0]),
    "one node": ([7.5], [0.125], [0.0, 0.3, 1.0], [7.5, 7.5, 7.5]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_by_hand(name):
    v, p, q, want = CASES[name]
    assert np.array_equal(one(v, p, q), want), name


def test_the_sums_of_the_cases_are_what_the_comments_say():
    assert (0.1 + 0.2) + 0.3 == Q_ABOVE and (0.3 + 0.2) + 0.1 == 0.6 and 0.1 + (0.2 + 0.3) == 0.6 and Q_ABOVE > 0.6
    assert ((0.1 + 0.2) + 0.3) + 0.4 == 1.0 and ((0.3 + 0.2) + 0.1) + 0.4 == 1.0 and (0.1 + 0.2) + (0.3 + 0.4) == 1.0
    assert np.array_equal(bo.ordered_sums([0.1, 0.2, 0.3, 0.4]), [0.1, 0.1 + 0.2, Q_ABOVE, 1.0])
    assert bo.ordered_sums([0.1, 0.2, 0.3, 0.4], "pairwise")[2] == 0.6


# a two-stage tree for the stage bookkeeping: root, then three children
TREE = {"ancestor": [0, 1, 1, 1], "stages": [0, 1, 1, 1]}
X = np.array([[10.0, -1.0], [3.0, 5.0], [1.0, 6.0], [2.0, 4.0]])
P = np.array([1.0, 0.5, 0.25, 0.25])


def test_stages_and_paths_by_hand():
    parent, stage = bo.tree_arrays(TREE)
    assert parent.tolist() == [-1, 0, 0, 0]
    got = bo.quantiles(X, P, stage, [0.0, 0.5, 1.0])
    assert got.shape == (2, 2, 3)
    assert np.array_equal(got[0], [[10.0] * 3, [-1.0] * 3])
    # stage 1, component 0: values 1 (p .25), 2 (.25), 3 (.5): c = .25 .5 1; component 1: 4 (.25), 5 (.5), 6 (.25): c = .25 .75 1
    assert np.array_equal(got[1], [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    pth, leaf = bo.paths(X, parent, stage)
    assert leaf.tolist() == [1, 2, 3] and pth.shape == (3, 2, 2)
    for l, n in enumerate(leaf):
        assert np.array_equal(pth[l], [X[0], X[n]])


@pytest.mark.parametrize("mistake", bo.MISTAKES)
def test_every_mistake_changes_a_result(mistake):
    changed = [name for name, (v, p, q, want) in CASES.items() if not np.array_equal(one(v, p, q, mistake), want)]
    _, stage = bo.tree_arrays(TREE)
    if not np.array_equal(bo.quantiles(X, P, stage, [0.0, 0.5, 1.0], mistake), bo.quantiles(X, P, stage, [0.0, 0.5, 1.0])):
        changed.append("two-stage tree")
    print("%s changes: %s" % (mistake, changed))
    assert changed, mistake
    expected = {"gt": "even count, equal p, q = 0.5", "desc_index": "ties in value", "keep_zero": "zero-probability node holds the minimum",      # (kept at the far end it is never reached: >= stops before it)
                "pairwise": "ordered summation", "next_stage": "two-stage tree"}[mistake]
    assert expected in changed, (mistake, changed)
