"""tests/shift_oracle.py, the numpy restatement of the shifted warm start (rn_shift_warm_start), on hand-made cases -- without a GPU and
without the library.  The restatement is what tests/test_gpu_shift_warm_start.py holds the kernel to, so it is checked here against answers
worked out by hand, and each of its deliberate mistakes is shown to change one of them."""
import numpy as np
import pytest

import shift_oracle as so
from rapidnet_amd import synth


def tree_of(name):
    t = synth.make_problem(name)["tree"]
    parent, stage = so.tree_arrays(t)
    return t, parent, stage


def test_a_root_with_one_child():
    """`late`: stages of 1, 1, 1, 3, 3, 6, ... nodes.  The root inherits from its only child, the chain moves up, the first fan of three
    collapses onto the first node of the stage below it (its source has one child: the clamp), the last stage repeats itself"""
    _, parent, stage = tree_of("late")
    assert (parent == 0).sum() == 1
    m = so.shift_map(parent, 0)
    assert m[:3].tolist() == [1, 2, 3]
    assert m[3:6].tolist() == [6, 6, 6]              # children 0, 1, 2 of node 2 from the children of m(2) = 3, which has one
    assert (stage[m] == np.minimum(stage + 1, stage.max())).all()
    last = np.flatnonzero(stage == stage.max())
    assert set(m[last]) <= set(last)


def test_a_lone_root():
    _, parent, stage = tree_of("horizon1")
    assert len(parent) == 1 and so.shift_map(parent, 0).tolist() == [0]
    y = so.shift_duals(np.array([[1.5, -2.0, 0.25]]), [1.0], np.array([[2.0, 3.0, 4.0]]), stage, [0])
    assert np.array_equal(y, [[1.5, -2.0, 0.25]])     # f = sqrt(1) * (d / d) = 1 exactly


def test_the_clamp_on_ragged():
    """`ragged`: the root's three children have 2, 4 and 1 children (nodes 4-5, 6-9, 10)"""
    _, parent, stage = tree_of("ragged")
    kids = so.children(parent)
    assert [len(kids[c]) for c in kids[0]] == [2, 4, 1]
    # along child 0 (node 1, children 4 and 5): node 2's four children take children 0, 1, 1, 1 of m(2) = 5 ... which has kids[5]
    m = so.shift_map(parent, 0)
    assert m[0] == 1 and m[1:4].tolist() == [4, 5, 5]
    assert [m[j] for j in kids[2]] == [kids[5][min(r, len(kids[5]) - 1)] for r in range(4)]
    # along child 2 (node 3, ONE child, node 10): all three children of the root inherit from node 10
    m = so.shift_map(parent, 2)
    assert m[0] == 3 and m[1:4].tolist() == [10, 10, 10]
    # along child 1 (node 2, four children): nothing is clamped at the first level, node 3's only child takes child 0 of m(3) = 8
    m = so.shift_map(parent, 1)
    assert m[1:4].tolist() == [6, 7, 8] and m[10] == kids[8][0]
    assert not np.array_equal(so.shift_map(parent, 0, "no_clamp"), so.shift_map(parent, 0))


def test_the_last_stage_repeats_itself():
    for name in ("tiny", "small", "ragged", "fan"):
        _, parent, stage = tree_of(name)
        for child in range(int((parent == 0).sum())):
            m = so.shift_map(parent, child)
            last = stage == stage.max()
            assert (stage[m[last]] == stage.max()).all() and (stage[m[~last]] == stage[~last] + 1).all()
            before = np.flatnonzero(stage == stage.max() - 1)
            # a leaf inherits from what its parent inherits from: the parent's source is a leaf already
            for j in np.flatnonzero(last):
                assert m[j] == m[parent[j]]
            assert set(m[before]) <= set(np.flatnonzero(last))


def small_case():
    t, parent, stage = tree_of("small")
    prob = np.asarray(t["probNode"], float).ravel()[: len(parent)]
    ny, N = 5, int(stage.max()) + 1
    return parent, stage, prob, ny, N


def test_constant_per_stage_moves_up_one_stage_times_the_root_of_the_probability_ratio():
    parent, stage, prob, ny, N = small_case()
    d = np.full((N, ny), 0.7)
    yp = np.repeat((10.0 + np.arange(N))[stage][:, None], ny, axis=1)          # y+ = 10 + stage
    for child in range(3):
        m = so.shift_map(parent, child)
        got = so.shift_duals(yp, prob, d, stage, m)
        want = (10.0 + np.minimum(stage + 1, N - 1)) * np.sqrt(prob / prob[m])
        assert np.array_equal(got, np.repeat(want[:, None], ny, axis=1))       # d / d = 1 exactly: no rounding beyond the restatement's own
    assert got[0, 0] == 11.0 * np.sqrt(1.0 / prob[m[0]])


def hand_case():
    """a root with two children, two leaves each: stages 0 | 1 1 | 2 2 2 2; p and d chosen as powers of two and squares, so every factor is
    exact and the answers below are worked out by hand"""
    parent = np.array([-1, 0, 0, 1, 1, 2, 2])
    stage = np.array([0, 1, 1, 2, 2, 2, 2])
    prob = np.array([1.0, 0.25, 0.75, 0.0625, 0.1875, 0.25, 0.5])
    d = np.array([[1.0, 2.0], [2.0, 8.0], [4.0, 2.0]])
    yp = np.array([[1.0, 1.0], [2.0, 3.0], [5.0, 7.0], [11.0, 13.0], [17.0, 19.0], [23.0, 29.0], [31.0, 37.0]])
    y = yp + 100.0
    return parent, stage, prob, d, yp, y


def test_a_case_worked_out_by_hand():
    parent, stage, prob, d, yp, _ = hand_case()
    m = so.shift_map(parent, 0)
    assert m.tolist() == [1, 3, 4, 3, 3, 4, 4]
    got = so.shift_duals(yp, prob, d, stage, m)
    # node 0 <- 1: sqrt(1 / 0.25) = 2, d1 / d0 = (2, 4): f = (4, 8)
    assert got[0].tolist() == [8.0, 24.0]
    # node 1 <- 3: sqrt(0.25 / 0.0625) = 2, d2 / d1 = (2, 0.25): f = (4, 0.5)
    assert got[1].tolist() == [44.0, 6.5]
    # node 2 <- 4: sqrt(0.75 / 0.1875) = 2: f = (4, 0.5)
    assert got[2].tolist() == [68.0, 9.5]
    # node 3 <- 3: 1; node 4 <- 3: sqrt(0.1875 / 0.0625) = sqrt(3); node 5 <- 4: sqrt(0.25 / 0.1875); node 6 <- 4: sqrt(0.5 / 0.1875)
    assert got[3].tolist() == [11.0, 13.0]
    assert np.array_equal(got[4], np.sqrt(3.0) * yp[3]) and np.array_equal(got[6], np.sqrt(0.5 / 0.1875) * yp[4])


@pytest.mark.parametrize("mistake", so.MISTAKES)
def test_every_deliberate_mistake_changes_a_hand_made_case(mistake):
    parent, stage, prob, d, yp, y = hand_case()
    if mistake == "no_clamp":
        _, parent, stage = tree_of("ragged")
        assert not np.array_equal(so.shift_map(parent, 0, mistake), so.shift_map(parent, 0))
        return
    m = so.shift_map(parent, 0)
    good = so.shift_duals(yp, prob, d, stage, m, y=y)
    bad = so.shift_duals(yp, prob, d, stage, m, y=y, mistake=mistake)
    assert not np.array_equal(good, bad), mistake
    if mistake == "in_place":        # the rows whose source was written before them: 3 .. 6 read rows 3 and 4; row 4 <- 3 is still right
        assert np.array_equal(good[:4], bad[:4]) and not np.array_equal(good[5], bad[5])
    if mistake == "d_inverted":      # the last stage onto itself has d / d = 1 either way
        assert np.array_equal(good[3:], bad[3:]) and not np.array_equal(good[0], bad[0])


def test_zero_probabilities_zero_diagonals_and_rows_from_zero():
    parent, stage, prob, d, yp, _ = hand_case()
    m = so.shift_map(parent, 0)
    p0 = prob.copy(); p0[3] = 0.0                      # node 3 is the source of 1, 3 and 4
    got = so.shift_duals(yp, p0, d, stage, m)
    assert np.isfinite(got).all() and not got[[1, 3, 4]].any() and got[[0, 2, 5, 6]].all()
    d0 = d.copy(); d0[1, 1] = 0.0                      # stage 1, component 1: the rows of stage 1 read 0 there, the root's row reads d1 / d0 = 0
    got = so.shift_duals(yp, prob, d0, stage, m)
    assert np.isfinite(got).all() and got[1, 1] == 0.0 and got[2, 1] == 0.0 and got[0, 1] == 0.0 and got[1, 0] == 44.0
    own = m.copy(); own[[2, 6]] = -1
    got = so.shift_duals(yp, prob, d, stage, own)
    assert not got[[2, 6]].any() and np.array_equal(got[[0, 1, 3, 4, 5]], so.shift_duals(yp, prob, d, stage, m)[[0, 1, 3, 4, 5]])
    ident = np.arange(len(parent))
    assert np.array_equal(so.shift_duals(yp, prob, d, stage, ident), yp)          # the identity keeps the duals: f = 1 exactly
    neg = yp.copy(); neg[3, 0] = -0.0
    assert not np.signbit(so.shift_duals(neg, prob, d, stage, ident)[3, 0])       # a zero enters as +0


def test_most_probable_child_and_the_row_helpers():
    parent, stage, prob, d, yp, _ = hand_case()
    assert so.most_probable_child(parent, prob) == 1
    assert so.most_probable_child(parent, [1.0, 0.5, 0.5, 0, 0, 0, 0]) == 0        # ties to the lowest index
    assert so.most_probable_child([-1], [1.0]) == 0
    xi, psi = np.arange(12.0), 100 + np.arange(9.0)
    rows = so.y_rows(xi, psi, 2, 3)
    assert rows.shape == (3, 7) and rows[1].tolist() == [4, 5, 6, 7, 103, 104, 105]
    a, b = so.split_rows(rows, 2)
    assert np.array_equal(a, xi) and np.array_equal(b, psi)
    dg = so.diag_y_order(np.arange(14.0), 2, 2, 3)
    assert dg[0].tolist() == [3, 4, 5, 6, 0, 1, 2] and dg[1].tolist() == [10, 11, 12, 13, 7, 8, 9]
