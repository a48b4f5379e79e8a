"""The numpy restatement of rn_estimate_lipschitz (tests/lipschitz_oracle.py) checked against the definition and shown to have teeth,
without a GPU.

1. The hashed start vector equals a table of entries computed by hand (64-bit integer arithmetic, written out below).
2. On `toy`, `tiny`, `odd`, `small` and `ragged` the loop over the dense M = K H^-1 K' built from first_principles.Model obeys, after 10, 20
   and 40 iterations, RAYLEIGH <= NORM (1 + 1e-12) and NORM <= lambda_max (1 + 1e-12) (eigvalsh); after 40, NORM >= 0.9999 lambda_max --
   a condition on the inputs: the hashed start of seed 0 meets it on all five shapes (NORM / lambda_max after 10 / 20 / 40 iterations:
   toy 1.000000 / 1.000000 / 1.000000, tiny 0.999845 / 1.000000 / 1.000000, odd 0.992036 / 0.999979 / 1.000000, small 0.999736 / 0.999994 /
   1.000000, ragged 0.987732 / 0.999958 / 1.000000), so no shape needs another seed (SEED).
3. The same loop over synth._Structured.apply reproduces synth.lipschitz_estimate to 1e-12 from its start vector.
4. Negative controls: five ways of getting the loop wrong, each of which moves NORM by more than 1e-6 relative or moves a history row.

The helpers (problem, dense M, the cached histories) are shared with tests/test_gpu_lipschitz.py."""
import numpy as np
import pytest

import lipschitz_oracle as lo
from first_principles import Model
from rapidnet_amd import synth

SHAPES = ("toy", "tiny", "odd", "small", "ragged")
SEED = {name: 0 for name in SHAPES}      # the seed of the hashed start per shape (0 meets the 0.9999 condition everywhere)
_PROBLEMS, _DENSE = {}, {}


def problem(name):
    if name not in _PROBLEMS:
        p = synth.make_problem(name)
        _PROBLEMS[name] = (p, synth.forecast_at(p["forecast"], 0))
    return _PROBLEMS[name]


def dims(p):
    nx, nu = int(p["network"]["nx"][0]), int(p["network"]["nu"][0])
    return int(p["tree"]["nodes"][0]), nx, nu


def dense(name):
    """(M, lambda_max, apply) of the definition, once per session"""
    if name not in _DENSE:
        p, fc = problem(name)
        M = lo.dense_M(Model(p["network"], p["tree"], p["config"], fc))
        nodes, nx, nu = dims(p)
        _DENSE[name] = (M, float(np.linalg.eigvalsh(M)[-1]), lo.dense_apply(M, nodes, nx, nu))
    return _DENSE[name]


def test_hash_start_equals_a_hand_computed_table():
    # i = g * ny + c;  x = seed + (i + 1) * 0x9E3779B97F4A7C15 mod 2^64, then the three xor-shift / multiply rounds; value = (x >> 11) 2^-52 - 1
    # x after the rounds is splitmix64's output number i + 1 from the state `seed`: its published first outputs are the table
    table = {(0, 0): 0xE220A8397B1DCDAF, (0, 1): 0x6E789E6AA1B965F4, (0, 2): 0x06C45D188009454F, (1, 0): 0x910A2DEC89025CC1}
    for (seed, i), x in table.items():
        assert lo.hash_value(seed, i) == float(x >> 11) * 2.0 ** -52 - 1.0
    # ... and as decimals: 0xE220A8397B1DCDAF >> 11 = 7956156453446585, / 2^52 = 1.76662161..., - 1
    assert lo.hash_value(0, 0) == 7956156453446585 / 4503599627370496 - 1.0
    assert abs(lo.hash_value(0, 0) - 0.7666216164272852) < 1e-15 and abs(lo.hash_value(0, 1) + 0.13694400590298006) < 1e-15
    assert abs(lo.hash_value(0, 2) + 0.9471324568148045) < 1e-15 and abs(lo.hash_value(1, 0) - 0.1331231503445618) < 1e-15
    # the vector form: the same entries, laid out [node][xi | psi], by GLOBAL node
    nx, nu = 2, 3
    ny = 2 * nx + nu
    xi, psi = lo.hash_start(4, nx, nu, seed=5)
    for g in range(4):
        for c in range(ny):
            want = lo.hash_value(5, g * ny + c)
            assert (xi[g, c] if c < 2 * nx else psi[g, c - 2 * nx]) == want
    assert -1.0 <= min(xi.min(), psi.min()) and max(xi.max(), psi.max()) < 1.0
    xi32, _ = lo.hash_start(4, nx, nu, seed=5, dtype=np.float32)
    assert np.array_equal(xi32, xi.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("name", SHAPES)
def test_loop_over_the_dense_definition(name):
    p, _ = problem(name)
    M, lam, apply = dense(name)
    nodes, nx, nu = dims(p)
    xi, psi = lo.hash_start(nodes, nx, nu, SEED[name])
    hist = lo.power_loop(apply, xi, psi, 40)
    for it in (10, 20, 40):
        h = lo.power_loop(apply, xi, psi, it)
        assert np.array_equal(h, hist[:it])      # a shorter run is a prefix
        assert h[-1, lo.RAYLEIGH] <= h[-1, lo.NORM] * (1 + 1e-12)
        assert h[-1, lo.NORM] <= lam * (1 + 1e-12)
    print("%s: lambda_max %.9g, NORM / lambda_max after 10 / 20 / 40: %.6f %.6f %.6f" % (name, lam, hist[9, 0] / lam, hist[19, 0] / lam, hist[39, 0] / lam))
    assert hist[39, lo.NORM] >= 0.9999 * lam


@pytest.mark.parametrize("name", SHAPES)
def test_loop_over_the_structured_operator_reproduces_synth(name):
    p, _ = problem(name)
    op = synth._Structured(p["network"], p["tree"], p["config"])
    rng = np.random.default_rng(0)
    xi = rng.standard_normal((op.nodes, 2 * op.nx))
    psi = rng.standard_normal((op.nodes, op.nu))
    for it in (1, 40):
        want = synth.lipschitz_estimate(p["network"], p["tree"], p["config"], iters=it, seed=0)
        got = lo.power_loop(op.apply, xi, psi, it)[-1, lo.NORM]
        assert abs(got - want) <= 1e-12 * want


def _hand_case():
    """a 3-node chain with a 2-node 'crown', ny = 3: a symmetric positive definite M with a clear gap, and a start far from its top vector"""
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.standard_normal((9, 9)))
    M = Q @ np.diag([10.0, 7.0, 5.0, 3.0, 2.0, 1.5, 1.0, 0.5, 0.25]) @ Q.T
    return 0.5 * (M + M.T), lo.dense_apply(M, 3, 1, 1)


def test_negative_controls_move_the_result():
    M, apply = _hand_case()
    xi, psi = lo.hash_start(3, 1, 1, 0)
    good = lo.power_loop(apply, xi, psi, 6)

    def moved(h):
        rel = abs(h[-1, lo.NORM] - good[-1, lo.NORM]) / good[-1, lo.NORM]
        rows = h.shape != good.shape or not np.allclose(h, good, rtol=1e-9, atol=0)
        return rel > 1e-6, rows
    # normalising by s instead of sqrt(s): the loop is scale invariant, so NORM survives -- but t = <v, w> is taken against a v that is not a
    # unit vector, and RAYLEIGH / RESIDUAL rows move
    assert moved(lo.power_loop(apply, xi, psi, 6, mistake=("normalise_by_s",)))[1]
    # skipping the replicated crown (the first two nodes) where it must count: NORM itself moves
    assert moved(lo.power_loop(apply, xi, psi, 6, mistake=("skip_crown",), first=2))[0]
    # a start indexed by local instead of global node: a 'shard' holding nodes (0, 2) of the tree starts from other values
    gx, gp = lo.hash_start(2, 1, 1, 0, global_nodes=[0, 2])
    lx, lp = lo.hash_start(2, 1, 1, 0)
    assert np.array_equal(gx[0], lx[0]) and not np.array_equal(gx[1], lx[1]) and np.array_equal(gx[1], xi[2]) and np.array_equal(gp[1], psi[2])
    # an off-by-one in the history row
    assert moved(lo.power_loop(apply, xi, psi, 6, mistake=("history_off_by_one",)))[1]
    # t against the un-normalised v
    h = lo.power_loop(apply, xi, psi, 6, mistake=("t_unnormalised",))
    assert moved(h)[1] and abs(h[-1, lo.RAYLEIGH] - good[-1, lo.RAYLEIGH]) > 1e-6 * good[-1, lo.RAYLEIGH]


def test_early_stop_is_a_prefix_and_stops_at_a_multiple():
    M, apply = _hand_case()
    xi, psi = lo.hash_start(3, 1, 1, 0)
    full = lo.power_loop(apply, xi, psi, 40)
    h = lo.power_loop(apply, xi, psi, 40, tol=1e-2, check_every=5)
    assert len(h) % 5 == 0 and 5 <= len(h) < 40 and h[-1, lo.RESIDUAL] <= 1e-2
    assert np.array_equal(h[-1], full[len(h) - 1])
    assert len(h) == 5 or full[len(h) - 6, lo.RESIDUAL] > 1e-2
