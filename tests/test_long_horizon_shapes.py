"""The long-horizon shapes of tests/test_gpu_long_horizon.py, guarded without a GPU.

No named shape of rapidnet_amd.synth has a chain (the part of the tree below the last branching, L = N - chainStage stages) longer than 23
stages, and the chain kernels of csrc/k_walks.hpp are written around batches of prefetched stages: UP_PF = 24 (k_up_chain, the Bs branch of
up_chain_lin_walk), LIN_PF = CHAIN_PF = 12 (the other branches, k_up_chain_cut, k_down_chain, k_down_chain_dual).  The shapes here have
L in {24, 25, 36, 37, 48, 49}: a full last batch and one stage past it, for both batch sizes -- and 33 / 34 on the Barcelona network, either
side of the 64 KB of LDS the fused walk + dual update may take in fp64 (N ny sizeof(T), ny = 240: N = 34 fits, N = 35 does not).

Every reference the GPU file compares against is built here, once per shape, and guarded:
  * the oracle's APG history stays finite over 60 iterations and never exceeds its first entry by more than 10x (a long horizon behind a
    single-child stage can make the 40 power iterations of synth.lipschitz_estimate undershoot: such a shape does not get in);
  * ONE STEP FROM NON-TRIVIAL DUALS (random xi, psi, updXi, updPsi of scale 50: from zero a plain APG run leaves the duals of many stages
    at rounding dust, and a seam bug in the m2 / q / Bu branches would multiply by zero): in every stage, every compared buffer's maximum
    is at least 1e-4 of the buffer's tree-wide maximum, and at most N / 8 stages of a buffer sit below stagewise.FLOOR -- the per-stage
    measure of stagewise.py then divides nearly every stage's error by that stage's own magnitude.

The self-test (test_a_walk_that_mishandles_the_seam_is_refused) restates the solve step in numpy with the up walk's running sum in the
kernel's form -- s_i = beta_i + rho, rho = s_i + m_i -- and a switch that mishandles the seam between the first and the second batch of
UP_PF stages.  The per-stage check refuses either mistake by orders of magnitude at L = 25; at L = 23 the same switch changes no bit."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from rapidnet_amd import synth
from stagewise import FLOOR, node_stages, stage_relmax, worst_by_buffer

UP_PF, LIN_PF, CHAIN_PF = 24, 12, 12      # csrc/k_walks.hpp
LENGTHS = (24, 25, 36, 37, 48, 49)
REL_TOL = 1e-9
NAMES = ("x", "u", "v", "xi", "psi", "accXi", "accPsi", "updXi", "updPsi", "primalXi", "primalPsi", "dualXi", "dualPsi", "resXi", "resPsi")
BATCHES = (20, 17, 3)                     # two optimistic batches (>= 16 iterations) and an exact tail
ITERS = sum(BATCHES)

# name -> ((seed index, nx, nu, nd, ne, N, branching), L)
SHAPES = {}
for _L in LENGTHS:
    SHAPES["s22_%d" % _L] = ((50, 3, 6, 4, 2, _L + 2, [2, 2]), _L)
    SHAPES["s3_%d" % _L] = ((51, 5, 9, 6, 3, _L + 1, [3]), _L)
SHAPES.update({
    "m42_36": ((52, 21, 38, 30, 6, 38, [4, 2]), 36),     # ny = 80: k_dual_stage and the fused launch
    "m42_37": ((52, 21, 38, 30, 6, 39, [4, 2]), 37),
    "m5_25": ((52, 21, 38, 30, 6, 26, [5]), 25),
    "b5_33": ((53, 63, 114, 88, 17, 34, [5]), 33),       # 34 * 240 * 8 = 65 280 B: the fused launch
    "b5_34": ((53, 63, 114, 88, 17, 35, [5]), 34),       # 35 * 240 * 8 = 67 200 B: two launches
    "one_49": ((54, 3, 6, 4, 2, 49, []), 49),            # one scenario: the chain is the tree
    "rag_25": ((55, 6, 11, 5, 3, 28, [3, [2, 4, 1], [1, 2, 1, 3, 1, 2, 1]]), 25),
    "odd_37": ((56, 7, 13, 5, 4, 39, [2, 3]), 37),       # ny = 27: the flat dual update
})
SMALL = tuple(n for n in SHAPES if n.startswith(("s22_", "s3_")))
MEDIUM = ("m42_36", "m42_37", "m5_25")
BARCELONA = ("b5_33", "b5_34")
# dualXi of the single-scenario shape falls to 3e-6 of its maximum in some stages: it is not compared there
NOT_COMPARED = {"one_49": ("dualXi",)}

_PROBLEMS, _STEP, _APG = {}, {}, {}


class registered:
    """the long shapes as names of synth.CONFIGS for the length of a `with` block (the bodies of other test files take names)"""

    def __init__(self, *names):
        self.names = names

    def __enter__(self):
        for n in self.names:
            assert n not in synth.CONFIGS
            synth.CONFIGS[n] = SHAPES[n][0]

    def __exit__(self, *exc):
        for n in self.names:
            del synth.CONFIGS[n]


def problem(name, **kw):
    """(problem, forecast of time 0), built once per shape"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _PROBLEMS:
        with registered(name):
            p = synth.make_problem(name, **kw)
        _PROBLEMS[key] = (p, synth.forecast_at(p["forecast"], 0))
    return _PROBLEMS[key]


def chain_stage(tree):
    """the first stage from which the tree is K parallel chains (Ctx's rule restated: every node of the stages behind has one child)"""
    nps = [int(v) for v in tree["nodesPerStage"]][: int(tree["N"][0])]
    cs = len(nps) - 1
    while cs > 0 and nps[cs - 1] == nps[cs]:
        cs -= 1
    return cs


def compared(name):
    return tuple(nm for nm in NAMES if nm not in NOT_COMPARED.get(name, ()))


def duals(nodes, nx, nu):
    """the non-trivial duals of the one step (test_gpu_parity.test_stepwise_known_answer): xi, psi, updXi, updPsi"""
    rng = np.random.default_rng(7)
    nxi, nps = nodes * 2 * nx, nodes * nu
    return [rng.standard_normal(n) * 50 for n in (nxi, nps, nxi, nps)]


def oracle_of(name, precision="f64"):
    p, fc = problem(name)
    o = Oracle(p["network"], p["tree"], p["config"], precision=precision)
    o.initialise(*fc)
    return o


def frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def one_step(o, lam=0.618):
    for nm, v in zip(("xi", "psi", "updXi", "updPsi"), duals(o.nodes, o.nx, o.nu)):
        o.set(nm, v)
    o.extrapolate(lam); o.solve_step(); o.prox(); o.residual(); o.dual_update()


def step_reference(name):
    """the fp64 oracle's buffers after one step from the non-trivial duals, and its primal infeasibility; computed once, read only"""
    if name not in _STEP:
        o = oracle_of(name)
        one_step(o)
        ref = {nm: o.get(nm) for nm in NAMES}
        ref["infeasibility"] = o.primal_infeasibility()
        _STEP[name] = frozen(ref)
    return _STEP[name]


def apg_reference(name):
    """the fp64 oracle after ITERS iterations from cold: ({buffer}, history); computed once, read only"""
    if name not in _APG:
        o = oracle_of(name)
        hist = o.apg(ITERS)
        hist.setflags(write=False)
        _APG[name] = (frozen({nm: o.get(nm) for nm in NAMES}), hist)
    return _APG[name]


def dims(p):
    return int(p["network"]["nx"][0]), int(p["network"]["nu"][0]), int(p["config"]["nv"][0])


def stage_errors(got, ref, tree, nx, nu, nv):
    """{buffer: (worst per-stage error, the stage it is in)} of the buffers of `got` by stagewise.worst_by_buffer's rules"""
    from stagewise import DIM_OF, FAMILIES, SCALE_OF
    d = {"nx": nx, "nu": nu, "nv": nv, "2nx": 2 * nx}
    fam = {}
    for f in FAMILIES:
        present = [nm for nm in f if nm in ref]
        if present:
            m = max(float(np.abs(np.asarray(ref[nm])).max()) for nm in present)
            fam.update({nm: m for nm in present})
    out = {}
    for nm, g in got.items():
        e = stage_relmax(g, ref[nm], tree, d[DIM_OF[nm]], scale=ref.get(SCALE_OF.get(nm, "")), family_max=fam.get(nm, 0.0))
        out[nm] = (float(e.max()), int(e.argmax()))
    worst = worst_by_buffer(got, ref, tree, nx, nu, nv)
    assert all(out[nm][0] == worst[nm] for nm in got)          # the same measure, with the stage beside it
    return out


# ---------------------------------------------------------------------------------------------------------------
# the shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_chain_length_and_size(name):
    (_, nx, nu, _, _, N, _), L = SHAPES[name]
    p, _ = problem(name)
    assert N - chain_stage(p["tree"]) == L
    assert int(p["tree"]["nodes"][0]) <= 301
    assert L > 23, "no longer than the chains the suite already walks"


def test_the_lengths_sit_on_both_sides_of_every_batch_seam():
    ls = sorted({L for _, L in SHAPES.values()})
    for pf in (UP_PF, LIN_PF, CHAIN_PF):
        for full in range(max(pf, 24), 49, pf):
            assert full in ls and full + 1 in ls, (pf, full)
    # the Barcelona pair: N ny sizeof(double) on either side of 64 KB
    (_, nx, nu, _, _, n_fit, _), (_, _, _, _, _, n_not, _) = SHAPES["b5_33"][0], SHAPES["b5_34"][0]
    ny = 2 * nx + nu
    assert n_fit * ny * 8 <= 64 * 1024 < n_not * ny * 8 and n_not == n_fit + 1
    for name in MEDIUM:
        (_, nx, nu, _, _, _, _), _ = SHAPES[name]
        assert (2 * nx + nu) % 4 == 0                           # whole 16-byte vectors in both precisions: k_dual_stage
    (_, nx, nu, _, _, _, _), _ = SHAPES["odd_37"]
    assert (2 * nx + nu) % 2 == 1


@pytest.mark.parametrize("name", list(SHAPES))
def test_oracle_history_is_finite_and_does_not_grow(name):
    o = oracle_of(name)
    hist = o.apg(60)
    assert np.isfinite(hist).all() and all(np.isfinite(o.get(nm)).all() for nm in NAMES)
    assert np.abs(hist).max() <= 10 * abs(hist[0]), (name, hist[0], np.abs(hist).max())
    h40 = apg_reference(name)[1]
    assert np.array_equal(h40, hist[:ITERS])


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_stage_of_the_one_step_reference_carries_weight(name):
    """per buffer: the smallest per-stage maximum against the tree-wide one (>= 1e-4), and how many stages the floor decides (<= N / 8)"""
    from stagewise import DIM_OF, SCALE_OF
    p, _ = problem(name)
    nx, nu, nv = dims(p)
    d = {"nx": nx, "nu": nu, "nv": nv, "2nx": 2 * nx}
    ref = step_reference(name)
    st = node_stages(p["tree"])
    N = int(st.max()) + 1
    assert np.isfinite(ref["infeasibility"]) and ref["infeasibility"] != 0
    for nm in compared(name):
        a = np.abs(np.asarray(ref.get(SCALE_OF.get(nm, ""), ref[nm]))).reshape(len(st), d[DIM_OF[nm]]).max(axis=1)
        mag = np.zeros(N)
        np.maximum.at(mag, st, a)
        assert mag.min() >= 1e-4 * mag.max(), (name, nm, int(mag.argmin()), mag.min() / mag.max())
        assert int((mag < FLOOR * mag.max()).sum()) <= N // 8, (name, nm, mag / mag.max())


# ---------------------------------------------------------------------------------------------------------------
# the fp32 cases: the driver, the reference and the yardstick of test_gpu_apg_f32.py on two long shapes
# ---------------------------------------------------------------------------------------------------------------
# (of the L = 49 shapes s3_49 is the one on which the yardstick is sharp: on s22_49 and one_49 the fp32 oracle itself is 2.5e-5 off in x at a
#  stage whose x is small, 4 e_cpu + 32 * 2^-24 = 1e-4 there -- above FP32_TOL / 4, where the bound says little more than the suite's tolerance)
F32_SHAPES = ("m42_37", "s3_49")
_F32 = {}


def f32_case(name):
    import test_gpu_apg_f32 as apg32

    if name not in _F32:
        p, fc = problem(name)
        _F32[name] = apg32.Case(name, p, fc)
    return _F32[name]


@pytest.mark.parametrize("name", F32_SHAPES)
def test_f32_bound_says_more_than_the_suites_tolerance(name):
    """4 e_cpu + 32 * 2^-24 <= FP32_TOL / 4 for every buffer and distance of every (state, form), and no batch trips a soft threshold"""
    case = f32_case(name)
    bad = case.cap_violations()
    assert not bad, bad
    assert not any(case.tripped.values()), case.tripped


# ---------------------------------------------------------------------------------------------------------------
# the self-test: a numpy solve step whose up walk mishandles the seam between two batches
# ---------------------------------------------------------------------------------------------------------------
def numpy_solve_step(o, tree, seam=None):
    """SmpcController::solveStep restated on the oracle's own inputs (accXi, accPsi, beta, the stored blocks), the chain recursion in
    k_up_chain's form: s_i = beta_i + rho, rho = s_i + m_i with m_i = D_i xi_i + Ftil_i psi_i + Gtil q_child, batches of UP_PF stages
    counted from the leaf.  seam: None (correct), "drop_m" (the first stage of the second batch loses its m term) or "restart" (the running
    sum starts again there).  Returns {v, u, x, primalXi, primalPsi}."""
    nx, nu, nv, nodes = o.nx, o.nu, o.nv, o.nodes
    parent = np.asarray(tree["ancestor"], int).ravel()[:nodes] - 1
    st = node_stages(tree)
    N = int(st.max()) + 1
    cum = np.asarray(tree["nodesPerStageCumul"], int)
    K = int(cum[N] - cum[N - 1])
    fb = o.final_branch_node
    op = np.array([(fb - K + (i - cum[st[i]])) if fb <= cum[st[i]] else i for i in range(nodes)])
    # blocks are column-major rows x cols: reshaped [cols][rows], applied transposed
    Om, Th = o.get("Omega").reshape(-1, nv, nv), o.get("Theta").reshape(-1, nx, nv)
    Phi, D = o.get("Phi").reshape(nodes, 2 * nx, nv), o.get("D").reshape(nodes, 2 * nx, nv)
    Psi, Ft = o.get("Psi").reshape(nodes, nu, nv), o.get("Ftil").reshape(nodes, nu, nv)
    Gt = o.get("Gtil").reshape(nx, nv).T
    F = o.get("sysF").reshape(nodes, nx, 2 * nx)            # column t of F_i (2nx x nx): rows t and nx + t
    G = o.get("sysG").reshape(nodes, nu, nu)
    xi, psi, beta = o.get("accXi").reshape(nodes, 2 * nx), o.get("accPsi").reshape(nodes, nu), o.get("beta").reshape(nodes, nv)
    cs = chain_stage(tree)
    r, q, v = np.zeros((nodes, nv)), np.zeros((nodes, nx)), np.zeros((nodes, nv))
    rin, qin = np.zeros((nodes, nv)), np.zeros((nodes, nx))
    for i in range(nodes - 1, -1, -1):
        k = st[i]
        sig = beta[i] + rin[i]
        m = D[i].T @ xi[i] + Ft[i].T @ psi[i] + Gt @ qin[i]
        depth = N - 1 - k                                  # 0 at the leaf
        if seam is not None and k >= cs and depth == UP_PF:
            if seam == "drop_m":
                m = np.zeros(nv)
            elif seam == "restart":
                sig = beta[i].copy()
            else:
                raise ValueError(seam)
        v[i] = -0.5 * (Om[op[i]].T @ sig) + Th[op[i]].T @ qin[i] + Psi[i].T @ psi[i] + Phi[i].T @ xi[i]
        r[i] = sig + m
        a = np.array([F[i, t, t] * xi[i, t] + F[i, t, nx + t] * xi[i, nx + t] for t in range(nx)])
        q[i] = a + qin[i]
        if parent[i] >= 0:
            rin[parent[i]] += r[i]
            qin[parent[i]] += q[i]
    Lm, B = o.get("L").reshape(nv, nu).T, o.get("B").reshape(nu, nx).T
    uhat, e = o.get("uhat").reshape(nodes, nu), o.get("e").reshape(nodes, nx)
    u, x = np.zeros((nodes, nu)), np.zeros((nodes, nx))
    for i in range(nodes):
        w = (o.get("prevU") - o.get("prevUhat")) if parent[i] < 0 else u[parent[i]] - uhat[parent[i]]
        u[i] = uhat[i] + w + Lm @ v[i]
        x[i] = (o.get("curX") if parent[i] < 0 else x[parent[i]]) + e[i] + B @ u[i]
    pxi = np.array([[F[i, t, t] * x[i, t] for t in range(nx)] + [F[i, t, nx + t] * x[i, t] for t in range(nx)] for i in range(nodes)])
    ppsi = np.array([np.diag(G[i]) * u[i] for i in range(nodes)])
    return {"v": v.ravel(), "u": u.ravel(), "x": x.ravel(), "primalXi": pxi.ravel(), "primalPsi": ppsi.ravel()}


def walked(name, cfg=None):
    """(oracle behind extrapolate + solve_step from the non-trivial duals, tree, the oracle's own v, u, x, primalXi, primalPsi)"""
    if cfg is not None:
        SHAPES[name] = cfg
    try:
        p, fc = problem(name)
    finally:
        if cfg is not None:
            del SHAPES[name]
    o = Oracle(p["network"], p["tree"], p["config"])
    o.initialise(*fc)
    for nm, val in zip(("xi", "psi", "updXi", "updPsi"), duals(o.nodes, o.nx, o.nu)):
        o.set(nm, val)
    o.extrapolate(0.618); o.solve_step()
    return o, p, {nm: o.get(nm) for nm in ("v", "u", "x", "primalXi", "primalPsi")}


@pytest.mark.parametrize("seam", ["drop_m", "restart"])
def test_a_walk_that_mishandles_the_seam_is_refused(seam):
    o, p, ref = walked("s3_25")
    nx, nu, nv = dims(p)
    assert SHAPES["s3_25"][1] == UP_PF + 1
    good = stage_errors(numpy_solve_step(o, p["tree"]), ref, p["tree"], nx, nu, nv)
    assert max(e for e, _ in good.values()) <= REL_TOL, good                     # the restatement IS the solve step
    bad = stage_errors(numpy_solve_step(o, p["tree"], seam), ref, p["tree"], nx, nu, nv)
    print("\n%s at L = 25: %s" % (seam, {k: "%.1e (stage %d)" % v for k, v in bad.items()}))
    assert all(e > 1e4 * REL_TOL for e, _ in bad.values()), bad                   # refused in every buffer, by orders of magnitude
    # the mistake sits in the chain's top stage (stage 1 of this tree): v is wrong there or above it, nowhere below
    top = chain_stage(p["tree"])
    ev = stage_relmax(numpy_solve_step(o, p["tree"], seam)["v"], ref["v"], p["tree"], nv)
    assert (ev[top + 1:] <= REL_TOL).all() and ev[:top + 1].max() > 1e4 * REL_TOL, ev
    # the same mistake on the 23 stages the suite's longest chain has: the second batch does not exist, nothing changes
    cfg = SHAPES["s3_25"][0]
    o23, p23, ref23 = walked("s3_23", (cfg[:5] + (24, [3]), 23))
    assert 24 - chain_stage(p23["tree"]) == 23
    a, b = numpy_solve_step(o23, p23["tree"]), numpy_solve_step(o23, p23["tree"], seam)
    for nm in a:
        assert np.array_equal(a[nm], b[nm]), nm
    assert max(e for e, _ in stage_errors(a, ref23, p23["tree"], nx, nu, nv).values()) <= REL_TOL
