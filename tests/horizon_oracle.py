"""A receding-horizon loop on the CPU oracle, one record per control step (test infrastructure, like restart_oracle.py and stagewise.py).

run_horizon drives ONE oracle through T control steps around the oracle's own plant (move_forward, the bookkeeping of
test_gpu_closed_loop._oracle_loop): at step t it installs (x_t, u_{t-1}, d_{t-1}), eliminates with the step's forecast and solves for the
step's own iteration count -- cold (oracle.apg) or, from the second step on, warm: xi := updXi, psi := updPsi, then the plain loop from
theta = {1, 1} (the recipe of test_warm_start_against_the_oracle_started_from_the_same_duals).  Every record carries what the step was
given and what it left behind, so that a context of the library can be handed the SAME (x_t, u_{t-1}, d_{t-1}) at every step: both sides
then solve the same problem at every step, and a step's error is that step's own.

The iteration counts are part of the design: COUNTS covers an odd count above one batch, exactly one batch, an even number of batches plus
an odd tail, less than one batch and a single iteration (the library's shortest optimistic batch is BATCH = 16 iterations), so that what
a step inherits -- which of the two rotating dual buffers holds y+, whether the accelerated dual is current, where in a batch the count
ended -- has seen both parities and both batch positions."""
import numpy as np

BATCH = 16                          # RN_OPT_LOCAL_MIN (csrc/rapidnet_capi.hip)
COUNTS = (23, 16, 37, 5, 1)
NAMES = ("x", "u", "v", "xi", "psi", "accXi", "accPsi", "updXi", "updPsi", "primalXi", "primalPsi", "dualXi", "dualPsi", "resXi", "resPsi")
AFFINE = ("uhat", "e", "beta", "alpha")
DUALS = ("xi", "psi", "updXi", "updPsi")
CORRUPTIONS = ("wrong_buffer", "stale_theta", "stale_affine")


def steps_of(forecast, forecast_at, counts=COUNTS):
    """[(dh, ah, n)] of the forecasts of time instants 0 .. len(counts) - 1"""
    return [forecast_at(forecast, t) + (n,) for t, n in enumerate(counts)]


def keep_duals(o):
    """the warm start: y := y+, y+ kept"""
    o.set("xi", o.get("updXi"))
    o.set("psi", o.get("updPsi"))


def transplant(old, new):
    """the duals of `old` into `new` (an oracle of other tree data or bounds that takes over between two steps)"""
    for nm in DUALS:
        new.set(nm, old.get(nm))
    return new


def solve(o, n, theta=None, tol=0.0, every=0, dists=None):
    """n iterations one at a time (bit for bit oracle.apg / apg_continue(n): theta travels unchanged), from theta (None: after apg_reset);
    with tol > 0 the loop ends behind the first batch of `every` iterations whose last residual is <= tol.  dists: a list that receives
    the two prox distances of every iteration.  Returns (history, theta)."""
    if theta is None:
        o.apg_reset()
        theta = [1.0, 1.0]
    hist = []
    while len(hist) < n:
        theta = list(o.apg_continue(1, theta))
        hist.append(o.primal_infeasibility())
        if dists is not None:
            dists.append(o.dist())
        if tol > 0 and len(hist) % every == 0 and hist[-1] <= tol:
            break
    return np.array(hist), theta


def run_horizon(o, steps, warm, plant_modes=None, before_step=None, tol=0.0, every=20, corrupt=None, affine=False, track_dist=False):
    """o: an oracle after factor_step; steps: [(dh, ah, n_iterations)]; plant_modes: one per step (default 0, 1, 0, ...).
    before_step(t, o): called before step t is set up; may return another oracle (after ITS factor step), which then takes over -- with
    the duals of the old one when the step is warm.
    tol, every: the stop tolerance of rn_set_stop_tolerance, n is then the step's maximum.
    corrupt: one of CORRUPTIONS, the sharpness self-tests' stand-ins for a library that is wrong from the second step on.
    track_dist: every record carries dists, the two prox distances of every iteration of the step.
    Returns one dict per step: x, prevU, prevD (what the step was given), dh, ah, n (iterations run), hist, u_raw, u (projected on the
    root's bounds), bufs (a copy of every buffer of NAMES; affine=True: of AFFINE as well, as they stood when the solve began)."""
    assert corrupt is None or corrupt in CORRUPTIONS
    T = len(steps)
    plant_modes = [t % 2 for t in range(T)] if plant_modes is None else list(plant_modes)
    c = o.config
    x, u, d = (np.asarray(c[k], float).ravel().copy() for k in ("currentX", "prevU", "prevDemand"))
    out, theta, prev_n = [], None, 0
    for t, (dh, ah, n) in enumerate(steps):
        if before_step is not None:
            new = before_step(t, o)
            if new is not None and new is not o:
                o = transplant(o, new) if warm and t > 0 else new
        o.update_state_control(x, u, d)
        if not (corrupt == "stale_affine" and t > 0):
            o.eliminate(dh, ah)
        aff = {nm: o.get(nm) for nm in AFFINE} if affine else {}
        dists = [] if track_dist else None
        if warm and t > 0:
            if corrupt == "wrong_buffer" and prev_n % 2 == 1:      # the other of the two rotating buffers taken for y+
                o.set("updXi", o.get("xi")); o.set("updPsi", o.get("psi"))
            keep_duals(o)
            hist, theta = solve(o, n, theta if corrupt == "stale_theta" else [1.0, 1.0], tol, every, dists)
        elif tol > 0 or track_dist or corrupt == "stale_theta":     # (the corrupted second step wants the first one's theta)
            hist, theta = solve(o, n, None, tol, every, dists)
        else:
            hist = o.apg(n).copy()
        bufs = {nm: o.get(nm) for nm in NAMES}
        bufs.update(aff)
        u_raw = bufs["u"][: o.nu].copy()
        rec = dict(t=t, x=x, prevU=u, prevD=d, dh=dh, ah=ah, n=len(hist), hist=hist, u_raw=u_raw,
                   u=np.clip(u_raw, o.get("umin")[: o.nu], o.get("umax")[: o.nu]), bufs=bufs, plant_mode=plant_modes[t], dists=dists)
        out.append(rec)
        prev_n = len(hist)
        o.set("controlAction", rec["u"])                            # what oracle_control_action(project) leaves for the plant
        x, u, d = o.move_forward(dh, ah, weight_economical=1.0, plant_mode=plant_modes[t])
    for rec in out:
        for a in list(rec["bufs"].values()) + [rec["x"], rec["prevU"], rec["prevD"], rec["hist"], rec["u_raw"], rec["u"]]:
            a.setflags(write=False)
    return out


# ---- the checks of one step, shared by the GPU tests and the sharpness self-tests -------------------------------------------------------
def relmax(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def step_errors(got, rec, tree, nx, nu, nv):
    """{"u_raw", "u", "hist", every buffer of got["bufs"]: its worst per-stage error} of one step against the oracle's record.
    got: dict(u_raw, u, hist, bufs) -- any of them may be missing"""
    from stagewise import worst_by_buffer

    out = {}
    for k in ("u_raw", "u"):
        if got.get(k) is not None:
            out[k] = relmax(got[k], rec[k])
    if got.get("hist") is not None:
        h = np.asarray(got["hist"], float)
        assert h.shape == rec["hist"].shape, (h.shape, rec["hist"].shape)
        out["hist"] = float(np.abs(h - rec["hist"]).max() / max(np.abs(rec["hist"]).max(), 1e-300))
    if got.get("bufs"):
        out.update(worst_by_buffer(got["bufs"], rec["bufs"], tree, nx, nu, nv))
    return out


def old_step_errors(got, rec):
    """what the suite checked of a control step behind a warm start before (test_warm_start_against_the_oracle_started_from_the_same_duals):
    the root control and the whole-buffer relmax of x, updXi, updPsi, xi"""
    out = {"u_raw": relmax(got["u_raw"], rec["u_raw"])}
    for nm in ("x", "updXi", "updPsi", "xi"):
        out[nm] = relmax(got["bufs"][nm], rec["bufs"][nm])
    return out
