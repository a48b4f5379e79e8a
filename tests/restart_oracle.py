"""The gradient restart of the APG momentum (rn_set_restart) restated on the CPU oracle, for the tests and tools/ab_restart.py.

The oracle has no restart of its own and stays as it is: the loop below drives it one iteration at a time through Oracle.apg_continue with
theta threaded by the caller, evaluates g = <w_k - y_{k+1}, y_{k+1} - y_k> in numpy at every batch end and, when g > 0, restarts by hand:
xi := updXi, psi := updPsi, theta = {1, 1} (the next extrapolation then gives w = y+, whatever xi held)."""
import numpy as np


def gradient_test(w, yp, y):
    """(g, na2, nb2, sum |terms of g|) of the vectors given (any layout, the same for all three), in fp64; the terms of na2 and nb2 are
    squares, so na2 and nb2 are themselves the sums of their terms' magnitudes"""
    w, yp, y = (np.asarray(v, dtype=np.float64).ravel() for v in (w, yp, y))
    d1, d2 = w - yp, yp - y
    t = d1 * d2
    return float(t.sum()), float((d1 * d1).sum()), float((d2 * d2).sum()), float(np.abs(t).sum())


def oracle_vectors(o):
    """(w_k, y_{k+1}, y_k) of the oracle behind an iteration: xi part, then psi part"""
    return tuple(np.concatenate([o.get(a), o.get(b)]) for a, b in (("accXi", "accPsi"), ("updXi", "updPsi"), ("xi", "psi")))


def residual_norm(o):
    return float(np.sqrt((o.get("resXi") ** 2).sum() + (o.get("resPsi") ** 2).sum()))


def restart_loop(o, iterations, every=20, restart=True, tol=0.0, at_batch_end=None, theta=None, reset=True):
    """The loop of rn_apg_solve under RN_RESTART_GRADIENT on an initialised oracle: batches of `every` iterations; at a batch end first the
    tolerance (the residual of the batch's last iteration <= tol > 0 ends the solve, without a restart), then the gradient test.
    at_batch_end(done, o) is called BEHIND the restart of a boundary (what the library's getters then show).  Returns a dict: fires (iteration
    counts at which the momentum was restarted), hist (vecPrimalInfs), norms (||(resXi, resPsi)|| at every batch end), tests ((g, na2, nb2,
    sum |terms|) of every batch end that was tested), iterations."""
    if reset:
        o.apg_reset()
    theta = [1.0, 1.0] if theta is None else list(theta)
    out = dict(fires=[], hist=[], norms=[], tests=[], iterations=0)
    done = 0
    while done < iterations:
        n = min(every, iterations - done)
        for _ in range(n):
            theta = list(o.apg_continue(1, theta))
            out["hist"].append(o.primal_infeasibility())
        done += n
        out["iterations"] = done
        out["norms"].append(residual_norm(o))
        if tol > 0 and out["hist"][-1] <= tol:
            if at_batch_end:
                at_batch_end(done, o)
            break
        if restart:
            t = gradient_test(*oracle_vectors(o))
            out["tests"].append(t)
            if t[0] > 0:
                o.set("xi", o.get("updXi"))
                o.set("psi", o.get("updPsi"))
                theta = [1.0, 1.0]
                out["fires"].append(done)
        if at_batch_end:
            at_batch_end(done, o)
    out["hist"] = np.array(out["hist"])
    return out


def iterations_to(norms, every, levels=(1e-2, 1e-3, 1e-4)):
    """first iteration count (a batch end) at which the residual norm is <= level x its value after the first batch, or None"""
    r = np.asarray(norms) / norms[0]
    return [next(((i + 1) * every for i, v in enumerate(r) if v <= lv), None) for lv in levels]


def cosine(t):
    g, na2, nb2 = t[0], t[1], t[2]
    return g / np.sqrt(na2 * nb2) if na2 > 0 and nb2 > 0 else 0.0
