"""rn_estimate_lipschitz in numpy (test infrastructure, like plan_oracle.py and bands_oracle.py): no library, no oracle import.

The estimate is a power iteration over the dual Hessian M = K H^-1 K', K = [F Tx; G Tu], H = 2 Td' (p (x) W) Td in the notation of
first_principles.py.  With w_0 = the start vector, for k = 1 .. iterations:

    s = <w, w> ;  t = <v, w> (k >= 2) ;  v = w / sqrt(s) ;  w = apply(v)

and record j (j = 1 .. iterations) is formed from the w of application j:  NORM = sqrt(s) <= lambda_max,  RAYLEIGH = |t| <= NORM,
RESIDUAL = sqrt(max(s - t^2, 0)) / sqrt(s).  What is restated here: the hashed start vector (bit for bit), the loop over any
apply(xi, psi) -> (xi, psi) callable, the three record columns, and the dense M of the definition.  `mistake` holds the names of deliberate
mistakes (MISTAKES) for the negative controls of tests/test_lipschitz_oracle.py."""
import numpy as np

NORM, RAYLEIGH, RESIDUAL = 0, 1, 2
MISTAKES = ("normalise_by_s", "skip_crown", "local_start", "history_off_by_one", "t_unnormalised")
_M64 = (1 << 64) - 1


def hash_value(seed, i):
    """element i of the library's start vector: splitmix64's finaliser of seed + (i + 1) * golden, mapped to [-1, 1)"""
    x = (int(seed) + (int(i) + 1) * 0x9E3779B97F4A7C15) & _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return float(x >> 11) * 2.0 ** -52 - 1.0


def hash_start(nodes, nx, nu, seed=0, global_nodes=None, dtype=np.float64):
    """(xi [nodes, 2nx], psi [nodes, nu]) of the library's own start; global_nodes: the index of every (local) node in the whole tree"""
    ny = 2 * nx + nu
    g = np.arange(nodes, dtype=np.uint64) if global_nodes is None else np.asarray(global_nodes).astype(np.uint64)
    i = g[:, None] * np.uint64(ny) + np.arange(ny, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        x = np.uint64(int(seed) & _M64) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    y = ((x >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0).astype(dtype).astype(np.float64)
    return y[:, :2 * nx].copy(), y[:, 2 * nx:].copy()


def power_loop(apply, xi, psi, iterations, tol=0.0, check_every=20, mistake=(), first=0, round_to=None):
    """history [iterations run][3] of the loop over apply.  tol > 0: stops at the first multiple of check_every whose record has
    RESIDUAL <= tol.  first: rows of the start below which the elements do not COUNT in s and t (a shard's replicated crown on ranks
    other than 0; the mistake skip_crown applies it where it must not).  round_to: v and w rounded to that type after every step."""
    mistake = set(mistake)
    assert mistake <= set(MISTAKES), mistake
    rnd = (lambda a: a) if round_to is None else (lambda a: a.astype(round_to).astype(np.float64))
    w = np.hstack([np.asarray(xi, float), np.asarray(psi, float)])
    n2 = np.asarray(xi).shape[1]
    w = rnd(w)
    v = None
    hist = np.zeros((iterations, 3))

    def dots(w, v):
        lo = first
        s = float((w[lo:] ** 2).sum())
        t = 0.0 if v is None else float((v[lo:] * w[lo:]).sum())
        return s, t

    def record(row, s, t):
        if "history_off_by_one" in mistake:
            row += 1
        if 0 <= row < iterations:
            hist[row] = (np.sqrt(s), abs(t), np.sqrt(max(s - t * t, 0.0)) / np.sqrt(s))

    done = 0
    for k in range(1, iterations + 1):
        s, t = dots(w, v)
        if k >= 2:
            record(k - 2, s, t)
        vprev = w
        v = rnd(w / (s if "normalise_by_s" in mistake else np.sqrt(s)))
        a, b = apply(v[:, :n2], v[:, n2:])
        w = rnd(np.hstack([a, b]))
        if "t_unnormalised" in mistake:
            v = vprev
        done = k
        if tol > 0 and k % check_every == 0 and k < iterations:
            s, t = dots(w, v)
            record(k - 1, s, t)
            if hist[k - 1, RESIDUAL] <= tol:
                return hist[:done]
    s, t = dots(w, v)
    record(done - 1, s, t)
    return hist[:done]


def dense_M(model):
    """M = K H^-1 K' of a first_principles.Model, rows and columns in the y layout ([node][xi (2nx) | psi (nu)]), symmetrised"""
    Td, Tu, Tx, pw, H = model._matrices()
    nodes, nx, nu = model.nodes, model.nx, model.nu
    ny = 2 * nx + nu
    K = np.zeros((nodes * ny, Tu.shape[1]))
    for i in range(nodes):
        K[i * ny: i * ny + nx] = model.fx[i][:, None] * Tx[i * nx:(i + 1) * nx]
        K[i * ny + nx: i * ny + 2 * nx] = model.fs[i][:, None] * Tx[i * nx:(i + 1) * nx]
        K[i * ny + 2 * nx: (i + 1) * ny] = model.g[i][:, None] * Tu[i * nu:(i + 1) * nu]
    M = K @ np.linalg.solve(H, K.T)
    return 0.5 * (M + M.T)


def dense_apply(M, nodes, nx, nu):
    ny = 2 * nx + nu

    def apply(xi, psi):
        y = (M @ np.hstack([xi, psi]).ravel()).reshape(nodes, ny)
        return y[:, :2 * nx], y[:, 2 * nx:]
    return apply
