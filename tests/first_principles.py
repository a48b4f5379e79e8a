"""The problem's definition in numpy (test infrastructure, like numpy_engine.py and stagewise.py): no oracle, no library import.

Every parity test of the suite ends at the CPU oracle, a restatement of the reference's sweep.  This module restates nothing: it builds the
Lagrangian of SURVEY.md sections 3.4-3.5 from the JSON data alone and asks what its minimiser is.  Nothing derived by the factor step (Omega,
Phi, Psi, Theta, D, Ftil, beta, ...) is used.  The sweep assumes matA = I (the tanks integrate); Model asserts it.

    d_i     = dhat_stage(i) + errDemand_i                              (demand uncertainty off: every errDemand_i = 0, as the oracle does;
                                                                        the reference zeroes a prefix only)
    alpha_i = w_e (ahat_stage(i) + errPrice_i + alpha1)
    uhat_i  = Lhat d_i
    u_i     = uhat_i + L v_i + (u_anc(i) - uhat_anc(i)),               the root with prevU - Lhat prevDemand
    x_i     = x_anc(i) + Gd d_i + B u_i,                               the root with currentX
    Phi(V)  = sum_i p_i [du_i' W du_i + alpha_i' u_i] + sum_i xi_i' F_i x_i + psi_i' G_i u_i,      du_i = u_i - u_anc(i), du_0 = u_0 - prevU
    F_i     = sqrt(p_i) [diag(d_x); diag(d_xs)],  G_i = sqrt(p_i) diag(d_u),   stage k of matDiagPrecnd = (d_u | d_x | d_xs)

Phi is strictly convex in V = (v_i) because L'WL is positive definite, so a feasible and stationary (x, u, v) is THE argmin.
Matrices are column-major.  `perturb` holds the names of deliberate mistakes (PERTURBATIONS) for the negative controls of
tests/test_first_principles.py: a model with a mistake must be refused by the oracle, or the data do not exercise that datum."""
import numpy as np

from stagewise import stage_relmax

DENSE_LIMIT = 1500      # nodes * nv above which argmin refuses (a dense solve of `medium`, 6 560, takes ~50 s)
PERTURBATIONS = ("p_in_F", "p_in_G", "swap_dx_dxs", "drop_child_term", "drop_Gd", "drop_root_prev", "alpha_without_errPrice", "shared_distance")


def _s(d, k):
    v = d[k]
    return v[0] if isinstance(v, (list, tuple, np.ndarray)) else v


def _mat(a, rows, cols):
    return np.asarray(a, float).ravel().reshape(cols, rows).T.copy()


class Model:
    def __init__(self, network, tree, config, forecast, currentX=None, prevU=None, prevDemand=None, weightEconomical=1.0,
                 demandUncertainty=True, priceUncertainty=True, probNode=None, errorDemandNode=None, errorPriceNode=None, bounds=None,
                 penaltyStateX=None, penaltySafetyX=None, stepSize=None, perturb=(), perturb_node=None):
        """forecast: (dhat [N][nd], ahat [N][nu]).  bounds: None (the network's, shared) or a dict with `granularity` "shared" | "stage" | "node"
        and any of xmin, xmax, xsafe [rows][nx], umin, umax [rows][nu] (physical values; a missing one is the network's).
        perturb_node: the node at which drop_child_term (a branching node) / drop_Gd act."""
        assert set(perturb) <= set(PERTURBATIONS), perturb
        self.perturb = set(perturb)
        nx, nu, nd = (int(_s(network, k)) for k in ("nx", "nu", "nd"))
        nv, N, nodes = int(_s(config, "nv")), int(_s(tree, "N")), int(_s(tree, "nodes"))
        self.nx, self.nu, self.nd, self.nv, self.N, self.nodes = nx, nu, nd, nv, N, nodes
        assert np.array_equal(_mat(network["matA"], nx, nx), np.eye(nx)), "the sweep assumes matA = I"
        self.B, self.Gd = _mat(network["matB"], nx, nu), _mat(network["matGd"], nx, nd)
        self.L, self.Lhat, self.W = _mat(config["matL"], nu, nv), _mat(config["matLhat"], nu, nd), _mat(config["costW"], nu, nu)
        assert np.allclose(self.W, self.W.T, rtol=1e-14, atol=0), "the gradient 2 W du needs a symmetric W"
        self.stage = np.asarray(tree["stages"], int).ravel()[:nodes]
        self.anc = np.asarray(tree["ancestor"], int).ravel()[:nodes] - 1          # -1 at the root
        assert self.anc[0] == -1 and (self.anc[1:] < np.arange(1, nodes)).all() and (self.anc[1:] >= 0).all()
        self.kids = [[] for _ in range(nodes)]
        for c in range(1, nodes):
            self.kids[self.anc[c]].append(c)
        self.p = np.asarray(tree["probNode"] if probNode is None else probNode, float).ravel()[:nodes]
        diag = np.asarray(config["matDiagPrecnd"], float).reshape(N, 2 * nx + nu)
        d_u, d_x, d_xs = diag[:, :nu], diag[:, nu:nu + nx], diag[:, nu + nx:]
        if "swap_dx_dxs" in self.perturb:
            d_x, d_xs = d_xs, d_x
        sp = np.sqrt(self.p)[:, None]
        self.fx = (self.p[:, None] if "p_in_F" in self.perturb else sp) * d_x[self.stage]        # F_i = [diag(fx_i); diag(fs_i)]
        self.fs = (self.p[:, None] if "p_in_F" in self.perturb else sp) * d_xs[self.stage]
        self.g = (self.p[:, None] if "p_in_G" in self.perturb else sp) * d_u[self.stage]         # G_i = diag(g_i)
        self.x0 = np.asarray(config["currentX"] if currentX is None else currentX, float).ravel()
        self.prevU = np.asarray(config["prevU"] if prevU is None else prevU, float).ravel()
        self.prevD = np.asarray(config["prevDemand"] if prevDemand is None else prevDemand, float).ravel()
        dhat, ahat = np.asarray(forecast[0], float).reshape(N, nd), np.asarray(forecast[1], float).reshape(N, nu)
        errD = np.asarray(tree["errorDemandNode"] if errorDemandNode is None else errorDemandNode, float).reshape(nodes, nd)
        errA = np.asarray(tree["errorPriceNode"] if errorPriceNode is None else errorPriceNode, float).reshape(nodes, nu)
        if not demandUncertainty:
            errD = np.zeros_like(errD)
        if not priceUncertainty or "alpha_without_errPrice" in self.perturb:
            errA = np.zeros_like(errA)
        self.d = dhat[self.stage] + errD
        self.alpha = float(weightEconomical) * (ahat[self.stage] + errA + np.asarray(network["costAlpha1"], float).ravel())
        self.uhat = self.d @ self.Lhat.T
        self.e = self.d @ self.Gd.T                                                 # Gd d_i
        branching = [i for i in range(nodes) if len(self.kids[i]) > 1]
        self.perturb_node = (branching[-1] if "drop_child_term" in self.perturb else nodes // 2) if perturb_node is None else int(perturb_node)
        if "drop_Gd" in self.perturb:
            self.e[self.perturb_node] = 0.0
        # du_i = L v_i + c_i
        self.c = np.empty((nodes, nu))
        self.c[0] = self.uhat[0] - (0.0 if "drop_root_prev" in self.perturb else self.Lhat @ self.prevD)
        self.c[1:] = self.uhat[1:] - self.uhat[self.anc[1:]]
        self.u_root = np.zeros(nu) if "drop_root_prev" in self.perturb else self.prevU    # what the root's u is an increment of
        self.step = float(_s(config, "stepSize") if stepSize is None else stepSize)
        self.gammaX = float(_s(config, "penaltyStateX") if penaltyStateX is None else penaltyStateX)
        self.gammaS = float(_s(config, "penaltySafetyX") if penaltySafetyX is None else penaltySafetyX)
        self._bounds(network, bounds or {})
        self._dense = None
        self.tree = {"stages": self.stage, "nodes": [nodes]}                       # what stagewise.stage_relmax reads

    def _bounds(self, network, b):
        rows_of = {"shared": lambda: np.zeros(self.nodes, int), "stage": lambda: self.stage, "node": lambda: np.arange(self.nodes)}
        row = rows_of[b.get("granularity", "shared")]()
        def phys(key, net_key, dim):
            a = np.asarray(b[key] if b.get(key) is not None else network[net_key], float).reshape(-1, dim)
            return a[row] if a.shape[0] > 1 else np.repeat(a, self.nodes, axis=0)
        self.xmin, self.xmax = phys("xmin", "vecXmin", self.nx) * self.fx, phys("xmax", "vecXmax", self.nx) * self.fx
        self.xs = phys("xsafe", "vecXsafe", self.nx) * self.fs
        self.umin, self.umax = phys("umin", "vecUmin", self.nu) * self.g, phys("umax", "vecUmax", self.nu) * self.g

    # ---- the tree recursion ------------------------------------------------------------------------------------------------------------
    def rollout(self, v, homogeneous=False):
        """(x, u, du) from v by the recursion of the definition; homogeneous: all affine data (d, prevU, prevDemand, currentX) zero"""
        v = np.asarray(v, float).reshape(self.nodes, self.nv)
        du = v @ self.L.T + (0.0 if homogeneous else self.c)
        u, x = np.empty((self.nodes, self.nu)), np.empty((self.nodes, self.nx))
        for i in range(self.nodes):
            a = self.anc[i]
            u[i] = du[i] + ((0.0 if homogeneous else self.u_root) if a < 0 else u[a])
            x[i] = ((0.0 if homogeneous else self.x0) if a < 0 else x[a]) + (0.0 if homogeneous else self.e[i]) + self.B @ u[i]
        return x, u, du

    def _du_cost(self, u, homogeneous=False):
        """du as the COST sees it (u_i - u_anc(i), the root against prevU), from u itself"""
        u = np.asarray(u, float).reshape(self.nodes, self.nu)
        du = u.copy()
        du[1:] -= u[self.anc[1:]]
        if not homogeneous:
            du[0] -= self.u_root
        return du

    def Fx(self, x):
        x = np.asarray(x, float).reshape(self.nodes, self.nx)
        return np.concatenate([self.fx * x, self.fs * x], axis=1)

    def Ft(self, xi):
        xi = np.asarray(xi, float).reshape(self.nodes, 2 * self.nx)
        return self.fx * xi[:, :self.nx] + self.fs * xi[:, self.nx:]

    # ---- argmin by one dense solve -----------------------------------------------------------------------------------------------------
    def _matrices(self):
        """u = u(0) + Tu V, x = x(0) + Tx V, du = c + Td V as dense matrices (node-major), and the Hessian 2 Td' (p W) Td"""
        if self._dense is None:
            n = self.nodes * self.nv
            if n > DENSE_LIMIT:
                raise ValueError("argmin: nodes * nv = %d > %d: use residuals()" % (n, DENSE_LIMIT))
            path = np.zeros((self.nodes, self.nodes))                   # path[i, j] = 1: j is on the way from the root to i (i included)
            for i in range(self.nodes):
                if self.anc[i] >= 0:
                    path[i] = path[self.anc[i]]
                path[i, i] = 1.0
            Td = np.kron(np.eye(self.nodes), self.L)
            Tu = np.kron(path, self.L)
            Tx = np.kron(path, self.B) @ Tu
            pw = np.kron(np.diag(self.p), self.W)
            H = 2.0 * Td.T @ pw @ Td
            self._dense = (Td, Tu, Tx, pw, 0.5 * (H + H.T))
        return self._dense

    def _linear_term(self, xi, psi, homogeneous):
        Td, Tu, Tx, pw, _ = self._matrices()
        psi = np.asarray(psi, float).reshape(self.nodes, self.nu)
        g = Tu.T @ (self.g * psi).ravel() + Tx.T @ self.Ft(xi).ravel()
        if not homogeneous:
            g = g + 2.0 * Td.T @ (pw @ self.c.ravel()) + Tu.T @ (self.p[:, None] * self.alpha).ravel()
        return g

    def _solve(self, g):
        H = self._matrices()[4]
        V = np.linalg.solve(H, -g)
        r = (-g.astype(np.longdouble) - (H.astype(np.longdouble) @ V.astype(np.longdouble))).astype(float)   # residual in extended precision
        dV = np.linalg.solve(H, r)
        return V + dV, float(np.abs(dV).max() / max(np.abs(V).max(), 1e-300))

    def argmin(self, xi, psi, homogeneous=False):
        """dict(x, u, v, primalXi, primalPsi, correction): the minimiser of Phi at the dual (xi, psi); correction = the refinement step / |V|"""
        if "drop_child_term" in self.perturb:
            raise ValueError("drop_child_term perturbs the stationarity sum, not the data: it is judged by residuals()")
        V, corr = self._solve(self._linear_term(xi, psi, homogeneous))
        x, u, _ = self.rollout(V, homogeneous)
        return {"x": x.ravel(), "u": u.ravel(), "v": V, "primalXi": self.Fx(x).ravel(), "primalPsi": (self.g * u).ravel(), "correction": corr}

    def hessian_direction(self, dXi, dPsi):
        """dict(x, u, v, primalXi, primalPsi, correction): argmin(w + d) - argmin(w), the linear part of the argmin map"""
        return self.argmin(dXi, dPsi, homogeneous=True)

    # ---- residuals: any size, no solve ---------------------------------------------------------------------------------------------------
    def gradient(self, xi, psi, u, homogeneous=False):
        """(dPhi/dv [nodes][nv], the sum of the absolute values of each component's terms) by two leaf-to-root accumulations:
        dPhi/dv_i = L' sum_{j in subtree(i)} [2 p_j W du_j - sum_{c child of j} 2 p_c W du_c + p_j alpha_j + G_j' psi_j + B' sum_{m in subtree(j)} F_m' xi_m]"""
        psi = np.asarray(psi, float).reshape(self.nodes, self.nu)
        du = self._du_cost(u, homogeneous)
        wdu = 2.0 * self.p[:, None] * (du @ self.W.T)
        q = self.Ft(xi)                                                 # first accumulation: q_j = sum_{m in subtree(j)} F_m' xi_m
        qa = np.abs(q)
        for i in range(self.nodes - 1, 0, -1):
            q[self.anc[i]] += q[i]
            qa[self.anc[i]] += qa[i]
        lin = np.zeros_like(wdu) if homogeneous else self.p[:, None] * self.alpha
        t = wdu + lin + self.g * psi + q @ self.B
        ta = np.abs(wdu) + np.abs(lin) + np.abs(self.g * psi) + qa @ np.abs(self.B)
        for c in range(1, self.nodes):
            if "drop_child_term" in self.perturb and self.anc[c] == self.perturb_node:
                continue
            t[self.anc[c]] -= wdu[c]
            ta[self.anc[c]] += np.abs(wdu[c])
        for i in range(self.nodes - 1, 0, -1):                          # second accumulation: over subtree(i)
            t[self.anc[i]] += t[i]
            ta[self.anc[i]] += ta[i]
        return t @ self.L, ta @ np.abs(self.L)

    def _per_stage(self, err_node):
        out = np.zeros(self.N)
        np.maximum.at(out, self.stage, err_node)
        return out

    def residuals(self, xi, psi, x, u, v, homogeneous=False):
        """dict of per-stage arrays: feas_u, feas_x (u and x recomputed from v by the tree recursion, relative to the stage's own maximum)
        and stationarity (every component of dPhi/dv over the sum of the absolute values of its terms, worst of the stage)"""
        xr, ur, _ = self.rollout(v, homogeneous)
        out = {"feas_u": stage_relmax(u, ur, self.tree, self.nu, floor=0.0), "feas_x": stage_relmax(x, xr, self.tree, self.nx, floor=0.0)}
        g, scale = self.gradient(xi, psi, u, homogeneous)
        assert np.isfinite(g).all() and (scale > 0).all()
        out["stationarity"] = self._per_stage((np.abs(g) / scale).max(axis=1))
        return out

    # ---- prox, value -----------------------------------------------------------------------------------------------------------------------
    def prox(self, primalXi, primalPsi, wXi, wPsi):
        """dict(dualXi, dualPsi (z), distX, distS (tree-global, one per xi half), resXi, resPsi (Hx - z), updXi, updPsi (y+ = w + lambda (Hx - z)))"""
        nx, lam = self.nx, self.step
        hx, hp = np.asarray(primalXi, float).reshape(self.nodes, 2 * nx), np.asarray(primalPsi, float).reshape(self.nodes, self.nu)
        wx, wp = np.asarray(wXi, float).reshape(self.nodes, 2 * nx), np.asarray(wPsi, float).reshape(self.nodes, self.nu)
        t, tp = hx + wx / lam, hp + wp / lam
        zb, zs = np.clip(t[:, :nx], self.xmin, self.xmax), np.maximum(t[:, nx:], self.xs)          # the safety half has no upper bound
        db, ds = t[:, :nx] - zb, t[:, nx:] - zs
        distX, distS = float(np.sqrt((db * db).sum())), float(np.sqrt((ds * ds).sum()))
        if "shared_distance" in self.perturb:
            distX = distS = float(np.sqrt(distX ** 2 + distS ** 2))
        if distX > self.gammaX / lam:                                                              # prox of gamma * dist(., C)
            zb = zb + (1.0 - self.gammaX / (lam * distX)) * db
        if distS > self.gammaS / lam:
            zs = zs + (1.0 - self.gammaS / (lam * distS)) * ds
        z, zp = np.concatenate([zb, zs], axis=1), np.clip(tp, self.umin, self.umax)
        return {"dualXi": z.ravel(), "dualPsi": zp.ravel(), "distX": distX, "distS": distS, "resXi": (hx - z).ravel(), "resPsi": (hp - zp).ravel(),
                "updXi": (wx + lam * (hx - z)).ravel(), "updPsi": (wp + lam * (hp - zp)).ravel()}

    def primal_value(self, u):
        """sum_i p_i (du_i' W du_i + alpha_i' u_i): the primal terms of computeValueFbe"""
        u = np.asarray(u, float).reshape(self.nodes, self.nu)
        du = self._du_cost(u)
        return float((self.p * ((du @ self.W.T) * du).sum(axis=1)).sum() + (self.p[:, None] * self.alpha * u).sum())

    # ---- a whole state ---------------------------------------------------------------------------------------------------------------------
    def check_state(self, get, prox=True, scales="stage"):
        """get(name) -> the buffer `name` of a context or of the oracle in global node order (x u v accXi accPsi primalXi primalPsi, and for the
        prox chain dualXi dualPsi resXi resPsi updXi updPsi).  Checks at the accelerated dual w = (accXi, accPsi), the last sweep's input:
        feasibility and stationarity of (x, u, v), Hx = (F x, G u), and the chain z = prox(Hx + w / lambda), Hx - z, y+ = w + lambda (Hx - z).
        Returns {quantity: per-stage error}.  scales="stage": residuals are scaled by their primal and the floors are stagewise.py's (fp64);
        scales="z": the fp32 tests' scales (tests/test_gpu_apg_f32.py): with Z_s = max over stage s of |primalXi|, |primalPsi|, |accXi| / lambda,
        |accPsi| / lambda, an error of Hx, z or Hx - z is over Z_s, one of y+ over lambda Z_s, feasibility over the stage's own maximum."""
        b = {nm: np.asarray(get(nm), float) for nm in ("x", "u", "v", "accXi", "accPsi", "primalXi", "primalPsi")}
        out = self.residuals(b["accXi"], b["accPsi"], b["x"], b["u"], b["v"])
        want = {"primalXi": self.Fx(b["x"]).ravel(), "primalPsi": (self.g * b["u"].reshape(self.nodes, self.nu)).ravel()}
        names = ["primalXi", "primalPsi"]
        if prox:
            want.update(self.prox(b["primalXi"], b["primalPsi"], b["accXi"], b["accPsi"]))
            names += ["dualXi", "dualPsi", "resXi", "resPsi", "updXi", "updPsi"]
        got = {nm: b[nm] if nm in b else np.asarray(get(nm), float) for nm in names}
        dim = lambda nm: self.nu if nm.endswith("Psi") else 2 * self.nx
        if scales == "z":
            smax = lambda a, d: self._per_stage(np.abs(np.asarray(a, float).reshape(self.nodes, d)).max(axis=1))
            Z = np.maximum(np.maximum(smax(b["primalXi"], 2 * self.nx), smax(b["primalPsi"], self.nu)),
                           np.maximum(smax(b["accXi"], 2 * self.nx), smax(b["accPsi"], self.nu)) / self.step)
            assert (Z > 0).all()
            for nm in names:
                out[nm] = smax(got[nm] - want[nm], dim(nm)) / (self.step * Z if nm.startswith("upd") else Z)
            return out
        fam = max(np.abs(b["primalXi"]).max(), np.abs(b["primalPsi"]).max())
        famy = max(np.abs(want["updXi"]).max(), np.abs(want["updPsi"]).max()) if prox else 0.0
        for nm in names:
            scale = b["primalXi"] if nm == "resXi" else b["primalPsi"] if nm == "resPsi" else None
            out[nm] = stage_relmax(got[nm], want[nm], self.tree, dim(nm), scale=scale, family_max=famy if nm.startswith("upd") else fam)
        return out


def worst(errors):
    """(worst value, quantity, stage) of a {quantity: per-stage error} dict"""
    nm = max(errors, key=lambda k: float(np.max(errors[k])))
    return float(np.max(errors[nm])), nm, int(np.argmax(errors[nm]))


def argmin_errors(model, got, ref):
    """per-stage errors of got (dict or get(name)) against argmin's dict ref for x, u, v, primalXi, primalPsi"""
    dims = {"x": model.nx, "u": model.nu, "v": model.nv, "primalXi": 2 * model.nx, "primalPsi": model.nu}
    fam = max(np.abs(ref["primalXi"]).max(), np.abs(ref["primalPsi"]).max())
    g = got if callable(got) else got.__getitem__
    return {nm: stage_relmax(g(nm), ref[nm], model.tree, d, family_max=fam if nm.startswith("primal") else 0.0) for nm, d in dims.items()}
