"""The products with the SHARED operators (csrc/k_slab.hpp) as plain numpy, for tests/test_gpu_slab_product.py: the products of the definition,
the data they are held to, a restatement of the host's launch rules (sweep.inc: slab_waves, slab_stride, few_slabs, wide_ct; rapidnet_capi.hip:
pad16, pad4), the cells of the kernels' schedule a case runs, and deliberate mistakes that show a wrong product cannot pass.

Conventions: operators are [m][k] arrays, node-major operands [nodes][k]; `p` the probabilities of the epilogue scale s_i = -1 / (2 p_i).
Integer data is multiplied in int64 (exact); everything else in np.longdouble, together with each output row's sum of |terms|, which is what
the rounding bound of a sum in ANY order is taken of:  |fl(sum) - sum| <= (n - 1) u sum|terms| + O(u^2)  (Higham, Accuracy and Stability, 3.1)."""
import numpy as np

UNIT_ROUNDOFF = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
EXACT_BELOW = {"f64": 2 ** 53, "f32": 2 ** 24}
KU = 4            # RN_SLAB_KU: k-steps of 4 columns per group of the MFMA loop
GROUP = 4 * KU    # columns per group
MAX_WAVES = 8     # RN_SLAB_MAX_WAVES


# ---- the host's launch rules, restated ------------------------------------------------------------------------------------------------
def pad_rows(m):
    """pad16: operator rows are stored padded to one 64-row wave tile of k_gemm_shared"""
    return (m + 63) // 64 * 64


def pad_cols(k):
    """pad4: operator columns in whole groups of the MFMA loop (zero columns)"""
    return (k + GROUP - 1) // GROUP * GROUP


def slab_stride(kp):
    """elements per LDS slab row: >= kp and = 4 (mod 64)"""
    return (kp + 59) // 64 * 64 + 4


def tiles(m):
    return (m + 15) // 16


def slab_waves(tiles_a, ksteps_a, tiles_b, ksteps_b, nodes, num_cus):
    """waves per slab workgroup: with more slabs than CUs the count in {4, 6, 8} with the least nw * path (throughput), otherwise the
    count with the shortest path, 16 path + nw (latency); ties go to the smaller count"""
    few = (nodes + 15) // 16 <= num_cus
    best, best_cost = 4, None
    for nw in (4, 6, 8, 12, 16):
        if nw > MAX_WAVES or (nw > 8 and not few):
            continue
        path = -(-tiles_a // nw) * ksteps_a + -(-tiles_b // nw) * ksteps_b
        cost = path * 16 + nw if few else nw * path
        if best_cost is None or cost < best_cost:
            best, best_cost = nw, cost
    return best


def few_slabs(nodes, num_cus, form, knob=-1):
    """the software-pipelined MFMA loop: at most one slab per CU, or fp32; RN_KNOB_SLAB_PIPE forces either"""
    return knob != 0 if knob >= 0 else ((nodes + 15) // 16 <= num_cus or form == "f32")


def wide_ct(nodes, num_cus, lds_per_slab, knob=-1):
    """slabs per workgroup of k_gemm_vlv_wide (0: k_gemm_vlv)"""
    want = 3 if (nodes + 15) // 16 > 4 * num_cus else 0
    if knob >= 0:
        want = min(3, knob)
    while want >= 2:
        if lds_per_slab * want <= 160 * 1024:
            return want
        want -= 1
    return 0


def expected_launch(form, nodes, num_cus, first, second=None, knobs=None, kind="pair"):
    """what the hook's info must say for products `first` = (m, k) and `second` (pair only); kind: pair | comp | prep_m2 | single"""
    knobs = knobs or {}
    size = 8 if form == "f64" else 4
    (m, k), kp = first, pad_cols(first[1])
    n_slabs = (nodes + 15) // 16
    pipe = few_slabs(nodes, num_cus, form, knobs.get("slab_pipe", -1))
    frag = knobs.get("slab_frag", -1) != 0
    out = {"m": m, "k": k, "kp": kp}
    if kind != "pair":
        lds = 16 * slab_stride(kp) * size
        if lds <= 64 * 1024:
            name = {"comp": "k_gemm_comp", "prep_m2": "k_gemm_prep_m2", "single": "k_gemm_slab"}[kind]
            out.update(kernel=name, kernel2=None, nw=slab_waves(tiles(m), kp // 4, 0, 0, nodes, num_cus), pipe=int(pipe), frag=int(frag and kind != "single"),
                       ct=0, grid=n_slabs, lds=lds)
        else:
            out.update(kernel="k_gemm_shared", kernel2=None, nw=4, pipe=0, frag=0, ct=0, grid=pad_rows(m) // 64 * n_slabs, lds=0)
        return out
    (m2, k2), kp2 = second, pad_cols(second[1])
    out.update(m2=m2, k2=k2, kp2=kp2)
    lds = 16 * (slab_stride(kp) + slab_stride(kp2)) * size
    if lds > 64 * 1024:
        for tag, (mm, kk) in (("", (m, kp)), ("2", (m2, kp2))):
            one = 16 * slab_stride(kk) * size
            if one <= 64 * 1024:
                out.update({"kernel" + tag: "k_gemm_slab", "nw" + tag: slab_waves(tiles(mm), kk // 4, 0, 0, nodes, num_cus), "grid" + tag: n_slabs, "lds" + tag: one})
            else:
                out.update({"kernel" + tag: "k_gemm_shared", "nw" + tag: 4, "grid" + tag: pad_rows(mm) // 64 * n_slabs, "lds" + tag: 0})
        out.update(frag=0, ct=0, pipe=int(pipe and out["kernel"] == "k_gemm_slab"))
        return out
    ct = wide_ct(nodes, num_cus, lds, knobs.get("vlv_wide", -1))
    if ct >= 2:
        out.update(kernel="k_gemm_vlv_wide", kernel2=None, nw=8, pipe=1, frag=int(frag), ct=ct, grid=-(-n_slabs // ct), lds=lds * ct)
    else:
        out.update(kernel="k_gemm_vlv", kernel2=None, nw=slab_waves(tiles(m), kp // 4, tiles(m2), kp2 // 4, nodes, num_cus), pipe=int(pipe), frag=int(frag), ct=1,
                   grid=n_slabs, lds=lds)
    return out


# ---- the cells of the schedule ---------------------------------------------------------------------------------------------------------
def product_cells(tag, m, k, nw, nodes, grid, pipe, kernel):
    """the cells one product of a launch runs, as strings.  tag: which product ("V", "L", "C", "M2", "S")"""
    c = set()
    kp, t = pad_cols(k), tiles(m)
    G = kp // GROUP
    c.add("%s: %s" % (tag, kernel))
    if kernel == "k_gemm_shared":
        c.add("%s: shared mp/64=%d" % (tag, pad_rows(m) // 64))
        per = -(-(kp // 4) // 4)
        c.add("%s: shared K quarters %s" % (tag, "even" if (kp // 4) % 4 == 0 else "ragged"))
        if per * 3 >= kp // 4:
            c.add("%s: shared idle last quarter" % tag)
    else:
        c.add("%s: G=%s" % (tag, G if G <= 2 else ">2"))
        if pipe:
            c.add("%s: pipelined G%%3=%d" % (tag, G % 3))
        else:
            c.add("%s: lean" % tag)
        c.add("%s: chunks/row=%s" % (tag, min((kp + 63) // 64, 2)) + ("+" if (kp + 63) // 64 > 2 else ""))
        if kernel == "k_gemm_vlv_wide":
            c.add("%s: wide tiles/wave=%d%s" % (tag, -(-t // nw), " ragged" if t % nw else ""))
        else:
            per = -(-t // nw)
            tg = min(per, 3)
            c.add("%s: tg=%d" % (tag, tg))
            if t < nw:
                c.add("%s: idle waves" % tag)
            haves = {min(-(-(t - t0) // nw), tg) for owner in range(nw) for t0 in range(owner, t, nw * tg)}
            if len(haves) > 1:
                c.add("%s: have remainder" % tag)
            if per > 3:
                c.add("%s: several passes" % tag)
    c.add("%s: m%%16=%s" % (tag, "0" if m % 16 == 0 else "1" if m % 16 == 1 else "other"))
    c.add("%s: k%%16=%s" % (tag, "0" if k % 16 == 0 else "1" if k % 16 == 1 else "other"))
    if k % 4:
        c.add("%s: k%%4!=0" % tag)
    if m % 4:
        c.add("%s: m%%4!=0" % tag)
    if grid >= 8 and kernel not in ("k_gemm_shared", "k_gemm_vlv_wide"):
        c.add("rotation b>=8")
    if grid >= 256 and kernel not in ("k_gemm_shared", "k_gemm_vlv_wide"):
        c.add("rotation b>=256")
    return c


def cells(dims, info, stored_v=True, aux=True, split=False, pipe2=None):
    """the cells a case ran, from its dimensions and the hook's info.  dims: {"nodes", "form"}; info: Solver.slabProduct's.  pipe2: the loop of a
    second LAUNCH (info's `pipe` is the first launch's; None: the same)"""
    nodes, c = dims["nodes"], set()
    c.add(dims["form"])
    k1 = info["kernel"]
    first_tag = {"k_gemm_comp": "C", "k_gemm_prep_m2": "M2"}.get(k1, "V" if info["m2"] else "S")
    c |= product_cells(first_tag, info["m"], info["k"], info["nw"], nodes, info["grid"], info["pipe"], k1)
    if info["m2"]:
        second = info["kernel2"] or k1
        c |= product_cells("L", info["m2"], info["k2"], info["nw2"] if info["kernel2"] else info["nw"], nodes, info["grid2"] if info["kernel2"] else info["grid"],
                           info["pipe"] if pipe2 is None or not info["kernel2"] else int(pipe2), second)
        if k1 in ("k_gemm_vlv", "k_gemm_vlv_wide"):
            c.add("v tile in LDS, v %s" % ("stored" if stored_v else "not stored"))
    if info["ldin"] != info["k"]:
        c.add("ldin != k, offset %s" % ("> 0" if info["inOffset"] else "0"))
    c.add("%s: aux %s" % (first_tag, "split" if split else "yes" if aux else "none"))
    c.add("frag" if info["frag"] else "column-major")
    if k1 == "k_gemm_vlv_wide":
        per = 16 * info["ct"]
        last = nodes - (info["grid"] - 1) * per
        c.add("wide CT=%d last workgroup: %d slab(s), last slab %s" % (info["ct"], -(-last // 16), {1: "1 node", 15: "15 nodes", 0: "full"}.get(last % 16, "partial")))
    elif k1 != "k_gemm_shared":
        c.add("last slab %s" % {1: "1 node", 15: "15 nodes", 0: "full"}.get(nodes % 16, "partial"))
    return c


# ---- the products ---------------------------------------------------------------------------------------------------------------------
def is_integer(*arrays):
    return all(a is None or np.array_equal(a, np.rint(a)) for a in arrays)


def product(M, X, p=None, aux=None, aux2=None, split=None):
    """out_i = aux_i (+ aux2_{i - split}) + s_i M x_i with s_i = -1 / (2 p_i) (p None: s = 1).  Returns (value, sum of |terms| per entry):
    int64 arrays where every operand is an integer and every s_i is, np.longdouble otherwise."""
    nodes = X.shape[0]
    s = np.ones(nodes) if p is None else -0.5 / np.asarray(p, float)
    exact = is_integer(M, X, aux, aux2, s)
    ty = np.int64 if exact else np.longdouble
    Mt, Xt, st = np.asarray(M).astype(ty), np.asarray(X).astype(ty), (np.asarray(s).astype(ty) if p is not None else np.ones(nodes, ty))
    if not exact and p is not None:
        st = np.longdouble(-0.5) / np.asarray(p).astype(np.longdouble)
    acc = Xt @ Mt.T
    mag = np.abs(Xt) @ np.abs(Mt).T
    val, mag = st[:, None] * acc, np.abs(st)[:, None] * mag
    if aux is not None:
        a = np.asarray(aux).astype(ty)[:, :M.shape[0]].copy()
        am = np.abs(a)
        if aux2 is not None:
            a2 = np.asarray(aux2).astype(ty)[:, :M.shape[0]]
            a[split:] += a2
            am[split:] += np.abs(a2)
        val, mag = val + a, mag + am
    return val, mag


def pair(MV, ML, X, p, aux=None, aux2=None, split=None, v_fed=None):
    """v_i = aux_i (+ aux2_i) - MV x_i / (2 p_i), lv_i = ML v_i; v_fed: the v the second product is taken of (None: the first's own).
    Returns ((v, |v| terms), (lv, |lv| terms))"""
    v = product(MV, X, p, aux, aux2, split)
    vin = v[0] if v_fed is None else v_fed
    return v, product(ML, np.asarray(vin, dtype=np.float64) if v_fed is not None else vin, None)


def prep_slab(W, stage, p, diag_precnd, nx, nu, form):
    """the slab rows [a_i; b_i] of k_gemm_prep_m2 from the dual W [nodes][2 nx + nu]: a_i = F_i' xi_i, b_i = G_i' psi_i with F_i = sqrt(p_i)
    [diag(d_x); diag(d_xs)], G_i = sqrt(p_i) diag(d_u); stage k of matDiagPrecnd = (d_u | d_x | d_xs) (tests/first_principles.py).  sqrt(p) is
    taken in double and rounded to the context's type, as are the diagonal's entries.  Returns (slab, sum of |terms|) in np.longdouble."""
    ty = np.float32 if form == "f32" else np.float64
    diag = np.asarray(diag_precnd, float).reshape(-1, 2 * nx + nu).astype(ty).astype(np.longdouble)
    d_u, d_x, d_xs = diag[:, :nu][stage], diag[:, nu:nu + nx][stage], diag[:, nu + nx:][stage]
    sp = np.sqrt(np.asarray(p, float)).astype(ty).astype(np.longdouble)[:, None]
    Wl = np.asarray(W).astype(np.longdouble)
    t1, t2 = sp * d_x * Wl[:, :nx], sp * d_xs * Wl[:, nx:2 * nx]
    b = sp * d_u * Wl[:, 2 * nx:]
    return np.concatenate([t1 + t2, b], axis=1), np.concatenate([np.abs(t1) + np.abs(t2), np.abs(b)], axis=1)


def prep_m2(M, W, stage, p, diag_precnd, nx, nu, form):
    """((m2, |terms|), (qa, |terms|)) of the first structured product: m2_i = M [a_i; b_i], qa_i = a_i"""
    slab, smag = prep_slab(W, stage, p, diag_precnd, nx, nu, form)
    Ml = np.asarray(M).astype(np.longdouble)
    return (slab @ Ml.T, smag @ np.abs(Ml).T), (slab[:, :nx], smag[:, :nx])


def bound(mag, k, form, extra=0):
    """(k + 4 + extra) u sum|terms|: k - 1 additions of the dot product, the epilogue's scale, its product and its sum, and the rounding of s itself"""
    return (k + 4 + extra) * UNIT_ROUNDOFF[form] * mag


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def round_to(form, a):
    return None if a is None else (np.asarray(a, float).astype(np.float32).astype(np.float64) if form == "f32" else np.asarray(a, float))


def integer_data(seed, form, nodes, dims, aux_rows=None, split=None, second=None, with_p=True):
    """operators in [-r, r], inputs and aux in [-2 r, 2 r] with r = 4 narrowed until the int64 reference shows every sum of |terms| of both products
    below 2^24 (fp32) or 2^53 (fp64): a sum whose absolute terms stay below that bound is exact in every order of accumulation.  Probabilities
    are 1/2, 1/4, 1/8, so that s = -1 / (2 p) is -1, -2, -4.  dims = (m, k); second = (m2, k2 = m); aux_rows: the row length of aux (None: none).
    Returns a dict: MA, MB, X, p, aux, aux2."""
    m, k = dims
    rng = np.random.default_rng(seed)
    r = 4
    while True:
        d = {"MA": rng.integers(-r, r + 1, (m, k)).astype(float), "X": rng.integers(-2 * r, 2 * r + 1, (nodes, k)).astype(float),
             "p": 0.5 ** rng.integers(1, 4, nodes) if with_p else None, "MB": None, "aux": None, "aux2": None}
        if aux_rows:
            d["aux"] = rng.integers(-2 * r, 2 * r + 1, (nodes, aux_rows)).astype(float)
            if split is not None:
                d["aux2"] = rng.integers(-2 * r, 2 * r + 1, (nodes - split, aux_rows)).astype(float)
        if second:
            d["MB"] = rng.integers(-r, r + 1, second).astype(float)
        v = product(d["MA"], d["X"], d["p"], d["aux"], d["aux2"], split)
        assert v[0].dtype == np.int64
        worst = int(v[1].max())
        if second:
            lv = product(d["MB"], v[0], None)
            assert lv[0].dtype == np.int64
            # (the second product's |terms| are taken of |v| <= the first's sum of |terms|: every partial sum of either product lies below)
            worst = max(worst, int((v[1] @ np.abs(d["MB"]).astype(np.int64).T).max()))
        if worst < EXACT_BELOW[form]:
            d["worst"] = worst
            return d
        assert r > 1, ("no integer range keeps the sums exact", dims, second, form)
        r -= 1


def real_data(seed, form, nodes, dims, aux_rows=None, split=None, second=None, with_p=True):
    """normal deviates of scale 1, probabilities uniform in [0.05, 1); everything rounded to the context's type, so that the reference multiplies
    what the context holds"""
    m, k = dims
    rng = np.random.default_rng(seed)
    d = {"MA": rng.standard_normal((m, k)), "X": rng.standard_normal((nodes, k)), "p": rng.uniform(0.05, 1.0, nodes) if with_p else None,
         "MB": rng.standard_normal(second) if second else None, "aux": rng.standard_normal((nodes, aux_rows)) if aux_rows else None,
         "aux2": rng.standard_normal((nodes - split, aux_rows)) if aux_rows and split is not None else None}
    return {key: round_to(form, val) for key, val in d.items()}


def signed_patterns(nodes, dims, second=None):
    """integer data in which a dropped column or row cannot hide in a sum: node i has ONE nonzero input column -- k - 1, k - 17, the 64-element
    chunk boundaries 63 and 64, and 0, by turns (those that exist) -- of value (-1)^i (1 + i mod 5), the operator is 1 + (r + 2 c) mod 7 with the
    sign (-1)^(r + c), and its last row m - 1 is the only one whose entries exceed 8.  Yields one data dict."""
    m, k = dims
    cols = [c for c in (k - 1, k - 17, 63, 64, 0) if 0 <= c < k]
    X = np.zeros((nodes, k))
    for i in range(nodes):
        X[i, cols[i % len(cols)]] = (-1) ** i * (1 + i % 5)
    rr, cc = np.meshgrid(np.arange(m), np.arange(k), indexing="ij")
    MA = ((1 + (rr + 2 * cc) % 7) * (-1.0) ** (rr + cc))
    MA[m - 1] = 9 + np.arange(k) % 5
    d = {"MA": MA, "X": X, "p": np.full(nodes, 0.5), "MB": None, "aux": None, "aux2": None}
    if second:
        m2, k2 = second
        r2, c2 = np.meshgrid(np.arange(m2), np.arange(k2), indexing="ij")
        d["MB"] = ((1 + (2 * r2 + c2) % 5) * (-1.0) ** (r2 + c2))
        d["MB"][m2 - 1] = 7 + np.arange(k2) % 3
    return d


# ---- deliberate mistakes: each is a wrong PRODUCT; a named case must notice, an interior case must not --------------------------------------
def mistake_drop_last_group(M, X, p=None, aux=None, aux2=None, split=None):
    """the pipelined loop's second tail step left out: the last group of 16 columns is dropped when G mod 3 = 2"""
    kp = pad_cols(M.shape[1])
    G = kp // GROUP
    if G % 3 != 2:
        return product(M, X, p, aux, aux2, split)
    keep = (G - 1) * GROUP
    return product(M[:, :keep], X[:, :keep], p, aux, aux2, split)


def mistake_last_tile_rows(M, X, p=None, aux=None, aux2=None, split=None):
    """the rows of a partial last tile all taken at m - 1 (the epilogue's clamp applied to the operator row as well)"""
    m = M.shape[0]
    val, mag = product(M, X, p, aux, aux2, split)
    if m % 16:
        t0 = m // 16 * 16
        val, mag = val.copy(), mag.copy()
        val[:, t0:m] = val[:, m - 1:m]
        mag[:, t0:m] = mag[:, m - 1:m]
    return val, mag


def mistake_stale_v_tile(MV, ML, X, p, aux=None, aux2=None, split=None):
    """a last slab's absent nodes not zeroed in the v tile: harmless for the rows of present nodes only if the second product never mixes
    nodes -- modelled as the LAST node of a partial last slab receiving the sum of its own and the absent nodes' (aux-only) v in the second product"""
    v, lv = pair(MV, ML, X, p, aux, aux2, split)
    nodes = X.shape[0]
    if nodes % 16 == 0:
        return v, lv
    ty = v[0].dtype
    stale = np.ones(MV.shape[0]).astype(ty)          # what a not-zeroed LDS row holds: anything; here ones
    val = lv[0].copy()
    val[nodes - 1] = np.asarray(ML).astype(ty) @ (v[0][nodes - 1] + stale)
    return v, (val, lv[1])


def mistake_aux2_index(M, X, p=None, aux=None, aux2=None, split=None):
    """aux2 indexed by i instead of i - auxSplit (clamped into the buffer)"""
    if aux2 is None:
        return product(M, X, p, aux, aux2, split)
    nodes = X.shape[0]
    idx = np.minimum(np.arange(split, nodes), aux2.shape[0] - 1)
    return product(M, X, p, aux, aux2[idx], split)


def mistake_ldin_is_k(M, X_rows, k_off, p=None, aux=None):
    """the input read with ldin = k in the linear form: X_rows is the buffer as the sweep lays it out, [nodes][ldin] with the product's k columns at
    k_off; the mistaken read takes node i's columns at i * k + k_off of the flat buffer"""
    nodes, ldin = X_rows.shape
    k = M.shape[1]
    flat = np.concatenate([X_rows.ravel(), np.zeros(k + k_off)])
    X = np.stack([flat[i * k + k_off:i * k + k_off + k] for i in range(nodes)])
    return product(M, X, p, aux)
