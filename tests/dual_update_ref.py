"""A plain numpy / Python restatement of the dual update of one APG iteration (csrc/common.hpp dual_elem; csrc/k_dual.hpp: the dist^2 sums, the trip
decision, the signed arg-max, the fix-up pass), for tests/test_gpu_dual_update.py.  It gets nothing from the library but the inputs.

Roundings.  dual_elem spells its roundings out: three fused multiply-adds, every other operation rounded by itself.  Here every plain operation is ONE
numpy operation in the element type, and the fused ones are exactly rounded: fma64 / fma32 form the exact rational a b + c (fractions.Fraction) and round
it ONCE to the type, to nearest, ties to even.  (np.float32(float(q)) would round twice.)  The restatement does not carry the sign of a zero: outputs are
compared as numbers (np.array_equal) and must hold no NaN.  Infinite bounds are compared before anything becomes a rational: a clamp against +-inf never
selects the bound, so no infinity reaches an FMA.

Element order: rows [node][ny], ny = 2 nx + nu: columns [0, nx) the box half of xi, [nx, 2 nx) its safety half, [2 nx, ny) psi.  Element index = node *
ny + column (the index the kernels' arg-max carries)."""
import math
from fractions import Fraction

import numpy as np

DTYPES = {"f64": np.float64, "f32": np.float32}


# ---- exactly rounded fused multiply-adds ---------------------------------------------------------------------------------------------------------------
def round_fraction(q, mant, emin, emax):
    """the rational q rounded ONCE to a binary format with `mant` significand bits (hidden one included), minimum normal exponent emin, maximum emax:
    nearest, ties to even; returns a Python float (every such value is a double when mant <= 53)"""
    if q == 0:
        return 0.0
    sign = -1.0 if q < 0 else 1.0
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()      # 2^(e - 1) < q < 2^(e + 1)
    if q < Fraction(2) ** e:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, emin) - (mant - 1))            # spacing of the format at q (subnormals: the fixed spacing below 2^emin)
    n = q / quantum
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    r = Fraction(fl) * quantum
    if r >= Fraction(2) ** (emax + 1):
        return sign * math.inf
    return sign * float(r)      # exact: r has at most `mant` bits


def fma64(a, b, c):
    return round_fraction(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)), 53, -1022, 1023)


def fma32(a, b, c):
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    return np.float32(round_fraction(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)), 24, -126, 127))


def fma_two_roundings(a, b, c, dtype):
    """a b + c as a product and a sum: what a build that lost the fusion computes (the deliberate mistakes, and the measure of how often it shows)"""
    dt = np.dtype(dtype).type
    return dt(dt(a) * dt(b)) + dt(c)


def fma_array(a, b, c, dtype):
    """element-wise exactly rounded a * b + c in dtype; a, b, c broadcast; all finite"""
    dt = np.dtype(dtype).type
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=dt), np.asarray(b, dtype=dt), np.asarray(c, dtype=dt))
    assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all(), "an FMA operand is not finite"
    out = np.empty(a.shape, dtype=dt)
    fa, fb, fc, fo = a.ravel(), b.ravel(), c.ravel(), out.reshape(-1)
    if dt is np.float32:
        # the product of two fp32 values is exact in a double; where the double sum with c is exact too (TwoSum's error term is zero) the one rounding
        # to fp32 is the only one.  Everything else goes through the rational.
        p = fa.astype(np.float64) * fb.astype(np.float64)
        c64 = fc.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        fo[:] = s.astype(np.float32)
        for i in np.flatnonzero(err != 0):
            fo[i] = fma32(fa[i], fb[i], fc[i])
    else:
        # error-free transformations: a b = p + e (Dekker / Veltkamp), p + c = s + e2 (Knuth).  Where e + e2 = r is exact as well, the exact value is
        # s + r, two doubles, and their one floating-point sum is its correct rounding.  Everything else, and anything near the ends of the exponent
        # range (where the splitting itself rounds), goes through the rational.
        with np.errstate(all="ignore"):
            p = fa * fb
            split = 134217729.0      # 2^27 + 1
            ah = fa * split
            ah = ah - (ah - fa)
            al = fa - ah
            bh = fb * split
            bh = bh - (bh - fb)
            bl = fb - bh
            e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
            s = p + fc
            bb = s - p
            e2 = (p - (s - bb)) + (fc - bb)
            r = e + e2
            rb = r - e
            e3 = (e - (r - rb)) + (e2 - rb)
            fo[:] = s + r
            mag = np.maximum(np.maximum(np.abs(fa), np.abs(fb)), np.abs(fc))
            small = np.minimum(np.where(fa != 0, np.abs(fa), 1.0), np.where(fb != 0, np.abs(fb), 1.0))
            safe = (e3 == 0) & (mag < 1e100) & (small > 1e-100) & np.isfinite(fo)
        for i in np.flatnonzero(~safe):
            fo[i] = fma64(fa[i], fb[i], fc[i])
    return out


# ---- the update of one element (common.hpp, dual_elem) ---------------------------------------------------------------------------------------------------
def dual_elem_ref(hx, w, lo, hi, yp, lam, inv_lam, ln, sc, dtype, mistake=None):
    """(yn, wn, z, res, diff) of dual_elem over arrays.  sc: None = the main pass (no fix-up), else the per-element scale of the fix-up pass (0 on psi and
    on halves that did not trip).  lam, inv_lam, ln: the values the kernel's type holds.  mistake: "unfuse_t" | "unfuse_yn" | "unfuse_wn" | "unfuse_z"."""
    dt = np.dtype(dtype).type
    hx, w, lo, hi, yp = (np.asarray(v, dtype=dt) for v in (hx, w, lo, hi, yp))
    lam, inv_lam, ln = dt(lam), dt(inv_lam), dt(ln)
    fm = lambda name, a, b, c: fma_two_roundings(a, b, c, dt) if mistake == name else fma_array(a, b, c, dt)
    assert not (np.isnan(lo).any() or np.isnan(hi).any())
    t = fm("unfuse_t", inv_lam, w, hx)
    z = np.where(t < lo, lo, np.where(t > hi, hi, t)).astype(dt)
    assert np.isfinite(z).all(), "the clamp selected an infinite bound"
    diff = (t - z).astype(dt)
    if sc is not None:
        sc = np.broadcast_to(np.asarray(sc, dtype=dt), z.shape)
        on = sc != 0
        if on.any():
            z = z.copy()
            z[on] = fm("unfuse_z", sc[on], diff[on], z[on])
    res = (hx - z).astype(dt)
    yn = fm("unfuse_yn", lam, res, w)
    a = ((dt(1) + ln) * yn).astype(dt)
    wn = fm("unfuse_wn", -ln, yp, a)
    return yn, wn, z, res, diff


def extrap_ref(y1, y0, ln, dtype):
    """common.hpp, extrap_elem: w = (1 + ln) y1 - ln y0 with dual_elem's roundings"""
    dt = np.dtype(dtype).type
    a = ((dt(1) + dt(ln)) * np.asarray(y1, dtype=dt)).astype(dt)
    return fma_array(-dt(ln), np.asarray(y0, dtype=dt), a, dt)


# ---- the scaled bounds from the tables (k_dual.hpp: k_dual_fused's regen branch, dual_slot_use) ---------------------------------------------------------------
def scale_factor(sqrtp, dy, stage_of, dtype):
    """k = sqrt(p_node) * d[stage][c], [nodes][ny], one product in the element type"""
    dt = np.dtype(dtype).type
    return (np.asarray(sqrtp, dtype=dt)[:, None] * np.asarray(dy, dtype=dt)[np.asarray(stage_of)]).astype(dt)


def bounds_from_tables(sqrtp, dy, blo, bhi, stage_of, stride_stage, stride_node, nx, dtype):
    """lo = k * blo, hi = k * bhi, unscaled on the safety half; the row of a node: stage * stride_stage + node * stride_node elements into the tables"""
    dt = np.dtype(dtype).type
    nodes, ny = len(sqrtp), np.asarray(dy).shape[1]
    k = scale_factor(sqrtp, dy, stage_of, dt)
    idx = (np.asarray(stage_of, dtype=np.int64) * stride_stage + np.arange(nodes, dtype=np.int64) * stride_node)[:, None] + np.arange(ny)[None, :]
    bl, bh = np.asarray(blo, dtype=dt).ravel()[idx], np.asarray(bhi, dtype=dt).ravel()[idx]
    with np.errstate(invalid="ignore", over="ignore"):
        lo = (k * bl).astype(dt)
        hi = (k * bh).astype(dt)
    hi[:, nx:2 * nx] = bh[:, nx:2 * nx]
    return lo, hi, k


# ---- the bookkeeping ----------------------------------------------------------------------------------------------------------------------------------------
def column_groups(nodes, nx, ny):
    c = np.tile(np.arange(ny), nodes).reshape(nodes, ny)
    return c < nx, (c >= nx) & (c < 2 * nx), c >= 2 * nx


def dist2_exact(diff, nx, counted=None):
    """(d2x, d2s, terms summed): the EXACT sums (rationals, returned as the nearest double) of the squares the kernels add -- each the product
    (double) diff * (double) diff as a double holds it -- over the box and the safety half.  counted [nodes]: rows that count (a shard's crown rows count
    on rank 0 only)."""
    d = np.asarray(diff).astype(np.float64)
    nodes, ny = d.shape
    box, safe, _ = column_groups(nodes, nx, ny)
    if counted is not None:
        box, safe = box & np.asarray(counted, bool)[:, None], safe & np.asarray(counted, bool)[:, None]
    sq = d * d
    fx = sum((Fraction(float(v)) for v in sq[box]), Fraction(0))
    fs = sum((Fraction(float(v)) for v in sq[safe]), Fraction(0))
    return float(fx), float(fs), int(box.sum()), int(safe.sum())


def decide(d2x, d2s, thr_x, thr_s, mistake=None):
    """the decision from a GIVEN pair of sums, in double, the kernels' expression: (tripped, scaleX, scaleS, distX, distS)"""
    dX, dS = float(np.sqrt(np.float64(d2x))), float(np.sqrt(np.float64(d2s)))
    gt = (lambda a, b: a >= b) if mistake == "ge" else (lambda a, b: a > b)
    trX, trS = gt(dX, thr_x), gt(dS, thr_s)
    scX = float(np.float64(1.0) - np.float64(thr_x) / np.float64(dX)) if trX else 0.0
    scS = float(np.float64(1.0) - np.float64(thr_s) / np.float64(dS)) if trS else 0.0
    return (1 if (trX or trS) else 0), scX, scS, dX, dS


def scale_columns(scX, scS, nodes, nx, ny, dtype, mistake=None):
    """the fix-up pass's per-element scale: (T) scaleX on the box half, (T) scaleS on the safety half, 0 on psi"""
    dt = np.dtype(dtype).type
    sc = np.zeros((nodes, ny), dtype=dt)
    sc[:, :nx] = dt(scX)
    sc[:, nx:2 * nx] = dt(scS)
    if mistake == "scale_psi":
        sc[:, 2 * nx:] = dt(scX)
    return sc


def argmax_ref(res, nx, mistake=None):
    """((|.|, signed value, element index) of the xi half, the same of psi, history entry): the largest |res| at its LOWEST element index (idamax), the
    history entry the larger of the two SIGNED entries.  mistake: "last" keeps the last occurrence, "positive" prefers the positive entry among ties."""
    r = np.asarray(res).astype(np.float64)
    nodes, ny = r.shape
    assert not np.isnan(r).any()
    idx = np.arange(nodes * ny).reshape(nodes, ny)
    out = []
    for cols in (slice(0, 2 * nx), slice(2 * nx, ny)):
        v, i = r[:, cols].ravel(), idx[:, cols].ravel()
        a = np.abs(v)
        tied = np.flatnonzero(a == a.max())
        k = tied[0]
        if mistake == "last":
            k = tied[-1]
        elif mistake == "positive":
            pos = tied[v[tied] > 0]
            k = pos[0] if pos.size else tied[0]
        out.append((float(a[k]), float(v[k]), int(i[k])))
    (aX, vX, iX), (aP, vP, iP) = out
    return (aX, vX, iX), (aP, vP, iP), (vX if vX > vP else vP)


def restate(inp, dtype, thr_x, thr_s, d2=None, counted=None, mistake=None):
    """One iteration, exact form.  inp: dict(hx, w, yp, lo, hi [nodes][ny], lam, inv_lam, ln, nx).  d2: the pair of sums the decision is taken from (None:
    the restatement's own exact sums).  Returns dict(main=(yn, wn, z, res, diff), d2x, d2s, nX, nS, tripped, scaleX, scaleS, distX, distS,
    out=(yn, wn, z, res) after the fix-up where it tripped, argmax=..., hist=...; main_argmax / main_hist the same of the main pass)."""
    dt = np.dtype(dtype).type
    nx = inp["nx"]
    nodes, ny = np.asarray(inp["hx"]).shape
    em = mistake if mistake in ("unfuse_t", "unfuse_yn", "unfuse_wn", "unfuse_z") else None
    main = dual_elem_ref(inp["hx"], inp["w"], inp["lo"], inp["hi"], inp["yp"], inp["lam"], inp["inv_lam"], inp["ln"], None, dt, mistake=em)
    if mistake == "crown_every_rank":
        counted = None
    d2x, d2s, nX, nS = dist2_exact(main[4], nx, counted)
    use = (d2x, d2s) if d2 is None else d2
    tripped, scX, scS, dX, dS = decide(use[0], use[1], thr_x, thr_s, mistake="ge" if mistake == "ge" else None)
    r = dict(main=main, d2x=d2x, d2s=d2s, nX=nX, nS=nS, tripped=tripped, scaleX=scX, scaleS=scS, distX=dX, distS=dS)
    am = mistake if mistake in ("last", "positive") else None
    r["main_argmax"] = argmax_ref(main[3], nx, am)
    if tripped:
        sc = scale_columns(scX, scS, nodes, nx, ny, dt, mistake="scale_psi" if mistake == "scale_psi" else None)
        fx = dual_elem_ref(inp["hx"], inp["w"], inp["lo"], inp["hi"], inp["yp"], inp["lam"], inp["inv_lam"], inp["ln"], sc, dt, mistake=em)
        r["out"] = fx[:4]
    else:
        r["out"] = main[:4]
    r["argmax"] = argmax_ref(r["out"][3], nx, am)
    r["hist"], r["main_hist"] = r["argmax"][2], r["main_argmax"][2]
    return r


# ---- integer data: every value and every sum exact ---------------------------------------------------------------------------------------------------------
def is_square(n):
    r = math.isqrt(int(n))
    return r * r == int(n)


def integer_case(nodes, nx, ny, seed, lam_log2=-3, bound=8, dtype=np.float64, reserve=48):
    """hx, w / lambda integers in [-bound, bound], lambda = 2^lam_log2, for a context whose box and input bounds are all zero (lo = hi = 0; on the safety
    half lo = 0 and hi is the unscaled upper bound, far above).  Then t = hx + w / lambda is an integer, the box diff is t, the safety diff min(t, 0),
    and the last `reserve` box / safety elements are chosen so that both sums of squares are perfect squares D^2.  `bound` is narrowed until every sum is
    below 2^24 (fp32) / 2^53.  Returns dict(hx, w, yp, lam, DX, DS, tint [nodes][ny] int64, bound)."""
    rng = np.random.default_rng(seed)
    limit = 2 ** 24 if np.dtype(dtype) == np.float32 else 2 ** 53
    box, safe, psi = column_groups(nodes, nx, ny)
    reserve = max(2, min(reserve, int(box.sum()) // 4))
    tries = 0
    while True:
        h = rng.integers(-bound, bound + 1, (nodes, ny))
        m = rng.integers(-bound, bound + 1, (nodes, ny))          # w / lambda
        hh, mm = h.reshape(-1), m.reshape(-1)
        ok = True
        for grp, neg_only in ((box, False), (safe, True)):
            pos = np.flatnonzero(grp.ravel())[-reserve:]
            hh[pos] = 0
            mm[pos] = 0
            t = h + m
            d = np.where(grp, np.minimum(t, 0) if neg_only else t, 0)
            S = int((d.astype(np.int64) ** 2).sum())
            D = math.isqrt(S) + 1
            R = D * D - S
            k = 0
            while R > 0 and k < reserve:
                q = min(bound, math.isqrt(R))
                hh[pos[k]] = -q      # (negative: counts on the safety half too)
                R -= q * q
                k += 1
            ok = ok and R == 0
        t = h + m
        DX2 = int((np.where(box, t, 0).astype(np.int64) ** 2).sum())
        DS2 = int((np.where(safe, np.minimum(t, 0), 0).astype(np.int64) ** 2).sum())
        if ok and is_square(DX2) and is_square(DS2):
            if max(DX2, DS2) < limit:
                break
            assert bound > 1, "no exact integer case at this size"
            bound -= 1      # the sums must stay exact: narrower values
            continue
        tries += 1
        assert tries < 100, "the reserved elements cannot complete the squares"
    lam = 2.0 ** lam_log2
    dt = np.dtype(dtype).type
    hx, w = h.astype(dt), (m * lam).astype(dt)
    assert np.array_equal(w.astype(np.float64) / lam, m)
    yp = rng.integers(-bound, bound + 1, (nodes, ny)).astype(dt)
    return dict(hx=hx, w=w, yp=yp, lam=lam, DX=math.isqrt(DX2), DS=math.isqrt(DS2), tint=t.astype(np.int64), bound=bound, nx=nx)


def integer_main_ref(case, nx):
    """the main pass on integer data with zero bounds, plain int64 / exact binary fractions (ln = 0: iteration 0): (yn, wn, z, res, d2x, d2s)"""
    t = case["tint"]
    nodes, ny = t.shape
    box, safe, psi = column_groups(nodes, nx, ny)
    z = np.where(safe, np.maximum(t, 0), 0).astype(np.float64)
    hx, w = case["hx"].astype(np.float64), case["w"].astype(np.float64)
    res = hx - z
    yn = w + case["lam"] * res          # exact: small integers times a power of two
    d = np.where(box, t, np.where(safe, np.minimum(t, 0), 0)).astype(np.int64)
    return yn, yn.copy(), z, res, int((np.where(box, d, 0) ** 2).sum()), int((np.where(safe, d, 0) ** 2).sum())


def plant_tie(case, first, second, nx, magnitude=None):
    """the largest |res| twice with opposite signs, the NEGATIVE one at the lower element index: hx = -M at `first`, +M at `second`, w = 0 there (element
    indices, both on the box half or both on psi, where lo = hi = 0 makes res = hx).  The planted entries join the box sum of squares: the caller
    takes DX from the returned case's tint only where it needs it.  Returns a copy."""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    nodes, ny = c["hx"].shape
    assert first < second
    M = float(np.abs(c["hx"]).max() + 1) if magnitude is None else float(magnitude)
    for i, v in ((first, -M), (second, M)):
        col = i % ny
        assert col < nx or col >= 2 * nx, "ties are planted on the box half or on psi"
        c["hx"].ravel()[i] = v
        c["w"].ravel()[i] = 0
        c["tint"].ravel()[i] = int(v)
    return c


# ---- normal data ---------------------------------------------------------------------------------------------------------------------------------------------
def normal_case(lo, hi, lam, nx, seed, dtype, psi_scale=3.0):
    """hx, w, yp of normal deviates placed around the bounds: per column group a third of the elements below lo, a third inside, a third above hi
    (safety half: hi is far away, so below / inside only); t == lo and t == hi planted (w = 0, hx = the bound).  The xi and psi halves use different
    scales.  Asserts the mix on the restated t."""
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, dtype=dt), np.asarray(hi, dtype=dt)
    nodes, ny = lo.shape
    box, safe, psi = column_groups(nodes, nx, ny)
    span = np.where(np.isfinite(hi - lo) & (hi > lo) & ~safe, (hi - lo).astype(np.float64), 1.0)
    span = np.where(span > 1e6, 1.0, span)
    scale = np.where(psi, psi_scale, 1.0)
    cat = rng.integers(0, 3, (nodes, ny))
    cat[safe] = rng.integers(0, 2, int(safe.sum()))
    g = np.abs(rng.standard_normal((nodes, ny))) + 0.05
    u = rng.uniform(0.05, 0.95, (nodes, ny))
    lo64, hi64 = lo.astype(np.float64), np.where(safe, lo.astype(np.float64) + span, hi.astype(np.float64))
    target = np.where(cat == 0, lo64 - g * span * scale, np.where(cat == 1, lo64 + u * (hi64 - lo64), hi64 + g * span * scale))
    target = np.where(hi64 <= lo64, np.where(cat == 0, lo64 - g, np.where(cat == 1, lo64, hi64 + g)), target)
    part = rng.standard_normal((nodes, ny)) * span * scale
    hx = (target - part).astype(dt)
    w = (part * lam).astype(dt)
    yp = (rng.standard_normal((nodes, ny)) * span * scale * lam).astype(dt)
    flat = rng.permutation(nodes * ny)[:8]
    for j, i in enumerate(flat):      # t == lo, t == hi exactly
        b = (lo if j % 2 == 0 else hi).ravel()[i]
        if np.isfinite(b) and abs(float(b)) < 1e6:
            hx.ravel()[i] = b
            w.ravel()[i] = 0
    return dict(hx=hx, w=w, yp=yp, nx=nx)


def assert_mix(t, lo, hi, nx):
    """each of below lo / inside / above hi holds for at least a tenth of the elements of each column group (the safety half has no upper bound to exceed)"""
    nodes, ny = t.shape
    for name, grp in zip(("box", "safety", "psi"), column_groups(nodes, nx, ny)):
        n = int(grp.sum())
        below, above = int((t[grp] < lo[grp]).sum()), int((t[grp] > hi[grp]).sum())
        inside = n - below - above
        assert below * 10 >= n and inside * 10 >= n, (name, below, inside, above, n)
        if name != "safety":
            assert above * 10 >= n, (name, below, inside, above, n)


# ---- from a launch record to the cells it ran ----------------------------------------------------------------------------------------------------------------
ELT_THREADS = 256


def coordinates(info, nodes, ny, dtype):
    """Where every element of the main pass was computed: dict of int arrays [nodes * ny]: block, tid (thread in the workgroup), wave, trip (k_dual_stage:
    the trip; k_dual_fused: the grid-stride round), crown (1: a crown workgroup), stage_block (k_dual_stage: the stage index a regular workgroup
    serves, -1 in the crown), tail (1: the flat kernel's scalar tail), vec (vector index)."""
    VN = 16 // np.dtype(dtype).itemsize
    n = nodes * ny
    e = np.arange(n, dtype=np.int64)
    out = {}
    if info["kernel"] == "k_dual_stage":
        vpn, tile = int(info["vpn"]), ELT_THREADS * int(info["trips"])
        node0, K, cb, bps = int(info["node0"]), int(info["K"]), int(info["crownBlocks"]), int(info["bps"])
        assert vpn * VN == ny
        iv = e // VN
        node = iv // vpn
        crown = node < node0
        s = np.where(crown, 0, (node - node0) // max(K, 1))
        J = np.where(crown, iv, iv - (node0 + s * K) * vpn)
        block = np.where(crown, J // tile, cb + s * bps + J // tile)
        off = J % tile
        out.update(block=block, tid=off % ELT_THREADS, trip=off // ELT_THREADS, crown=crown.astype(np.int64), stage_block=np.where(crown, -1, s), tail=np.zeros(n, np.int64), vec=iv)
    else:
        grid = int(info["grid"])
        stride = grid * ELT_THREADS
        nvec = n // VN
        iv = e // VN
        tail = e >= nvec * VN
        gid = np.where(tail, e - nvec * VN, iv % stride)
        out.update(block=gid // ELT_THREADS, tid=gid % ELT_THREADS, trip=np.where(tail, 0, iv // stride), crown=np.zeros(n, np.int64), stage_block=np.full(n, -1, np.int64),
                   tail=tail.astype(np.int64), vec=iv)
    out["wave"] = out["tid"] // 64
    return out


def stage_cells(info, N, dtype):
    """the cells of a k_dual_stage launch, from its record: dict(trips, pipe, vectors per stage, tiles per stage, last tile's vectors, idle trips of the
    last tile, odd trip count under the double-buffered loop, crown workgroups, crown vectors, vpn)"""
    trips, vpn, K, node0, bps, cb = (int(info[k]) for k in ("trips", "vpn", "K", "node0", "bps", "crownBlocks"))
    tile = ELT_THREADS * trips
    per_stage = K * vpn
    last = per_stage - (bps - 1) * tile
    crown_vec = node0 * vpn
    crown_last = crown_vec - (cb - 1) * tile if cb else 0
    return dict(trips=trips, pipe=int(info["pipe"]), stage_vectors=per_stage, tiles=bps, last_tile_vectors=last, idle_trips=trips - -(-last // ELT_THREADS),
                partial_tile=last < tile, odd_trips_pipe2=int(info["pipe"]) == 2 and trips % 2 == 1, crown_blocks=cb, crown_vectors=crown_vec,
                crown_idle_trips=(trips - -(-crown_last // ELT_THREADS)) if cb else 0, vpn=vpn, grid=int(info["grid"]), stages=(int(info["grid"]) - cb) // max(bps, 1))


def pick_pair(coord, eligible, pred):
    """the first pair (i < j) of eligible element indices for which pred(coord, i, js) holds (js an index array: pred is vectorised over the second
    element); None if there is none"""
    idx = np.flatnonzero(eligible)
    for a in idx:
        js = idx[idx > a]
        if js.size == 0:
            break
        hit = np.flatnonzero(pred(coord, int(a), js))
        if hit.size:
            return int(a), int(js[hit[0]])
    return None
