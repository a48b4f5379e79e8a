"""tests/slab_product_ref.py on the CPU: the reference products against a loop over the definition, the integer builder's exactness assertion,
the launch rules against values worked out by hand from the comments in sweep.inc / rapidnet_capi.hip, the cell function on hand-made
inputs, and the deliberate mistakes -- each must change its named case and leave an interior case untouched."""
import numpy as np
import pytest

import slab_product_ref as ref


def loop_product(M, X, p=None, aux=None, aux2=None, split=None):
    """the definition, one scalar at a time, in Python's exact rationals where the data are integers and in longdouble otherwise"""
    m, k = M.shape
    out = np.zeros((X.shape[0], m), dtype=np.longdouble)
    for i in range(X.shape[0]):
        s = np.longdouble(1) if p is None else np.longdouble(-0.5) / np.longdouble(p[i])
        for r in range(m):
            acc = np.longdouble(0)
            for c in range(k):
                acc += np.longdouble(M[r, c]) * np.longdouble(X[i, c])
            out[i, r] = s * acc + (0 if aux is None else np.longdouble(aux[i, r])) + (np.longdouble(aux2[i - split, r]) if aux2 is not None and i >= split else 0)
    return out


@pytest.mark.parametrize("form", ["f64", "f32"])
def test_integer_products_are_int64_and_equal_the_definition(form):
    d = ref.integer_data(1, form, 21, (17, 37), aux_rows=34, split=18, second=(9, 17))
    v, lv = ref.pair(d["MA"], d["MB"], d["X"], d["p"], d["aux"], d["aux2"], 18)
    assert v[0].dtype == np.int64 and lv[0].dtype == np.int64
    want_v = loop_product(d["MA"], d["X"], d["p"], d["aux"], d["aux2"], 18)
    assert np.array_equal(v[0], want_v)
    assert np.array_equal(lv[0], loop_product(d["MB"], want_v))
    assert (np.abs(v[0]) <= v[1]).all() and (np.abs(lv[0]) <= lv[1]).all() and d["worst"] < ref.EXACT_BELOW[form]


def test_real_products_equal_the_definition_and_carry_their_magnitudes():
    d = ref.real_data(2, "f32", 5, (19, 23), aux_rows=19)
    for key in ("MA", "X", "p", "aux"):
        assert np.array_equal(d[key], d[key].astype(np.float32).astype(np.float64)), key
    val, mag = ref.product(d["MA"], d["X"], d["p"], d["aux"])
    assert val.dtype == np.longdouble
    want = loop_product(d["MA"], d["X"], d["p"], d["aux"])
    assert np.max(np.abs(val - want)) <= 64 * np.finfo(np.longdouble).eps * mag.max()
    want_mag = np.abs(d["aux"]) + (0.5 / d["p"])[:, None] * (np.abs(d["X"]) @ np.abs(d["MA"]).T)
    assert np.allclose(mag.astype(float), want_mag, rtol=1e-12)
    assert ref.bound(mag, 23, "f32").shape == val.shape and np.isclose(float(ref.bound(mag, 23, "f32")[0, 0]), 27 * 2.0 ** -24 * float(mag[0, 0]))


def test_integer_builder_narrows_until_the_sums_are_exact():
    """a wide fp32 pair: rows of about 2.2 * 4.4 * 1050 * 4 (the scale) = 40 000 in the first product, times 400 * 2.2 in the second, is above 2^24 at r = 4"""
    d = ref.integer_data(3, "f32", 5, (400, 1050), aux_rows=400, second=(60, 400))
    assert max(np.abs(d["MA"]).max(), np.abs(d["MB"]).max()) < 4 and d["worst"] < 2 ** 24
    v, lv = ref.pair(d["MA"], d["MB"], d["X"], d["p"], d["aux"])
    assert lv[1].max() < 2 ** 24
    # in float32 arithmetic, in two different orders, the products are then the int64 values
    X32, M32 = d["X"].astype(np.float32), d["MA"].astype(np.float32)
    fwd = np.zeros((5, 400), np.float32)
    bwd = np.zeros((5, 400), np.float32)
    for c in range(1050):
        fwd += X32[:, c:c + 1] * M32[:, c][None, :]
        bwd += X32[:, 1049 - c:1050 - c] * M32[:, 1049 - c][None, :]
    s = (-0.5 / d["p"]).astype(np.float32)[:, None]
    assert np.array_equal((d["aux"].astype(np.float32) + s * fwd).astype(np.int64), v[0]) and np.array_equal(fwd, bwd)
    big = ref.integer_data(3, "f64", 5, (400, 1050), aux_rows=400, second=(60, 400))
    assert np.abs(big["MA"]).max() == 4      # fp64 has the room


def test_signed_patterns_isolate_columns_and_the_last_row():
    d = ref.signed_patterns(12, (33, 81), second=(20, 33))
    nz = [np.flatnonzero(row) for row in d["X"]]
    assert all(len(z) == 1 for z in nz) and {int(z[0]) for z in nz} == {80, 64, 63, 0}      # k - 1, k - 17 = 64, the chunk edge, 0
    assert (np.abs(d["MA"][:-1]) <= 7).all() and (d["MA"][-1] >= 9).all() and (d["MA"] != 0).all()
    val, _ = ref.product(d["MA"], d["X"], d["p"])
    assert val.dtype == np.int64 and (val != 0).all()      # every row of every node carries its one column


def test_prep_slab_follows_the_dual_layout():
    nx, nu, nodes = 2, 3, 4
    diag = np.arange(1, 2 * (2 * nx + nu) + 1, dtype=float).reshape(2, -1)      # stage rows (d_u | d_x | d_xs)
    stage, p = np.array([0, 1, 1, 1]), np.array([1.0, 0.25, 0.25, 0.5])
    W = np.arange(1, nodes * (2 * nx + nu) + 1, dtype=float).reshape(nodes, -1)
    slab, mag = ref.prep_slab(W, stage, p, diag, nx, nu, "f64")
    i = 2      # stage 1: d_u = 8 9 10, d_x = 11 12, d_xs = 13 14; sqrt(p) = 0.5; W row = 15 .. 21 = (xi_x 15 16 | xi_xs 17 18 | psi 19 20 21)
    assert np.allclose(slab[i].astype(float), [0.5 * (11 * 15 + 13 * 17), 0.5 * (12 * 16 + 14 * 18), 0.5 * 8 * 19, 0.5 * 9 * 20, 0.5 * 10 * 21])
    assert np.array_equal(mag, np.abs(mag)) and (mag >= np.abs(slab)).all()
    M = np.arange(1, 11, dtype=float).reshape(2, 5)
    (m2, _), (qa, _) = ref.prep_m2(M, W, stage, p, diag, nx, nu, "f64")
    assert np.allclose(m2.astype(float), slab.astype(float) @ M.T) and np.array_equal(qa, slab[:, :nx])
    s32 = ref.prep_slab(W, stage, np.array([1.0, 0.3, 0.3, 0.5]), diag, nx, nu, "f32")[0]
    assert np.isclose(float(s32[i, 2]), float(np.float32(np.sqrt(0.3))) * 8 * 19, rtol=1e-15)      # sqrt in double, THEN rounded


def test_padding_and_stride_by_hand():
    assert [ref.pad_cols(k) for k in (1, 4, 16, 17, 48, 64, 65)] == [16, 16, 16, 32, 48, 64, 80]
    assert [ref.pad_rows(m) for m in (1, 16, 17, 64, 65, 490)] == [64, 64, 64, 64, 128, 512]
    # >= kp and = 4 (mod 64): 16 -> 68, 64 -> 68 (60 elements of slack are enough), 65 .. 124 -> 132
    assert [ref.slab_stride(kp) for kp in (16, 48, 64, 80, 240, 192)] == [68, 68, 68, 132, 260, 196]
    assert all(ref.slab_stride(kp) >= kp and ref.slab_stride(kp) % 64 == 4 for kp in range(16, 2048, 16))
    assert 16 * (260 + 196) * 8 == 58368      # the fp64 pair of nx 60, nu 200, ne 20: 57 KB of the 64


@pytest.mark.parametrize("tiles_a,ks_a,tiles_b,ks_b,nodes,want,why", [
    (1, 4, 1, 4, 5, 4, "one tile each: every count has the path 8, the smallest wins"),
    (3, 20, 5, 12, 33, 6, "nx 20 nu 46 ne 1: 4 waves 20 + 2 * 12 = 44, 6 and 8 waves 32"),
    (6, 32, 9, 24, 17, 6, "nx 40 nu 90 ne 5: 4 waves 2 * 32 + 3 * 24 = 136, 6 and 8 waves 32 + 48 = 80"),
    (12, 60, 17, 48, 17, 6, "nx 60 nu 200 ne 20: 4 waves 3 * 60 + 5 * 48 = 420, 6 and 8 waves 2 * 60 + 3 * 48 = 264"),
    (7, 44, 12, 24, 16 * 256, 8, "Barcelona, one slab per CU: 6 waves 2 * 44 + 2 * 24 = 136, 8 waves 44 + 48 = 92"),
    (7, 44, 12, 24, 16 * 256 + 1, 4, "Barcelona, more slabs than CUs: nw * path = 4 * 160 = 640, 6 * 136 = 816, 8 * 92 = 736"),
    (1, 4, 1, 4, 4100, 4, "throughput rule on the small network: 4 * 8 against 6 * 8"),
])
def test_slab_waves_by_hand(tiles_a, ks_a, tiles_b, ks_b, nodes, want, why):
    assert ref.slab_waves(tiles_a, ks_a, tiles_b, ks_b, nodes, 256) == want, why


def test_loop_and_wide_rules_by_hand():
    assert ref.few_slabs(16 * 256, 256, "f64") and not ref.few_slabs(16 * 256 + 1, 256, "f64") and ref.few_slabs(10 ** 6, 256, "f32")
    assert not ref.few_slabs(5, 256, "f32", knob=0) and ref.few_slabs(10 ** 6, 256, "f64", knob=1)
    assert ref.wide_ct(16 * 4 * 256, 256, 30000) == 0 and ref.wide_ct(16 * 4 * 256 + 1, 256, 30000) == 3      # more than four slabs per CU
    assert ref.wide_ct(33, 256, 30000, knob=2) == 2 and ref.wide_ct(33, 256, 58368, knob=3) == 2 and ref.wide_ct(33, 256, 90000, knob=3) == 0
    assert ref.wide_ct(33, 256, 30000, knob=1) == 0


def test_expected_launch_by_hand():
    e = ref.expected_launch("f64", 33, 256, (45, 65), (66, 45))
    assert e == {"m": 45, "k": 65, "kp": 80, "m2": 66, "k2": 45, "kp2": 48, "kernel": "k_gemm_vlv", "kernel2": None, "nw": 6, "pipe": 1, "frag": 1, "ct": 1, "grid": 3,
                 "lds": 16 * (132 + 68) * 8}
    e = ref.expected_launch("f64", 49, 256, (45, 65), (66, 45), knobs={"vlv_wide": 3, "slab_frag": 0})
    assert (e["kernel"], e["ct"], e["grid"], e["lds"], e["frag"], e["nw"]) == ("k_gemm_vlv_wide", 3, 2, 3 * 16 * 200 * 8, 0, 8)
    # nx 30, nu 500, ne 10 in fp64: k_V = 520 -> stride 580, 74 240 bytes > 64 KB: the tile kernel, 512 / 64 = 8 row groups per 16 nodes
    e = ref.expected_launch("f64", 5, 256, (490, 520), (530, 490))
    assert (e["kernel"], e["grid"], e["kernel2"], e["grid2"], e["lds"]) == ("k_gemm_shared", 8, "k_gemm_shared", 9, 0)
    e = ref.expected_launch("f32", 5, 256, (490, 520), (530, 490))      # fp32: 16 * (580 + 516) * 4 = 70 144 > 64 KB, each alone fits
    assert (e["kernel"], e["kernel2"], e["lds"], e["lds2"]) == ("k_gemm_slab", "k_gemm_slab", 16 * 580 * 4, 16 * 516 * 4)
    e = ref.expected_launch("f64", 20, 256, (177, 177), kind="comp")
    assert (e["kernel"], e["nw"], e["kp"], e["grid"]) == ("k_gemm_comp", 6, 192, 2)      # 12 tiles: 6 waves carry 2 each


INFO0 = {"kernel2": None, "m2": 0, "k2": 0, "kp2": 0, "ldin2": 0, "nw2": 0, "grid2": 0, "lds2": 0, "inOffset": 0, "ct": 0, "frag": 1}


def test_cells_on_hand_made_inputs():
    info = dict(INFO0, kernel="k_gemm_vlv", m=45, k=65, kp=80, ldin=65, m2=66, k2=45, kp2=48, ldin2=45, nw=6, pipe=1, grid=3, ct=1)
    c = ref.cells({"nodes": 33, "form": "f64"}, info, stored_v=False, aux=True)
    assert {"f64", "V: k_gemm_vlv", "V: G=>2", "V: pipelined G%3=2", "V: chunks/row=2", "V: tg=1", "V: idle waves", "V: k%16=1", "V: k%4!=0", "V: m%4!=0", "L: G=>2",
            "L: pipelined G%3=0", "L: chunks/row=1", "L: tg=1", "L: idle waves", "v tile in LDS, v not stored", "V: aux yes", "frag", "last slab 1 node"} <= c, sorted(c)
    assert "rotation b>=8" not in c and "L: have remainder" not in c
    # 9 tiles on 6 waves: three waves carry two tiles, three carry one
    info = dict(info, m2=130, k2=85, kp2=96, m=85, k=125, kp=128, grid=9, pipe=0)
    c = ref.cells({"nodes": 129, "form": "f32"}, info, split=True)
    assert {"L: tg=2", "L: have remainder", "V: tg=1", "V: lean", "rotation b>=8", "V: aux split", "V: G=>2", "last slab 1 node"} <= c and "L: idle waves" not in c, sorted(c)
    wide = dict(info, kernel="k_gemm_vlv_wide", ct=2, grid=2, nw=8, pipe=1)
    assert "wide CT=2 last workgroup: 2 slab(s), last slab 15 nodes" in ref.cells({"nodes": 63, "form": "f64"}, wide)
    assert "wide CT=2 last workgroup: 1 slab(s), last slab 1 node" in ref.cells({"nodes": 33, "form": "f64"}, wide)
    lin = dict(INFO0, kernel="k_gemm_comp", m=177, k=177, kp=192, ldin=265, inOffset=88, nw=6, pipe=1, grid=260)
    c = ref.cells({"nodes": 4150, "form": "f64"}, lin, aux=False)
    assert {"C: k_gemm_comp", "ldin != k, offset > 0", "C: aux none", "rotation b>=256", "C: tg=2", "C: m%16=1", "C: k%16=1"} <= c, sorted(c)
    sh = dict(INFO0, kernel="k_gemm_shared", m=490, k=520, kp=528, ldin=520, nw=4, pipe=0, grid=8, frag=0)
    c = ref.cells({"nodes": 5, "form": "f64"}, sh)
    assert {"S: k_gemm_shared", "S: shared mp/64=8", "S: shared K quarters even"} <= c and not any("rotation" in x or "last slab" in x for x in c), sorted(c)
    two = dict(INFO0, kernel="k_gemm_shared", kernel2="k_gemm_slab", m=400, k=800, kp=800, ldin=800, m2=820, k2=400, kp2=400, ldin2=400, nw=4, nw2=8, pipe=0, grid=7, grid2=1, frag=0)
    c = ref.cells({"nodes": 11, "form": "f64"}, two, pipe2=True)      # the tile kernel in front of a slab launch that runs the pipelined loop
    assert {"V: k_gemm_shared", "L: k_gemm_slab", "L: pipelined G%3=1", "L: several passes", "L: tg=3"} <= c and "L: lean" not in c, sorted(c)


# ---- the deliberate mistakes ---------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return not np.array_equal(a[0], b[0])


def test_mistake_last_group_dropped_when_G_mod_3_is_2():
    named = ref.integer_data(10, "f32", 5, (45, 65))      # kp = 80: G = 5
    interior = ref.integer_data(10, "f32", 5, (45, 48))      # G = 3
    assert _differs(ref.mistake_drop_last_group(named["MA"], named["X"], named["p"]), ref.product(named["MA"], named["X"], named["p"]))
    assert not _differs(ref.mistake_drop_last_group(interior["MA"], interior["X"], interior["p"]), ref.product(interior["MA"], interior["X"], interior["p"]))
    pat = ref.signed_patterns(5, (45, 65))      # the pattern's column k - 1 = 64 alone sits in the dropped group
    got, want = ref.mistake_drop_last_group(pat["MA"], pat["X"], pat["p"])[0], ref.product(pat["MA"], pat["X"], pat["p"])[0]
    assert not got[0].any() and want[0].all() and np.array_equal(got[2], want[2])      # node 0 reads column 64, node 2 column 63


def test_mistake_last_tile_rows_at_m_minus_1():
    named = ref.signed_patterns(5, (17, 16))
    interior = ref.signed_patterns(5, (32, 16))
    got, want = ref.mistake_last_tile_rows(named["MA"], named["X"], named["p"]), ref.product(named["MA"], named["X"], named["p"])
    assert not _differs(got, want)      # one row in the last tile: taking it at m - 1 is right, the case that needs m = 16 t + 2 ...
    named = ref.signed_patterns(5, (18, 16))
    got, want = ref.mistake_last_tile_rows(named["MA"], named["X"], named["p"]), ref.product(named["MA"], named["X"], named["p"])
    assert _differs(got, want) and np.array_equal(got[0][:, :16], want[0][:, :16]) and np.array_equal(got[0][:, 17], want[0][:, 17])
    assert not _differs(ref.mistake_last_tile_rows(interior["MA"], interior["X"], interior["p"]), ref.product(interior["MA"], interior["X"], interior["p"]))


def test_mistake_stale_v_tile_of_a_partial_last_slab():
    named = ref.integer_data(11, "f64", 17, (17, 20), aux_rows=34, second=(21, 17))
    interior = ref.integer_data(11, "f64", 16, (17, 20), aux_rows=34, second=(21, 17))
    a = lambda d: (d["MA"], d["MB"], d["X"], d["p"], d["aux"])      # noqa: E731
    assert _differs(ref.mistake_stale_v_tile(*a(named))[1], ref.pair(*a(named))[1]) and not _differs(ref.mistake_stale_v_tile(*a(named))[0], ref.pair(*a(named))[0])
    assert not _differs(ref.mistake_stale_v_tile(*a(interior))[1], ref.pair(*a(interior))[1])


def test_mistake_aux2_indexed_by_the_node():
    named = ref.integer_data(12, "f64", 20, (17, 20), aux_rows=34, split=14)
    got = ref.mistake_aux2_index(named["MA"], named["X"], named["p"], named["aux"], named["aux2"], 14)
    want = ref.product(named["MA"], named["X"], named["p"], named["aux"], named["aux2"], 14)
    assert _differs(got, want) and np.array_equal(got[0][:14], want[0][:14])      # the nodes in front of the split have no second partial
    interior = ref.integer_data(12, "f64", 20, (17, 20), aux_rows=34)
    assert not _differs(ref.mistake_aux2_index(interior["MA"], interior["X"], interior["p"], interior["aux"]), ref.product(interior["MA"], interior["X"], interior["p"], interior["aux"]))


def test_mistake_input_read_with_ldin_equal_k():
    d = ref.integer_data(13, "f64", 6, (9, 7))
    rows = np.full((6, 12), 7777.0)      # the linear form: k = nx + nu = 7 columns at offset nv = 5 of rows of 12
    rows[:, 5:] = d["X"]
    got, want = ref.mistake_ldin_is_k(d["MA"], rows, 5, d["p"]), ref.product(d["MA"], d["X"], d["p"])
    assert _differs(got, want) and np.array_equal(got[0][0], want[0][0])      # node 0 is read at the right place either way
    dense = np.ascontiguousarray(d["X"])      # ldin = k, offset 0: the interior case
    assert not _differs(ref.mistake_ldin_is_k(d["MA"], dense, 0, d["p"]), want)
