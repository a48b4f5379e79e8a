"""The numpy side of tests/test_gpu_stream_product.py (stream_product_ref.py) is checked here, without a GPU: a reference that is wrong, or a
pattern that does not realise the live counts it is asked for, would make the GPU test pass or fail for the wrong reason."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import stream_product_ref as ref
from conftest import ROOT

# (ny, G, unit_cols, chunk_units): whole spans only; a ragged span of one unit; of two units; three chunks with a ragged span; spans walked whole
# in chunks of 32 (NL = 2 without the half-span skip)
SHAPES = [(240, 8, 4, 64), (201, 8, 4, 64), (236, 16, 8, 64), (1542, 64, 64, 64), (760, 4, 4, 64), (282, 8, 4, 64), (282, 8, 8, 32)]


@pytest.mark.parametrize("ny,G,ucols,cu", SHAPES)
@pytest.mark.parametrize("chunk", [0, -1])
def test_realised_live_counts_are_the_ones_asked_for(ny, G, ucols, cu, chunk):
    first, U = ref.chunk_capacity(ny, G, ucols, chunk, cu)
    nodes = U + 3
    for integer in (True, False):
        W, counts = ref.live_count_duals(nodes, ny, G, ucols, chunk, seed=5, integer=integer, chunk_units=cu)
        assert W.shape == (nodes, ny) and np.isfinite(W).all()
        whole = ref.whole_units(ny, G, ucols)
        chunks = -(-whole // cu)
        assert counts.shape == (nodes, chunks) and first == (chunk % chunks) * cu and U == min(cu, whole - first)
        assert np.array_equal(counts[:, chunk % chunks], np.arange(nodes) % (U + 1))      # every count 0 .. U, in the chosen chunk
        # counted again by hand: unit u of node i is live iff one of its columns is nonzero
        for i in (0, 1, nodes // 2, nodes - 1):
            live = [bool((W[i, u * ucols:(u + 1) * ucols] != 0).any()) for u in range(-(-ny // ucols))]
            for c in range(chunks):
                assert sum(live[c * cu:min((c + 1) * cu, whole)]) == counts[i, c], (i, c)
        other = np.delete(counts, chunk % chunks, axis=1)
        if other.size:
            assert other.min() >= 0 and len(np.unique(other)) > 3                          # the other chunks: random counts
        _, ragged, live = ref.live_counts(W, G, ucols, cu)
        assert ragged.shape == (nodes, -(-ny // ucols) - whole)
        if ragged.shape[1]:
            assert 0 < ragged[:, 0].sum() < nodes                                          # live in some nodes, dead in others
        if ragged.shape[1] == 2:
            assert len({tuple(r) for r in ragged}) == 4                                    # each half by itself
        if integer:
            assert np.array_equal(W, np.rint(W)) and np.abs(W).max() <= 8
        _, rag0, _ = ref.live_counts(ref.live_count_duals(nodes, ny, G, ucols, chunk, seed=5, ragged=False, chunk_units=cu)[0], G, ucols, cu)
        assert not rag0.any()


def test_counts_inside_a_range_of_units_and_a_given_rule():
    """the second workgroup of a split block walks [unit0, units): chunks are counted from unit0; `want` sets the counts, -1 leaves a node random"""
    ny, G, ucols, unit0 = 236, 8, 4, 24
    want = np.array([-1, -1] + list(range(24)))
    W, counts = ref.live_count_duals(len(want), ny, G, ucols, 0, seed=9, unit0=unit0, want=want)
    first, U = ref.chunk_capacity(ny, G, ucols, 0, unit0=unit0)
    assert (first, U) == (24, 58 - 24)
    assert np.array_equal(counts[2:, 0], want[2:])
    front = ref.live_counts(W, G, ucols, unit1=unit0)[0]
    assert len(np.unique(front)) > 3                                                       # the other half: random
    W1, c1 = ref.live_count_duals(len(want), ny, G, ucols, 0, seed=9, unit1=unit0, want=want)
    assert np.array_equal(c1[2:, 0], want[2:]) and ref.live_counts(W1, G, ucols, unit1=unit0)[1].shape[1] == 0


def small_case(integer, seed=3, nodes=3, nx=2, nu=3, nv=2):
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.integers(-4, 5, s).astype(float)) if integer else (lambda *s: rng.standard_normal(s))
    blocks = {"Phi": draw(nodes, 2 * nx * nv), "Psi": draw(nodes, nu * nv), "D": draw(nodes, 2 * nx * nv), "Ftil": draw(nodes, nu * nv)}
    W = draw(nodes, 2 * nx + nu)
    return blocks, W, (nodes, nx, nu, nv)


def fraction_gemv(blocks, W, dims, c0=0, c1=None):
    """A_i w_i in exact rationals, from the layout written out entry by entry: operator `op` of node i is col-major nv x columns"""
    nodes, nx, nu, nv = dims
    ny = 2 * nx + nu
    out = np.empty((nodes, 2 * nv), object)
    for i in range(nodes):
        for r in range(2 * nv):
            s = Fraction(0)
            for c in range(c0, ny if c1 is None else c1):
                name = ("Phi" if r < nv else "D") if c < 2 * nx else ("Psi" if r < nv else "Ftil")
                col = c if c < 2 * nx else c - 2 * nx
                s += Fraction(float(blocks[name][i][col * nv + r % nv])) * Fraction(float(W[i][c]))
            out[i, r] = s
    return out


@pytest.mark.parametrize("integer", [True, False])
def test_reference_is_a_rational_gemv(integer):
    blocks, W, dims = small_case(integer)
    got, want = ref.reference(blocks, W), fraction_gemv(blocks, W, dims)
    assert got.shape == want.shape and got.dtype == (np.float64 if integer else np.longdouble)
    mag = ref.magnitude(blocks, W)
    wantMag = fraction_gemv({k: np.abs(v) for k, v in blocks.items()}, np.abs(W), dims)
    for i in range(dims[0]):
        for r in range(2 * dims[3]):
            if integer:
                assert Fraction(float(got[i, r])) == want[i, r] and Fraction(float(mag[i, r])) == wantMag[i, r]
            else:      # seven terms in long double: a few units of its 2^-64
                g = Fraction(*[int(v) for v in np.longdouble(got[i, r]).as_integer_ratio()])
                assert abs(g - want[i, r]) <= 8 * Fraction(1, 2 ** 64) * wantMag[i, r]
                assert abs(Fraction(float(mag[i, r])) - wantMag[i, r]) <= Fraction(1, 2 ** 50) * wantMag[i, r]


@pytest.mark.parametrize("integer", [True, False])
def test_column_ranges_add_up_to_the_whole(integer):
    blocks, W, dims = small_case(integer, seed=4, nodes=4, nx=3, nu=4, nv=3)
    ny = 2 * dims[1] + dims[2]
    whole = ref.reference(blocks, W)
    for cut in (0, 1, 5, ny - 1, ny):
        a, b = ref.reference(blocks, W, (0, cut)), ref.reference(blocks, W, (cut, ny))
        part = fraction_gemv(blocks, W, dims, 0, cut)
        if integer:
            assert np.array_equal(a + b, whole)
            assert all(Fraction(float(a[i, r])) == part[i, r] for i in range(dims[0]) for r in range(2 * dims[3]))
        else:
            assert np.abs(a + b - whole).max() <= 4 * np.finfo(np.longdouble).eps * np.abs(ref.magnitude(blocks, W)).max()
    assert not ref.reference(blocks, W, (2, 2)).any()


def test_group_sizes_follow_stream_depth():
    """the transcribed table against StreamDepth's rule restated, with the two depths read from csrc/common.hpp"""
    src = open(os.path.join(ROOT, "rapidnet_amd", "csrc", "common.hpp")).read()
    D = int(re.search(r"#define\s+RN_STREAM_D\s+(\d+)", src).group(1))
    DW = int(re.search(r"#define\s+RN_STREAM_D_WIDE\s+(\d+)", src).group(1))
    seen = set()
    for form in ("f64", "f32", "f64_on_f32"):
        native, four = form != "f64_on_f32", form == "f32"
        for NL in (1, 2, 3, 4):
            for split, NR in ((False, 1), (True, 1), (False, 2)):
                short = NR == 2 and (four if native else NL >= 3)
                d0 = (D - 1 if split else D) if NL <= 2 else DW
                d = (1 if NL == 4 else d0 - 1) if short else d0
                du = 2 * d - (1 if native and short else 0)
                assert ref.group_size(form, NL, split, NR) == (du if NL == 2 else d), (form, NL, split, NR)
                seen.add((form, NL, split, NR))
    assert seen == set(ref.GROUP_SIZE)
    assert ref.cells(range(15), 3) == {(h, g) for h in range(3) for g in range(5)}


def test_pair_of_vectors_has_different_live_sets_with_the_given_union():
    W, _ = ref.live_count_duals(40, 201, 8, 4, 0, seed=2)
    w, y = ref.split_pair(W, 4, seed=8)
    lw, ly, lu = (ref.live_counts(v, 8, 4)[2] for v in (w, y, W))
    assert np.array_equal(lw | ly, lu) and (lw & ~ly).any() and (ly & ~lw).any() and (lw & ly).any()
    assert np.array_equal(y, np.rint(y)) and np.abs(y).max() <= 8
