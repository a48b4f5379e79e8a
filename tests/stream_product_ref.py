"""What k_stream_gemv (csrc/k_stream.hpp) computes, restated in plain numpy: [m1_i; m2_i] = A_i w_i per node, from the STORED blocks.

reference()         the product from what Solver.getOperators() returns, exact for integer data (int64), np.longdouble otherwise; col_range
                    restricts the columns (the two partials of a block of the split last round)
magnitude()         sum_c |A_rc| |w_c| per row: the scale of the textbook error bound of a sum in any order
live_count_duals()  dual vectors whose per-node count of live units in one chunk of the walk runs through 0 .. U: one launch on a tree of U + 1
                    nodes meets every partial group and every tail of the group schedule, without the test restating the schedule
live_counts()       the counts a dual vector realises (any bit but the sign makes an entry live), chunk by chunk
group_size()        StreamDepth transcribed: used to assert that a shape reaches every cell, and to name the cells a case covered

Nothing here knows how the kernel schedules its loads: a unit is `unit_cols` consecutive columns, a chunk is `chunk_units` consecutive units of
the range a workgroup walks, and the units of the ragged last span (ny % G columns) are counted apart, as the walk treats them apart."""
import numpy as np

# k_stream_gemv<T, NL, SPLIT, NR, ST>: live units per group (spans; NL = 2: half-spans) by (form, NL, SPLIT, NR), transcribed from StreamDepth
# (RN_STREAM_D = 5, RN_STREAM_D_WIDE = 3).  Two right-hand sides exist unsplit only.
GROUP_SIZE = {
    ("f64", 1, False, 1): 5, ("f64", 1, True, 1): 4, ("f64", 2, False, 1): 10, ("f64", 2, True, 1): 8,
    ("f64", 3, False, 1): 3, ("f64", 3, True, 1): 3, ("f64", 4, False, 1): 3, ("f64", 4, True, 1): 3,
    ("f32", 1, False, 1): 5, ("f32", 1, True, 1): 4, ("f32", 2, False, 1): 10, ("f32", 2, True, 1): 8,
    ("f32", 3, False, 1): 3, ("f32", 3, True, 1): 3, ("f32", 4, False, 1): 3, ("f32", 4, True, 1): 3,
    ("f64_on_f32", 1, False, 1): 5, ("f64_on_f32", 1, True, 1): 4, ("f64_on_f32", 2, False, 1): 10, ("f64_on_f32", 2, True, 1): 8,
    ("f64_on_f32", 3, False, 1): 3, ("f64_on_f32", 3, True, 1): 3, ("f64_on_f32", 4, False, 1): 3, ("f64_on_f32", 4, True, 1): 3,
    ("f64", 1, False, 2): 5, ("f64", 2, False, 2): 10, ("f64", 3, False, 2): 3, ("f64", 4, False, 2): 3,
    ("f32", 1, False, 2): 4, ("f32", 2, False, 2): 7, ("f32", 3, False, 2): 2, ("f32", 4, False, 2): 1,
    ("f64_on_f32", 1, False, 2): 5, ("f64_on_f32", 2, False, 2): 10, ("f64_on_f32", 3, False, 2): 2, ("f64_on_f32", 4, False, 2): 1,
}


def group_size(form, NL, split, NR):
    return GROUP_SIZE[(form, int(NL), bool(split), int(NR))]


def cells(counts, group):
    """the (nHead, nGroups) cells of the schedule that chunks with these live counts run"""
    return {(int(n) % group, int(n) // group) for n in np.asarray(counts).ravel()}


def block_columns(blocks, nx, nu, nv):
    """[nodes][ny][2 nv]: column c of node i's block, rows 0 .. nv - 1 of [Phi | Psi] over rows nv .. 2 nv - 1 of [D | Ftil],
    from arrays in the reference's layout [nodes][columns][nv]"""
    nodes = np.asarray(blocks["Phi"]).shape[0]
    top = np.concatenate([np.asarray(blocks["Phi"]).reshape(nodes, 2 * nx, nv), np.asarray(blocks["Psi"]).reshape(nodes, nu, nv)], axis=1)
    bot = np.concatenate([np.asarray(blocks["D"]).reshape(nodes, 2 * nx, nv), np.asarray(blocks["Ftil"]).reshape(nodes, nu, nv)], axis=1)
    return np.concatenate([top, bot], axis=2)


def _integral(a):
    return bool(np.all(np.isfinite(a)) and np.all(a == np.rint(a)) and np.abs(a).max(initial=0) < 2 ** 31)


def _product(At, W, col_range):
    nodes, ny, rows = At.shape
    W = np.asarray(W, np.float64).reshape(nodes, ny)
    c0, c1 = (0, ny) if col_range is None else col_range
    At, W = At[:, c0:c1, :], W[:, c0:c1]
    if _integral(At) and _integral(W):      # exact: |sum| < 2^31 * 2^31 * ny is far from the cases here, which stay below 2^24
        return np.einsum("icr,ic->ir", At.astype(np.int64), W.astype(np.int64)).astype(np.float64)
    out = np.zeros((nodes, rows), np.longdouble)
    for i in range(nodes):      # (node by node: the temporaries of the wide shapes stay small)
        out[i] = (At[i].astype(np.longdouble) * W[i].astype(np.longdouble)[:, None]).sum(axis=0)
    return out


def reference(blocks, W, col_range=None):
    """[nodes][2 nv]: A_i w_i.  blocks: {"Phi", "Psi", "D", "Ftil"} as getOperators() returns them, or the [nodes][ny][2 nv] array of
    block_columns; W [nodes][ny]; col_range (c0, c1): the columns c0 <= c < c1 only.  int64 for integer data, np.longdouble otherwise."""
    At = blocks if isinstance(blocks, np.ndarray) else block_columns(blocks, *_dims(blocks, W))
    return _product(At, W, col_range)


def magnitude(blocks, W, col_range=None):
    """[nodes][2 nv]: sum_c |A_rc| |w_c|"""
    At = blocks if isinstance(blocks, np.ndarray) else block_columns(blocks, *_dims(blocks, W))
    return _product(np.abs(At), np.abs(np.asarray(W, np.float64)), col_range)


def _dims(blocks, W):
    """(nx, nu, nv) from the shapes: Phi is [nodes][2 nx * nv], Psi [nodes][nu * nv], W [nodes][2 nx + nu]"""
    nodes = np.asarray(blocks["Phi"]).shape[0]
    ny = np.asarray(W).size // nodes
    phi, psi = np.asarray(blocks["Phi"]).size // nodes, np.asarray(blocks["Psi"]).size // nodes
    nv = (phi + psi) // ny
    assert nv * ny == phi + psi and phi % (2 * nv) == 0, (phi, psi, ny)
    return phi // (2 * nv), psi // nv, nv


def whole_units(ny, G, unit_cols):
    """units of unit_cols columns that lie in whole spans of G columns: the ragged last span's are counted apart"""
    assert G % unit_cols == 0
    return (ny // G) * (G // unit_cols)


def live_counts(W, G, unit_cols, chunk_units=64, unit0=0, unit1=None):
    """(counts [nodes][chunks], ragged [nodes][units of the ragged span], live [nodes][units]) that W realises on the range [unit0, unit1) of units
    of unit_cols columns: live whole units per chunk of chunk_units units counted from unit0, liveness of the ragged last span's units (where the
    range holds it), and the liveness of every unit of the block.  Any bit but the sign makes an entry live."""
    W = np.asarray(W)
    nodes, ny = W.shape
    units = -(-ny // unit_cols)
    pad = np.zeros((nodes, units * unit_cols), bool)
    pad[:, :ny] = W != 0      # (-0.0 == 0: zero; a denormal != 0: live)
    live = pad.reshape(nodes, units, unit_cols).any(axis=2)
    whole = whole_units(ny, G, unit_cols)
    unit1 = units if unit1 is None else unit1
    end = min(unit1, whole)
    chunks = max(1, -(-(end - unit0) // chunk_units))
    counts = np.zeros((nodes, chunks), int)
    for c in range(chunks):
        counts[:, c] = live[:, unit0 + c * chunk_units:min(unit0 + (c + 1) * chunk_units, end)].sum(axis=1)
    ragged = live[:, whole:units] if unit1 > whole else live[:, :0]
    return counts, ragged, live


def chunk_capacity(ny, G, unit_cols, chunk, chunk_units=64, unit0=0, unit1=None):
    """(first unit, U): the whole units chunk `chunk` (negative: from the last) of the range holds"""
    whole = whole_units(ny, G, unit_cols)
    end = whole if unit1 is None else min(unit1, whole)
    chunks = max(1, -(-(end - unit0) // chunk_units))
    c = chunk % chunks
    first = unit0 + c * chunk_units
    return first, max(0, min(first + chunk_units, end) - first)


def live_count_duals(nodes, ny, G, unit_cols, chunk, seed, ragged=True, integer=True, chunk_units=64, unit0=0, unit1=None, want=None):
    """(W [nodes][ny], counts [nodes][chunks]): node i has exactly i mod (U + 1) live units in chunk `chunk` (negative: from the last) of the range
    [unit0, unit1) of units (default: the block), U the whole units that chunk holds; `want` [nodes] replaces that rule (-1: a random count).
    The positions are drawn per node from the seed; every other chunk of the range, and every unit outside it, gets a random live count; each
    unit of the ragged last span is live in half the nodes, independently (ragged=False: never).  A live unit has every entry nonzero in half
    the cases and a random non-empty subset otherwise.  Entries: nonzero integers in [-8, 8], or normal deviates (integer=False).  counts is
    what W REALISES (live_counts), not what was asked for."""
    rng = np.random.default_rng(seed)
    units = -(-ny // unit_cols)
    whole = whole_units(ny, G, unit_cols)
    first, U = chunk_capacity(ny, G, unit_cols, chunk, chunk_units, unit0, unit1)
    liveU = np.zeros((nodes, units), bool)
    end = min(whole if unit1 is None else unit1, whole)
    for i in range(nodes):
        liveU[i, :whole] = rng.random(whole) < rng.random()      # outside the range: unit by unit
        for f in range(unit0, end, chunk_units):                 # inside: a random count per chunk, at random positions
            n = min(chunk_units, end - f)
            liveU[i, f:f + n] = False
            liveU[i, f + rng.permutation(n)[:rng.integers(0, n + 1)]] = True
        k = i % (U + 1) if want is None else int(want[i])
        if k >= 0:
            assert k <= U, (k, U)
            liveU[i, first:first + U] = False
            liveU[i, first + rng.permutation(U)[:k]] = True
        if ragged:
            liveU[i, whole:] = rng.random(units - whole) < 0.5
    val = rng.integers(1, 9, (nodes, units * unit_cols)) * rng.choice([-1, 1], (nodes, units * unit_cols)) if integer else rng.standard_normal((nodes, units * unit_cols))
    val = val.astype(np.float64)
    val[val == 0] = 1.0
    keep = rng.random((nodes, units, unit_cols)) < 0.5
    keep[rng.random((nodes, units)) < 0.5] = True
    pos = rng.integers(0, unit_cols, (nodes, units))
    pos = np.minimum(pos, np.maximum(0, np.minimum(unit_cols, ny - np.arange(units) * unit_cols) - 1)[None, :])      # (a column the block has)
    np.put_along_axis(keep, pos[:, :, None], True, axis=2)                                                          # never an empty subset
    W = np.where(keep & liveU[:, :, None], val.reshape(nodes, units, unit_cols), 0.0).reshape(nodes, units * unit_cols)[:, :ny]
    W = np.ascontiguousarray(W)
    return W, live_counts(W, G, unit_cols, chunk_units, unit0, unit1)[0]


def split_pair(W, unit_cols, seed, integer=True):
    """(w, y): two vectors whose live units are DIFFERENT sets with the union W's: every live unit of W goes to w alone, to y alone or to
    both (a third each); y's entries are its own"""
    rng = np.random.default_rng(seed)
    nodes, ny = W.shape
    units = -(-ny // unit_cols)
    who = np.repeat(rng.integers(0, 3, (nodes, units)), unit_cols, axis=1)[:, :ny]
    val = (rng.integers(1, 9, W.shape) * rng.choice([-1, 1], W.shape)).astype(np.float64) if integer else rng.standard_normal(W.shape)
    val[val == 0] = 1.0
    w = np.where(who != 1, W, 0.0)
    y = np.where((who != 0) & (W != 0), val, 0.0)
    return np.ascontiguousarray(w), np.ascontiguousarray(y)
