"""Per-stage error measure for tree-shaped iterates (test infrastructure, like numpy_engine.py).

A global relmax divides the worst error by the largest reference value of the whole tree.  The dual-side vectors (xi, psi,
primalXi, dualXi, updXi, resPsi, ...) carry the preconditioner's factor sqrt(p_i), which is 1/64 at the leaves of a 4 096-scenario
tree, so a global relmax dilutes a leaf-stage error up to 64x against a root-stage one.  stage_relmax measures every stage against
its own scale, with a floor of 1e-3 of the tree's scale so that components that sit at rounding level (psi when no input bound is
active) do not compare noise with noise."""
import numpy as np

FLOOR = 1e-3


def node_stages(tree):
    return np.asarray(tree["stages"], int).ravel()[: int(np.asarray(tree["nodes"]).ravel()[0])]


def stage_relmax(got, ref, tree, dim, floor=FLOOR, scale=None, family_max=0.0):
    """[max |got - ref| over the nodes of stage k / max(max |ref| over stage k, floor * max |ref| over the tree) for every stage k]

    scale: an array of ref's shape whose magnitudes set the scale in place of ref's.  A fixed-point residual res = primal - dual
    goes to zero as APG converges while its rounding error stays at the size of primal: it is measured against primal.
    family_max: the largest |.| of the whole vector that ref is one half of (xi / psi are the two halves of one dual vector); the
    floor is taken from it too, so that a half that sits at rounding level throughout (psi when no input bound is active) is
    measured against the vector's scale."""
    stages = node_stages(tree)
    got = np.asarray(got, float).reshape(len(stages), dim)
    ref = np.asarray(ref, float).reshape(len(stages), dim)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    err = np.abs(got - ref).max(axis=1)
    mag = np.abs(ref if scale is None else np.asarray(scale, float).reshape(len(stages), dim)).max(axis=1)
    n_stage = int(stages.max()) + 1
    err_k, mag_k = np.zeros(n_stage), np.zeros(n_stage)
    np.maximum.at(err_k, stages, err)
    np.maximum.at(mag_k, stages, mag)
    return err_k / np.maximum(np.maximum(mag_k, floor * max(mag.max(), family_max)), 1e-300)


def worst_stage(got, ref, tree, dim, scale=None):
    """(worst per-stage error, the stage it is in)"""
    e = stage_relmax(got, ref, tree, dim, scale=scale)
    k = int(np.argmax(e))
    return float(e[k]), k


# the buffer whose magnitudes scale each buffer's error: a residual is measured against the primal it is the difference of
SCALE_OF = {"resXi": "primalXi", "resPsi": "primalPsi"}
# the halves of one vector: the dual iterates (y) and the vectors of its image (z)
FAMILIES = (("xi", "psi", "accXi", "accPsi", "updXi", "updPsi"), ("primalXi", "primalPsi", "dualXi", "dualPsi", "resXi", "resPsi"))
# the per-node dimension of every iterate, as a key of dims(nx, nu, nv)
DIM_OF = {"x": "nx", "u": "nu", "v": "nv", "xi": "2nx", "psi": "nu", "accXi": "2nx", "accPsi": "nu", "updXi": "2nx",
          "updPsi": "nu", "primalXi": "2nx", "primalPsi": "nu", "dualXi": "2nx", "dualPsi": "nu", "resXi": "2nx", "resPsi": "nu"}


def worst_by_buffer(got, ref, tree, nx, nu, nv):
    """{name: worst per-stage error} of the buffers in got (dict name -> array) against ref (a dict with at least the same names).
    Residuals are scaled by their primal when ref holds it; the floor of a half of the dual vector (or of its image) is taken
    from the largest |.| over the halves that ref holds."""
    dims = {"nx": nx, "nu": nu, "nv": nv, "2nx": 2 * nx}
    fam = {}
    for f in FAMILIES:
        present = [nm for nm in f if nm in ref]
        if present:
            m = max(float(np.abs(np.asarray(ref[nm])).max()) for nm in present)
            fam.update({nm: m for nm in present})
    out = {}
    for nm, g in got.items():
        sc = ref.get(SCALE_OF.get(nm, ""))
        out[nm] = float(stage_relmax(g, ref[nm], tree, dims[DIM_OF[nm]], scale=sc, family_max=fam.get(nm, 0.0)).max())
    return out
