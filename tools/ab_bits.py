#!/usr/bin/env python3
"""Bit-for-bit A/B of two BUILDS of the library, the sibling of tools/ab_lib.sh (which times them): the tree's own against
rapidnet_amd/librapidnet_hip_<variant>.so (e.g. the previous commit's, built as ab_lib.sh says).  Every case runs in one fresh child process per
library, each under a time limit of its own: apgIterate in batches of 20, 17 and 3 (optimistic, optimistic, exact), then the history, the batch
counters and the fifteen buffers of tests/test_gpu_fused_walk_dual.py, compared with np.array_equal.  The cases are the small trees of the suite
that reach every chain walk: k_up_chain / k_down_chain / k_down_chain_dual (dense, structured, fp32, a batch that trips and is replayed through the
exact path, 1 / 3 / L workgroups per chain), k_up_chain_cut and the crown-writer workgroups (in-process ranks), the SPLIT up-walks (trees of
numCUs + r nodes).  One line per case; the first child that ends with a nonzero status ends the run; the status is nonzero when any case differs.

    python3 tools/ab_bits.py <variant> [--out profiles/ab_walk_bits.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

INFEASIBLE = {"penalty_x": 20.0, "penalty_xs": 5.0}
# (problem, make_problem arguments, Solver arguments, in-process ranks)
SINGLE = [("medium", {}, {}, 0), ("medium", {}, {"structured": True}, 0), ("medium", {}, {"precision": "f32"}, 0), ("ragged", {}, {"structured": True}, 0),
          ("barcelona31", {}, {}, 0), ("late", {}, {}, 0), ("widecrown", {}, {}, 0), ("barcelona31_infeasible", INFEASIBLE, {}, 0)]
RANKED = [("medium", {}, {}, 2), ("medium", {}, {}, 4), ("ragged", {}, {}, 3)]
CASES = [(n, kw, sk, w, fuse) for n, kw, sk, w in SINGLE + RANKED + [("split", {}, {}, 0), ("split", {}, {}, 2)] for fuse in "01"] + \
        [("medium", {}, {"knobs": {"fuse_split": n}}, 0, "1") for n in (1, 3, 1000)]
BATCHES = (20, 17, 3)


def child(index, out):
    """one case on the library $RAPIDNET_LIB names (the tree's own when unset): everything it computed into `out`"""
    import test_gpu_stream_split as split
    from rapidnet_amd import capi, synth
    from test_gpu_fused_walk_dual import BUFS
    from test_gpu_sharded_batched import Ranks

    name, kw, skw, world, fuse = CASES[index]
    os.environ["RAPIDNET_FUSE_DOWN_DUAL"] = fuse
    cut = 0
    if name == "split" and world:      # two shards whose merged up-walk adds the second partials (k_up_chain_cut<SPLIT>)
        p, fc, cut, _ = split.sharded_split_problem()
    elif name == "split":              # k_up_chain<SPLIT>: the split round spans three stages, odd group count, ragged span
        p, fc = split.problem("b236", "three")
    else:
        p = synth.make_problem(name, **kw)
        fc = synth.forecast_at(p["forecast"], 0)

    def solve(s):
        s.initialiseSmpcController(*fc)
        s.apgReset()
        hist = np.concatenate([s.apgIterate(n) for n in BATCHES])
        return dict({"buf%d" % b: s.get(b) for b in BUFS}, hist=hist, counters=np.array(json.dumps(s.counters(), sort_keys=True)),
                    split=np.array(json.dumps(s.streamInfo(), sort_keys=True)))

    if world:
        rk = Ranks(p, world, cut, **skw)
        try:
            res = {"r%d_%s" % (r, k): v for r, d in enumerate(rk.run(solve)) for k, v in d.items()}
        finally:
            rk.close()
    else:
        s = capi.Solver(p["network"], p["tree"], p["config"], **skw)
        res = solve(s)
        s.close()
    np.savez(out, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_walk_bits.txt"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--child", nargs=2, metavar=("CASE", "FILE"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(int(args.child[0]), args.child[1])
    other = os.path.join(ROOT, "rapidnet_amd", "librapidnet_hip_%s.so" % args.variant)
    assert os.path.exists(other), other
    lines, bad = ["# tools/ab_bits.py %s: the tree's library against %s; apgIterate %s, history + counters + 15 buffers per context" % (args.variant, os.path.basename(other), BATCHES)], 0
    with tempfile.TemporaryDirectory() as tmp:
        for i, (name, kw, skw, world, fuse) in enumerate(CASES):
            got = []
            for tag, lib in (("tree", None), (args.variant, other)):
                env = {k: v for k, v in os.environ.items() if k != "RAPIDNET_LIB"}
                if lib:
                    env["RAPIDNET_LIB"] = lib
                f = os.path.join(tmp, "%d_%s.npz" % (i, tag))
                rc = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), args.variant, "--child", str(i), f], env=env).returncode
                if rc != 0:
                    lines.append("case %d (%s): the child on the %s library ended with status %d -- stopped here" % (i, name, tag, rc))
                    print(lines[-1], flush=True)
                    open(args.out, "w").write("\n".join(lines) + "\n")
                    return 2
                got.append(dict(np.load(f)))
            a, b = got
            diff = sorted(k for k in set(a) | set(b) if k not in a or k not in b or not np.array_equal(a[k], b[k]))
            bad += bool(diff)
            info = json.loads(str(a.get("split", a.get("r0_split"))))
            what = " ".join("%s=%s" % kv for d in (kw, skw.get("knobs", {}), {k: v for k, v in skw.items() if k != "knobs"}) for kv in d.items())
            lines.append("%-22s %-30s ranks %d  fused %s  splitFirst %4d  %2d arrays  %s" % (name, what, world, fuse, info["splitFirst"], len(a),
                                                                                         "DIFFERENT: %s" % diff if diff else "equal"))
            print(lines[-1], flush=True)
    lines.append("%d of %d cases differ" % (bad, len(CASES)))
    print(lines[-1])
    open(args.out, "w").write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
