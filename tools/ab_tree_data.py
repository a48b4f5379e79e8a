#!/usr/bin/env python3
"""Wall time of re-weighting the scenario tree of a live context (new probabilities and errors, same topology) on the headline tree
(barcelona493), three routes in one process, interleaved, in dense, structured and RN_STORE_F32 operator storage:

    today   what a caller had to do before rn_set_tree_data existed: rn_destroy + rn_create + rn_set_tree_errors + rn_factor_step on the new tree
    host    rn_set_tree_data: the three host arrays in one call (k_tree_data behind a staging copy; synchronises)
    device  rn_set_tree_data_device: the three arrays already in device memory (launches on the context's stream)

each followed by the same rn_update_state_control + rn_eliminate_input_disturbance_coupling + rn_synchronize, which a re-weighted context needs
before it iterates; host clock around the whole route.  The repeats alternate between two trees, so every call changes every value; the median
of the repeats is reported.  At the end the in-place context's next 20 iterations are compared with the re-created one's (bitwise).

    python3 tools/ab_tree_data.py [--workload barcelona493] [--reps 7] > profiles/ab_tree_data.txt
"""
import argparse
import copy
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rapidnet_amd import build, capi, synth  # noqa: E402

KEYS = (("prob", "probNode"), ("errorDemand", "errorDemandNode"), ("errorPrice", "errorPriceNode"))
STORAGES = (("dense", "native"), ("structured", "native"), ("dense", "f32"))


def reweighted(tree, fc, seed):
    """same topology, every non-leaf node's probability dealt anew among its children (weights from [0.2, 1]), new errors at synth.make_tree's scale"""
    rng = np.random.default_rng(seed)
    nodes, N = int(tree["nodes"][0]), int(tree["N"][0])
    nd, nu = int(tree["dimDemand"][0]), int(tree["dimPrice"][0])
    anc, stages = np.asarray(tree["ancestor"], int) - 1, np.asarray(tree["stages"], int)
    kids = [[] for _ in range(nodes)]
    for c in range(1, nodes):
        kids[anc[c]].append(c)
    prob = np.ones(nodes)
    for i in range(nodes):
        if kids[i]:
            w = rng.uniform(0.2, 1.0, len(kids[i]))
            prob[kids[i]] = prob[i] * w / w.sum()
    dh, ah = np.asarray(fc[0], float).reshape(N, nd), np.asarray(fc[1], float).reshape(N, nu)
    err_d, err_a = 0.05 * rng.standard_normal((nodes, nd)) * dh[stages], 0.05 * rng.standard_normal((nodes, nu)) * ah[stages]
    err_d[0], err_a[0] = 0.0, 0.0
    new = copy.copy(tree)
    new["probNode"], new["errorDemandNode"], new["errorPriceNode"] = prob, err_d.ravel(), err_a.ravel()
    return new


def as_arrays(tree):
    """every list of the tree as a numpy array once, so that no route pays for Python's list conversion"""
    return {k: (np.asarray(v, dtype=np.float64) if isinstance(v, (list, tuple)) else v) for k, v in tree.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    p = synth.make_problem(a.workload)
    fc = synth.forecast_at(p["forecast"], 0)
    trees = [as_arrays(reweighted(p["tree"], fc, seed)) for seed in (1, 2)]
    nodes, nd, nu = int(trees[0]["nodes"][0]), int(trees[0]["dimDemand"][0]), int(trees[0]["dimPrice"][0])
    print("workload %s: %d nodes, nd %d, nu %d, %.2f MB of tree data (fp64); kernel sources %s"
          % (a.workload, nodes, nd, nu, nodes * (1 + nd + nu) * 8 / 1e6, build.kernel_sources_sha256()[:16]))

    def tail(s):
        s.updateStateControl()
        s.eliminateInputDistubanceCoupling(*fc)
        s.synchronize()

    for mode, storage in STORAGES:
        def create(tree):
            s = capi.Solver(p["network"], tree, p["config"], operator_mode=mode, operator_storage=storage)
            s.factorStep()
            return s

        live, again = create(trees[0]), create(trees[0])
        tail(live); tail(again)
        dev = [{k: torch.from_numpy(np.ascontiguousarray(t[j])).cuda() for k, j in KEYS} for t in trees]
        torch.cuda.synchronize()
        times = {"today": [], "host": [], "device": []}
        for rep in range(a.reps + 1):               # first = warm-up
            t = trees[(rep + 1) % 2]
            d = dev[(rep + 1) % 2]
            t0 = time.perf_counter()
            again.close()
            again = create(t)
            tail(again)
            t1 = time.perf_counter()
            live.setTreeData(t["probNode"], t["errorDemandNode"], t["errorPriceNode"])
            tail(live)
            t2 = time.perf_counter()
            live.setTreeDataDevice("f64", **{k: v.data_ptr() for k, v in d.items()})
            tail(live)
            t3 = time.perf_counter()
            if rep:
                times["today"].append(t1 - t0); times["host"].append(t2 - t1); times["device"].append(t3 - t2)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("\n== fp64 context, %s operators, %s block storage (%d repeats, alternating trees) ==" % (mode, storage, a.reps))
        for k, what in (("today", "rn_destroy + rn_create + rn_set_tree_errors + rn_factor_step"), ("host", "rn_set_tree_data (host arrays)"),
                        ("device", "rn_set_tree_data_device (device arrays)")):
            v = times[k]
            print("%-7s %-66s %10.3f ms median (min %.3f, max %.3f)%s" % (k, what + " + elimination:", 1e3 * med[k], 1e3 * min(v), 1e3 * max(v),
                                                                         "" if k == "today" else "   %.0fx today's route" % (med["today"] / med[k])), flush=True)
        hists = []
        for s in (live, again):
            s.apgReset()
            hists.append((s.apgIterate(20), s.get(capi.BUF_X), s.get(capi.BUF_U)))
        assert all(np.isfinite(v).all() and np.array_equal(v, w) for v, w in zip(*hists)), "the re-weighted context differs from the re-created one"
        assert live.operatorMode() == again.operatorMode()
        print("20 iterations of the re-weighted context and of the re-created one: bitwise equal (operator mode %s)" % (live.operatorMode(),), flush=True)
        live.close(); again.close()
        del dev


if __name__ == "__main__":
    main()
