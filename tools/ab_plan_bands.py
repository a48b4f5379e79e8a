#!/usr/bin/env python3
"""Wall time of the plan bands (rn_plan_quantiles, rn_plan_paths: per-stage weighted quantiles and scenario paths of x and u) on the headline
tree (barcelona493), against what a caller does today, in one process, interleaved regions, the median of the repeats:

    quantiles  rn_plan_quantiles of x at three levels (0.05, 0.5, 0.95): one launch of k_plan_bands, the table on the host
    device     rn_plan_quantiles_device + rn_synchronize: the launch alone, the table left on the device
    paths      rn_plan_paths of x: one launch, [scenarios][stages][nx] doubles on the host
    get        today: rn_get of x (the read-back the caller needs first)
    numpy      today: the quantiles and the paths in numpy on the host -- per stage and component a stable sort on (value, index), np.cumsum
               of the probabilities in that order, np.searchsorted for the levels; the paths by fancy indexing through the ancestors (the
               tree bookkeeping and the probabilities are read outside the timed region)

At the end both results are compared with the numpy ones, bit for bit.  With --parent DIR (a built checkout of the parent commit) bench.py
runs there and here alternately, --bench-runs times each, and the headline figures are printed side by side.

    python3 tools/ab_plan_bands.py [--workload barcelona493] [--reps 7] [--parent DIR] > profiles/ab_plan_bands.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from rapidnet_amd import build, capi, synth  # noqa: E402

LEVELS = (0.05, 0.5, 0.95)


def numpy_bands(x, prob, stage_nodes, anc, q):
    """today's route on the host: ([N][dim][nq] quantiles, [leaves][N][dim] paths)"""
    N, dim = len(stage_nodes), x.shape[1]
    out = np.empty((N, dim, len(q)))
    for k, idx in enumerate(stage_nodes):
        idx = idx[prob[idx] > 0]
        p = prob[idx]
        for c in range(dim):
            v = x[idx, c]
            order = np.lexsort((idx, v))
            cs = np.cumsum(p[order])
            out[k, c] = v[order][np.searchsorted(cs, np.asarray(q) * cs[-1], side="left")]
    return out, x[anc]


def bench(cwd, steps, warmup):
    """the headline figure of one bench.py run in `cwd` (a fresh process), or None"""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-traffic", "--profile-steps", "0",
           "--repeats", "2", "--other-configs", "", "--no-shard-ceiling", "--no-quasi-newton"]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900)
    lines = [t for t in r.stdout.splitlines() if t.startswith("{") and '"metric"' in t]
    if r.returncode != 0 or not lines:
        print("bench.py in %s failed (rc %d): %s" % (cwd, r.returncode, r.stderr[-400:]))
        return None
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py runs there and here alternately")
    ap.add_argument("--bench-runs", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=300)
    a = ap.parse_args()
    p = synth.make_problem(a.workload)
    fc = synth.forecast_at(p["forecast"], 0)
    s = capi.Solver(p["network"], p["tree"], p["config"], operator_mode="dense")
    s.initialiseSmpcController(*fc)
    s.algorithmApg(a.iterations)
    nodes, nx, N = s.nodes, s.nx, s.N
    leaves = s.bandLeaves()
    parent, stage = np.asarray(p["tree"]["ancestor"], int) - 1, np.asarray(p["tree"]["stages"], int)
    print("workload %s: %d nodes, %d stages, %d scenarios, nx %d, widest stage %d; kernel sources %s"
          % (a.workload, nodes, N, leaves, nx, int(np.bincount(stage).max()), build.kernel_sources_sha256()[:16]))
    prob = s.getTreeData()["prob"]
    stage_nodes = [np.flatnonzero(stage == k) for k in range(N)]
    anc = np.empty((leaves, N), int)      # the ancestors of every leaf, root first
    anc[:, N - 1] = stage_nodes[N - 1]
    for k in range(N - 1, 0, -1):
        anc[:, k - 1] = parent[anc[:, k]]

    times = {k: [] for k in ("quantiles", "device", "paths", "get", "numpy")}
    got_q = got_p = ref = None
    for i in range(a.reps + 1):               # first = warm-up (and the one allocation)
        t0 = time.perf_counter()
        got_q = s.planQuantiles("x", LEVELS)
        t1 = time.perf_counter()
        s.planQuantilesDevice("x", LEVELS)
        s.synchronize()
        t2 = time.perf_counter()
        got_p, _ = s.planPaths("x")
        t3 = time.perf_counter()
        x = s.get(capi.BUF_X).reshape(nodes, nx)
        t4 = time.perf_counter()
        ref = numpy_bands(x, prob, stage_nodes, anc, LEVELS)
        t5 = time.perf_counter()
        if i:
            for k, v in (("quantiles", t1 - t0), ("device", t2 - t1), ("paths", t3 - t2), ("get", t4 - t3), ("numpy", t5 - t4)):
                times[k].append(v)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, what in (("quantiles", "rn_plan_quantiles (x, 3 levels, the table on the host)"), ("device", "rn_plan_quantiles_device + rn_synchronize"),
                    ("paths", "rn_plan_paths (x, on the host)"), ("get", "today: rn_get of x"), ("numpy", "today: sort, cumsum and paths in numpy on the host")):
        v = times[k]
        print("%-10s %-60s %10.3f ms median (min %.3f, max %.3f)" % (k, what + ":", 1e3 * med[k], 1e3 * min(v), 1e3 * max(v)))
    print("today's route / (quantiles + paths): %.1fx" % ((med["get"] + med["numpy"]) / (med["quantiles"] + med["paths"])))
    same = np.array_equal(got_q.view(np.int64), ref[0].view(np.int64)) and np.array_equal(got_p.view(np.int64), np.ascontiguousarray(ref[1]).view(np.int64))
    assert same, "the library's tables differ from the numpy ones"
    print("quantiles and paths equal the numpy ones bit for bit")
    s.close()
    if a.parent:
        res = {"parent": [], "this": []}
        for _ in range(a.bench_runs):
            for who, cwd in (("parent", a.parent), ("this", ROOT)):
                line = bench(cwd, a.bench_steps, 20)
                res[who].append(line["value"] if line else float("nan"))
        print("bench.py --gpus 1 --steps %d --warmup 20, alternating, iterations/s: parent %s | this change %s"
              % (a.bench_steps, " ".join("%.0f" % v for v in res["parent"]), " ".join("%.0f" % v for v in res["this"])))


if __name__ == "__main__":
    main()
