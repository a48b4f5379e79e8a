#!/usr/bin/env python3
"""Wall time of the dual Lipschitz estimate (rn_estimate_lipschitz: power sweeps over the context's Hessian sweep, the loop kept on the
device) on the headline tree (barcelona493), dense and structured, against what a caller can do today.  One process, interleaved regions,
the median of the repeats, the host clock around a synchronise (every region ends in a read-back):

    device    rn_estimate_lipschitz, 40 iterations, tol 0: one synchronisation at the end
    host      the same 40 sweeps driven from the host: rn_set of the unit vector, rn_compute_hessian_oracle, rn_get of H * v, numpy norm and
              normalisation (a NAMA context: the step-wise oracle reads its residual buffers)
    cpu       rapidnet_amd.synth.lipschitz_estimate, 40 iterations of its numpy restatement of the structured operator (--cpu-reps times, default 1)

and the three values side by side (device and host from the library's hashed start, synth from its own).  The first pass is the warm-up
(and the estimate's one allocation) and is not counted.

    python3 tools/ab_lipschitz.py [--workload barcelona493] [--reps 7] [--iterations 40] > profiles/ab_lipschitz.txt
"""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import lipschitz_oracle as lo  # noqa: E402
from rapidnet_amd import build, capi, synth  # noqa: E402


def host_loop(s, xi, psi, iterations):
    """the power loop with every vector operation on the host: what a caller of the step-wise API can do today"""
    w = np.hstack([xi, psi])
    n2 = xi.shape[1]
    nrm = 0.0
    for _ in range(iterations):
        v = w / np.sqrt((w * w).sum())
        s.set(capi.BUF_RES_XI, v[:, :n2]); s.set(capi.BUF_RES_PSI, v[:, n2:])
        s.computeHessianOracalGlobalFbe()
        w = np.hstack([s.get(capi.BUF_PRIMAL_XI_DIR).reshape(s.nodes, n2), s.get(capi.BUF_PRIMAL_PSI_DIR).reshape(s.nodes, s.nu)])
        nrm = float(np.sqrt((w * w).sum()))
    return nrm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--cpu-reps", type=int, default=1)
    a = ap.parse_args()
    p = synth.make_problem(a.workload)
    fc = synth.forecast_at(p["forecast"], 0)
    print("workload %s, %d iterations, %d repeats; kernel sources %s" % (a.workload, a.iterations, a.reps, build.kernel_sources_sha256()[:16]))
    values = {}
    for mode in ("dense", "structured"):
        s = capi.Solver(p["network"], p["tree"], p["config"], operator_mode=mode)
        s.initialiseSmpcController(*fc)
        s.setAlgorithm("namaAlgorithm", 5)
        xi, psi = lo.hash_start(s.nodes, s.nx, s.nu, 0)
        times = {"device": [], "host": []}
        for i in range(a.reps + 1):
            t0 = time.perf_counter()
            r = s.estimateLipschitz(a.iterations)
            t1 = time.perf_counter()
            h = host_loop(s, xi, psi, a.iterations)
            t2 = time.perf_counter()
            if i:
                times["device"].append(t1 - t0); times["host"].append(t2 - t1)
        values[mode] = (r, h, float(np.median(times["device"])))
        print("%-10s %d nodes, ny %d" % (mode, s.nodes, s.ny))
        for k, what in (("device", "rn_estimate_lipschitz"), ("host", "rn_set + rn_compute_hessian_oracle + rn_get + numpy, per estimate")):
            v = times[k]
            print("  %-7s %-66s %10.3f ms median (min %.3f, max %.3f) = %.3f ms per iteration"
                  % (k, what + ":", 1e3 * np.median(v), 1e3 * min(v), 1e3 * max(v), 1e3 * np.median(v) / a.iterations))
        print("  host / device: %.1fx;  NORM device %.9g (RAYLEIGH %.9g, RESIDUAL %.3e), host loop %.9g, relative difference %.2e"
              % (np.median(times["host"]) / np.median(times["device"]), r["norm"], r["rayleigh"], r["residual"], h, abs(h - r["norm"]) / h))
        s.close()
    cpu = []
    for _ in range(max(1, a.cpu_reps)):
        t0 = time.perf_counter()
        val = synth.lipschitz_estimate(p["network"], p["tree"], p["config"], iters=a.iterations)
        cpu.append(time.perf_counter() - t0)
    print("cpu        synth.lipschitz_estimate (numpy, its own start):                          %10.3f ms median of %d = %.3f ms per iteration" %
          (1e3 * np.median(cpu), len(cpu), 1e3 * np.median(cpu) / a.iterations))
    d = values["dense"][0]["norm"]
    print("values     device dense %.9g | device structured %.9g | synth %.9g;  config.stepSize * NORM(dense) = %.4f"
          % (d, values["structured"][0]["norm"], val, float(p["config"]["stepSize"][0]) * d))
    print("cpu / device: dense %.0fx, structured %.0fx" % (np.median(cpu) / values["dense"][2], np.median(cpu) / values["structured"][2]))


if __name__ == "__main__":
    main()
