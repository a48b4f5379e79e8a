#!/usr/bin/env python3
"""Wall time of the plan report (rn_plan_report ...: costs and bound violations of the plan a context holds, per stage and per scenario) on
the headline tree (barcelona493), against what a caller does today, in one process, interleaved regions, the median of the repeats:

    report    rn_plan_report + rn_plan_report_scenarios: both tables on the host (two runs of k_plan_report's two launches, two read-backs)
    device    rn_plan_report_device + rn_synchronize: the two launches alone, tables left on the device
    today     rn_get of x and u (the read-back), then the numpy restatement tests/plan_oracle.py on the host (needs alpha, p and the bounds
              as well, read outside the timed region)
    restart   rn_debug_restart_test: k_restart_test, one flat fp64 reduction over three [nodes][ny] vectors and a read-back of three
              doubles -- a kernel of similar bytes, for scale

The bytes the kernel has to move (x, u twice, alpha, the bounds rows, p, the node table written once and read once) over the `device`
time are set against rn_measure_hbm's read probe of the same run.  At the end the report is compared with the restatement.

    python3 tools/ab_plan_report.py [--workload barcelona493] [--reps 7] > profiles/ab_plan_report.txt
"""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import plan_oracle as po  # noqa: E402
from rapidnet_amd import build, capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=100)
    a = ap.parse_args()
    p = synth.make_problem(a.workload)
    fc = synth.forecast_at(p["forecast"], 0)
    s = capi.Solver(p["network"], p["tree"], p["config"], operator_mode="dense")
    s.initialiseSmpcController(*fc)
    s.algorithmApg(a.iterations)
    nodes, nx, nu, ny, N = s.nodes, s.nx, s.nu, s.ny, s.N
    leaves = s.planLeaves()
    moved = 8.0 * (nodes * (nx + 3 * nu + 1) + 2 * ny + 2 * 9 * nodes + 9 * (N + leaves))
    print("workload %s: %d nodes, %d stages, %d scenarios, nx %d, nu %d; %.2f MB to move per report (fp64, shared bounds); kernel sources %s"
          % (a.workload, nodes, N, leaves, nx, nu, moved / 1e6, build.kernel_sources_sha256()[:16]))
    parent, stage = np.asarray(p["tree"]["ancestor"], int) - 1, np.asarray(p["tree"]["stages"], int)
    alpha, prob, b = s.get(capi.BUF_ALPHA).reshape(nodes, nu), s.getTreeData()["prob"], s.getBounds()
    W, prevU = np.asarray(p["config"]["costW"], float), np.asarray(p["config"]["prevU"], float).ravel()
    s.debugRestartTest()      # (allocates its partials once)

    def today():
        t0 = time.perf_counter()
        x, u = s.get(capi.BUF_X).reshape(nodes, nx), s.get(capi.BUF_U).reshape(nodes, nu)
        t1 = time.perf_counter()
        r = po.evaluate(x, u, alpha, prevU, prob, W, parent, stage, b["xmin"], b["xmax"], b["xsafe"], b["umin"], b["umax"], np.zeros(nodes, int))
        return t1 - t0, time.perf_counter() - t1, r

    def device():
        s.planReportDevice()
        s.synchronize()

    times = {k: [] for k in ("report", "device", "get", "numpy", "restart")}
    rep, ref = None, None
    for i in range(a.reps + 1):               # first = warm-up (and the report's one allocation)
        t0 = time.perf_counter()
        rep = s.planReport()
        t1 = time.perf_counter()
        device()
        t2 = time.perf_counter()
        tg, tn, ref = today()
        t3 = time.perf_counter()
        s.debugRestartTest()
        t4 = time.perf_counter()
        if i:
            for k, v in (("report", t1 - t0), ("device", t2 - t1), ("get", tg), ("numpy", tn), ("restart", t4 - t3)):
                times[k].append(v)
    med = {k: float(np.median(v)) for k, v in times.items()}
    read_gbs, _ = s.measureHbm()
    for k, what in (("report", "rn_plan_report + rn_plan_report_scenarios (both tables on the host)"), ("device", "rn_plan_report_device + rn_synchronize"),
                    ("get", "today: rn_get of x and u"), ("numpy", "today: the numpy restatement on the host"), ("restart", "rn_debug_restart_test (k_restart_test + 24 bytes back)")):
        v = times[k]
        print("%-8s %-76s %10.3f ms median (min %.3f, max %.3f)" % (k, what + ":", 1e3 * med[k], 1e3 * min(v), 1e3 * max(v)))
    print("today's route / report: %.1fx" % ((med["get"] + med["numpy"]) / med["report"]))
    print("device form: %.2f MB in %.3f ms = %.1f GB/s, %.3f of the read probe of this run (%.0f GB/s)"
          % (moved / 1e6, 1e3 * med["device"], moved / med["device"] / 1e9, moved / med["device"] / 1e9 / read_gbs, read_gbs))
    got = np.stack([rep["stage"][k] for k in capi.PLAN_COLUMNS], 1)
    bound = 2.0 * (ref["stage_m"] + 2.0) * 2.0 ** -53 * ref["stage_abs"]
    assert (np.abs(got[:, :po.SUMS] - ref["stage"][:, :po.SUMS]) <= bound).all() and np.array_equal(got[:, po.SUMS:], ref["stage"][:, po.SUMS:])
    print("the report equals the restatement: sums within 2 (m + 2) 2^-53 sum|terms|, maxima bit for bit")
    s.close()


if __name__ == "__main__":
    main()
