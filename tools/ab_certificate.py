#!/usr/bin/env python3
"""The solve certificate (rn_solve_certificate: dual bound and optimality gap of the multiplier at hand) in figures.  Two halves.

CPU half (default; no GPU): DUAL, PRIMAL, U_EXCESS and GAP / |DUAL| of the numpy restatement tests/certificate_oracle.py on the CPU oracle
after 1, 5, 20, 50, 100, 200 and 500 APG iterations on `tiny`, `small`, `ragged`, `medium` and `barcelona31` (made feasible) -- plain, and under the gradient
restart (tests/restart_oracle.py, batches of 20): the comparison of two solves by their dual bound that nobody could make before.

--gpu half, on the headline tree (barcelona493), dense and structured, one process, interleaved regions, the median of the repeats, host clock
around a synchronise:

    call      rn_solve_certificate: the sweep at y+, k_plan_report's node phase, k_certificate, 128 bytes back
    device    rn_solve_certificate_device + rn_synchronize
    iterate   rn_apg_iterate(1) + rn_synchronize on the same context, for scale
    manual    what a caller had to do before: rn_set of the accelerated dual to y+, rn_solve_step, rn_get of x, u and the two halves of Hz, and
              the restatement's numpy on the host (alpha, p, the scaled bounds are read outside the timed region); the accelerated dual is put
              back afterwards, outside the timed region

    python3 tools/ab_certificate.py > profiles/ab_certificate.txt            # CPU half
    python3 tools/ab_certificate.py --gpu [--reps 7] >> profiles/ab_certificate.txt
"""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import certificate_oracle as co  # noqa: E402
import first_principles as fp  # noqa: E402
from rapidnet_amd import synth  # noqa: E402

COUNTS = (1, 5, 20, 50, 100, 200, 500)
PROBLEMS = ("tiny", "small", "ragged", "medium", "barcelona31")


def cpu_half():
    from oracle.oracle import Oracle
    from restart_oracle import gradient_test, oracle_vectors

    print("CPU half: the restatement on the CPU oracle, forecast 0, every fixture made feasible (synth.make_feasible); gradient restart tested every 20 iterations")
    print("%-12s %-8s %5s %18s %18s %11s %11s %6s %s" % ("problem", "run", "iter", "DUAL", "PRIMAL", "U_EXCESS", "GAP/|DUAL|", "VALID", "restarts so far"))
    for name in PROBLEMS:
        p = synth.make_problem(name, feasible=True)
        fc = synth.forecast_at(p["forecast"], 0)
        m = fp.Model(p["network"], p["tree"], p["config"], fc)
        ubox = co.physical_ubox(p["network"], m.nodes)
        for run in ("plain", "restart"):
            o = Oracle(p["network"], p["tree"], p["config"])
            o.initialise(*fc)
            rows = {}

            def look(done, orc):
                if done in COUNTS:
                    rows[done] = co.oracle_certificate(orc, m, ubox)

            # one iteration at a time, as restart_oracle.restart_loop drives the oracle; under the restart the gradient test at every 20th
            o.apg_reset()
            theta, fires = [1.0, 1.0], []
            for it in range(1, COUNTS[-1] + 1):
                theta = list(o.apg_continue(1, theta))
                if run == "restart" and it % 20 == 0 and gradient_test(*oracle_vectors(o))[0] > 0:
                    o.set("xi", o.get("updXi"))
                    o.set("psi", o.get("updPsi"))
                    theta = [1.0, 1.0]
                    fires.append(it)
                look(it, o)
            for c in COUNTS:
                r = rows[c]
                print("%-12s %-8s %5d %18.9f %18.9f %11.3e %11.3e %6d %s" % (name, run, c, r["dual"], r["primal"], r["uExcess"], r["gap"] / abs(r["dual"]), r["valid"],
                                                                          ",".join(str(f) for f in fires if f <= c) if run == "restart" else ""))
    print("DUAL is a lower bound of the optimal expected cost where VALID = 1; GAP is a gap only where U_EXCESS = 0.")


def gpu_half(a):
    import types

    from rapidnet_amd import build, capi

    p = synth.make_problem(a.workload)
    fc = synth.forecast_at(p["forecast"], 0)
    print("--gpu half: workload %s, %d iterations from cold, %d repeats; kernel sources %s" % (a.workload, a.iterations, a.reps, build.kernel_sources_sha256()[:16]))
    for mode in ("dense", "structured"):
        s = capi.Solver(p["network"], p["tree"], p["config"], operator_mode=mode)
        s.initialiseSmpcController(*fc)
        s.apgReset()
        s.apgIterate(a.iterations)
        n, nx, nu = s.nodes, s.nx, s.nu
        parent = np.asarray(p["tree"]["ancestor"], int) - 1
        sc = {k: s.get(b).reshape(n, -1) for k, b in (("xmin", capi.BUF_XMIN), ("xmax", capi.BUF_XMAX), ("xs", capi.BUF_XS), ("umin", capi.BUF_UMIN), ("umax", capi.BUF_UMAX))}
        m = types.SimpleNamespace(nodes=n, nx=nx, nu=nu, p=s.getTreeData()["prob"], W=np.asarray(p["config"]["costW"], float).reshape(nu, nu).T,
                                  alpha=s.get(capi.BUF_ALPHA).reshape(n, nu), anc=parent, u_root=np.ravel(p["config"]["prevU"]).astype(float),
                                  gammaX=float(np.ravel(p["config"]["penaltyStateX"])[0]), gammaS=float(np.ravel(p["config"]["penaltySafetyX"])[0]), **sc)
        ubox = co.physical_ubox(p["network"], n)

        def manual():
            t0 = time.perf_counter()
            xi, psi = s.get(capi.BUF_UPD_XI), s.get(capi.BUF_UPD_PSI)
            s.set(capi.BUF_ACC_XI, xi)
            s.set(capi.BUF_ACC_PSI, psi)
            s.solveStep()
            x, u, hxi, hpsi = s.get(capi.BUF_X), s.get(capi.BUF_U), s.get(capi.BUF_PRIMAL_XI), s.get(capi.BUF_PRIMAL_PSI)
            t1 = time.perf_counter()
            r = co.certificate(x, u, xi, psi, m, ubox, hz=(hxi, hpsi))
            return t1 - t0, time.perf_counter() - t1, r

        times = {k: [] for k in ("call", "device", "iterate", "manual_gpu", "manual_numpy")}
        rec = ref = None
        for i in range(a.reps + 1):      # first = warm-up (and the certificate's one allocation)
            t0 = time.perf_counter()
            rec = s.solveCertificate()
            t1 = time.perf_counter()
            s.solveCertificateDevice()
            s.synchronize()
            t2 = time.perf_counter()
            keep = s.get(capi.BUF_ACC_XI), s.get(capi.BUF_ACC_PSI)
            tg, tn, ref = manual()
            s.set(capi.BUF_ACC_XI, keep[0])
            s.set(capi.BUF_ACC_PSI, keep[1])
            s.synchronize()
            t3 = time.perf_counter()
            s.apgIterate(1, history=False)
            s.synchronize()
            t4 = time.perf_counter()
            if i:
                for k, v in (("call", t1 - t0), ("device", t2 - t1), ("manual_gpu", tg), ("manual_numpy", tn), ("iterate", t4 - t3)):
                    times[k].append(v)
        for k, what in (("call", "rn_solve_certificate"), ("device", "rn_solve_certificate_device + rn_synchronize"), ("iterate", "rn_apg_iterate(1) + rn_synchronize"),
                        ("manual_gpu", "manual: 2 rn_get + 2 rn_set + rn_solve_step + 4 rn_get"), ("manual_numpy", "manual: the numpy restatement on the host")):
            v = times[k]
            print("%-10s %-12s %-58s %10.3f ms median (min %.3f, max %.3f)" % (mode, k, what + ":", 1e3 * float(np.median(v)), 1e3 * min(v), 1e3 * max(v)))
        print("%-10s the last record: DUAL %.9g PRIMAL %.9g U_EXCESS %.3g VALID %d; the manual route's DUAL differs by %.1e of ABS_TERMS"
              % (mode, rec["dual"], rec["primal"], rec["uExcess"], rec["valid"], abs(rec["dual"] - ref["dual"]) / rec["absTerms"]))
        s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=100)
    args = ap.parse_args()
    gpu_half(args) if args.gpu else cpu_half()
