#!/usr/bin/env python3
"""What stopping APG at a residual tolerance costs and what it buys (rn_apg_solve, rn_set_stop_tolerance), dense and structured, on the
493-scenario tree and on the closed-loop fixture (the reference's 3-tank files).

(a) Overhead: ms per iteration of rn_apg_solve(500, tol = 0, checkEvery = 20) -- 25 batch closes, each with its synchronisation -- against
    rn_apg_iterate(500) as ONE batch.  With --parent-root (a built checkout of the parent commit) the one-batch figure is the
    parent's, through the parent's own binding and library: a worker process per checkout and storage mode is started in alternation
    (parent, this, parent, this, ...), each timing its regions; medians over all regions.  Without it the one-batch figure is this
    checkout's own rn_apg_iterate(500), alternating regions inside one process.
(b) Gain: iterations and ms per control step (rn_control_action, maxIterations of the configuration) at a stated tolerance, cold and with
    rn_set_warm_start(1): a first step, then --steps further steps from a state moved 3 % per step; against the fixed-count step.

    python3 tools/ab_stop_tolerance.py [--parent-root DIR] [--rounds 5] [--tol 1e-2] [--steps 3] > profiles/ab_stop_tolerance.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if "--root" in sys.argv:      # a worker of another checkout: that checkout's package and library, this file's timing loop
    sys.path.insert(0, sys.argv[sys.argv.index("--root") + 1])
else:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def load_problem(name):
    """"fixture": the reference's 3-tank closed-loop files; otherwise a named synthetic workload"""
    from rapidnet_amd import synth

    if name == "fixture":
        d = os.path.join(ROOT, "tests", "golden", "reference_fixture")
        rd = lambda f: json.load(open(os.path.join(d, f)))  # noqa: E731
        p = {"network": rd("network.json"), "tree": rd("scenarioTree.json"), "config": rd("controllerConfig.json"), "forecast": rd("forecastor.json")}
    else:
        p = synth.make_problem(name)
    return p, synth.forecast_at(p["forecast"], 0), synth.forecast_at(p["forecast"], 1)


def solver(p, structured, f0, **kw):
    from rapidnet_amd import capi

    s = capi.Solver(p["network"], p["tree"], p["config"], structured=structured, **kw)
    s.initialiseSmpcController(*f0)
    return s


def region(s, fn, iters):
    s.synchronize()
    t0 = time.perf_counter()
    fn()
    s.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def worker(args):
    """one library, one workload, one storage mode: prints a JSON line {"solve": [...], "batch": [...]} of ms-per-iteration regions"""
    p, f0, _ = load_problem(args.workload)
    s = solver(p, args.structured, f0)
    has_solve = hasattr(s, "apg_solve")
    s.reserveIterations(args.iters)
    out = {"solve": [], "batch": []}
    s.apgReset(); s.apgIterate(40, history=False)
    for _ in range(args.rounds):
        s.apgReset()
        out["batch"].append(region(s, lambda: s.apgIterate(args.iters, history=False), args.iters))
        if has_solve:
            out["solve"].append(region(s, lambda: s.apg_solve(args.iters, 0.0, args.every, history=False), args.iters))
    print("REGIONS " + json.dumps(out), flush=True)


def spawn(args, root, structured):
    env = dict(os.environ)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + (["--root", os.path.abspath(root)] if root else []) + ["--workload", args.workload_now, "--iters", str(args.iters), "--every", str(args.every),
           "--rounds", str(args.worker_rounds)] + (["--structured"] if structured else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("worker failed (rc %d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("REGIONS ")][-1][8:])


def med(v):
    return "median %.4f (min %.4f max %.4f, %d regions)" % (np.median(v), min(v), max(v), len(v))


def overhead(args):
    for wl in args.workloads:
        args.workload_now = wl
        for structured in (False, True):
            mode = "structured" if structured else "dense"
            mine = {"solve": [], "batch": []}
            parent = {"batch": []}
            for _ in range(args.rounds):
                if args.parent_root:
                    parent["batch"] += spawn(args, args.parent_root, structured)["batch"]
                r = spawn(args, None, structured)
                mine["solve"] += r["solve"]; mine["batch"] += r["batch"]
            print("(a) %s, %s, %d iterations: rn_apg_solve(tol 0, checkEvery %d) ms/iteration %s" % (wl, mode, args.iters, args.every, med(mine["solve"])))
            print("    this checkout's rn_apg_iterate(%d), one batch:                 ms/iteration %s" % (args.iters, med(mine["batch"])))
            ref = mine["batch"]
            if args.parent_root:
                print("    the parent commit's rn_apg_iterate(%d), one batch:             ms/iteration %s" % (args.iters, med(parent["batch"])))
                ref = parent["batch"]
            d = float(np.median(mine["solve"]) - np.median(ref))
            print("    %d batch closes instead of one: %+.4f ms per iteration = %+.1f us per extra close (%+.1f %%)"
                  % (-(-args.iters // args.every), d, 1e3 * d * args.iters / max(-(-args.iters // args.every) - 1, 1), 100.0 * d / float(np.median(ref))), flush=True)


def gain(args):
    for wl in args.workloads:
        p, f0, f1 = load_problem(wl)
        maxit = int(np.ravel(p["config"]["maxIterations"])[0])
        x0 = np.asarray(p["config"]["currentX"], float).ravel()
        for structured in (False, True):
            mode = "structured" if structured else "dense"
            for tag, tol, warm in (("fixed count", 0.0, False), ("tolerance, cold", args.tol, False), ("tolerance, warm start", args.tol, True)):
                s = solver(p, structured, f0, stop_tolerance=tol, stop_check_every=args.every if tol else 0)
                s.setWarmStart(warm)
                s.controlAction(*f0)          # (the first step is cold either way; it also warms the box up)
                rows, u = [], None
                for k in range(args.steps):
                    fc = f1 if k % 2 == 0 else f0
                    s.synchronize()
                    t0 = time.perf_counter()
                    u = s.controlAction(fc[0], fc[1], currentX=x0 * (1.0 - 0.03 * (k + 1)), prevU=u)
                    ms = 1e3 * (time.perf_counter() - t0)
                    rows.append((s.last_solve()["iterations"], ms))
                print("(b) %s, %s, %-22s tol %-8g maxIterations %d: iterations per control step %s, ms per control step %s"
                      % (wl, mode, tag, tol, maxit, [r[0] for r in rows], ["%.2f" % r[1] for r in rows]), flush=True)
                s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--workloads", default="fixture,barcelona493")
    ap.add_argument("--structured", action="store_true")
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the worker processes")
    ap.add_argument("--worker-rounds", type=int, default=3, help="regions per worker process")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--root", default=None, help="(worker) the checkout whose package and library are measured")
    ap.add_argument("--tol", type=float, default=1e-2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-gain", action="store_true")
    args = ap.parse_args()
    if args.worker:
        args.rounds = args.worker_rounds
        return worker(args)
    args.workloads = args.workloads.split(",")
    print("# tools/ab_stop_tolerance.py --iters %d --every %d --rounds %d --worker-rounds %d --tol %g --steps %d%s"
          % (args.iters, args.every, args.rounds, args.worker_rounds, args.tol, args.steps, " --parent-root (the parent commit, built)" if args.parent_root else ""))
    overhead(args)
    if not args.skip_gain:
        gain(args)


if __name__ == "__main__":
    main()
