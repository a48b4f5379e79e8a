#!/usr/bin/env python3
"""What the shifted warm start (rn_shift_warm_start) buys and what it costs, written to profiles/ab_shift_warm_start.txt.

CPU half (no GPU needed): a receding-horizon loop of 6 control steps on the CPU oracle (tests/horizon_oracle.run_horizon; soft penalties
32 / 2.5, plant mode 0 at every step, the forecasts of time instants 0 .. 5) with a fixed iteration budget per step, started three ways:
cold (every step from zero), keep (rn_set_warm_start: the duals of the previous step where they are) and shift (the duals moved one stage
toward the root along the root's most probable child first, restated in numpy: tests/shift_oracle.py).  Reported: the fixed-point residual
||(resXi, resPsi)||_2 at the end of control steps 2 to 6; smaller is better.  Problems small, medium, ragged, barcelona31; budgets 10, 40,
150, 400 iterations per step.

GPU half (--gpu, needs an MI355X): the cost of one rn_shift_warm_start on the 493-scenario tree (10 864 nodes x 240 duals) against the
manual route (rn_get x 2, the numpy shift, rn_set x 4), one process, regions interleaved (call, manual, call, manual, ...), median of
--rounds.  With --parent DIR (a built checkout of the parent commit) bench.py then runs there and here alternately: nothing inside an
iteration is touched, so the two figures are expected to agree within the run-to-run spread.

    python3 tools/ab_shift_warm_start.py [--gpu] [--rounds 7] [--parent DIR] [--keep-gpu FILE] > profiles/ab_shift_warm_start.txt

--keep-gpu FILE: the GPU half is not run; the lines of FILE from "== GPU half" on (an earlier --gpu run) are appended instead."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

PROBLEMS = ("small", "medium", "ragged", "barcelona31")
BUDGETS = (10, 40, 150, 400)
STEPS = 6
SOFT = {"penalty_x": 32.0, "penalty_xs": 2.5}


def shift_inputs(p):
    import shift_oracle as so

    parent, stage = so.tree_arrays(p["tree"])
    nx, nu, N = int(p["network"]["nx"][0]), int(p["network"]["nu"][0]), int(p["tree"]["N"][0])
    prob = np.asarray(p["tree"]["probNode"], float).ravel()[: len(parent)]
    d = so.diag_y_order(p["config"]["matDiagPrecnd"], N, nx, nu)
    child = so.most_probable_child(parent, prob)
    return dict(nx=nx, nu=nu, prob=prob, d=d, stage=stage, child=child, m=so.shift_map(parent, child))


def numpy_shift(si, upd_xi, upd_psi):
    import shift_oracle as so

    new = so.shift_duals(so.y_rows(upd_xi, upd_psi, si["nx"], si["nu"]), si["prob"], si["d"], si["stage"], si["m"])
    return so.split_rows(new, si["nx"])


def cpu_half():
    import horizon_oracle as ho
    from oracle.oracle import Oracle
    from rapidnet_amd import synth

    print("== CPU half: the fp64 oracle, %d control steps, soft penalties %g / %g, plant mode 0, root child = the most probable" % (STEPS, SOFT["penalty_x"], SOFT["penalty_xs"]))
    print("   ||(resXi, resPsi)||_2 at the end of control steps 2 .. %d after a fixed iteration count per step; last column: shift against keep at the last step" % STEPS)
    print("%-12s %5s | %-36s | %-36s | %-36s | %s" % ("problem", "iters", "cold", "keep duals", "shifted", "shift / keep - 1"))
    for name in PROBLEMS:
        p = synth.make_problem(name, sim_horizon=STEPS, **SOFT)
        si = shift_inputs(p)

        def hook(t, o):
            if t > 0:
                xi, psi = numpy_shift(si, o.get("updXi"), o.get("updPsi"))
                for a, b in (("xi", "psi"), ("updXi", "updPsi")):
                    o.set(a, xi)
                    o.set(b, psi)

        for n in BUDGETS:
            steps = ho.steps_of(p["forecast"], synth.forecast_at, (n,) * STEPS)
            rows = {}
            for how, warm, before in (("cold", False, None), ("keep", True, None), ("shift", True, hook)):
                o = Oracle(p["network"], p["tree"], p["config"])
                o.factor_step()
                recs = ho.run_horizon(o, steps, warm, plant_modes=[0] * STEPS, before_step=before)
                rows[how] = [float(np.sqrt((r["bufs"]["resXi"] ** 2).sum() + (r["bufs"]["resPsi"] ** 2).sum())) for r in recs[1:]]
            fmt = lambda v: " ".join("%6.3g" % x for x in v)  # noqa: E731
            print("%-12s %5d | %-36s | %-36s | %-36s | %+.0f %%" % (name, n, fmt(rows["cold"]), fmt(rows["keep"]), fmt(rows["shift"]),
                                                                   100 * (rows["shift"][-1] / rows["keep"][-1] - 1)))
            sys.stdout.flush()


def gpu_half(rounds):
    from rapidnet_amd import capi, synth

    p = synth.make_problem("barcelona493")
    f0 = synth.forecast_at(p["forecast"], 0)
    si = shift_inputs(p)
    print("== GPU half: barcelona493 (%d nodes x %d duals, fp64), one rn_shift_warm_start against rn_get x 2 + numpy + rn_set x 4; median of %d interleaved regions" % (
        len(si["prob"]), 2 * si["nx"] + si["nu"], rounds))
    for structured in (False, True):
        s = capi.Solver(p["network"], p["tree"], p["config"], structured=structured)
        s.initialiseSmpcController(*f0)
        s.setWarmStart(True)
        s.controlAction(*f0, maxIterations=20)
        s.shiftWarmStart(si["child"])                             # warm-up: the index arrays, the code object
        s.synchronize()
        t = {"call": [], "call -1": [], "manual": []}
        for _ in range(rounds):
            for how, child in (("call", si["child"]), ("call -1", -1)):
                s.synchronize()
                t0 = time.perf_counter()
                s.shiftWarmStart(child)
                s.synchronize()
                t[how].append(1e3 * (time.perf_counter() - t0))
            s.synchronize()
            t0 = time.perf_counter()
            xi, psi = numpy_shift(si, s.get(capi.BUF_UPD_XI), s.get(capi.BUF_UPD_PSI))
            for bid, v in ((capi.BUF_XI, xi), (capi.BUF_PSI, psi), (capi.BUF_UPD_XI, xi), (capi.BUF_UPD_PSI, psi)):
                s.set(bid, v)
            s.synchronize()
            t["manual"].append(1e3 * (time.perf_counter() - t0))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print("%-10s rn_shift_warm_start(child) %.4f ms (min %.4f max %.4f) | rootChild = -1 %.4f ms | manual route %.3f ms (min %.3f max %.3f) | manual / call %.0f x" % (
            "structured" if structured else "dense", med["call"], min(t["call"]), max(t["call"]), med["call -1"], med["manual"], min(t["manual"]), max(t["manual"]),
            med["manual"] / med["call"]))
        s.close()
        sys.stdout.flush()


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


def bench_half(parent, runs, steps):
    res = {"parent": [], "this": []}
    for _ in range(runs):
        for who, cwd in (("parent", parent), ("this", ROOT)):
            line = bench(cwd, steps, 20)
            if line is None:      # a run that failed ends the comparison: nothing more is started
                sys.exit(1)
            res[who].append(line["value"])
    print("bench.py --gpus 1 --steps %d --warmup 20, alternating, iterations/s: parent %s | this change %s"
          % (steps, " ".join("%.0f" % v for v in res["parent"]), " ".join("%.0f" % v for v in res["this"])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--keep-gpu", default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py runs there and here alternately")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=300)
    a = ap.parse_args()
    if not a.gpu_only:
        cpu_half()
    if a.gpu or a.gpu_only:
        gpu_half(a.rounds)
        if a.parent:
            bench_half(a.parent, a.bench_runs, a.bench_steps)
    elif a.keep_gpu and os.path.exists(a.keep_gpu):
        txt = open(a.keep_gpu).read()
        print(txt[txt.index("== GPU half"):].rstrip() if "== GPU half" in txt else "== GPU half: not measured")
    else:
        print("== GPU half: not measured (needs an MI355X: python3 tools/ab_shift_warm_start.py --gpu)")
