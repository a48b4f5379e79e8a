#!/usr/bin/env python3
"""What the gradient restart of the APG momentum buys and what it costs (rn_set_restart), written to profiles/ab_restart.txt.

CPU half (no GPU needed): the restart restated on the CPU oracle (tests/restart_oracle.py: Oracle.apg_continue with theta threaded by the caller,
g = <w_k - y_{k+1}, y_{k+1} - y_k> in numpy at every batch end, the restart by hand) on tiny, small, medium, barcelona31 (synthetic, feasible,
forecast 0) and on the reference fixture (tests/golden/reference_fixture).  Reported: the iterations at which ||(resXi, resPsi)||_2 first
falls to 1e-2, 1e-3, 1e-4 of its value after the first batch, with and without the restart; the iterations at which the momentum restarted;
the smallest |cos| = |g| / sqrt(na2 nb2) over the boundaries (how marginal the closest decision was).

GPU half (--gpu, needs an MI355X): ms per batch of --every iterations of rn_apg_solve(tol = 0) with the mode on and off on the 493-scenario
tree, dense and structured, regions interleaved (off, on, off, on, ...), median of --rounds; and the time of k_restart_test per batch from
the context's own profile events (class 3 of rn_profile_read with the mode on minus with it off, over the same solve).

    python3 tools/ab_restart.py [--every 20] [--gpu] [--rounds 7] [--batches 10] [--keep-gpu FILE] > profiles/ab_restart.txt

--keep-gpu FILE: the GPU half is not run; the lines of FILE from "== GPU half" on (an earlier --gpu run) are appended instead."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

CPU_CASES = (("tiny", 600), ("small", 4000), ("medium", 3000), ("barcelona31", 1200), ("fixture", 1200))


def load_problem(name):
    from rapidnet_amd import synth

    if name == "fixture":
        d = os.path.join(ROOT, "tests", "golden", "reference_fixture")
        rd = lambda f: json.load(open(os.path.join(d, f)))  # noqa: E731
        p = {"network": rd("network.json"), "tree": rd("scenarioTree.json"), "config": rd("controllerConfig.json"), "forecast": rd("forecastor.json")}
    else:
        p = synth.make_problem(name, feasible=True)
    return p, synth.forecast_at(p["forecast"], 0)


def cpu_half(every):
    import restart_oracle as ro
    from oracle.oracle import Oracle

    print("== CPU half: the fp64 oracle, checkEvery = %d; residual = ||(resXi, resPsi)||_2 relative to its value after the first batch" % every)
    print("%-12s %6s | %-24s %10s | %-24s %10s | %s" % ("problem", "iters", "plain: to 1e-2/1e-3/1e-4", "final", "restart: to 1e-2/-3/-4", "final", "restarts at (min |cos| over the boundaries)"))
    for name, iters in CPU_CASES:
        p, (dh, ah) = load_problem(name)
        res = {}
        for restart in (False, True):
            o = Oracle(p["network"], p["tree"], p["config"])
            o.initialise(dh, ah)
            res[restart] = ro.restart_loop(o, iters, every, restart=restart)
        fmt = lambda r: "/".join("-" if v is None else str(v) for v in ro.iterations_to(r["norms"], every))  # noqa: E731
        fin = lambda r: "%.3g" % (r["norms"][-1] / r["norms"][0]) if r["norms"][0] > 0 else "0/0"  # noqa: E731
        cs = [abs(ro.cosine(t)) for t in res[True]["tests"]]
        same = np.array_equal(res[False]["hist"], res[True]["hist"])
        print("%-12s %6d | %-24s %10s | %-24s %10s | %s (%.3g)%s" % (name, iters, fmt(res[False]), fin(res[False]), fmt(res[True]), fin(res[True]),
                                                                   res[True]["fires"] or "never", min(cs), "  [run identical to plain APG]" if same else ""))
        sys.stdout.flush()


def gpu_half(every, rounds, batches):
    from rapidnet_amd import capi, synth

    print("== GPU half: barcelona493 (10 864 nodes), rn_apg_solve(%d, tol = 0, checkEvery = %d), ms per batch; median of %d interleaved regions" % (batches * every, every, rounds))
    p = synth.make_problem("barcelona493")
    f0 = synth.forecast_at(p["forecast"], 0)
    n = batches * every
    for structured in (False, True):
        s = {m: capi.Solver(p["network"], p["tree"], p["config"], structured=structured, restart=m) for m in ("off", "gradient")}
        for v in s.values():
            v.initialiseSmpcController(*f0)
            v.apg_solve(n, 0.0, every, history=False)           # warm-up: tables, checkpoints, code objects
        t = {m: [] for m in s}
        for _ in range(rounds):
            for m in ("off", "gradient"):
                s[m].synchronize()
                t0 = time.perf_counter()
                s[m].apg_solve(n, 0.0, every, history=False)
                s[m].synchronize()
                t[m].append(1e3 * (time.perf_counter() - t0) / batches)
        prof = {}
        for m in ("off", "gradient"):
            s[m].profileEnable(1)
            s[m].profileReset()
            s[m].apg_solve(n, 0.0, every, history=False)
            ms, cnt = s[m].profileRead()
            s[m].profileEnable(0)
            prof[m] = (float(ms[3]), int(cnt[3]))
        info = s["gradient"].last_restarts()
        off, on = float(np.median(t["off"])), float(np.median(t["gradient"]))
        print("%-10s off %.4f ms/batch (min %.4f max %.4f) | on %.4f ms/batch (min %.4f max %.4f) | on - off %+.4f ms (%+.2f %%)" % (
            "structured" if structured else "dense", off, min(t["off"]), max(t["off"]), on, min(t["gradient"]), max(t["gradient"]), on - off, 100 * (on - off) / off))
        print("%-10s profile class 3 over the solve: off %.4f ms in %d launches, on %.4f ms in %d launches -> k_restart_test %.2f us per batch; restarts %d, batches tested %d" % (
            "", prof["off"][0], prof["off"][1], prof["gradient"][0], prof["gradient"][1],
            1e3 * (prof["gradient"][0] - prof["off"][0]) / max(1, prof["gradient"][1] - prof["off"][1]), info["restarts"], info["tested"]))
        for v in s.values():
            v.close()
        sys.stdout.flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--keep-gpu", default=None)
    a = ap.parse_args()
    if not a.gpu_only:
        cpu_half(a.every)
    if a.gpu or a.gpu_only:
        gpu_half(a.every, a.rounds, a.batches)
    elif a.keep_gpu and os.path.exists(a.keep_gpu):
        txt = open(a.keep_gpu).read()
        print(txt[txt.index("== GPU half"):].rstrip() if "== GPU half" in txt else "== GPU half: not measured")
    else:
        print("== GPU half: not measured (needs an MI355X: python3 tools/ab_restart.py --gpu)")
