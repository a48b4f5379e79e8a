#!/usr/bin/env python3
"""Wall time of changing the box and safety bounds of a live context on the headline tree (barcelona493), in one process, routes interleaved,
with dense fp64 blocks, in structured mode and with fp32-stored blocks:

    today          what a caller had to do before rn_set_bounds existed: rn_factor_step with new vectors (one row for the whole tree only)
    host shared    rn_set_bounds, RN_BOUNDS_SHARED (host arrays; synchronises)
    host stage     ... RN_BOUNDS_PER_STAGE, N rows
    host node      ... RN_BOUNDS_PER_NODE, one row per node
    device ...     rn_set_bounds_device at the three granularities (arrays already in device memory; launches on the context's stream)

each followed by the same rn_update_state_control + rn_eliminate_input_disturbance_coupling + rn_synchronize of a control step; host clock
around the whole route.  The repeats alternate between two sets of values, so every call changes every value; the median of the repeats is
reported.  At the end 20 iterations after a shared set are compared with those of a context whose factor step was given the same vectors
(bitwise).

    python3 tools/ab_bounds.py [--workload barcelona493] [--reps 7] > profiles/ab_bounds.txt
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rapidnet_amd import build, capi, synth  # noqa: E402

KEYS = ("xmin", "xmax", "xsafe", "umin", "umax")
NET = {"xmin": "vecXmin", "xmax": "vecXmax", "xsafe": "vecXsafe", "umin": "vecUmin", "umax": "vecUmax"}
STORAGES = (("dense", "native"), ("structured", "native"), ("dense", "f32"))
GRANS = ("shared", "stage", "node")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    p = synth.make_problem(a.workload)
    fc = synth.forecast_at(p["forecast"], 0)
    tree = p["tree"]
    N, nodes = int(tree["N"][0]), int(tree["nodes"][0])
    stages = np.asarray(tree["stages"], int)
    own = {k: np.asarray(p["network"][NET[k]], float)[None, :] for k in KEYS}
    nx, nu = own["xmin"].shape[1], own["umin"].shape[1]

    def values(which):
        """two sets of values per granularity: the safety volume and the capacities move by a few per cent, differently per row"""
        f = 1.0 + 0.02 * (which + 1)
        out = {}
        for g, rows in (("shared", 1), ("stage", N), ("node", nodes)):
            ramp = 1.0 + 0.1 * np.arange(rows)[:, None] / max(rows - 1, 1)
            out[g] = {k: np.ascontiguousarray(np.repeat(v, rows, axis=0) * ((f * ramp) if k == "xsafe" else (1.0 / (f * ramp) if k in ("xmax", "umax") else 1.0)))
                      for k, v in own.items()}
        return out

    sets = [values(0), values(1)]
    print("workload %s: %d nodes, %d stages, nx %d, nu %d; per-node arrays %.2f MB (fp64); kernel sources %s"
          % (a.workload, nodes, N, nx, nu, nodes * (3 * nx + 2 * nu) * 8 / 1e6, build.kernel_sources_sha256()[:16]))

    def tail(s):
        s.updateStateControl()
        s.eliminateInputDistubanceCoupling(*fc)
        s.synchronize()

    for mode, storage in STORAGES:
        live = capi.Solver(p["network"], tree, p["config"], operator_mode=mode, operator_storage=storage)
        again = capi.Solver(dict(p["network"]), tree, p["config"], operator_mode=mode, operator_storage=storage)
        for s in (live, again):
            s.factorStep()
            tail(s)
        dev = [{g: {k: torch.from_numpy(v).cuda() for k, v in st[g].items()} for g in GRANS} for st in sets]
        torch.cuda.synchronize()
        for g in GRANS:                              # the tables of every granularity exist before anything is timed
            live.setBounds(g, **sets[0][g])
        routes = ["today"] + ["host " + g for g in GRANS] + ["device " + g for g in GRANS]
        times = {r: [] for r in routes}
        for rep in range(a.reps + 1):               # first = warm-up
            st, dv = sets[(rep + 1) % 2], dev[(rep + 1) % 2]
            for k in KEYS:
                again.network[NET[k]] = st["shared"][k][0]
            t0 = time.perf_counter()
            again.factorStep()
            tail(again)
            dt = {"today": time.perf_counter() - t0}
            for g in GRANS:
                t0 = time.perf_counter()
                live.setBounds(g, **st[g])
                tail(live)
                dt["host " + g] = time.perf_counter() - t0
            for g in GRANS:
                t0 = time.perf_counter()
                live.setBoundsDevice(g, "f64", **{k: v.data_ptr() for k, v in dv[g].items()})
                tail(live)
                dt["device " + g] = time.perf_counter() - t0
            if rep:
                for r in routes:
                    times[r].append(dt[r])
        med = {r: float(np.median(v)) for r, v in times.items()}
        print("\n== fp64 context, %s operators, %s block storage (%d repeats, alternating values) ==" % (mode, storage, a.reps))
        for r in routes:
            what = "rn_factor_step (new shared vectors)" if r == "today" else ("rn_set_bounds%s, %s" % ("_device" if r.startswith("device") else "", r.split()[1]))
            v = times[r]
            print("%-14s %-48s %10.3f ms median (min %.3f, max %.3f)%s" % (r, what + " + elimination:", 1e3 * med[r], 1e3 * min(v), 1e3 * max(v),
                                                                          "" if r == "today" else "   %.1fx today's route" % (med["today"] / med[r])), flush=True)
        last = sets[(a.reps + 1) % 2]["shared"]           # what `again` was given last
        live.setBounds("shared", **last)
        tail(live)
        hists = []
        for s in (live, again):
            s.apgReset()
            hists.append((s.apgIterate(20), s.get(capi.BUF_X), s.get(capi.BUF_U)))
        assert all(np.isfinite(v).all() and np.array_equal(v, w) for v, w in zip(*hists)), "a shared set differs from a factor step with the same vectors"
        assert live.operatorMode() == again.operatorMode()
        print("20 iterations after a shared set and after a factor step with the same vectors: bitwise equal (operator mode %s)" % (live.operatorMode(),), flush=True)
        live.close(); again.close()
        del dev


if __name__ == "__main__":
    main()
