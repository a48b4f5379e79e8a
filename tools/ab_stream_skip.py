#!/usr/bin/env python3
"""Same-process A/B of k_stream_gemv's skip of operator spans that meet no nonzero dual entry (RN_KNOB_STREAM_SKIP, csrc/k_stream.hpp):

    knob 0: every span of every block is walked  |  knob 1: only the live spans, whole ones (the library's default also skips single
    half-spans: tools/ab_stream_half.py)

Contexts of one workload live side by side and are timed in ALTERNATING regions (rn_apg_reset, 20 iterations, then `--steps` timed ones; a region
of one context, then of the next, ...; several rounds), so that whatever the box does in the meantime hits all alike: ms per iteration min /
median / max.  Then per context the launch classes of rn_profile_read, the streaming launch's bandwidth from rn_algorithmic_bytes (the bytes of
the spans the launch walked), and the live shares of rn_debug_stream_live at iterations 25 and 320 after a reset.  Legs: the headline tree in
fp64 (with the skip also one | two workgroups per CU forced), in fp32, with fp32-stored blocks, barcelona31, and the dense-vector case -- one
sweep (rn_solve_step) at an all-nonzero dual, where the skip can only cost.

    python3 tools/ab_stream_skip.py [--steps 300] [--rounds 5] > profiles/ab_stream_skip.txt
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from rapidnet_amd import capi, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X, specification


def contexts(problem, variants):
    dh, ah = synth.forecast_at(problem["forecast"], 0)
    out = []
    for tag, kw in variants:
        s = capi.Solver(problem["network"], problem["tree"], problem["config"], **kw)
        s.initialiseSmpcController(dh, ah)
        out.append((tag, s))
    return out


def shares(s):
    v = s.streamLive()
    return v["liveSpans"] / max(v["spans"], 1), v["liveColumns"] / max(v["columns"], 1)


def measure(title, ctxs, steps, rounds, profile_steps=40):
    print("\n== %s ==" % title, flush=True)
    regions = {tag: [] for tag, _ in ctxs}
    for _ in range(rounds):
        for tag, s in ctxs:
            s.apgReset()
            s.apgIterate(20, history=False)
            s.synchronize()
            t0 = time.perf_counter()
            s.apgIterate(steps, history=False)
            s.synchronize()
            regions[tag].append(1e3 * (time.perf_counter() - t0) / steps)
    rows = {}
    for tag, s in ctxs:
        s.apgReset()
        s.apgIterate(25, history=False)
        at25 = shares(s)
        s.apgIterate(295, history=False)
        at320 = shares(s)
        s.apgReset()
        s.apgIterate(5, history=False)
        s.profileEnable(1); s.profileReset()
        s.apgIterate(profile_steps, history=False)
        ms, n = s.profileRead()
        s.profileEnable(0)
        us = [1e3 * ms[i] / max(int(n[i]), 1) for i in range(4)]
        bwd = s.algorithmicBytes()[0]
        k, info = s.kernelInfo(), s.streamInfo()
        r = regions[tag]
        gbs = bwd / (us[0] * 1e-6) / 1e9 if us[0] > 0 else 0.0
        rows[tag] = (float(np.median(r)), us[0], gbs)
        print("%-34s nodes %5d  ms/iteration median %.4f (min %.4f max %.4f, %d regions of %d)  stream %7.1f us  %5.3f GB  %6.0f GB/s = %.3f of peak  "
              "recursion+products %.1f us  dual update %.1f us  bookkeeping %.1f us  live spans | columns at iteration 25: %.4f | %.4f, at 320: %.4f | %.4f  "
              "G %d NL %d twoPerCU %d split@%d  storage %s"
              % (tag, s.nodes, np.median(r), min(r), max(r), len(r), steps, us[0], bwd / 1e9, gbs, gbs / HBM_PEAK_GBS, us[1], us[2], us[3],
                 at25[0], at25[1], at320[0], at320[1], k["stream_G"], k["stream_NL"], info["twoPerCU"], info["splitFirst"], "/".join(s.operatorStorage())), flush=True)
    return rows


def dense_vector(title, ctxs, sweeps=60):
    """one sweep at an all-nonzero dual (what FBE / NAMA Hessian sweeps, noise-filled warm starts and callers' dense duals look like): the streaming
    launch's time per context, alternating, from rn_profile_read"""
    print("\n== %s: rn_solve_step at an all-nonzero dual, streaming launch us (median of %d rounds of %d sweeps) ==" % (title, 5, sweeps), flush=True)
    rng = np.random.default_rng(3)
    times = {tag: [] for tag, _ in ctxs}
    for tag, s in ctxs:
        w = rng.standard_normal(s.nodes * s.ny) * 50
        w[w == 0] = 1.0
        w = w.reshape(s.nodes, s.ny)
        s.set(capi.BUF_ACC_XI, np.ascontiguousarray(w[:, :2 * s.nx]).ravel())
        s.set(capi.BUF_ACC_PSI, np.ascontiguousarray(w[:, 2 * s.nx:]).ravel())
        for _ in range(5):
            s.solveStep()
        s.synchronize()
    for _ in range(5):
        for tag, s in ctxs:
            s.profileEnable(1); s.profileReset()
            for _ in range(sweeps):
                s.solveStep()
            ms, n = s.profileRead()
            s.profileEnable(0)
            times[tag].append(1e3 * ms[0] / max(int(n[0]), 1))
    for tag, s in ctxs:
        t = times[tag]
        print("%-34s stream %7.1f us (min %.1f max %.1f)  live spans | columns %.4f | %.4f" % ((tag, float(np.median(t)), min(t), max(t)) + shares(s)), flush=True)


def leg(title, problem, variants, steps, rounds, dense=False):
    ctxs = contexts(problem, variants)
    rows = measure(title, ctxs, steps, rounds)
    if dense:
        dense_vector(title, ctxs[:2])
    for _, s in ctxs:
        s.close()
    a, b = rows[variants[0][0]], rows[variants[1][0]]
    print("skip against every span: iteration x%.3f (%.4f -> %.4f ms), streaming launch x%.3f (%.1f -> %.1f us)" % (a[0] / b[0], a[0], b[0], a[1] / b[1], a[1], b[1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--headline-only", action="store_true")
    args = ap.parse_args()
    print("# tools/ab_stream_skip.py --workload %s --steps %d --rounds %d; dense operator mode; HBM peak taken as %.0f GB/s; the bytes of a launch are those of "
          "the spans it walked (rn_algorithmic_bytes)" % (args.workload, args.steps, args.rounds, HBM_PEAK_GBS))
    p = synth.make_problem(args.workload)
    off, on = {"knobs": {"stream_skip": 0}}, {"knobs": {"stream_skip": 1}}
    leg("%s, fp64" % args.workload, p, [("every span", off), ("skip", on),
                                         ("every span, two per CU", {"knobs": {"stream_skip": 0, "stream_two_per_cu": 1}}),
                                         ("skip, one per CU", {"knobs": {"stream_skip": 1, "stream_two_per_cu": 0}}),
                                         ("skip, two per CU", {"knobs": {"stream_skip": 1, "stream_two_per_cu": 1}})], args.steps, args.rounds, dense=True)
    if args.headline_only:
        return
    leg("%s, fp32 context" % args.workload, p, [("every span", dict(off, precision="f32")), ("skip", dict(on, precision="f32"))], args.steps, args.rounds, dense=True)
    leg("%s, fp64 iterates on fp32 blocks" % args.workload, p, [("every span", dict(off, operator_storage="f32")), ("skip", dict(on, operator_storage="f32"))], args.steps, args.rounds)
    p31 = synth.make_problem("barcelona31")
    leg("barcelona31, fp64", p31, [("every span", off), ("skip", on)], args.steps, args.rounds)


if __name__ == "__main__":
    main()
