#!/usr/bin/env python3
"""Same-process A/B of k_stream_gemv's skip at half-span granularity (RN_KNOB_STREAM_HALF, csrc/k_stream.hpp, stream_walk_half):

    knob 0: a live span is walked whole  |  default: each half of a span is walked or skipped by itself (where Ctx::stream_half_on admits it)

The sibling of tools/ab_stream_skip.py, whose machinery it reuses: contexts of one workload side by side, timed in ALTERNATING regions (reset, 20
iterations, then `--steps` timed ones; several rounds): ms per iteration min / median / max.  Then per context the streaming launch's time
from rn_profile_read, the bytes it requested (rn_algorithmic_bytes: those of the units it walked) and the
live shares of spans and units at iterations 25 and 320 after a reset.  Legs: the headline tree in fp64 with one | two workgroups per CU forced,
in fp32, with fp32-stored blocks, and barcelona31.

    python3 tools/ab_stream_half.py [--steps 300] [--rounds 5] > profiles/ab_stream_half.txt
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import ab_stream_skip as ab  # noqa: E402
from rapidnet_amd import synth  # noqa: E402


def unit_share(s):
    u, v = s.streamUnits(), s.streamLive()
    return u["liveUnits"] / max(u["units"], 1), v["liveSpans"] / max(v["spans"], 1), u["columnsPerUnit"]


def requested_bytes(s):
    """the block bytes of the units the last launch walked plus the vectors (rn_algorithmic_bytes)"""
    return s.algorithmicBytes()[0]


def leg(title, problem, variants, steps, rounds, profile_steps=40):
    ctxs = ab.contexts(problem, variants)
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
        at25 = unit_share(s)
        s.apgIterate(295, history=False)
        at320 = unit_share(s)
        s.apgReset()
        s.apgIterate(5, history=False)
        s.profileEnable(1); s.profileReset()
        s.apgIterate(profile_steps, history=False)
        ms, n = s.profileRead()
        s.profileEnable(0)
        us = [1e3 * ms[i] / max(int(n[i]), 1) for i in range(4)]
        req, k, info, r = requested_bytes(s), s.kernelInfo(), s.streamInfo(), regions[tag]
        gbs = req / (us[0] * 1e-6) / 1e9 if us[0] > 0 else 0.0
        rows[tag] = (float(np.median(r)), min(r), max(r), us[0])
        print("%-26s nodes %5d  ms/iteration median %.4f (min %.4f max %.4f, %d regions of %d) = %.1f it/s  stream %7.1f us  %5.3f GB requested  %6.0f GB/s = %.3f of peak  "
              "recursion+products %.1f us  dual update %.1f us  bookkeeping %.1f us  live units (of %d columns) | spans at iteration 25: %.4f | %.4f, at 320: %.4f | %.4f  "
              "G %d NL %d twoPerCU %d split@%d  storage %s"
              % (tag, s.nodes, np.median(r), min(r), max(r), len(r), steps, 1e3 / np.median(r), us[0], req / 1e9, gbs, gbs / ab.HBM_PEAK_GBS, us[1], us[2], us[3],
                 at25[2], at25[0], at25[1], at320[0], at320[1], k["stream_G"], k["stream_NL"], info["twoPerCU"], info["splitFirst"], "/".join(s.operatorStorage())), flush=True)
    for _, s in ctxs:
        s.close()
    a, b = rows[variants[0][0]], rows[variants[1][0]]
    print("halves against spans: iteration x%.3f (%.4f -> %.4f ms; slowest of the halves against the fastest of the spans x%.3f), streaming launch x%.3f (%.1f -> %.1f us)"
          % (a[0] / b[0], a[0], b[0], a[1] / b[2], a[3] / b[3], a[3], b[3]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--headline-only", action="store_true")
    args = ap.parse_args()
    print("# tools/ab_stream_half.py --workload %s --steps %d --rounds %d; dense operator mode; HBM peak taken as %.0f GB/s; the bytes of a launch are those of "
          "the units it walked (rn_debug_stream_units)" % (args.workload, args.steps, args.rounds, ab.HBM_PEAK_GBS))
    p = synth.make_problem(args.workload)
    off, on = {"knobs": {"stream_half": 0}}, {"knobs": {}}
    leg("%s, fp64" % args.workload, p, [("spans", off), ("halves", on),
                                         ("spans, one per CU", {"knobs": {"stream_half": 0, "stream_two_per_cu": 0}}),
                                         ("halves, one per CU", {"knobs": {"stream_two_per_cu": 0}}),
                                         ("spans, two per CU", {"knobs": {"stream_half": 0, "stream_two_per_cu": 1}}),
                                         ("halves, two per CU", {"knobs": {"stream_two_per_cu": 1}})], args.steps, args.rounds)
    if args.headline_only:
        return
    leg("%s, fp32 context" % args.workload, p, [("spans", dict(off, precision="f32")), ("halves", dict(on, precision="f32"))], args.steps, args.rounds)
    leg("%s, fp64 iterates on fp32 blocks" % args.workload, p, [("spans", dict(off, operator_storage="f32")), ("halves", dict(on, operator_storage="f32"))], args.steps, args.rounds)
    p31 = synth.make_problem("barcelona31")
    leg("barcelona31, fp64", p31, [("spans", off), ("halves", on)], args.steps, args.rounds)


if __name__ == "__main__":
    main()
