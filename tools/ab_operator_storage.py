#!/usr/bin/env python3
"""Same-process A/B of the dense operator storage on the headline tree (barcelona493) and on rank 0's 1/8 shard of it:

    fp64 native  |  fp64 iterates on fp32 blocks (rn_set_operator_storage, k_stream_gemv<double, ..., float>)  |  fp32 context

The three contexts live side by side and are timed in ALTERNATING regions of rn_apg_iterate (a region of one, then of the next, ...;
several rounds), so that whatever the box does in the meantime hits all three alike; medians per context.  Then, with rn_profile_enable,
the streaming class's time per launch and its bandwidth from rn_algorithmic_bytes.  The yardstick of the mixed kernel is the fp32
context's k_stream_gemv of the same run: the same block bytes.  The mixed context is run twice more with RN_KNOB_STREAM_TWO_PER_CU
forced to 0 and to 1 (which instantiation its launches take).

    python3 tools/ab_operator_storage.py [--steps 200] [--rounds 5] [--workload barcelona493] [--no-shard] > profiles/ab_operator_storage.txt

The NAMA leg (--nama, or --nama-only without the APG part): ms per NAMA iteration on the whole tree with fp32-stored blocks, the two Hessian
sweeps one after the other (rn_set_sweep_pairing(RN_PAIR_OFF)) and in one pass (RN_PAIR_ON, k_stream_gemv over fp32 storage with two right-hand sides),
the native fp64 context's paired figure beside them, rn_fbe_counters of each; alternating regions of rn_algorithm_fbe_nama, medians and the
run-to-run spread (min, max over the regions).  --append FILE adds the leg's lines to FILE.  On a checkout from before rn_set_sweep_pairing
the leg runs what exists there: the sequential fp32-storage figure and the native paired one (the comparison that counts is that checkout's
sequential figure against this one's RN_PAIR_ON).

    python3 tools/ab_operator_storage.py --nama-only [--nama-iters 40] [--rounds 5] --append profiles/ab_operator_storage.txt
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from rapidnet_amd import capi, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X, specification


def contexts(problem, tree, shard, variants):
    dh, ah = synth.forecast_at(problem["forecast"], 0)
    out = []
    for tag, kw in variants:
        s = capi.Solver(problem["network"], tree, problem["config"], **kw)
        if shard is not None:
            s.commInit(0, 1, capi.comm_unique_id())
            s.setCutStage(shard[0], shard[1])
        s.initialiseSmpcController(dh, ah)
        out.append((tag, s))
    return out


def measure(title, ctxs, steps, rounds, profile_steps=40):
    print("\n== %s ==" % title)
    for tag, s in ctxs:
        s.apgReset()
        for _ in range(3):
            s.apgIterate(20, history=False)
        s.synchronize()
    regions = {tag: [] for tag, _ in ctxs}
    for _ in range(rounds):
        for tag, s in ctxs:
            t0 = time.perf_counter()
            s.apgIterate(steps, history=False)
            s.synchronize()
            regions[tag].append(1e3 * (time.perf_counter() - t0) / steps)
    rows = {}
    for tag, s in ctxs:
        s.apgReset()
        s.apgIterate(5, history=False)
        s.profileEnable(1); s.profileReset()
        s.apgIterate(profile_steps, history=False)
        ms, n = s.profileRead()
        s.profileEnable(0)
        us = 1e3 * ms[0] / max(int(n[0]), 1)
        bwd = s.algorithmicBytes()[0]
        k, info, mem = s.kernelInfo(), s.streamInfo(), s.deviceMemoryInfo()
        r = regions[tag]
        rows[tag] = (float(np.median(r)), us, bwd / (us * 1e-6) / 1e9 if us > 0 else 0.0)
        print("%-28s nodes %5d  ms/iteration median %.4f (min %.4f max %.4f, %d regions of %d)  stream %7.1f us  %5.2f GB  %6.0f GB/s = %.3f of peak  "
              "G %d NL %d twoPerCU %d split@%d  context %.2f GB  storage %s"
              % (tag, s.nodes, np.median(r), min(r), max(r), len(r), steps, us, bwd / 1e9, rows[tag][2], rows[tag][2] / HBM_PEAK_GBS, k["stream_G"], k["stream_NL"],
                 info["twoPerCU"], info["splitFirst"], mem["context_bytes"] / 1e9, "/".join(s.operatorStorage())), flush=True)
    return rows


def summary(rows):
    n, m, f = rows["f64 native"], rows["f64 on fp32 blocks"], rows["f32"]
    print("mixed against native: iteration x%.3f, stream x%.3f;  mixed against the fp32 context's kernel: bandwidth %.3f (1.000 = the yardstick), stream %+.1f us"
          % (n[0] / m[0], n[1] / m[1], m[2] / f[2], m[1] - f[1]))
    for k in ("f64 on fp32 blocks, one per CU", "f64 on fp32 blocks, two per CU"):
        if k in rows:
            print("%s: ms/iteration %.4f, stream %.1f us" % (k, rows[k][0], rows[k][1]))


def nama_leg(problem, iters, rounds, label, sink):
    """ms per NAMA iteration, whole tree: fp32-stored blocks sequential | paired, native fp64 (paired by default)"""
    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    has_setting = hasattr(capi, "PAIRINGS")
    variants = [("f64 on fp32 blocks, two sweeps", dict(operator_storage="f32", **({"sweep_pairing": "off"} if has_setting else {})))]
    if has_setting:
        variants.append(("f64 on fp32 blocks, paired", dict(operator_storage="f32", sweep_pairing="on")))
    variants.append(("f64 native, paired", {}))
    dh, ah = synth.forecast_at(problem["forecast"], 0)
    ctxs = []
    for tag, kw in variants:
        s = capi.Solver(problem["network"], problem["tree"], problem["config"], **kw)
        s.initialiseSmpcController(dh, ah)
        s.setAlgorithm("namaAlgorithm", 5)
        ctxs.append((tag, s))
    say("\n== NAMA, whole tree, %s: %d iterations per region, %d alternating regions per context%s ==" %
        (label, iters, rounds, "" if has_setting else " (this checkout has no rn_set_sweep_pairing: fp32-stored blocks run the two sweeps)"))
    for _, s in ctxs:
        s.algorithmNama(min(iters, 10))
        s.synchronize()
    regions = {tag: [] for tag, _ in ctxs}
    for _ in range(rounds):
        for tag, s in ctxs:
            t0 = time.perf_counter()
            s.algorithmNama(iters)
            s.synchronize()
            regions[tag].append(1e3 * (time.perf_counter() - t0) / iters)
    rows = {}
    for tag, s in ctxs:
        r, c, info = regions[tag], s.fbeCounters(), s.streamInfo()
        rows[tag] = float(np.median(r))
        state = "/".join(str(v) for v in s.sweepPairing()) if has_setting else "n/a"
        say("%-32s nodes %5d  ms/NAMA iteration median %.4f (min %.4f max %.4f, spread %.1f %%)  counters %s  pairing %s  twoPerCU %d split@%d  storage %s"
            % (tag, s.nodes, rows[tag], min(r), max(r), 100.0 * (max(r) - min(r)) / rows[tag], c, state, info["twoPerCU"], info["splitFirst"], "/".join(s.operatorStorage())))
        s.close()
    if has_setting:
        a, b = rows["f64 on fp32 blocks, two sweeps"], rows["f64 on fp32 blocks, paired"]
        say("fp32-stored blocks, paired against two sweeps: x%.3f (%.4f -> %.4f ms per NAMA iteration); native paired %.4f" % (a / b, a, b, rows["f64 native, paired"]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--no-shard", action="store_true")
    ap.add_argument("--nama", action="store_true", help="also the NAMA leg")
    ap.add_argument("--nama-only", action="store_true", help="the NAMA leg alone")
    ap.add_argument("--nama-iters", type=int, default=40)
    ap.add_argument("--label", default="this checkout")
    ap.add_argument("--append", default=None, help="file the NAMA leg's lines are appended to")
    args = ap.parse_args()
    variants = [("f64 native", {}), ("f64 on fp32 blocks", {"operator_storage": "f32"}), ("f32", {"precision": "f32"}),
                ("f64 on fp32 blocks, one per CU", {"operator_storage": "f32", "knobs": {"stream_two_per_cu": 0}}),
                ("f64 on fp32 blocks, two per CU", {"operator_storage": "f32", "knobs": {"stream_two_per_cu": 1}})]
    p = synth.make_problem(args.workload)
    if args.nama or args.nama_only:
        sink = open(args.append, "a") if args.append else None
        nama_leg(p, args.nama_iters, args.rounds, "%s, %s" % (args.workload, args.label), sink)
        if sink:
            sink.close()
        if args.nama_only:
            return
    print("# tools/ab_operator_storage.py --workload %s --steps %d --rounds %d; dense operator mode; HBM peak taken as %.0f GB/s" % (args.workload, args.steps, args.rounds, HBM_PEAK_GBS))
    ctxs = contexts(p, p["tree"], None, variants)
    summary(measure("%s, whole tree" % args.workload, ctxs, args.steps, args.rounds))
    for _, s in ctxs:
        s.close()
    if not args.no_shard:
        cut = capi.default_cut_stage(p["tree"])
        part = capi.partition_tree(p["tree"], 0, 8, cut)
        ctxs = contexts(p, part["tree"], (cut, (part["momE"], part["momP"])), variants)
        summary(measure("%s, rank 0's shard of 8 (one-rank communicators: everything but the wire)" % args.workload, ctxs, args.steps, args.rounds))
        for _, s in ctxs:
            s.close()


if __name__ == "__main__":
    main()
