#!/usr/bin/env python3
"""Wall time of replacing all four per-node operators (Phi, Psi, D, Ftil) of every node of the headline tree (barcelona493: 10 864 nodes),
three routes in one process, fp64 and fp32 block storage:

    1  the per-node loop: rn_set_operator, nodes x 4 calls (two blocking copies of a whole block each) -- the only route there was, the yardstick
    2  rn_set_operators: the four host arrays in one call (k_pack_operators behind a bounded staging buffer)
    3  rn_set_operators_device: the four device arrays in one launch, timed between two hipEvents on the context's stream

and the kernel's GB/s of route 3 (bytes read + bytes written) beside rn_measure_hbm's copy figure of the same run; the read direction
(rn_get_operators_device) the same way.  After every route the stored blocks are compared with what route 1 left (bitwise).

    python3 tools/ab_operator_upload.py [--workload barcelona493] [--reps 5] [--per-node-nodes 0] > profiles/ab_operator_upload.txt

--per-node-nodes N > 0 times route 1 on the first N nodes only and scales to the tree (the loop is tens of seconds on the whole tree).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rapidnet_amd import capi, synth  # noqa: E402

NAMES = ("Phi", "Psi", "D", "Ftil")
OP = {"Phi": capi.OP_PHI, "Psi": capi.OP_PSI, "D": capi.OP_D, "Ftil": capi.OP_F}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="barcelona493")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--per-node-nodes", type=int, default=0)
    a = ap.parse_args()
    p = synth.make_problem(a.workload)
    dh, ah = synth.forecast_at(p["forecast"], 0)
    print("workload %s, kernel sources %s" % (a.workload, __import__("rapidnet_amd.build", fromlist=["x"]).kernel_sources_sha256()[:16]))
    for storage in ("native", "f32"):
        s = capi.Solver(p["network"], p["tree"], p["config"], operator_mode="dense", operator_storage=storage)
        s.initialiseSmpcController(dh, ah)
        read_gbs, copy_gbs = s.measureHbm(1 << 30, 3)
        elem = 4 if storage == "f32" else 8
        entries = s.nodes * 2 * s.nv * s.ny                   # entries of the four arrays together
        print("\n== fp64 context, %s blocks: %d nodes, nv %d, ny %d, %.2f GB of caller's arrays (fp64), %.2f GB stored; rn_measure_hbm: read %.0f GB/s, copy %.0f GB/s =="
              % (storage, s.nodes, s.nv, s.ny, entries * 8 / 1e9, entries * elem / 1e9, read_gbs, copy_gbs), flush=True)
        rng = np.random.default_rng(1)
        own = s.getOperators()
        new = {nm: b * (1.0 + 0.01 * rng.standard_normal(b.shape)) for nm, b in own.items()}
        del own
        # route 1
        n1 = s.nodes if a.per_node_nodes <= 0 else min(a.per_node_nodes, s.nodes)
        t0 = time.perf_counter()
        for node in range(n1):
            for nm in NAMES:
                s.setOperator(OP[nm], node, new[nm][node])
        s.synchronize()
        t1 = (time.perf_counter() - t0) * s.nodes / n1
        print("route 1  per-node rn_set_operator, %d calls%s: %10.1f ms" % (4 * n1, "" if n1 == s.nodes else " (scaled to %d nodes)" % s.nodes, 1e3 * t1), flush=True)
        ref = s.getOperators() if n1 == s.nodes else None
        # route 2
        t2 = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            s.setOperators(phi=new["Phi"], psi=new["Psi"], D=new["D"], F=new["Ftil"])
            t2.append(time.perf_counter() - t0)
        print("route 2  rn_set_operators (host arrays):            %10.1f ms median (min %.1f, max %.1f, %d calls)   %.0fx route 1"
              % (1e3 * np.median(t2), 1e3 * min(t2), 1e3 * max(t2), len(t2), t1 / np.median(t2)), flush=True)
        if ref is None:
            ref = s.getOperators()
        else:
            assert all(np.array_equal(ref[nm], v) for nm, v in s.getOperators().items()), "route 2 stored other bits than route 1"
        # route 3
        stream = torch.cuda.ExternalStream(int(s.lib.rn_stream(s.h)))
        for caller, dt in (("f64", torch.float64), ("f32", torch.float32)):
            dev = {nm: torch.from_numpy(new[nm]).to("cuda", dtype=dt) for nm in NAMES}
            out = {nm: torch.empty_like(v) for nm, v in dev.items()}
            torch.cuda.synchronize()
            csize = 8 if caller == "f64" else 4
            moved = entries * (csize + elem)
            for what, fn, arrs in (("rn_set_operators_device", s.setOperatorsDevice, dev), ("rn_get_operators_device", s.getOperatorsDevice, out)):
                ms = []
                for _ in range(a.reps + 1):       # first = warm-up
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn(caller, phi=arrs["Phi"].data_ptr(), psi=arrs["Psi"].data_ptr(), D=arrs["D"].data_ptr(), F=arrs["Ftil"].data_ptr())
                    e1.record(stream)
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                ms = ms[1:]
                med = float(np.median(ms))
                print("route 3  %s, %s arrays:      %10.3f ms median (min %.3f, max %.3f, %d launches)   %.2f GB read + written, %6.0f GB/s = %.2f of this run's copy figure%s"
                      % (what, caller, med, min(ms), max(ms), len(ms), moved / 1e9, moved / (med * 1e-3) / 1e9, moved / (med * 1e-3) / 1e9 / copy_gbs,
                         "   %.0fx route 1" % (t1 / (med * 1e-3)) if what.startswith("rn_set") else ""), flush=True)
            if caller == "f64":
                assert all(np.array_equal(ref[nm], v) for nm, v in s.getOperators().items()), "route 3 stored other bits than route 1"
                assert all(np.array_equal(ref[nm], out[nm].cpu().numpy()) for nm in NAMES), "rn_get_operators_device"
            del dev, out
        print("stored blocks of the three routes: bitwise equal", flush=True)
        s.close()
        del new, ref


if __name__ == "__main__":
    main()
