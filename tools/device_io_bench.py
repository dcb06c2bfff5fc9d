#!/usr/bin/env python3
"""What the host endpoints of a re-solve cost next to the device-resident ones (SCS.update_device / solve_device).

One CYCLE is what a sweep over one matrix does per step inside a torch program: new b and c (device tensors), a warm start
from the last solution, --iters ADMM iterations, the solution available as device tensors again.  Two ways, on two solvers over
the same data:

  host endpoints:    tensor -> numpy -> SCS.update / SCS.solve(warm_start=True) -> torch.as_tensor(x | y | s).cuda()
  device endpoints:  SCS.update_device / SCS.solve_device(warm_start=True)

The legs alternate cycle by cycle (same box, same minute), after --warmup untimed cycles of each; every cycle ends in a device
synchronise and is timed with the host clock.  Reported per leg: median, min, max and the spread (max - min) / median; the
comparison is median against median, judged against the host leg's spread.  Both legs see the same b, c in the same order and must
end every cycle with the same solution bits (checked outside the timed region).

  python tools/device_io_bench.py [--workloads target_lp_soc,config2_lp_soc] [--cycles 12] [--warmup 3] [--iters 20] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scs-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="target_lp_soc,config2_lp_soc")
    ap.add_argument("--cycles", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()

    import torch
    import scs
    from scs import _scs_hip
    import problem_gen as pg

    if _scs_hip.device_count() < 1:
        raise SystemExit("device_io_bench: no HIP device (there is nothing to measure without one)")
    proj = lambda z, K: _scs_hip.proj_cone(z, K, dual=True)  # noqa: E731
    common = dict(eps_abs=0.0, eps_rel=0.0, eps_infeas=0.0, verbose=False, acceleration_lookback=10,
                  linear_solver=scs.LinearSolver.HIP_INDIRECT, max_iters=args.iters)
    lines = ["device_io_bench: one warm-started re-solve cycle (update b and c, %d iterations, solution as device tensors), "
             "%d timed cycles per leg, legs alternating, %d warm-up cycles" % (args.iters, args.cycles, args.warmup),
             "%-16s %9s %9s | %-7s %9s %9s %9s %8s" % ("workload", "m", "n", "leg", "median ms", "min ms", "max ms", "spread")]
    for workload in args.workloads.split(","):
        K, n, k, seed = pg.workload(workload)
        data, _, _ = pg.gen_feasible(K, n, k, seed, proj)
        m = data["A"].shape[0]
        host_solver, dev_solver = scs.SCS(data, K, **common), scs.SCS(data, K, **common)
        b0, c0 = torch.as_tensor(data["b"]).cuda(), torch.as_tensor(data["c"]).cuda()
        host_solver.solve(warm_start=False)
        dev_solver.solve_device(warm_start=False)

        def host_cycle(b, c):
            host_solver.update(b.cpu().numpy(), c.cpu().numpy())
            r = host_solver.solve(warm_start=True)
            out = [torch.as_tensor(r[key]).cuda() for key in ("x", "y", "s")]
            torch.cuda.synchronize()
            return out

        def dev_cycle(b, c):
            dev_solver.update_device(b, c)
            r = dev_solver.solve_device(warm_start=True)
            torch.cuda.synchronize()
            return [r[key] for key in ("x", "y", "s")]

        times = {"host": [], "device": []}
        for cyc in range(args.warmup + args.cycles):
            b, c = b0 * (1.0 + 1e-3 * (cyc + 1)), c0 * (1.0 - 1e-3 * (cyc + 1))
            torch.cuda.synchronize()
            outs = {}
            for leg, fn in (("host", host_cycle), ("device", dev_cycle)) if cyc % 2 == 0 else (("device", dev_cycle), ("host", host_cycle)):
                t0 = time.perf_counter()
                outs[leg] = fn(b, c)
                if cyc >= args.warmup:
                    times[leg].append((time.perf_counter() - t0) * 1e3)
            for a, d in zip(outs["host"], outs["device"]):
                if not torch.equal(a, d) and not bool(((a == d) | (torch.isnan(a) & torch.isnan(d))).all()):
                    raise SystemExit("device_io_bench: the two legs disagree in cycle %d of %s" % (cyc, workload))
        med = {}
        for leg in ("host", "device"):
            t = np.array(times[leg])
            med[leg] = float(np.median(t))
            lines.append("%-16s %9d %9d | %-7s %9.2f %9.2f %9.2f %7.1f%%" % (workload, m, n, leg, med[leg], t.min(), t.max(),
                                                                          100.0 * (t.max() - t.min()) / med[leg]))
        host_t = np.array(times["host"])
        lines.append("%-16s device / host endpoints: %.3f  (saves %.2f ms per cycle; host-leg spread %.2f ms)" % (
            workload, med["device"] / med["host"], med["host"] - med["device"], host_t.max() - host_t.min()))
        if med["device"] > med["host"] + (host_t.max() - host_t.min()):
            lines.append("%-16s NOTE: the device-endpoint cycle is SLOWER than the host-endpoint cycle outside the host leg's spread" % workload)
        del host_solver, dev_solver
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
