#!/usr/bin/env python3
"""What new values of A cost on a live solver: SCS.update_matrix against the only way there was before it, a new scs.SCS.

Two patterns: the BASELINE workload's (m = 2e6, n = 1e6, 20 nonzeros per column: nnz = 2e7, column-sorted pass layouts) and the
small config-5 shape (m = 4050, n = 1350, CSR-stream).  Only the pattern matters here: A is uniform random, the cone is the
positive orthant, nothing is solved.  Every timed step gets a new set of values on the same pattern and ends in a device
synchronise; the host clock is read around it.

  (a) init           scs.SCS(data', K): validation, uploads, transposition, equilibration, layout builders, allocations
                     (--legs init runs this leg alone: it needs nothing this tool's commit added, so it also runs on older trees)
  (b) first update   the first SCS.update_matrix of a solver: includes the value-map build (a new solver per repetition)
  (c) update         SCS.update_matrix from the second call on (host values: includes the upload of 8 nnz bytes)
      update_device  SCS.update_matrix_device (values in a torch tensor on the GPU)

Legs (a) and (c) alternate repetition by repetition after --warmup untimed ones.  Reported per leg: median, min, max, spread =
(max - min) / median.  The comparison is median (c) against median (a), judged against the spread of (a).

  python tools/matrix_update_bench.py [--shapes baseline,config5] [--reps 7] [--warmup 2] [--legs init,first,update] [--out FILE]
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

SHAPES = {"baseline": (2000000, 1000000, 20), "config5": (4050, 1350, 40)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="baseline,config5")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="init,first,update")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    legs = set(args.legs.split(","))

    import torch
    import scs
    from scs import _scs_hip
    import problem_gen as pg

    if _scs_hip.device_count() < 1:
        raise SystemExit("matrix_update_bench: no HIP device (there is nothing to measure without one)")
    common = dict(verbose=False, linear_solver=scs.LinearSolver.HIP_INDIRECT, max_iters=10)
    lines = ["matrix_update_bench: new values of A on a fixed pattern; %d timed repetitions per leg after %d warm-up ones" % (args.reps, args.warmup),
             "%-9s %9s %9s %10s | %-14s %10s %10s %10s %8s" % ("shape", "m", "n", "nnz", "leg", "median ms", "min ms", "max ms", "spread")]

    def sync():
        torch.cuda.synchronize()

    for shape in args.shapes.split(","):
        m, n, per_col = SHAPES[shape]
        rng = np.random.default_rng(3)
        A = pg.random_sparse(m, n, per_col, rng)
        data = {"A": A, "b": np.abs(rng.standard_normal(m)) + 0.5, "c": rng.standard_normal(n)}
        K = {"l": m}
        base = A.data.copy()

        def values(k):
            return base * (1.0 + 0.01 * ((k % 7) + 1))

        times = {"init": [], "first": [], "update": [], "update_device": []}
        solver = scs.SCS(data, K, **common) if "update" in legs else None
        if solver is not None:
            solver.update_matrix(A=values(0))  # (the maps exist from here on)
        for rep in range(args.warmup + args.reps):
            vals = values(rep + 1)
            order = ("init", "update") if rep % 2 == 0 else ("update", "init")
            for leg in order:
                if leg not in legs:
                    continue
                sync()
                if leg == "init":
                    A2 = A.copy()
                    A2.data = vals
                    d2 = dict(data, A=A2)
                    t0 = time.perf_counter()
                    fresh = scs.SCS(d2, K, **common)
                    sync()
                    dt = (time.perf_counter() - t0) * 1e3
                    if "first" in legs:
                        v2 = values(rep + 2)
                        sync()
                        t1 = time.perf_counter()
                        fresh.update_matrix(A=v2)
                        sync()
                        if rep >= args.warmup:
                            times["first"].append((time.perf_counter() - t1) * 1e3)
                    del fresh
                    if rep >= args.warmup:
                        times["init"].append(dt)
                else:
                    t0 = time.perf_counter()
                    solver.update_matrix(A=vals)
                    sync()
                    dt = (time.perf_counter() - t0) * 1e3
                    tv = torch.as_tensor(vals).cuda()
                    sync()
                    t1 = time.perf_counter()
                    solver.update_matrix_device(A=tv)
                    sync()
                    dt_dev = (time.perf_counter() - t1) * 1e3
                    del tv
                    if rep >= args.warmup:
                        times["update"].append(dt)
                        times["update_device"].append(dt_dev)
        med = {}
        for leg in ("init", "first", "update", "update_device"):
            if not times[leg]:
                continue
            t = np.array(times[leg])
            med[leg] = float(np.median(t))
            lines.append("%-9s %9d %9d %10d | %-14s %10.2f %10.2f %10.2f %7.1f%%" % (shape, m, n, A.nnz, leg, med[leg], t.min(), t.max(),
                                                                                   100.0 * (t.max() - t.min()) / med[leg]))
        if "init" in med:
            ti = np.array(times["init"])
            spread = ti.max() - ti.min()
            for leg in ("first", "update", "update_device"):
                if leg in med:
                    verdict = "beats" if med["init"] - med[leg] > spread else "does NOT beat"
                    lines.append("%-9s %s / init = %.3f (init is %.1f x; saves %.1f ms; spread of init %.1f ms): %s init by more than its spread" % (
                        shape, leg, med[leg] / med["init"], med["init"] / med[leg], med["init"] - med[leg], spread, verdict))
        del solver
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
