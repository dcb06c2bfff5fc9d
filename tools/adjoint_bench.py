#!/usr/bin/env python3
"""What the adjoint of a solve costs next to the solve: LSQR iterations to tol, time per LSQR iteration next to the time per CG step
of the same workspace, adjoint time next to solve time.

Workloads: the BASELINE LP+SOC workload (target_lp_soc, m = 2e6, n = 1e6), target_qp, one config-5 member without its PSD cones
(config5_member) and with them (config5_sdp: 5 cones of order 20), and config 4 (config4_psd: 50 cones of order 200).  Each is solved with a cap on ADMM iterations (--solve-iters; a run that ends at the cap is
"solved (inaccurate)" and differentiable), then SCS.adjoint_device runs --reps times on random cotangents with a cap on LSQR
iterations (--lsqr-cap).  By bytes an LSQR iteration is the products of two CG steps (A, A', P once each for M v and for M' u) plus about
ten passes over (n + m)-vectors.  Large LPs are often degenerate: stop = 2 or 3 and long runs are reported as they are.

Workloads with PSD cones get a second line: the preparation (the eigen-decomposition of the fixed point, once per call) and one W apply
next to one K9 projection of the same workspace (scs_hip_time_psd).  Neither has a timer of its own; both come from differences of
whole calls: with t(k) = the time of an adjoint call capped at k LSQR iterations, ms/LSQR it = (t(k2) - t(k1)) / (k2 - k1),
fixed = t(k1) - k1 ms/LSQR it (preparation + right-hand side + results), and an LSQR iteration is two W applies, the products of two
CG steps and the vector passes, so  W apply <= (ms/LSQR it - 2 ms/CG step) / 2  — an upper estimate that still holds the vector passes.

  python tools/adjoint_bench.py [--workloads target_lp_soc,target_qp,config5_member,config5_sdp,config4_psd] [--reps 3] [--out profiles/adjoint.txt]
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
    ap.add_argument("--workloads", default="target_lp_soc,target_qp,config5_member,config5_sdp,config4_psd")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solve-iters", type=int, default=400)
    ap.add_argument("--lsqr-cap", type=int, default=400)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()

    import torch
    import scs
    from scs import _scs_hip
    import problem_gen as pg

    if _scs_hip.device_count() < 1:
        raise SystemExit("adjoint_bench: no HIP device (there is nothing to measure without one)")
    proj = lambda z, K: _scs_hip.proj_cone(z, K, dual=True)
    lines = ["adjoint_bench: SCS.adjoint_device (want b, c) after a solve; tol %g, LSQR cap %d, ADMM cap %d, %d repetitions (median)" % (
        args.tol, args.lsqr_cap, args.solve_iters, args.reps),
        "%-15s %9s %9s %10s | %-22s %7s %6s %5s %10s %10s | %10s %10s %8s | %10s %10s" % (
            "workload", "m", "n", "nnz(A)", "solve status", "ADMM it", "CG it", "stop", "residual", "normal res", "ms/LSQR it", "ms/CG step",
            "ratio", "adjoint ms", "solve ms")]
    for name in args.workloads.split(","):
        if name == "config5_member":
            K, n, k, seed = pg.workload("config5_small")
            K = {"l": K["l"], "q": K["q"]}
        elif name == "config5_sdp":
            K, n, k, seed = pg.workload("config5_small")
        else:
            K, n, k, seed = pg.workload(name)
        if pg.workload_qp(name):
            data, _, _ = pg.gen_feasible_qp(K, n, k, seed, proj, b_per_col=pg.workload_qp(name))
        else:
            data, _, _ = pg.gen_feasible(K, n, k, seed, proj)
        m = data["A"].shape[0]
        sv = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iters=args.solve_iters)
        sol = sv.solve_device(warm_start=False)
        info = sol["info"]
        ms_cg = info["lin_sys_time"] / max(info["cg_iters"], 1)
        rng = np.random.default_rng(1)
        g = [torch.as_tensor(rng.standard_normal(k_)).cuda() for k_ in (n, m, m)]
        runs = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = sv.adjoint_device(dx=g[0], dy=g[1], ds=g[2], tol=args.tol, max_iters=args.lsqr_cap)
            torch.cuda.synchronize()
            if rep > 0:  # (the first call allocates the scratch)
                runs.append(((time.perf_counter() - t0) * 1e3, res["info"]))
        ms = float(np.median([r[0] for r in runs]))
        li = runs[-1][1]
        ms_it = float(np.median([r[1]["time_ms"] for r in runs])) / max(li["iters"], 1)
        lines.append("%-15s %9d %9d %10d | %-22s %7d %6d %5d %10.2e %10.2e | %10.4f %10.4f %8.2f | %10.2f %10.2f" % (
            name, m, n, data["A"].nnz, info["status"][:22], info["iter"], info["cg_iters"], li["stop"], li["residual"], li["normal_residual"],
            ms_it, ms_cg, ms_it / ms_cg if ms_cg > 0 else float("nan"), ms, info["solve_time"]))
        lines.append("%-15s   LSQR iterations %d; lin_sys_solver: %s" % (name, li["iters"], info["lin_sys_solver"]))
        if K.get("s"):
            def capped(cap):
                ts = []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = sv.adjoint_device(dx=g[0], dy=g[1], ds=g[2], tol=1e-300, max_iters=cap)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return float(np.median(ts)), r["info"]["iters"]
            (t1, k1), (t2, k2) = capped(8), capped(40)
            per_it = (t2 - t1) / max(k2 - k1, 1)
            k9 = sv._solver._time_psd(reps=10)
            lines.append("%-15s   PSD: %d cones, largest order %d | fixed part of a call (preparation + right-hand side + results) %.3f ms | "
                         "ms/LSQR it %.4f (caps %d, %d) | W apply <= %s ms | one K9 projection (warm) %.4f ms" % (
                             name, k9["matrices"], k9["max_order"], t1 - k1 * per_it, per_it, k1, k2,
                             "%.4f" % ((per_it - 2 * ms_cg) / 2) if per_it > 2 * ms_cg else "n/a (launch-bound)", k9["ms"]))
        del sv, sol, g
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
