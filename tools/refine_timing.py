#!/usr/bin/env python
"""What a refine call costs, next to the ADMM iterations it replaces: first numbers, nothing asserted.

On the config-2 LP + SOC instance of problem_gen (m = 2e5, n = 1e5, nnz ~ 2e6) it reports
  (a) a cold solve at eps = 1e-4,
  (b) SCS.refine(tol=1e-8) after it, with steps / halvings / lsqr_iters and the residuals before and after,
  (c) the ADMM loop alone from the same point to eps = 1e-8: a second solver with eps = 1e-8, warm-started from (a)'s x, y, s — the only
      way to that accuracy without refine.
Times are wall-clock around the calls (each returns with its stream idle).

    python tools/refine_timing.py [--workload config2_lp_soc] [--tol 1e-8] [--lsqr-max-iters N] [--max-iters N]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scs-python_amd"))

import scs  # noqa: E402
from scs import _scs_hip  # noqa: E402
import problem_gen as pg  # noqa: E402


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="config2_lp_soc")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-steps", type=int, default=10)
    ap.add_argument("--lsqr-tol", type=float, default=1e-8)
    ap.add_argument("--lsqr-max-iters", type=int, default=None, help="cap of one inner solve (default: 4 (n + m))")
    ap.add_argument("--max-iters", type=int, default=100000, help="ADMM iteration cap of (a) and (c)")
    args = ap.parse_args()
    if _scs_hip.device_count() < 1:
        raise SystemExit("refine_timing: no HIP device visible")
    K, n, k, seed = pg.workload(args.workload)
    data, p_star, _ = pg.gen_feasible(K, n, k, seed, lambda z, K: _scs_hip.proj_cone(z, K, dual=True))
    m = data["A"].shape[0]
    print("workload %s: m = %d, n = %d, nnz(A) = %d" % (args.workload, m, n, data["A"].nnz))
    stg = dict(verbose=False, max_iters=args.max_iters, linear_solver=scs.LinearSolver.HIP_INDIRECT)
    loose = scs.SCS(data, K, eps_abs=1e-4, eps_rel=1e-4, **stg)
    loose.solve(warm_start=False)  # (warm-up: kernels loaded, lazy setup done)
    sol, ms_a = timed(lambda: loose.solve(warm_start=False))
    ia = sol["info"]
    print("(a) solve at eps 1e-4: %.1f ms, %s, %d iterations, %d CG steps, res_pri %.2e res_dual %.2e gap %.2e" %
          (ms_a, ia["status"], ia["iter"], ia["cg_iters"], ia["res_pri"], ia["res_dual"], ia["gap"]))
    ref, ms_b = timed(lambda: loose.refine(tol=args.tol, max_steps=args.max_steps, lsqr_tol=args.lsqr_tol, lsqr_max_iters=args.lsqr_max_iters))
    ib = ref["info"]
    print("(b) refine(tol=%g, lsqr_tol=%g, lsqr_max_iters=%s): %.1f ms, stop %d (%s), steps %d, halvings %d, lsqr_iters %d" %
          (args.tol, args.lsqr_tol, args.lsqr_max_iters, ms_b, ib["stop"], ib["stop_reason"], ib["steps"], ib["halvings"], ib["lsqr_iters"]))
    print("    merit %.3e -> %.3e; res_pri %.2e -> %.2e, res_dual %.2e -> %.2e, gap %.2e -> %.2e; pobj %.9f (p* %.9f)" %
          (ib["merit_before"], ib["merit_after"], ib["res_pri_before"], ib["res_pri"], ib["res_dual_before"], ib["res_dual"], ib["gap_before"],
           ib["gap"], ib["pobj"], p_star))
    tight = scs.SCS(data, K, eps_abs=args.tol, eps_rel=args.tol, **stg)
    st, ms_c = timed(lambda: tight.solve(warm_start=True, x=sol["x"], y=sol["y"], s=sol["s"]))
    ic = st["info"]
    print("(c) ADMM alone from (a)'s point to eps %g: %.1f ms, %s, %d iterations, %d CG steps, res_pri %.2e res_dual %.2e gap %.2e" %
          (args.tol, ms_c, ic["status"], ic["iter"], ic["cg_iters"], ic["res_pri"], ic["res_dual"], ic["gap"]))
    print("(b) / (c) = %.2f" % (ms_b / ms_c))


if __name__ == "__main__":
    main()
