#!/usr/bin/env python3
"""What the multi adjoint buys: K cotangents at ONE solved problem differentiated
  (a) one after the other, K `adjoint_device` calls        [--parent-root: in a child process from a checkout of the parent commit]
  (b) by ONE `adjoint_multi_device` call, with the lanes' product at lane tile 4 and at lane tile 8 (scs_hip_diff_lane_tile)
for K = 1, 4, 8, 16, 32 on three problems: a config-5-sized QP (l = 2000, q = [50] * 20, n = 1350, with P), the `problem_big` of
tests/adjoint_ref.py (n = 300, m = 700) and an SDP with 8 blocks of order 20.

The legs are interleaved (a, b4, b8, a, ...) and repeated; the table gives the median and the min .. max spread of each, the LSQR
iterations per direction, and the launches per LSQR iteration: of leg (b) from the grouped-launch counter (two calls capped at 8 and
at 16 iterations, the difference over 8), of leg (a) K times the figure of a K = 1 multi call — the solo call issues the same kernels,
one launch each, and has no counter of its own.  Every row's db and iteration count of leg (b) are compared with this commit's solo
call on that row (np.array_equal).

The big problems are solved with a cap on ADMM iterations (--solve-iters; a run that ends at the cap is "solved (inaccurate)" and
differentiable) and LSQR runs to --tol with a cap of --lsqr-cap iterations, as tools/adjoint_bench.py does.

  python tools/adjoint_multi_bench.py [--ks 1,4,8,16,32] [--reps 3] [--parent-root DIR] [--out profiles/adjoint_multi.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBLEMS = ("config5_qp", "problem_big", "sdp_8x20")


def setup_path(root):
    sys.path[:0] = [root, os.path.join(root, "scs-python_amd"), os.path.join(root, "tests")]


def build(name, kmax, args):
    """(the solved scs.SCS, [GX, GY, GS] device tensors of kmax rows)"""
    import numpy as np
    import torch
    import scs
    from scs import _scs_hip
    import problem_gen as pg

    def proj(z, cone):
        return _scs_hip.proj_cone(z, cone, dual=True)

    stg = dict(verbose=False, linear_solver=scs.LinearSolver.HIP_INDIRECT, max_iters=args.solve_iters)
    if name == "config5_qp":
        cone = {"l": 2000, "q": [50] * 20}
        data, _, _ = pg.gen_feasible_qp(cone, 1350, 40, 1000, proj)
    elif name == "sdp_8x20":
        cone = {"l": 200, "s": [20] * 8}
        data, _, _ = pg.gen_feasible(cone, 600, 40, 1001, proj)
    else:
        import adjoint_ref as ar
        p = ar.problem_big()
        data, cone = ar.data_of(p), p["cone"]
        stg.update(eps_abs=1e-9, eps_rel=1e-9, max_iters=100000)
    sv = scs.SCS(data, cone, **stg)
    sv.solve()
    m, n = data["A"].shape
    rng = np.random.default_rng(2026)
    G = [torch.as_tensor(rng.standard_normal((kmax, w)), dtype=torch.float64).cuda() for w in (n, m, m)]
    return sv, G


def solo(sv, G, K, tol, cap):
    t0 = time.perf_counter()
    res = [sv.adjoint_device(dx=G[0][k], dy=G[1][k], ds=G[2][k], tol=tol, max_iters=cap) for k in range(K)]
    return time.perf_counter() - t0, res


def multi(sv, G, K, tol, cap):
    t0 = time.perf_counter()
    res = sv.adjoint_multi_device(dx=G[0][:K], dy=G[1][:K], ds=G[2][:K], tol=tol, max_iters=cap)
    return time.perf_counter() - t0, res


def child(args):
    """leg (a) alone, from the checkout at --root: one JSON line {K: [seconds]}"""
    setup_path(args.root)
    ks = [int(k) for k in args.ks.split(",")]
    sv, G = build(args.child_problem, max(ks), args)
    solo(sv, G, 2, args.tol, 2)
    out = {}
    for K in ks:
        out[K] = [solo(sv, G, K, args.tol, args.lsqr_cap)[0] for _ in range(args.reps)]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,4,8,16,32")
    ap.add_argument("--problems", default=",".join(PROBLEMS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solve-iters", type=int, default=400)
    ap.add_argument("--lsqr-cap", type=int, default=200)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: leg (a) runs there, in child processes")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--root", default=None)
    ap.add_argument("--child-problem", default=None)
    args = ap.parse_args()
    if args.child_problem:
        child(args)
        return
    setup_path(HERE)
    import numpy as np
    from scs import _scs_hip
    if _scs_hip.device_count() < 1:
        raise SystemExit("adjoint_multi_bench: no HIP device (there is nothing to measure without one)")
    lib = _scs_hip._lib
    ks = [int(k) for k in args.ks.split(",")]

    def fmt(v):
        return "%8.1f [%8.1f .. %8.1f]" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))

    lines = ["adjoint_multi_bench: want (b, c), tol %g, LSQR cap %d, ADMM cap %d; %d interleaved repetitions, ms: median [min .. max]"
             % (args.tol, args.lsqr_cap, args.solve_iters, args.reps),
             "leg (a) = K adjoint_device calls in turn (%s); leg (b) = one adjoint_multi_device call at lane tile 4 / 8; launches = per LSQR iteration"
             % ("parent commit, child process" if args.parent_root else "this commit, same process"),
             "%-12s %3s | %-30s | %-30s | %-30s | %7s %7s | %-14s | %9s %9s | %5s" % (
                 "problem", "K", "(a) solo ms", "(b) tile 4 ms", "(b) tile 8 ms", "(a)/(b4)", "(a)/(b8)", "LSQR iters", "launch(a)", "launch(b)", "bits")]
    for name in args.problems.split(","):
        sv, G = build(name, max(ks), args)
        solo(sv, G, 2, args.tol, 2)
        for tile in (4, 8):
            lib.scs_hip_diff_lane_tile(tile)
            multi(sv, G, max(ks), args.tol, 2)  # warm-up: code objects, the lanes, the tables' blocks in the pool
        parent = None
        if args.parent_root:
            cmd = [sys.executable, os.path.abspath(__file__), "--root", args.parent_root, "--child-problem", name, "--ks", args.ks, "--reps",
                   str(args.reps), "--solve-iters", str(args.solve_iters), "--lsqr-cap", str(args.lsqr_cap), "--tol", str(args.tol)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("leg (a) at the parent failed:\n" + r.stderr[-3000:])
            parent = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

        def per_iter(K):
            counts = []
            for cap in (8, 16):
                before = _scs_hip.diff_group_launches()
                multi(sv, G, K, args.tol, cap)
                counts.append(_scs_hip.diff_group_launches() - before)
            return (counts[1] - counts[0]) / 8.0

        one = per_iter(1)
        for K in ks:
            ta, tb = [], {4: [], 8: []}
            same = True
            ra = solo(sv, G, K, args.tol, args.lsqr_cap)[1]  # (this commit's solo bits; timed below unless the parent serves leg (a))
            for _ in range(args.reps):
                if parent is None:
                    ta.append(solo(sv, G, K, args.tol, args.lsqr_cap)[0])
                for tile in (4, 8):
                    lib.scs_hip_diff_lane_tile(tile)
                    t, rb = multi(sv, G, K, args.tol, args.lsqr_cap)
                    tb[tile].append(t)
                    same = same and all(bool((ra[k]["db"] == rb["db"][k]).all()) and ra[k]["info"]["iters"] == rb["info"][k]["iters"] for k in range(K))
            if parent is not None:
                ta = parent[str(K)]
            iters = [i["iters"] for i in rb["info"]]
            lines.append("%-12s %3d | %-30s | %-30s | %-30s | %7.2f %7.2f | %4d %4d %4d | %9.1f %9.1f | %5s" % (
                name, K, fmt(ta), fmt(tb[4]), fmt(tb[8]), statistics.median(ta) / statistics.median(tb[4]),
                statistics.median(ta) / statistics.median(tb[8]), min(iters), int(np.median(iters)), max(iters), K * one, per_iter(K),
                "same" if same else "DIFFER"))
            print(lines[-1], flush=True)
        lib.scs_hip_diff_lane_tile(4)  # (the library's default)
        del sv, G
    text = "\n".join(lines)
    print("\n" + text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
