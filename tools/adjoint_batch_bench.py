#!/usr/bin/env python3
"""What the grouped adjoint buys: K solved config-5 members ({"l": 2000, "q": [50]*20, "s": [20]*5}, n = 1350, m = 4050) differentiated
  (a) one after the other, K `adjoint_device` calls        [--parent-root: in a child process from a checkout of the parent commit]
  (b) by ONE `adjoint_batch_device` call (clones: `adjoint_many_device`)
for K independent workspaces (own matrix copies, own b and c) and for K clones solved through `solve_many_device`.

The legs are interleaved (a, b, a, b, ...) and repeated; the table gives the median and the min .. max spread of each, the LSQR
iterations per member, the grouped launches of one call (`diff_group_launches`), and the fixed cost of a call — preparation (the fixed
point, the cone records, the eigen-decomposition of the PSD blocks), right-hand side and results — measured as a call capped at ONE
LSQR iteration, grouped next to K solo calls.  Every member's db of leg (b) is compared with leg (a)'s (np.array_equal).

Members are solved with a cap on ADMM iterations (--solve-iters; a run that ends at the cap is "solved (inaccurate)" and
differentiable) and LSQR runs to --tol with a cap of --lsqr-cap iterations, as tools/adjoint_bench.py does.

  python tools/adjoint_batch_bench.py [--members 64,512] [--clones 64] [--reps 3] [--parent-root DIR] [--out profiles/adjoint_batch.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def setup_path(root):
    sys.path[:0] = [root, os.path.join(root, "scs-python_amd")]


def build(K, clones, args):
    """K solved members and their cotangents: (solver objects with adjoint_device, the scs.SCS that owns clones or None, GX, GY, GS)"""
    import numpy as np
    import torch
    import scs
    from scs import _scs_hip
    import problem_gen as pg

    def proj(z, cone):
        return _scs_hip.proj_cone(z, cone, dual=True)

    cone, n, k, seed = pg.workload("config5_small")
    data, _, _ = pg.gen_feasible(cone, n, k, seed, proj)
    A = data["A"]
    m = A.shape[0]
    rng = np.random.default_rng(2025)
    B, Cm = np.empty((K, m)), np.empty((K, n))
    for i in range(K):  # problem_gen's construction over the fixed pattern: every member its own feasible (b, c)
        z = rng.standard_normal(m)
        y = np.asarray(proj(z, cone), dtype=np.float64)
        B[i] = A @ rng.standard_normal(n) + (y - z)
        Cm[i] = -(A.T @ y)
    stg = dict(verbose=False, linear_solver=scs.LinearSolver.HIP_INDIRECT, max_iters=args.solve_iters)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()
    if clones:
        owner = scs.SCS(data, cone, **stg)
        owner.solve_many_device(b=dev(B), c=dev(Cm))
        members = [owner._solver] + owner._solver._many
    else:
        owner = None
        members = [scs.SCS({"A": A, "b": B[i], "c": Cm[i]}, cone, **stg) for i in range(K)]
        scs.solve_batch(members)
    G = [dev(rng.standard_normal((K, w))) for w in (n, m, m)]
    return members, owner, G


def solo(members, G, tol, cap):
    t0 = time.perf_counter()
    res = [sv.adjoint_device(dx=G[0][i], dy=G[1][i], ds=G[2][i], tol=tol, max_iters=cap) for i, sv in enumerate(members)]
    return time.perf_counter() - t0, res


def grouped(members, owner, G, tol, cap):
    import scs
    t0 = time.perf_counter()
    if owner is not None:
        r = owner.adjoint_many_device(G[0], G[1], G[2], tol=tol, max_iters=cap)
        res = [{"db": r["db"][i], "info": r["info"][i]} for i in range(len(members))]
    else:
        res = scs.adjoint_batch_device(members, list(G[0]), list(G[1]), list(G[2]), tol=tol, max_iters=cap)
    return time.perf_counter() - t0, res


def child(args):
    """leg (a) alone, from the checkout at --root: one JSON line"""
    setup_path(args.root)
    K, clones = args.child_members, bool(args.child_clones)
    members, owner, G = build(K, clones, args)
    solo(members, G, args.tol, 1)  # warm-up: code objects, every member's DiffScratch
    full, prep = [], []
    for _ in range(args.reps):
        t, res = solo(members, G, args.tol, args.lsqr_cap)
        full.append(t)
        prep.append(solo(members, G, args.tol, 1)[0])
    print(json.dumps({"full": full, "prep": prep, "iters": [r["info"]["iters"] for r in res]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="64,512")
    ap.add_argument("--clones", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solve-iters", type=int, default=400)
    ap.add_argument("--lsqr-cap", type=int, default=200)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: leg (a) runs there, in child processes")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--root", default=None)
    ap.add_argument("--child-members", type=int, default=0)
    ap.add_argument("--child-clones", type=int, default=0)
    args = ap.parse_args()
    if args.child_members:
        child(args)
        return
    setup_path(HERE)
    import numpy as np
    import scs
    from scs import _scs_hip
    if _scs_hip.device_count() < 1:
        raise SystemExit("adjoint_batch_bench: no HIP device (there is nothing to measure without one)")

    def fmt(v):
        return "%8.1f [%8.1f .. %8.1f]" % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))

    lines = ["adjoint_batch_bench: config-5 members, want (b, c), tol %g, LSQR cap %d, ADMM cap %d; %d interleaved repetitions, ms: median [min .. max]"
             % (args.tol, args.lsqr_cap, args.solve_iters, args.reps),
             "leg (a) = K adjoint_device calls in turn (%s); leg (b) = one grouped call; fixed = the same calls capped at 1 LSQR iteration"
             % ("parent commit, child processes" if args.parent_root else "this commit, same process"),
             "%-18s %5s | %-30s | %-30s | %7s %10s | %-30s | %-30s | %-14s %9s %5s" % (
                 "members", "K", "(a) solo ms", "(b) grouped ms", "(a)/(b)", "(a) spread", "(a) fixed ms", "(b) fixed ms", "LSQR iters", "launches", "bits")]
    cases = [(int(k), False) for k in args.members.split(",") if k] + ([(args.clones, True)] if args.clones > 0 else [])
    for K, clones in cases:
        members, owner, G = build(K, clones, args)
        plan = scs.diff_batch_plan(members) if owner is None else _scs_hip.diff_batch_plan(members)
        assert plan == [0] * K, plan  # (one group: what leg (b) measures)
        solo(members[:2], G, args.tol, 2)
        grouped(members, owner, G, args.tol, 2)  # warm-up of both legs (every member's DiffScratch, the tables' blocks in the pool)
        ta, tb, pa, pb = [], [], [], []
        same = True
        for _ in range(args.reps):
            if args.parent_root:
                cmd = [sys.executable, os.path.abspath(__file__), "--root", args.parent_root, "--child-members", str(K), "--child-clones",
                       str(int(clones)), "--reps", "1", "--solve-iters", str(args.solve_iters), "--lsqr-cap", str(args.lsqr_cap), "--tol", str(args.tol)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    sys.exit("leg (a) at the parent failed:\n" + r.stderr[-3000:])
                rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                ta.extend(rec["full"])
                pa.extend(rec["prep"])
                ra = solo(members, G, args.tol, args.lsqr_cap)[1] if not tb else None  # (this commit's solo bits, once; not timed)
            else:
                t, ra = solo(members, G, args.tol, args.lsqr_cap)
                ta.append(t)
            before = scs.diff_group_launches()
            t, rb = grouped(members, owner, G, args.tol, args.lsqr_cap)
            launches = scs.diff_group_launches() - before
            tb.append(t)
            if ra is not None:
                same = same and all(bool((x["db"] == y["db"]).all()) and x["info"]["iters"] == y["info"]["iters"] for x, y in zip(ra, rb))
            if not args.parent_root:
                pa.append(solo(members, G, args.tol, 1)[0])
            pb.append(grouped(members, owner, G, args.tol, 1)[0])
        iters = [r["info"]["iters"] for r in rb]
        lines.append("%-18s %5d | %-30s | %-30s | %7.2f %8.1f ms | %-30s | %-30s | %4d %4d %4d %9d %5s" % (
            "clones (solve_many)" if clones else "independent", K, fmt(ta), fmt(tb), statistics.median(ta) / statistics.median(tb),
            1e3 * (max(ta) - min(ta)), fmt(pa), fmt(pb), min(iters), int(np.median(iters)), max(iters), launches,
            "same" if same else "DIFFER"))
        print(lines[-1], flush=True)
        del members, owner, G
    text = "\n".join(lines)
    print("\n" + text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
