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

--matrix is another leg: what the perturbation products of `derivative(db, dc, dA=, dP=)` (csrc/perturb.hpp) cost.  A workload is solved
as above; derivative_device then runs with a FIXED number of LSQR iterations (tol 1e-300, --lsqr-cap), without and with dA / dP, the two
interleaved and repeated: the difference of the medians is the cost of the three products and the vector kernel, and it stands next to
one LSQR iteration of the same run (the time of a call at the cap over the cap).  With --parent-root DIR (a built checkout of the
parent commit) the call WITHOUT dA / dP is also timed there, in child processes interleaved with child processes of this checkout:
it must not have become slower, the margin being the parent's own spread (max - min of its child medians) in that run.

  python tools/adjoint_bench.py --matrix [--workloads target_lp_soc,target_qp,config5_member] [--reps 5] [--parent-root DIR] [--out profiles/derivative_matrix.txt]

--cones is the leg of the box and power derivative (csrc/dproj_box_pow.hpp).  Two workloads built from a chosen primal-dual pair: box_qp, a
bounded QP in the MPC shape (--box-bounds variables, each with a lower and an upper bound: ONE box cone, t fixed to 1 by a zero row of
A, a third of the bounds active on each side; sparse positive definite P and --box-eq equality rows), and pow, --pow-cones power cones
(primal and dual exponents, a third each inside / polar / boundary) under a sparse square A and a diagonal P.  Each is solved, adjoint_device runs to --tol, then
with caps k1 < k2 on the LSQR iterations (tol 1e-300) ms/LSQR it = (t(k2) - t(k1)) / (k2 - k1); scs_hip_time_dproj times, with events on
the workspace's stream, one W apply of the cone — the box cone in BOTH forms at the same size — next to one projection of the same cone.
--box-sizes adds the two forms of the box apply at further sizes (the crossing of the two forms: kDboxMultiMin).

  python tools/adjoint_bench.py --cones [--box-bounds 60000] [--pow-cones 4000] [--box-sizes 1000,4000,16000,60000,99999] [--out profiles/adjoint_box_pow.txt]

--shared is the leg of the gradient of ONE matrix shared by a batch (csrc/grad_shared.hpp).  K config-5 members (config5_small, PSD cones
included) over one matrix are solved by solve_many_device; then, interleaved and repeated, leg (a) = adjoint_many_device(want b, c, A)
followed by .sum(0) over its (K, nnz) stack — the only way to that gradient before `reduce`, and the same entry with the same slots now —
and leg (b) = adjoint_many_device(want b, c, A, reduce="sum").  Per leg: the time of a call to --tol under --lsqr-cap, the time of the
gradient part (both legs capped at 1 LSQR iteration, tol 1e-300), and the device bytes a first call takes above the solve, on a freshly
solved batch after scs_hip_trim_pool: the growth of pool_stats()["live_bytes"] (the library's blocks: scratch, tables, panels) and of
torch's peak allocation (the results: the stack of leg (a) lives there).

  python tools/adjoint_bench.py --shared [--shared-k 64,512] [--reps 5] [--out profiles/adjoint_shared.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (child processes of --matrix: --root DIR imports the package of another checkout)
IMPORT_ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv[:-1] else ROOT
for p in (IMPORT_ROOT, os.path.join(IMPORT_ROOT, "scs-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_workload(name, pg, proj):
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
    return data, K, n


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def matrix_child(args):
    """one process: solve `--child-derivative`, print the median ms of --reps capped derivative_device(db, dc) calls (no dA / dP)"""
    import torch
    import scs
    from scs import _scs_hip
    import problem_gen as pg
    data, K, n = make_workload(args.child_derivative, pg, lambda z, K: _scs_hip.proj_cone(z, K, dual=True))
    m = data["A"].shape[0]
    sv = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iters=args.solve_iters)
    sv.solve_device(warm_start=False)
    rng = np.random.default_rng(1)
    db, dc = torch.as_tensor(rng.standard_normal(m)).cuda(), torch.as_tensor(rng.standard_normal(n)).cuda()
    ts = [timed(lambda: sv.derivative_device(db=db, dc=dc, tol=1e-300, max_iters=args.lsqr_cap), torch)[0] for _ in range(args.reps + 1)][1:]
    print("CHILD_MS %.6f" % float(np.median(ts)))


def matrix_leg(args):
    import subprocess
    import torch
    import scs
    from scs import _scs_hip
    import problem_gen as pg
    if _scs_hip.device_count() < 1:
        raise SystemExit("adjoint_bench: no HIP device (there is nothing to measure without one)")
    proj = lambda z, K: _scs_hip.proj_cone(z, K, dual=True)
    lines = ["adjoint_bench --matrix: SCS.derivative_device after a solve, %d LSQR iterations per call (tol 1e-300), ADMM cap %d, %d interleaved "
             "repetitions; ms: median [min .. max]" % (args.lsqr_cap, args.solve_iters, args.reps),
             "%-15s %9s %9s %10s %10s | %-26s %-26s %-26s %-26s | %10s | %10s %10s %10s" % (
                 "workload", "m", "n", "nnz(A)", "nnz(P)", "(db, dc) ms", "+ dA ms", "+ dP ms", "+ dA, dP ms", "ms/LSQR it", "dA cost", "dP cost",
                 "both cost")]
    fmt = lambda v: "%.3f [%.3f .. %.3f]" % (float(np.median(v)), min(v), max(v))
    for name in args.workloads.split(","):
        data, K, n = make_workload(name, pg, proj)
        m = data["A"].shape[0]
        has_P = data.get("P") is not None
        sv = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iters=args.solve_iters)
        info = sv.solve_device(warm_start=False)["info"]
        rng = np.random.default_rng(1)
        db, dc = torch.as_tensor(rng.standard_normal(m)).cuda(), torch.as_tensor(rng.standard_normal(n)).cuda()
        nnz_a = int(sv._solver._pattern["A"][1].shape[0])
        nnz_p = int(sv._solver._pattern["P"][1].shape[0]) if has_P else 0
        dA = torch.as_tensor(rng.standard_normal(nnz_a)).cuda()
        dP = torch.as_tensor(rng.standard_normal(nnz_p)).cuda() if has_P else None
        legs = {"plain": {}, "dA": {"dA": dA}}
        if has_P:
            legs["dP"] = {"dP": dP}
            legs["both"] = {"dA": dA, "dP": dP}
        call = lambda kw: sv.derivative_device(db=db, dc=dc, tol=1e-300, max_iters=args.lsqr_cap, **kw)
        for kw in legs.values():  # (the first call of each kind allocates: scratch, maps)
            call(kw)
        ms = {k: [] for k in legs}
        iters = 0
        for _ in range(args.reps):
            for k, kw in legs.items():
                t, r = timed(lambda: call(kw), torch)
                ms[k].append(t)
                iters = r["info"]["iters"]
        med = {k: float(np.median(v)) for k, v in ms.items()}
        per_it = med["plain"] / max(iters, 1)
        cost = lambda k: "%.4f" % (med[k] - med["plain"]) if k in med else "-"
        lines.append("%-15s %9d %9d %10d %10d | %-26s %-26s %-26s %-26s | %10.4f | %10s %10s %10s" % (
            name, m, n, nnz_a, nnz_p, fmt(ms["plain"]), fmt(ms["dA"]), fmt(ms["dP"]) if has_P else "-", fmt(ms["both"]) if has_P else "-",
            per_it, cost("dA"), cost("dP"), cost("both")))
        lines.append("%-15s   solve: %s, %d ADMM iterations; LSQR iterations per call %d; lin_sys_solver: %s" % (
            name, info["status"], info["iter"], iters, info["lin_sys_solver"]))
        del sv, db, dc, dA, dP
        if args.parent_root:
            here, there = [], []
            for _ in range(args.reps):
                for root, acc in ((args.parent_root, there), (ROOT, here)):
                    cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--child-derivative", name, "--reps", str(args.reps),
                           "--solve-iters", str(args.solve_iters), "--lsqr-cap", str(args.lsqr_cap)]
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                    if r.returncode != 0:
                        sys.exit("child at %s failed:\n%s" % (root, r.stderr[-3000:]))
                    acc.append(float([l for l in r.stdout.splitlines() if l.startswith("CHILD_MS")][-1].split()[1]))
            spread = max(there) - min(there)
            verdict = "not slower" if float(np.median(here)) <= float(np.median(there)) + spread else "SLOWER"
            lines.append("%-15s   derivative(db, dc) in child processes, parent commit / this commit interleaved: parent %s ms, this %s ms; "
                         "margin = the parent's spread %.3f ms: %s" % (name, fmt(there), fmt(here), spread, verdict))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def box_qp_workload(k, neq, seed=7):
    """(data, cone, pair): n = k variables, rows = neq equalities | t | k bounds; a third of the bounds active on each side"""
    from scipy import sparse
    rng = np.random.default_rng(seed)
    bl, bu = -rng.uniform(0.5, 2.0, k), rng.uniform(0.5, 2.0, k)
    kind = rng.integers(0, 20, k)
    bu[kind == 0] = np.inf
    bl[kind == 1] = 0.0
    sets = rng.integers(0, 3, k)
    sets[(sets == 0) & ~np.isfinite(bu)] = 2
    d = rng.uniform(0.3, 1.0, k)
    hi = np.where(np.isfinite(bu), bu, bl + 2.0)
    w = bl + rng.uniform(0.2, 0.8, k) * (hi - bl)
    U, L = sets == 0, sets == 1
    w[U], w[L] = bu[U] + d[U], bl[L] - d[L]
    v_box = np.concatenate([[1.0 - np.sum(d[U] * bu[U]) + np.sum(d[L] * bl[L])], w])
    s_box = np.concatenate([[1.0], np.where(U, bu, np.where(L, bl, w))])
    vz = rng.uniform(0.5, 1.5, neq) * rng.choice([-1.0, 1.0], neq)
    s = np.concatenate([np.zeros(neq), s_box])
    y = s - np.concatenate([vz, v_box])
    x = s_box[1:].copy()  # bound rows of A are -I with b = 0: s = x
    free = np.flatnonzero(sets == 2)  # (the equality rows couple free variables only: no row is decided by the active bounds alone)
    Aeq = sparse.csc_matrix((rng.standard_normal(8 * neq), (np.repeat(np.arange(neq), 8), rng.choice(free, 8 * neq))), shape=(neq, k))
    A = sparse.vstack([Aeq, sparse.csc_matrix((1, k)), -sparse.identity(k)]).tocsc()
    A.sort_indices()
    off = sparse.csc_matrix((rng.standard_normal(2 * k), (rng.integers(0, k, 2 * k), rng.integers(0, k, 2 * k))), shape=(k, k))
    P = sparse.csc_matrix(sparse.diags(1.0 + rng.random(k)) + 0.1 * (off + off.T))
    b = A @ x + s
    c = -(P @ x) - A.T @ y
    Pu = sparse.triu(P, format="csc")
    Pu.sort_indices()
    return {"A": A, "P": Pu, "b": b, "c": c}, {"z": neq, "bl": bl, "bu": bu}, (x, y, s)


def pow_workload(npow, n, seed=8):
    from scipy import sparse
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dproj_cones_ref as dr
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.1, 0.9, npow) * rng.choice([-1.0, 1.0], npow)
    v = np.concatenate([dr.pow_point(rng, a[i], ("in", "polar", "bd")[i % 3]) for i in range(npow)])
    s = np.concatenate([dr.pow_project(v[3 * i:3 * i + 3], a[i]) for i in range(npow)])
    y = s - v
    m = 3 * npow
    A = sparse.csc_matrix((rng.standard_normal(6 * m), (np.repeat(np.arange(m), 6), rng.integers(0, n, 6 * m))), shape=(m, n))
    A.sort_indices()
    x = rng.standard_normal(n)
    P = sparse.diags(1.0 + rng.random(n)).tocsc()
    return {"A": A, "P": P, "b": A @ x + s, "c": -(P @ x) - A.T @ y}, {"p": a}, (x, y, s)


def cones_leg(args):
    import torch
    import scs
    from scs import _scs_hip
    if _scs_hip.device_count() < 1:
        raise SystemExit("adjoint_bench: no HIP device (there is nothing to measure without one)")
    lines = ["adjoint_bench --cones: SCS.adjoint_device (want b, c) after a solve; tol %g, ADMM cap %d, %d repetitions (median); "
             "kernel times: %d launches between two events" % (args.tol, args.solve_iters, args.reps, args.kernel_reps)]
    works = (("box_qp", lambda: box_qp_workload(args.box_bounds, args.box_eq)), ("pow", lambda: pow_workload(args.pow_cones, 3 * args.pow_cones)))
    for name, make in works:
        data, K, (x0, _, _) = make()
        m, n = data["A"].shape
        sv = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, verbose=False, eps_abs=1e-8, eps_rel=1e-8, max_iters=args.solve_iters)
        sol = sv.solve_device(warm_start=False)
        info = sol["info"]
        rng = np.random.default_rng(1)
        g = [torch.as_tensor(rng.standard_normal(k_)).cuda() for k_ in (n, m, m)]
        call = lambda tol, cap: sv.adjoint_device(dx=g[0], dy=g[1], ds=g[2], tol=tol, max_iters=cap)
        call(args.tol, args.lsqr_cap)  # (the first call allocates the scratch)
        runs = [timed(lambda: call(args.tol, args.lsqr_cap), torch) for _ in range(args.reps)]
        li = runs[-1][1]["info"]

        def capped(cap):
            rs = [timed(lambda: call(1e-300, cap), torch) for _ in range(args.reps)]
            return float(np.median([r[0] for r in rs])), rs[-1][1]["info"]["iters"]
        (t1, k1), (t2, k2) = capped(8), capped(48)
        per_it = (t2 - t1) / max(k2 - k1, 1)
        tk = sv._solver._time_dproj(reps=args.kernel_reps)
        lines.append("%-7s m %d, n %d, nnz(A) %d | solve: %s, %d ADMM it, |x - x_built|_inf %.1e | adjoint to tol: %d LSQR it, stop %d, residual "
                     "%.2e, %.2f ms | ms/LSQR it %.4f (caps %d, %d), fixed part %.3f ms" % (
                         name, m, n, data["A"].nnz, info["status"], info["iter"], float(np.abs(sol["x"].cpu().numpy() - x0).max()), li["iters"],
                         li["stop"], li["residual"], float(np.median([r[0] for r in runs])), per_it, k1, k2, t1 - k1 * per_it))
        if tk["bsize"]:
            lines.append("%-7s box cone of %d bounds: W apply one workgroup %.4f ms | two launches %.4f ms | a call uses the %s form | one "
                         "projection (warm) %.4f ms" % (name, tk["bsize"] - 1, tk["box_apply_one_wg_ms"], tk["box_apply_two_launch_ms"],
                                                        "two-launch" if tk["bsize"] > 16384 else "one-workgroup", tk["box_proj_ms"]))
        if tk["pow_cones"]:
            lines.append("%-7s %d power cones: W apply %.4f ms | preparation of W (once per call) %.4f ms | one projection %.4f ms" % (
                name, tk["pow_cones"], tk["pow_apply_ms"], tk["pow_prep_ms"], tk["pow_proj_ms"]))
        del sv, sol, g
    if args.box_sizes:
        lines.append("box W apply by size (same generator, %d equality rows; ADMM cap 50: the kernels' time does not depend on the iterate):"
                     % args.box_eq)
        for k in [int(v) for v in args.box_sizes.split(",")]:
            data, K, _ = box_qp_workload(k, args.box_eq)
            sv = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iters=50)
            sv.solve_device(warm_start=False)
            tk = sv._solver._time_dproj(reps=args.kernel_reps)
            lines.append("  %7d bounds: one workgroup %.4f ms | two launches %.4f ms | projection %.4f ms" % (
                k, tk["box_apply_one_wg_ms"], tk["box_apply_two_launch_ms"], tk["box_proj_ms"]))
            del sv
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def shared_leg(args):
    import torch
    import scs
    from scs import _scs_hip
    import problem_gen as pg
    if _scs_hip.device_count() < 1:
        raise SystemExit("adjoint_bench: no HIP device (there is nothing to measure without one)")
    data, K, n = make_workload("config5_sdp", pg, lambda z, K: _scs_hip.proj_cone(z, K, dual=True))
    m, nnz = data["A"].shape[0], data["A"].nnz
    want = ("b", "c", "A")
    fmt = lambda v: "%8.2f [%8.2f .. %8.2f]" % (float(np.median(v)), min(v), max(v))
    lines = ["adjoint_bench --shared: config-5 members (m %d, n %d, nnz(A) %d) over one matrix, want (b, c, A); tol %g, LSQR cap %d, ADMM cap %d; "
             "%d interleaved repetitions, ms: median [min .. max]" % (m, n, nnz, args.tol, args.lsqr_cap, args.solve_iters, args.reps),
             "leg (a) = adjoint_many_device(want) + dA.sum(0) (the call of the parent commit: the same entry, the same slots); leg (b) = "
             "reduce=\"sum\"; gradient part = the same calls capped at 1 LSQR iteration; bytes = what a first call takes above the solve "
             "(library blocks + torch peak)",
             "%5s | %-30s | %-30s | %-12s | %-30s | %-30s | %-23s | %-23s | %10s | %s" % (
                 "K", "(a) stack + sum ms", "(b) reduce=sum ms", "(a) spread", "(a) gradient part ms", "(b) gradient part ms", "(a) bytes lib + torch",
                 "(b) bytes lib + torch", "K nnz 8", "max |dA_a - dA_b| / max |dA|")]

    def solved(count):
        rng = np.random.default_rng(count)
        B = data["b"][None, :] * (1.0 + 1e-3 * rng.standard_normal((count, 1)))
        C = data["c"][None, :] * (1.0 + 1e-3 * rng.standard_normal((count, 1)))
        sv = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iters=args.solve_iters)
        sv.solve_many_device(b=torch.as_tensor(B).cuda(), c=torch.as_tensor(C).cuda())
        g = [torch.as_tensor(rng.standard_normal((count, k_))).cuda() for k_ in (n, m, m)]
        return sv, g

    def leg_a(sv, g, tol, cap):
        r = sv.adjoint_many_device(g[0], g[1], g[2], want=want, tol=tol, max_iters=cap)
        return r["dA"].sum(0), r

    def leg_b(sv, g, tol, cap):
        r = sv.adjoint_many_device(g[0], g[1], g[2], want=want, tol=tol, max_iters=cap, reduce="sum")
        return r["dA"], r

    def first_call_bytes(count, leg):
        sv, g = solved(count)
        torch.cuda.synchronize()
        _scs_hip.trim_pool()
        torch.cuda.reset_peak_memory_stats()
        lib0, t0 = _scs_hip.pool_stats()["live_bytes"], torch.cuda.memory_allocated()
        leg(sv, g, 1e-300, 1)
        torch.cuda.synchronize()
        out = (_scs_hip.pool_stats()["live_bytes"] - lib0, torch.cuda.max_memory_allocated() - t0)
        del sv, g
        return out

    for count in [int(v) for v in args.shared_k.split(",")]:
        bytes_a, bytes_b = first_call_bytes(count, leg_a), first_call_bytes(count, leg_b)
        sv, g = solved(count)
        for leg in (leg_a, leg_b):  # (the first call of each kind allocates)
            leg(sv, g, args.tol, args.lsqr_cap)
            leg(sv, g, 1e-300, 1)
        ms = {k: [] for k in ("a", "b", "a1", "b1")}
        for _ in range(args.reps):
            for key, leg, tol, cap in (("a", leg_a, args.tol, args.lsqr_cap), ("b", leg_b, args.tol, args.lsqr_cap), ("a1", leg_a, 1e-300, 1),
                                       ("b1", leg_b, 1e-300, 1)):
                t, out = timed(lambda: leg(sv, g, tol, cap), torch)
                ms[key].append(t)
                if key == "a":
                    dA_a = out[0]
                if key == "b":
                    dA_b, iters = out[0], [i["iters"] for i in out[1]["info"]]
        spread = max(ms["a"]) - min(ms["a"])
        verdict = "not slower" if float(np.median(ms["b"])) <= float(np.median(ms["a"])) + spread else "SLOWER"
        diff = float((dA_a - dA_b).abs().max() / dA_a.abs().max())
        lines.append("%5d | %-30s | %-30s | %-12s | %-30s | %-30s | %10d + %10d | %10d + %10d | %10d | %.2e" % (
            count, fmt(ms["a"]), fmt(ms["b"]), "%.2f ms" % spread, fmt(ms["a1"]), fmt(ms["b1"]), bytes_a[0], bytes_a[1], bytes_b[0], bytes_b[1],
            count * nnz * 8, diff))
        lines.append("%5d   (b) against (a) + its spread: %s; LSQR iterations min %d max %d; panels of (b): 2 (n + m) min(K, 256) 8 = %d bytes" % (
            count, verdict, min(iters), max(iters), 2 * (n + m) * min(count, 256) * 8))
        del sv, g
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="target_lp_soc,target_qp,config5_member,config5_sdp,config4_psd")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solve-iters", type=int, default=400)
    ap.add_argument("--lsqr-cap", type=int, default=400)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--matrix", action="store_true", help="the leg that times derivative_device with and without dA / dP")
    ap.add_argument("--parent-root", default=None, help="--matrix: a built checkout of the parent commit for the comparison of derivative(db, dc)")
    ap.add_argument("--cones", action="store_true", help="the leg of the box and power derivative")
    ap.add_argument("--box-bounds", type=int, default=60000)
    ap.add_argument("--box-eq", type=int, default=200)
    ap.add_argument("--pow-cones", type=int, default=4000)
    ap.add_argument("--box-sizes", default="1000,4000,16000,60000,99999")
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--shared", action="store_true", help="the leg of the summed gradient of a shared matrix (reduce=\"sum\")")
    ap.add_argument("--shared-k", default="64,512")
    ap.add_argument("--child-derivative", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_derivative:
        return matrix_child(args)
    if args.matrix:
        return matrix_leg(args)
    if args.cones:
        return cones_leg(args)
    if args.shared:
        return shared_leg(args)

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
