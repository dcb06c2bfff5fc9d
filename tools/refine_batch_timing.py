#!/usr/bin/env python
"""What the grouped refine buys: K solved members polished to --tol
  (a) one after the other, K `SCS.refine` calls on twin solvers (the path of the parent commit, unchanged by the grouped one)
  (b) by ONE `scs.refine_batch` call
for K in --members problems of problem_gen.workload("config5_small") ({"l": 2000, "q": [50]*20, "s": [20]*5}, n = 1350, m = 4050;
member i is generated with seed + i) and, as a second case, for --small members of a small generator problem of the tests
(tests/dproj_cones_ref.py "mixed", n = 16, m = 35, b and c moved by a seeded relative 1e-2: the launch-bound end).

A refine consumes its starting point, so every repetition first solves both sets again, cold, at eps 1e-4 (solve_batch; deterministic:
the same starting points every time), then times leg (b) on the members and leg (a) on the twins.  The first repetition is a warm-up and
is dropped; the table gives the median and the min .. max spread of the others, their ratio, the steps / halvings / LSQR iterations
per member, and the grouped launches and host synchronisations of one `refine_batch` call (`diff_group_launches`,
`diff_group_syncs`).  Every member's x, y, s and info (without time_ms) of leg (b) are asserted equal to its twin's of leg (a).

One process.  --time-limit seconds (default 1100) end it at the next return from the library: the limit is a Python signal handler,
which runs between two library calls and cannot interrupt one (a solo refine or the one refine_batch call), so run it under an outer
`timeout` as well.  Every leg prints a line when it is done, and --out is rewritten after every case: what was measured survives.
The defaults are the cases that finish in minutes (the small case and K = 8 config-5 members); a config-5 refine to 1e-9 runs its
inner LSQR solves for thousands of iterations, so K = 64 and 512 (--members 8,64,512) take a run of their own, case by case.

  python tools/refine_batch_timing.py [--members 8] [--small 64] [--reps 3] [--tol 1e-9] [--lsqr-max-iters N] [--out FILE]
"""
import argparse
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scs-python_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import scs  # noqa: E402
from scs import _scs_hip  # noqa: E402
import problem_gen as pg  # noqa: E402

LOOSE = dict(eps_abs=1e-4, eps_rel=1e-4, verbose=False, max_iters=100000, linear_solver=scs.LinearSolver.HIP_INDIRECT)


def config5_members(K):
    cone, n, k, seed = pg.workload("config5_small")
    proj = lambda z, c: _scs_hip.proj_cone(z, c, dual=True)
    out = []
    for i in range(K):
        data, _, _ = pg.gen_feasible(cone, n, k, seed + i, proj)
        out.append((data, cone))
    return out


def small_members(K):
    import dproj_cones_ref as dr
    p = dr.PROBLEMS["mixed"]()
    out = []
    for i in range(K):
        rng = np.random.default_rng(7000 + i)
        data = {"A": p["A"], "P": p["P"], "b": p["b"] * (1.0 + 1e-2 * rng.standard_normal(p["b"].shape[0])),
                "c": p["c"] * (1.0 + 1e-2 * rng.standard_normal(p["c"].shape[0]))}
        out.append((data, p["cone"]))
    return out


def spread(ts):
    return "%9.1f ms (%.1f .. %.1f)" % (statistics.median(ts), min(ts), max(ts))


def without_time(info):
    return {k: v for k, v in info.items() if k != "time_ms"}


def measure(label, problems, args, lines):
    K = len(problems)
    members = [scs.SCS(d, c, **LOOSE) for d, c in problems]
    twins = [scs.SCS(d, c, **LOOSE) for d, c in problems]
    t_group, t_solo, launches, syncs = [], [], 0, 0
    for rep in range(args.reps + 1):
        for svs in (members, twins):
            res = scs.solve_batch(svs, warm_start=False)
            bad = [r["info"]["status"] for r in res if r["info"]["status"] != "solved"]
            assert not bad, bad
        l0, s0 = _scs_hip.diff_group_launches(), _scs_hip.diff_group_syncs()
        t0 = time.perf_counter()
        got = scs.refine_batch(members, tol=args.tol, lsqr_max_iters=args.lsqr_max_iters)
        t1 = time.perf_counter()
        launches, syncs = _scs_hip.diff_group_launches() - l0, _scs_hip.diff_group_syncs() - s0
        print("  [%s K = %d, repetition %d: refine_batch done in %.1f ms, %d launches, %d synchronisations]" %
              (label, K, rep, (t1 - t0) * 1e3, launches, syncs), flush=True)
        t2 = time.perf_counter()
        solo = [sv.refine(tol=args.tol, lsqr_max_iters=args.lsqr_max_iters) for sv in twins]
        t3 = time.perf_counter()
        for i, (a, b) in enumerate(zip(got, solo)):
            for key in ("x", "y", "s"):
                assert np.array_equal(a[key], b[key]), (label, i, key)
            assert without_time(a["info"]) == without_time(b["info"]), (label, i, a["info"], b["info"])
        print("  [%s K = %d, repetition %d%s: grouped %.1f ms, solo %.1f ms]" % (label, K, rep, " (warm-up)" if rep == 0 else "", (t1 - t0) * 1e3,
                                                                                 (t3 - t2) * 1e3), flush=True)
        if rep > 0:  # (rep 0: the warm-up — kernels loaded, scratch taken from the pool)
            t_group.append((t1 - t0) * 1e3)
            t_solo.append((t3 - t2) * 1e3)
    plan = scs.diff_batch_plan(members)
    steps = [r["info"]["steps"] for r in got]
    halv = [r["info"]["halvings"] for r in got]
    its = [r["info"]["lsqr_iters"] for r in got]
    stops = sorted(set(r["info"]["stop"] for r in got))
    ratio = statistics.median(t_solo) / statistics.median(t_group)
    lines.append("%s, K = %d (groups %d, alone %d)" % (label, K, len(set(g for g in plan if g >= 0)), sum(1 for g in plan if g < 0)))
    lines.append("  K solo refine calls : %s" % spread(t_solo))
    lines.append("  one refine_batch    : %s   solo / grouped = %.2f" % (spread(t_group), ratio))
    lines.append("  per member: steps %d .. %d (mean %.2f), halvings %d .. %d, lsqr_iters %d .. %d (mean %.0f), stop values %s" %
                 (min(steps), max(steps), sum(steps) / K, min(halv), max(halv), min(its), max(its), sum(its) / K, stops))
    lines.append("  one refine_batch call: %d grouped launches, %d host synchronisations; bits equal to the twins' solo calls: yes" % (launches, syncs))
    print("\n".join(lines[-5:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="8")
    ap.add_argument("--small", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--lsqr-max-iters", type=int, default=None, help="cap of one inner solve (default: 4 (n + m))")
    ap.add_argument("--time-limit", type=int, default=1100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _scs_hip.device_count() < 1:
        raise SystemExit("refine_batch_timing: no HIP device visible")

    def out_of_time(signum, frame):
        raise SystemExit("refine_batch_timing: the time limit of %d s ran out" % args.time_limit)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)
    lines = ["python tools/refine_batch_timing.py " + " ".join(sys.argv[1:]),
             "solves at eps 1e-4, refine to %g; %d timed repetitions after one warm-up: median (min .. max), wall clock" % (args.tol, args.reps), ""]
    def keep():  # (after every case: what was measured survives the time limit)
        lines.append("")
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines))
    if args.small > 0:  # (the cheap case first)
        measure("tests' generator problem \"mixed\" (n = 16, m = 35)", small_members(args.small), args, lines)
        keep()
    for K in [int(v) for v in args.members.split(",") if v]:
        measure("config5_small", config5_members(K), args, lines)
        keep()
    signal.alarm(0)


if __name__ == "__main__":
    main()
