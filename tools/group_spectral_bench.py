"""Grouped vs sequential solves of batches with spectral and complex PSD cones (csrc/batch.hpp).

For each case, `count` projection QPs  min 1/2 |z - w|^2  s.t. z in K  (one seeded w per member, the same cone for all) are
solved twice from fresh workspaces: once member after member with `.solve()`, once as one `scs.solve_batch` call.  The grouped
iterates are bit-identical to the sequential ones (checked here: `same_bits`), so both legs do the same iterations and the wall
times compare like for like.  Workspace setup (scs.SCS(...)) is outside both timings; the deferred part of the setup runs inside
either leg.  `plan` is what scs.batch_plan reports: the number of groups and of members solved alone.

Usage:  python tools/group_spectral_bench.py [--count 256] [--max-iters 2000] [--json] [--cases sl,d,nuc,cs]
Under `rocprofv3 --kernel-trace --stats -- python tools/group_spectral_bench.py --cases sl --count 256` the statistics show
the grouped kernels (k_grouped<...>) next to the one-problem kernels of the sequential leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scs-python_amd"))

import scs  # noqa: E402

CASES = {  # name -> (label, cone of one member)
    "sl": ("8 x sl n=16 k=4", {"sl_n": [16] * 8, "sl_k": [4] * 8}),
    "d": ("8 x d n=16", {"d": [16] * 8}),
    "nuc": ("8 x nuc 32x16", {"nuc_m": [32] * 8, "nuc_n": [16] * 8}),
    "cs": ("cs=[8, 4] + s=[6]", {"s": [6], "cs": [8, 4]}),
}


def rows(cone):
    sd = lambda n: n * (n + 1) // 2
    m = sum(sd(n) for n in cone.get("s", [])) + sum(k * k for k in cone.get("cs", []))
    m += sum(sd(n) + 2 for n in cone.get("d", []))
    m += sum(a * b + 1 for a, b in zip(cone.get("nuc_m", []), cone.get("nuc_n", [])))
    m += sum(n + 1 for n in cone.get("ell1", []))
    m += sum(sd(n) + 1 for n in cone.get("sl_n", []))
    return m


def members(cone, count, seed0):
    m = rows(cone)
    out = []
    for i in range(count):
        w = np.random.default_rng(seed0 + i).standard_normal(m)
        out.append(dict(P=sp.eye(m, format="csc"), A=-sp.eye(m, format="csc"), b=np.zeros(m), c=-w))
    return out


def run(name, count, max_iters):
    label, cone = CASES[name]
    datas = members(cone, count, 1000)
    stg = dict(linear_solver=scs.LinearSolver.HIP_INDIRECT, verbose=False, max_iters=max_iters)
    seq_solvers = [scs.SCS(d, cone, **stg) for d in datas]
    t0 = time.perf_counter()
    seq = [sv.solve(warm_start=False) for sv in seq_solvers]
    seq_s = time.perf_counter() - t0
    del seq_solvers
    grp_solvers = [scs.SCS(d, cone, **stg) for d in datas]
    plan = scs.batch_plan(grp_solvers)
    t0 = time.perf_counter()
    grp = scs.solve_batch(grp_solvers, warm_start=False)
    grp_s = time.perf_counter() - t0
    same = all(np.array_equal(a[k], b[k]) for a, b in zip(seq, grp) for k in ("x", "y", "s")) and \
        all(a["info"]["iter"] == b["info"]["iter"] for a, b in zip(seq, grp))
    iters = [r["info"]["iter"] for r in seq]
    return dict(case=label, members=count, m=rows(cone), groups=len({g for g in plan if g >= 0}), solo=plan.count(-1),
                iters_min=min(iters), iters_max=max(iters), iters_total=int(sum(iters)),
                sequential_s=round(seq_s, 3), grouped_s=round(grp_s, 3), speedup=round(seq_s / grp_s, 2),
                statuses=sorted({r["info"]["status"] for r in grp}), same_bits=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256, help="members per batch")
    ap.add_argument("--max-iters", type=int, default=2000)
    ap.add_argument("--cases", default="sl,d,nuc,cs")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    out = []
    for name in a.cases.split(","):
        r = run(name, a.count, a.max_iters)
        out.append(r)
        if not a.json:
            print("%-18s members %4d  m %5d  groups %d solo %3d  iters %4d..%4d (sum %7d)  sequential %8.3f s  grouped %7.3f s  "
                  "x%6.2f  same bits: %s  %s" % (r["case"], r["members"], r["m"], r["groups"], r["solo"], r["iters_min"], r["iters_max"],
                                                 r["iters_total"], r["sequential_s"], r["grouped_s"], r["speedup"], r["same_bits"],
                                                 ",".join(r["statuses"])), flush=True)
    if a.json:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
