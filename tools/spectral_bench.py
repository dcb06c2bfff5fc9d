"""Spectral cones (csrc/spectral.hpp): time one projection and one solve for a few shapes.

For each shape: a projection QP  min 1/2 |z - w|^2  s.t. z in K  (solution Pi_K(w)) is solved with the in-situ event timing of
the nonlinear cone projections on (scs_hip_set_profiling: out[8] / out[9] = total ms / samples of the queued iterations), so
`proj_ms` is the device time of one whole projection of all cones of the problem inside the ADMM loop; `solve_ms` is the wall
time of the solve and `iters` its iteration count.  No target exists for these numbers.

Usage:  python tools/spectral_bench.py [--count C] [--max-iters N] [--json]
Under `rocprofv3 --kernel-trace --stats -- python tools/spectral_bench.py` the kernel statistics show one launch of
k_proj_eig_cone / k_proj_nuc / k_proj_ell1 per kind and projection, whatever the number of cones.
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

SHAPES = [  # (name, cone builder of C cones)
    ("ell1 n=64", lambda C: {"ell1": [64] * C}),
    ("ell1 n=4096", lambda C: {"ell1": [4096] * C}),
    ("ell1 n=1e6 x1", lambda C: {"ell1": [1000000]}),
    ("sl n=16 k=4", lambda C: {"sl_n": [16] * C, "sl_k": [4] * C}),
    ("sl n=64 k=8", lambda C: {"sl_n": [64] * C, "sl_k": [8] * C}),
    ("d n=16", lambda C: {"d": [16] * C}),
    ("d n=64", lambda C: {"d": [64] * C}),
    ("nuc 32x16", lambda C: {"nuc_m": [32] * C, "nuc_n": [16] * C}),
    ("nuc 128x64", lambda C: {"nuc_m": [128] * C, "nuc_n": [64] * C}),
]


def rows(cone):
    sd = lambda n: n * (n + 1) // 2
    m = sum(sd(n) + 2 for n in cone.get("d", []))
    m += sum(a * b + 1 for a, b in zip(cone.get("nuc_m", []), cone.get("nuc_n", [])))
    m += sum(n + 1 for n in cone.get("ell1", []))
    m += sum(sd(n) + 1 for n in cone.get("sl_n", []))
    return m


def run(name, cone, max_iters, seed=0):
    m = rows(cone)
    w = np.random.default_rng(seed).standard_normal(m)
    data = dict(P=sp.eye(m, format="csc"), A=-sp.eye(m, format="csc"), b=np.zeros(m), c=-w)
    solver = scs.SCS(data, cone, linear_solver=scs.LinearSolver.HIP_INDIRECT, verbose=False, eps_abs=1e-7, eps_rel=1e-7,
                     max_iters=max_iters)
    solver._solver._set_profiling(True)
    t0 = time.perf_counter()
    sol = solver.solve()
    solve_ms = 1e3 * (time.perf_counter() - t0)
    kt = solver._solver._kernel_times()
    proj_ms = kt["cone_ms"] / kt["cone_n"] if kt["cone_n"] > 0 else float("nan")
    return dict(shape=name, cones=len(next(iter(cone.values()))), m=m, iters=sol["info"]["iter"], status=sol["info"]["status"],
                proj_ms=round(proj_ms, 4), proj_samples=kt["cone_n"], solve_ms=round(solve_ms, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=8, help="cones of the shape in one problem")
    ap.add_argument("--max-iters", type=int, default=2000)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    out = []
    for name, mk in SHAPES:
        r = run(name, mk(a.count), a.max_iters)
        out.append(r)
        if not a.json:
            print("%-14s cones %3d  m %7d  iters %5d  %-16s  projection %8.4f ms (%d samples)  solve %9.1f ms" % (
                r["shape"], r["cones"], r["m"], r["iters"], r["status"], r["proj_ms"], r["proj_samples"], r["solve_ms"]))
    if a.json:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
