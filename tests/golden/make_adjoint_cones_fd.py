"""Writes tests/golden/adjoint_cones_fd.json: the relative difference between the dense reference of tests/dproj_cones_ref.py (adjoint:
<gradient, direction>; forward: dx, dy, ds) and central differences (h = 1e-4) of the CPU oracle's solutions at eps 1e-9, on the three
problems of dproj_cones_ref.PROBLEMS with the seeds of dproj_cones_ref.FD_SEEDS, and cond2(J).  tests/test_dproj_cones_ref_cpu.py
asserts ten times the worst figure of a problem.  Run from the repository root:  python tests/golden/make_adjoint_cones_fd.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dproj_cones_ref as dr  # noqa: E402
from oracle import scs_oracle  # noqa: E402

H, EPS = 1e-4, 1e-9
FWD_SEED = 302


def oracle_solve(cone):
    def solve(data):
        r = scs_oracle.solve(data, cone, indirect=False, eps_abs=EPS, eps_rel=EPS, verbose=False, max_iters=200000)
        assert r["info"]["status"] == "solved", r["info"]
        return r
    return solve


def main():
    out = {"_comment": "relative difference between the dense reference of tests/dproj_cones_ref.py and central differences (h = 1e-4) "
                       "of the CPU oracle's solutions at eps 1e-9: bcA / P = <adjoint gradient, direction>, fwd = the worst of dx, dy, "
                       "ds of the forward derivative; cond = cond2(J).  Written by tests/golden/make_adjoint_cones_fd.py; "
                       "tests/test_dproj_cones_ref_cpu.py asserts ten times the worst figure of a problem.",
           "h": H, "eps": EPS, "fwd_seed": FWD_SEED}
    for name, fn in dr.PROBLEMS.items():
        p = fn()
        solve = oracle_solve(p["cone"])
        rec = {}
        for which in ("bcA", "P"):
            rel, cond = dr.fd_compare(p, solve, dr.FD_SEEDS[which], which, h=H)
            rec[which] = float("%.3e" % rel)
            rec["cond"] = float("%.4g" % cond)
        rec["fwd"] = float("%.3e" % dr.forward_fd_compare(p, solve, FWD_SEED, h=H))
        out[name] = rec
        print(name, rec)
    with open(os.path.join(HERE, "adjoint_cones_fd.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
