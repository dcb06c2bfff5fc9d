"""Writes tests/golden/derivative_matrix_fd.json: the relative differences between the dense forward reference with matrix perturbations
(tests/derivative_matrix_ref.py) and central differences of the CPU oracle's solutions, for the problems, seed, h and eps
tests/test_derivative_matrix_ref_cpu.py uses.  Run from the repository root after the oracle is built:

    python tests/golden/make_derivative_matrix_fd.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import adjoint_ref as ar  # noqa: E402
import derivative_matrix_ref as dr  # noqa: E402
from oracle import scs_oracle  # noqa: E402

H, EPS = 1e-4, 1e-9


def main():
    out = {"_comment": "relative difference |prediction - fd| / |fd| of dx, dy, ds between the forward reference of "
                       "tests/derivative_matrix_ref.py in one random direction (dA, dP) (seed derivative_matrix_ref.FD_SEED) and central "
                       "differences (h) of the CPU oracle's solutions at eps; cond = cond2(J).  Written by "
                       "tests/golden/make_derivative_matrix_fd.py.  The tests assert ten times the worst figure.",
           "h": H, "eps": EPS}
    for name, make in ar.PROBLEMS.items():
        p = make()

        def solve(data):
            r = scs_oracle.solve(data, p["cone"], indirect=False, eps_abs=EPS, eps_rel=EPS, verbose=False, max_iters=200000)
            assert r["info"]["status"] == "solved", r["info"]
            return r

        rec = dr.fd_compare(p, solve, dr.FD_SEED, H)
        out[name] = {k: float("%.4g" % v) for k, v in rec.items()}
        print(name, out[name])
    with open(os.path.join(ROOT, "tests", "golden", "derivative_matrix_fd.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
