"""The dense numpy reference of the solve's derivatives (tests/adjoint_ref.py: W, J, lstsq, the gradient formulas) against central
differences of the CPU oracle's solutions — an LP, a QP and a QP with second-order cones; and the pure-Python surface of the feature
(the methods, the header, `import scs` without torch).  No GPU.

The bound is ten times the worst relative difference recorded for the problem in tests/golden/adjoint_fd.json (h = 1e-4, oracle at
eps 1e-9): it covers step-size and solver noise, not formula errors — a wrong sign gives O(1)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import adjoint_ref as ar
from oracle import scs_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "adjoint_fd.json")))


def oracle_solve(cone):
    def solve(data):
        r = scs_oracle.solve(data, cone, indirect=False, eps_abs=GOLD["eps"], eps_rel=GOLD["eps"], verbose=False, max_iters=200000)
        assert r["info"]["status"] == "solved", r["info"]
        return r
    return solve


@pytest.mark.parametrize("name", ["lp", "qp", "qp_soc"])
def test_reference_matches_central_differences(name):
    p = ar.PROBLEMS[name]()
    rec = GOLD[name]
    bound = 10 * max(v for k, v in rec.items() if k != "cond")
    for which in ("bcA", "P"):
        if which == "P" and p["P"] is None:
            continue
        rel, cond = ar.fd_compare(p, oracle_solve(p["cone"]), ar.FD_SEEDS[which], which, h=GOLD["h"])
        print("%s %s: relative difference %.3e (recorded %.3e), cond(J) %.3e" % (name, which, rel, rec[which], cond))
        assert cond <= 1e4
        assert rel <= bound, (name, which, rel, bound)


def test_generator_returns_an_optimal_pair():
    for name, fn in ar.PROBLEMS.items():
        p = fn()
        A, x, y, s = p["A"], p["x"], p["y"], p["s"]
        Pd = ar.full_P(p["P"]) if p["P"] is not None else np.zeros((x.size, x.size))
        assert np.abs(A @ x + s - p["b"]).max() < 1e-12
        assert np.abs(Pd @ x + A.T @ y + p["c"]).max() < 1e-12
        assert abs(s @ y) < 1e-12
        assert np.allclose(ar.project(s - y, p["cone"]), s, atol=1e-14)
        sol = oracle_solve(p["cone"])(ar.data_of(p))
        assert np.abs(sol["x"] - x).max() < 1e-6, name


def test_forward_and_adjoint_references_are_dual():
    p = ar.problem_qp()
    good = ar.adjoint(p["A"], p["P"], p["cone"], p["x"], p["y"], p["s"], gx=np.ones(12))
    dv = ar.derivative(p["A"], p["P"], p["cone"], p["x"], p["y"], p["s"], db=good["db"], dc=good["dc"])
    # duality of the two modes: <gx, dx(db, dc)> = <db_bar, db> + <dc_bar, dc>
    assert abs(np.ones(12) @ dv["dx"] - (good["db"] @ good["db"] + good["dc"] @ good["dc"])) < 1e-9 * (good["db"] @ good["db"] + good["dc"] @ good["dc"])


def test_methods_exist_on_every_front_end():
    import scs
    from scs import _scs_hip, _scs_hip_dense
    for cls in (scs.SCS, _scs_hip.SCS, _scs_hip_dense.SCS):
        for name in ("adjoint", "adjoint_device", "derivative", "derivative_device"):
            assert callable(getattr(cls, name)), (cls, name)


def test_import_scs_does_not_import_torch():
    code = ("import sys; sys.path[:0] = [%r, %r]; import scs; assert 'torch' not in sys.modules; "
            "assert 'scs.autograd' not in sys.modules" % (ROOT, os.path.join(ROOT, "scs-python_amd")))
    subprocess.check_call([sys.executable, "-c", code])
