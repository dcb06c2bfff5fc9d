"""The dense numpy reference of the forward derivative with matrix perturbations (tests/derivative_matrix_ref.py): its duality with the
adjoint reference's dL/dA and dL/dP, the triangle convention, and central differences of the CPU oracle's solutions.  No GPU.

Duality: for any cotangent g and any direction (db, dc, dA, dP)
    <g, (dx, dy, ds)> = <dL/db, db> + <dL/dc, dc> + <dL/dA, dA> + <dL/dP, dP>;
both sides come from one dense solve with J each, so they agree to 100 cond(J) 2^-52 times the product of the norms involved.
Finite differences: ten times the worst relative difference recorded in tests/golden/derivative_matrix_fd.json (h = 1e-4, oracle at
eps 1e-9) — step-size and solver noise, not formula errors: a wrong sign or a missing mirror image gives O(1)."""
import json
import os

import numpy as np
import pytest
from scipy import sparse

import adjoint_psd_ref as apr
import adjoint_ref as ar
import derivative_matrix_ref as dr
from oracle import scs_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "derivative_matrix_fd.json")))

DUAL = {"lp3": (ar.problem_lp3, ar), "qp_soc": (ar.problem_qp_soc, ar), "big": (ar.problem_big, ar), "qp_sdp": (apr.problem_qp_sdp, apr)}


@pytest.mark.parametrize("name", list(DUAL))
def test_forward_with_matrix_perturbations_is_dual_to_the_matrix_gradients(name):
    make, ref = DUAL[name]
    p = make()
    A, P, x, y, s = p["A"], p["P"], p["x"], p["y"], p["s"]
    m, n = A.shape
    rng = np.random.default_rng(17)
    gx, gy, gs = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    db, dc, dAv, dPv = dr.directions(p, 18)
    ad = ref.adjoint(A, P, p["cone"], x, y, s, gx, gy, gs)
    fw = dr.derivative(A, P, p["cone"], x, y, s, db, dc, dAv, dPv, forward=ref.derivative)
    bar = [ad["db"], ad["dc"], ar.stored_values(ad["dA"], A)]
    move = [db, dc, dAv]
    if P is not None:
        bar.append(ar.stored_values(ad["dP"], P))
        move.append(dPv)
    lhs = gx @ fw["dx"] + gy @ fw["dy"] + gs @ fw["ds"]
    rhs = sum(a @ b for a, b in zip(bar, move))
    cond = float(np.linalg.cond(ad["J"]))
    g, d = np.concatenate([gx, gy, gs]), np.concatenate([fw["dx"], fw["dy"], fw["ds"]])
    scale = np.linalg.norm(g) * np.linalg.norm(d) + np.linalg.norm(np.concatenate(bar)) * np.linalg.norm(np.concatenate(move))
    bound = 100 * cond * 2.0 ** -52
    print("duality %s: lhs %.15e rhs %.15e, difference / scale %.3e, bound %.3e, cond(J) %.3e" % (name, lhs, rhs, abs(lhs - rhs) / scale, bound, cond))
    assert abs(lhs - rhs) <= bound * scale


def test_the_triangle_convention():
    P = sparse.csc_matrix(np.array([[2.0, 1.0, 0.0], [0.0, 3.0, 4.0], [0.0, 0.0, 5.0]]))
    full = dr.dense_dP(P, np.array([10.0, 20.0, 30.0, 40.0, 50.0]))  # stored order: (0,0) (0,1) (1,1) (1,2) (2,2)
    assert np.array_equal(full, np.array([[10.0, 20.0, 0.0], [20.0, 30.0, 40.0], [0.0, 40.0, 50.0]]))
    A = sparse.csc_matrix(np.array([[1.0, 0.0, 2.0], [0.0, 3.0, 0.0]]))
    assert np.array_equal(dr.dense_dA(A, np.array([7.0, 8.0, 9.0])), np.array([[7.0, 0.0, 9.0], [0.0, 8.0, 0.0]]))
    x, y = np.array([1.0, 2.0, 3.0]), np.array([-1.0, 0.5])
    out_c, out_b = dr.products(A, P, x, y, np.array([7.0, 8.0, 9.0]), np.array([10.0, 20.0, 30.0, 40.0, 50.0]))
    assert np.allclose(out_b, [7.0 + 27.0, 16.0]) and np.allclose(out_c, full @ x + np.array([-7.0, 4.0, -9.0]))
    db_eff, dc_eff = dr.effective(A, P, x, y, db=np.ones(2), dc=np.ones(3), dAv=np.array([7.0, 8.0, 9.0]))
    assert np.allclose(db_eff, 1.0 - out_b) and np.allclose(dc_eff, 1.0 + np.array([-7.0, 4.0, -9.0]))


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
    got = dr.fd_compare(p, oracle_solve(p["cone"]), dr.FD_SEED, GOLD["h"])
    print("%s: relative differences %s (recorded %s)" % (name, got, rec))
    assert got["cond"] <= 1e4
    for key in ("dx", "dy", "ds"):
        assert got[key] <= bound, (name, key, got[key], bound)
