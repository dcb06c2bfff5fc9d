"""The numpy reference of the box-cone and power-cone derivatives (tests/dproj_cones_ref.py) against central differences — of an
independent projection found by bisection for box_W and pow_W alone, of the CPU oracle's solutions for the dense adjoint and forward
references on the three problems.  No GPU.

The bound of the second is ten times the worst relative difference recorded for the problem in tests/golden/adjoint_cones_fd.json
(written by tests/golden/make_adjoint_cones_fd.py; h = 1e-4, oracle at eps 1e-9): it covers step-size and solver noise, not formula
errors — a wrong sign or a missing factor gives O(0.1)."""
import json
import os

import numpy as np
import pytest

import adjoint_ref as ar
import dproj_cones_ref as dr
from oracle import scs_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "adjoint_cones_fd.json")))
EPS = 2.0 ** -52


def oracle_solve(cone):
    def solve(data):
        r = scs_oracle.solve(data, cone, indirect=False, eps_abs=GOLD["eps"], eps_rel=GOLD["eps"], verbose=False, max_iters=200000)
        assert r["info"]["status"] == "solved", r["info"]
        return r
    return solve


@pytest.mark.parametrize("k", [1, 2, 3, 10, 40])
@pytest.mark.parametrize("mode", ["pos", "zero", "noU", "noL"])
def test_box_W_is_symmetric_and_matches_central_differences_of_the_projection(k, mode):
    rng = np.random.default_rng(100 * k + len(mode))
    tstar = 0.0 if mode == "zero" else rng.uniform(0.5, 1.5)
    v, bl, bu = dr.box_case(rng, k, tstar, empty={"noU": ("U",), "noL": ("L",)}.get(mode, ()))
    t = dr.box_tstar(v, bl, bu)
    assert abs(t - tstar) <= 1e-12 * max(1.0, np.abs(v).max())  # the generator's claim
    W = dr.box_W(v, bl, bu)
    assert np.abs(W - W.T).max() == 0.0
    # Within one choice of the sets the projection is LINEAR in v, and no row is within 0.1 of changing its set: the central
    # difference has no truncation error, only the rounding of the two projections, 2 eps |Pi(v)| / (2 h) per entry — times 8 for the
    # bisection's own last bits
    h = 1e-6
    bound = 8 * EPS * max(1.0, np.abs(v).max()) / h
    worst = 0.0
    for _ in range(3):
        u = rng.standard_normal(k + 1)
        fd = (dr.box_project(v + h * u, bl, bu) - dr.box_project(v - h * u, bl, bu)) / (2 * h)
        worst = max(worst, np.abs(W @ u - fd).max() / np.linalg.norm(u))
    print("box_W k = %d %s: worst |W u - central difference| / |u| %.2e (bound %.2e)" % (k, mode, worst, bound))
    assert worst <= bound
    if mode == "zero":
        assert not W[0].any() and not W[:, 0].any()


def test_box_W_active_zero_bound_is_not_a_free_row():
    v = np.array([1.0, -0.7, 0.3])
    bl, bu = np.array([0.0, -1.0]), np.array([2.0, 1.0])
    t, a, act, h = dr.box_coef(v, bl, bu)
    assert t == 1.0 and act.tolist() == [True, False] and a.tolist() == [0.0, 0.0] and h == 1.0
    W = dr.box_W(v, bl, bu)
    assert np.array_equal(W, np.diag([1.0, 0.0, 1.0]))


@pytest.mark.parametrize("a", [0.1, 0.3, 0.5, 0.9, -0.3, -0.5])
@pytest.mark.parametrize("case", ["in", "polar", "bd"])
def test_pow_W_is_symmetric_and_matches_central_differences_of_the_projection(a, case):
    rng = np.random.default_rng(int(1000 * abs(a)) + (7 if a < 0 else 0) + len(case))
    h = 1e-5
    worst_ratio = 0.0
    for _ in range(5):
        v = dr.pow_point(rng, a, case)
        assert dr.pow_case_of(v, a) == case
        W = dr.pow_W(v, a)
        assert np.abs(W - W.T).max() <= 4 * EPS * max(1.0, np.abs(W).max())
        if case == "in":
            assert np.array_equal(W, np.eye(3))
        if case == "polar":
            assert not W.any()
        # The projection is smooth away from the case boundaries; its central difference errs by h^2 |D^3 Pi| / 6 plus the rounding
        # 2 eps |v| / (2 h).  The length scale of the surface at the projected point p is rho = min(p_x, p_y) (the Hessian of
        # x^a y^(1-a) is r / x^2, r / (x y), r / y^2 up to factors a (1 - a) <= 1/4), and the generator keeps rho >= 0.05 |v| and the
        # distance to the surface >= 0.05, so |D^3 Pi| is a small multiple of 1 / rho^2: 60 / rho^2 is used, i.e. 10 h^2 / rho^2.
        # Inside the cone and its polar the projection is linear.
        p = dr.pow_project_primal(v if a >= 0 else -v, abs(a))
        rho = min(p[0], p[1]) if case == "bd" else np.inf
        bound = 10 * h * h / rho ** 2 + 8 * EPS * np.abs(v).max() / h
        for _ in range(3):
            u = rng.standard_normal(3)
            fd = (dr.pow_project(v + h * u, a) - dr.pow_project(v - h * u, a)) / (2 * h)
            err = np.abs(W @ u - fd).max() / np.linalg.norm(u)
            worst_ratio = max(worst_ratio, err / bound)
            assert err <= bound, (a, case, v, err, bound)
    print("pow_W a = %g %s: worst error / bound %.2e" % (a, case, worst_ratio))


def test_pow_dual_is_moreau_of_the_primal():
    rng = np.random.default_rng(5)
    for a in (0.2, 0.5, 0.8):
        for case in ("in", "polar", "bd"):
            v = dr.pow_point(rng, a, case)
            assert np.allclose(dr.pow_project(v, a) - dr.pow_project(-v, -a), v, rtol=0, atol=1e-15 * 4)
            assert np.allclose(dr.pow_W(v, a) + dr.pow_W(-v, -a), np.eye(3), rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", sorted(dr.PROBLEMS))
def test_generator_returns_an_optimal_pair_under_the_condition_cap(name):
    p = dr.PROBLEMS[name]()
    A, x, y, s, cone = p["A"], p["x"], p["y"], p["s"], p["cone"]
    Pd = ar.full_P(p["P"])
    assert np.abs(A @ x + s - p["b"]).max() < 1e-12
    assert np.abs(Pd @ x + A.T @ y + p["c"]).max() < 1e-12
    assert abs(s @ y) < 1e-10 * max(1.0, np.linalg.norm(s) * np.linalg.norm(y))
    assert np.allclose(dr.project(s - y, cone), s, atol=1e-12)
    W = dr.cone_W(s - y, cone)
    assert np.abs(W - W.T).max() <= 1e-14
    cond = np.linalg.cond(ar.jacobian(A, p["P"], W))
    print("%s: m = %d, n = %d, cond2(J) = %.1f" % (name, A.shape[0], A.shape[1], cond))
    assert cond <= dr.COND_CAP
    o_box, o_q, o_s, o_p, m = dr.offsets(cone)
    v = s - y
    if name == "box_qp":
        t, U, L = dr.box_sets(v[o_box:o_q], np.array(cone["bl"]), np.array(cone["bu"]))
        bl, bu = np.array(cone["bl"]), np.array(cone["bu"])
        assert abs(t - 1.0) < 1e-12 and not A[o_box].toarray().any()          # t fixed to 1 through a zero row
        assert U.sum() == 3 and L.sum() == 3 and (~(U | L)).sum() == 4          # active on each side, some free
        assert np.isinf(bu).any() and np.isinf(bl).any() and (bl[L] == 0).any()  # an infinite bound, an active zero bound
    if name == "pow":
        seen = {(a >= 0, dr.pow_case_of(v[o_p + 3 * i:o_p + 3 * i + 3], a)) for i, a in enumerate(cone["p"])}
        assert seen == {(sg, c) for sg in (True, False) for c in ("in", "polar", "bd")}
    if name == "mixed":
        assert cone["z"] and cone["l"] and cone["bu"] and cone["q"] and cone["s"] and cone["p"]


@pytest.mark.parametrize("name", sorted(dr.PROBLEMS))
def test_reference_matches_central_differences(name):
    p = dr.PROBLEMS[name]()
    rec = GOLD[name]
    bound = 10 * max(v for k, v in rec.items() if k != "cond")
    solve = oracle_solve(p["cone"])
    sol = solve(ar.data_of(p))
    print("%s: the oracle recovers the built x to %.1e" % (name, np.abs(sol["x"] - p["x"]).max()))
    assert np.abs(sol["x"] - p["x"]).max() < 1e-6
    for which in ("bcA", "P"):
        rel, cond = dr.fd_compare(p, solve, dr.FD_SEEDS[which], which, h=GOLD["h"])
        print("%s %s: relative difference %.3e (recorded %.3e), cond(J) %.3e" % (name, which, rel, rec[which], cond))
        assert cond <= dr.COND_CAP
        assert rel <= bound, (name, which, rel, bound)
    rel = dr.forward_fd_compare(p, solve, GOLD["fwd_seed"], h=GOLD["h"])
    print("%s forward: relative difference %.3e (recorded %.3e)" % (name, rel, rec["fwd"]))
    assert rel <= bound, (name, "fwd", rel, bound)
