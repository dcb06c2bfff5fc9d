"""The dense numpy reference of the derivatives of an SDP solve (tests/adjoint_psd_ref.py: svec / smat, the PSD block of W, J, lstsq)
against central differences — of the CPU oracle's solutions for the whole reference, of numpy's projection for psd_W alone.  No GPU.

The bound of the first is ten times the worst relative difference recorded for the problem in tests/golden/adjoint_psd_fd.json
(h = 1e-4, oracle at eps 1e-9): it covers step-size and solver noise, not formula errors — a wrong sqrt(2) or sign gives O(0.1)."""
import json
import os

import numpy as np
import pytest

import adjoint_ref as ar
import adjoint_psd_ref as pr
from oracle import scs_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "adjoint_psd_fd.json")))


def oracle_solve(cone):
    def solve(data):
        r = scs_oracle.solve(data, cone, indirect=False, eps_abs=GOLD["eps"], eps_rel=GOLD["eps"], verbose=False, max_iters=200000)
        assert r["info"]["status"] == "solved", r["info"]
        return r
    return solve


@pytest.mark.parametrize("name", ["qp_sdp", "lp_sdp"])
def test_reference_matches_central_differences(name):
    p = pr.PROBLEMS[name]()
    rec = GOLD[name]
    bound = 10 * max(v for k, v in rec.items() if k != "cond")
    sol = oracle_solve(p["cone"])(ar.data_of(p))
    print("%s: the oracle recovers the built x to %.1e" % (name, np.abs(sol["x"] - p["x"]).max()))
    assert np.abs(sol["x"] - p["x"]).max() < 1e-6
    for which in ("bcA", "P"):
        if which == "P" and p["P"] is None:
            continue
        rel, cond = pr.fd_compare(p, oracle_solve(p["cone"]), pr.FD_SEEDS[which], which, h=GOLD["h"])
        print("%s %s: relative difference %.3e (recorded %.3e), cond(J) %.3e" % (name, which, rel, rec[which], cond))
        assert cond <= 1e4
        assert rel <= bound, (name, which, rel, bound)


def test_generator_returns_an_optimal_pair():
    for fn in (pr.problem_qp_sdp, pr.problem_lp_sdp, pr.problem_mixed_sdp):
        p = fn()
        A, x, y, s = p["A"], p["x"], p["y"], p["s"]
        Pd = ar.full_P(p["P"]) if p["P"] is not None else np.zeros((x.size, x.size))
        assert np.abs(A @ x + s - p["b"]).max() < 1e-12
        assert np.abs(Pd @ x + A.T @ y + p["c"]).max() < 1e-12
        assert abs(s @ y) < 1e-10
        assert np.allclose(pr.project(s - y, p["cone"]), s, atol=1e-12)
        o = pr.split(p["cone"])[1]
        for order in p["cone"]["s"]:  # every block keeps the sign gap the bounds of the GPU tests rely on
            lam = np.linalg.eigvalsh(pr.smat((s - y)[o:o + pr.sd_size(order)], order))
            assert np.abs(lam).min() / (2 * np.abs(lam).max()) >= pr.GAP
            o += pr.sd_size(order)


def test_svec_and_smat_are_inverse_isometries():
    rng = np.random.default_rng(0)
    for p in (1, 2, 5):
        M = rng.standard_normal((p, p))
        M = M + M.T
        N = rng.standard_normal((p, p))
        N = N + N.T
        assert np.allclose(pr.smat(pr.svec(M), p), M, rtol=0, atol=1e-15)
        assert abs(pr.svec(M) @ pr.svec(N) - np.trace(M @ N)) < 1e-12


@pytest.mark.parametrize("p,rank", [(1, 1), (2, 1), (4, 2), (6, 1), (6, 6), (5, 0)])
def test_psd_W_is_symmetric_and_matches_central_differences_of_the_projection(p, rank):
    rng = np.random.default_rng(10 * p + rank)
    v = pr.psd_point(rng, p, rank)
    W = pr.psd_W(v, p)
    assert np.abs(W - W.T).max() <= 1e-14
    u0 = rng.standard_normal(v.size)
    assert np.abs(pr.psd_W_apply(v, u0, p) - W @ u0).max() <= 1e-14 * np.linalg.norm(u0)
    h = 1e-6  # the projection is smooth within the sign gap 0.5: the central difference errs by O(h^2) + O(eps / h) ~ 1e-10
    worst = 0.0
    for _ in range(3):
        u = rng.standard_normal(v.size)
        fd = (pr.psd_project(v + h * u, p) - pr.psd_project(v - h * u, p)) / (2 * h)
        worst = max(worst, np.abs(W @ u - fd).max() / np.linalg.norm(u))
    print("psd_W order %d rank %d: worst |W u - central difference| / |u| %.2e" % (p, rank, worst))
    assert worst <= 1e-8
    if rank == p:
        assert np.allclose(W, np.eye(v.size), atol=1e-13)
    if rank == 0:
        assert not W.any()
