"""Derivatives of a solve on the device (SCS.adjoint / derivative and their device twins, scs.autograd; csrc/dproj.hpp, lsqr.hpp, diff.hpp)
against the dense numpy reference of tests/adjoint_ref.py, evaluated at the GPU solve's own (x, y, s).

Error bound of the comparisons with the reference: LSQR stops at a relative residual `tol`, so the relative l2 error of its answer is at
most cond2(J) tol; a factor 100 covers the norm equivalences between lambda and the gradients formed from it.  The tests require
cond2(J) <= 1e4 of their inputs and assert 100 cond tol with tol = 1e-12.  (With `normalize` LSQR runs on the equilibrated system, whose
condition number is another one: the bound is exact without it.)"""
import gc
import json
import os

import numpy as np
import pytest
from scipy import sparse

import torch

import adjoint_ref as ar
import problem_gen as pg

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "adjoint_fd.json")))
IND, DEN = scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE
STG = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=False, max_iters=100000)
TOL = 1e-12
PROBLEMS = {"lp3": ar.problem_lp3, "qp_soc12": ar.problem_qp_soc, "big300": ar.problem_big}
_problems, _solved = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _finish_cached_solvers():
    """the solvers this module solves once and shares are finished with it: no device block of theirs outlives the module (the block
    pool's account is an invariant of tests/test_pool_lifecycle_gpu.py)"""
    def in_use():
        st = _scs_hip.pool_stats()
        return st["live_bytes"] - st["held_bytes"]
    before = in_use()
    yield
    _solved.clear()
    gc.collect()
    assert in_use() <= before, (in_use(), before)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def problem(name):
    if name not in _problems:
        _problems[name] = PROBLEMS[name]()
    return _problems[name]


def solved(name, normalize=True, solver=IND):
    """(solver, its solution, the reference's inputs), solved once per session; the tests only read them"""
    key = (name, normalize, solver)
    if key not in _solved:
        p = problem(name)
        sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=solver, normalize=normalize, **STG)
        sol = sv.solve(warm_start=False)
        assert sol["info"]["status"] == "solved", sol["info"]
        assert np.abs(sol["x"] - p["x"]).max() < 1e-5, name  # the generator's pair: every row and cone is in the case it was built in
        _solved[key] = (sv, sol, p)
    return _solved[key]


def cotangents(p, seed=5):
    rng = np.random.default_rng(seed)
    m, n = p["A"].shape
    return rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)


def rel(got, ref):
    return np.linalg.norm(got - ref) / np.linalg.norm(ref)


# ---- 1. W applied to a vector ------------------------------------------------------------------------------------------------
SOC_SIZES = (1, 2, 3, 9, 10, 18, 34, 66, 4100)  # every lane-group width (8, 16, 32, 64), the loop past 64 lanes, the block kernel


def dproj_vector(sizes, seed=3):
    """z = 3, l = 70 and every size in the cases inside / polar / boundary / t = 0"""
    rng = np.random.default_rng(seed)
    parts = [rng.standard_normal(3), np.where(rng.random(70) < 0.5, -1.0, 1.0) * rng.uniform(0.1, 2.0, 70)]
    q = []
    for size in sizes:
        for case in ("in", "polar", "bd", "t0"):
            zz = rng.standard_normal(size - 1)
            r = np.linalg.norm(zz) if size > 1 else 1.0
            t = {"in": 1.5 * r, "polar": -1.5 * r, "bd": 0.3 * r, "t0": 0.0}[case]
            parts.append(np.concatenate([[t], zz]))
            q.append(size)
    v = np.concatenate(parts)
    return v, rng.standard_normal(v.size), {"z": 3, "l": 70, "q": q}


def test_dproj_matches_numpy():
    v, u, cone = dproj_vector(SOC_SIZES)
    wu, wmiu = _scs_hip.dproj_cone(v, u, cone)
    assert np.array_equal(wmiu, wu - u)
    worst = 0.0
    bounds = [0, 3, 73] + list(73 + np.cumsum(cone["q"]))
    for k in range(len(bounds) - 1):
        lo, hi = bounds[k], bounds[k + 1]
        sub = {"z": 3, "l": 0} if k == 0 else {"z": 0, "l": 70} if k == 1 else {"z": 0, "l": 0, "q": [hi - lo]}
        ref = ar.cone_W(v[lo:hi], sub) @ u[lo:hi]
        err = np.abs(wu[lo:hi] - ref).max() / max(np.linalg.norm(u[lo:hi]), 1e-300)
        worst = max(worst, err)
        assert err <= 1e-13, (k, hi - lo, err)
    print("dproj: worst entry error / block norm %.2e" % worst)
    # the three cases really occur at every size, and a q = 1 cone is a nonnegative row
    o = 73
    for size in SOC_SIZES:
        blocks = [(wu[o + i * size:o + (i + 1) * size], u[o + i * size:o + (i + 1) * size]) for i in range(4)]
        assert np.array_equal(blocks[0][0], blocks[0][1]) and not blocks[1][0].any()
        if size > 1:
            assert not np.array_equal(blocks[2][0], blocks[2][1]) and blocks[2][0].any() and blocks[3][0].any()
        o += 4 * size


def test_dproj_bits_do_not_depend_on_the_group_width():
    v, u, cone = dproj_vector(SOC_SIZES)
    full = _scs_hip.dproj_cone(v, u, cone)[0]
    for nsizes in (4, 5, 6, 8):  # largest small cone 9 / 10 / 18 / 66: lane groups of 8 / 16 / 32 / 64
        q = cone["q"][:4 * nsizes]
        ln = 73 + sum(q)
        part = _scs_hip.dproj_cone(v[:ln], u[:ln], {"z": 3, "l": 70, "q": q})[0]
        assert np.array_equal(part, full[:ln]), nsizes


# ---- 2. adjoint against the reference ----------------------------------------------------------------------------------------------
def reference(p, sol, gx, gy, gs):
    ref = ar.adjoint(p["A"], p["P"], p["cone"], sol["x"], sol["y"], sol["s"], gx, gy, gs)
    cond = float(np.linalg.cond(ref["J"]))
    assert cond <= 1e4, cond  # (a condition on the test's inputs)
    out = {"db": ref["db"], "dc": ref["dc"], "dA": ar.stored_values(ref["dA"], p["A"])}
    if p["P"] is not None:
        out["dP"] = ar.stored_values(ref["dP"], p["P"])
    return out, cond, ref


@pytest.mark.parametrize("solver", [IND, DEN], ids=["indirect", "dense"])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("name", ["lp3", "qp_soc12", "big300"])
def test_adjoint_matches_the_reference(name, normalize, solver):
    sv, sol, p = solved(name, normalize, solver)
    gx, gy, gs = cotangents(p)
    want = ("b", "c", "A") + (("P",) if p["P"] is not None else ())
    got = sv.adjoint(dx=gx, dy=gy, ds=gs, want=want, tol=TOL)
    ref, cond, _ = reference(p, sol, gx, gy, gs)
    bound = 100 * cond * TOL
    for key in ref:
        err = rel(got[key], ref[key])
        print("%s normalize=%s %s %s: relative error %.3e, bound %.3e, cond(J) %.3e, LSQR %s" % (name, normalize, solver.name, key, err, bound,
                                                                                                 cond, got["info"]))
        assert got[key].shape == ref[key].shape
        assert err <= bound, (name, normalize, key, err, bound, got["info"])
    assert got["info"]["stop"] in (1, 2, 3) and got["info"]["iters"] >= 1


def test_missing_cotangents_count_as_zero_and_outputs_can_be_skipped():
    sv, sol, p = solved("qp_soc12")
    gx, gy, gs = cotangents(p)
    m, n = p["A"].shape
    a = sv.adjoint(dx=gx, want=("c",), tol=TOL)
    b = sv.adjoint(dx=gx, dy=np.zeros(m), ds=np.zeros(m), want=("b", "c", "A", "P"), tol=TOL)
    assert set(a) == {"dc", "info"} and np.array_equal(a["dc"], b["dc"])
    zero = sv.adjoint(want=("b", "c"))
    assert not zero["db"].any() and not zero["dc"].any() and zero["info"]["stop"] == 1


# ---- 3. forward mode and its duality with the adjoint -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp_soc12", "big300"])
def test_forward_and_adjoint_are_dual(name):
    sv, sol, p = solved(name)
    gx, gy, gs = cotangents(p)
    rng = np.random.default_rng(9)
    m, n = p["A"].shape
    db, dc = rng.standard_normal(m), rng.standard_normal(n)
    fw = sv.derivative(db=db, dc=dc, tol=TOL)
    ad = sv.adjoint(dx=gx, dy=gy, ds=gs, tol=TOL)
    ref, cond, _ = reference(p, sol, gx, gy, gs)
    fref = ar.derivative(p["A"], p["P"], p["cone"], sol["x"], sol["y"], sol["s"], db, dc)
    bound = 100 * cond * TOL
    for key in ("dx", "dy", "ds"):
        assert rel(fw[key], fref[key]) <= bound, (key, rel(fw[key], fref[key]), bound)
    lhs = gx @ fw["dx"] + gy @ fw["dy"] + gs @ fw["ds"]
    rhs = ad["db"] @ db + ad["dc"] @ dc
    # each side is an inner product of an exact vector with one whose relative error is at most `bound`
    g, d = np.concatenate([gx, gy, gs]), np.concatenate([fw["dx"], fw["dy"], fw["ds"]])
    scale = np.linalg.norm(g) * np.linalg.norm(d) + np.linalg.norm(np.concatenate([ad["db"], ad["dc"]])) * np.linalg.norm(np.concatenate([db, dc]))
    print("duality %s: lhs %.15e rhs %.15e, difference / scale %.3e, bound %.3e" % (name, lhs, rhs, abs(lhs - rhs) / scale, bound))
    assert abs(lhs - rhs) <= bound * scale


# ---- 4. one end-to-end finite difference on the GPU solver ---------------------------------------------------------------------------
def test_finite_differences_of_the_gpu_solver():
    p = ar.problem_qp_soc()
    rec = GOLD["qp_soc"]
    bound = 10 * max(v for k, v in rec.items() if k != "cond")
    holder = {}

    def solve(data):
        sv = scs.SCS(data, p["cone"], linear_solver=IND, **STG)
        r = sv.solve(warm_start=False)
        assert r["info"]["status"] == "solved"
        holder["sv"] = sv
        return r

    def grad(gx, gy, gs):
        return holder["sv"].adjoint(dx=gx, dy=gy, ds=gs, want=("b", "c", "A", "P"), tol=TOL)

    for which in ("bcA", "P"):
        err, cond = ar.fd_compare(p, solve, ar.FD_SEEDS[which], which, h=GOLD["h"], grad=grad)
        print("finite differences %s: relative difference %.3e, bound %.3e (CPU reference recorded %.3e)" % (which, err, bound, rec[which]))
        assert err <= bound, (which, err, bound)


# ---- 5. bits ---------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    for key in a:
        if key == "info":
            assert {k: v for k, v in a[key].items() if k != "time_ms"} == {k: v for k, v in b[key].items() if k != "time_ms"}
        else:
            ga = a[key].cpu().numpy() if isinstance(a[key], torch.Tensor) else a[key]
            gb = b[key].cpu().numpy() if isinstance(b[key], torch.Tensor) else b[key]
            assert np.array_equal(ga, gb), key


@pytest.mark.parametrize("name", ["qp_soc12", "big300"])
def test_two_calls_and_both_entries_give_the_same_bits(name):
    sv, sol, p = solved(name)
    gx, gy, gs = cotangents(p)
    want = ("b", "c", "A", "P")
    first = sv.adjoint(dx=gx, dy=gy, ds=gs, want=want)
    same_bits(first, sv.adjoint(dx=gx, dy=gy, ds=gs, want=want))
    on_device = sv.adjoint_device(dx=dev(gx), dy=dev(gy), ds=dev(gs), want=want)
    assert all(isinstance(on_device[k], torch.Tensor) and on_device[k].is_cuda for k in ("db", "dc", "dA", "dP"))
    same_bits(first, on_device)
    rng = np.random.default_rng(2)
    db, dc = rng.standard_normal(p["b"].size), rng.standard_normal(p["c"].size)
    fw = sv.derivative(db=db, dc=dc)
    same_bits(fw, sv.derivative(db=db, dc=dc))
    same_bits(fw, sv.derivative_device(db=dev(db), dc=dev(dc)))


def test_a_call_leaves_the_state_of_the_next_solve_alone_and_clones_agree():
    p = problem("big300")
    gx, gy, gs = cotangents(p)
    stg = dict(STG, eps_abs=1e-7, eps_rel=1e-7)
    a, twin = (scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **stg) for _ in range(2))
    sa, st = a.solve(warm_start=False), twin.solve(warm_start=False)
    assert np.array_equal(sa["x"], st["x"])
    got = a.adjoint(dx=gx, dy=gy, ds=gs, want=("b", "c", "A", "P"))
    a.derivative(db=gy, dc=gx)
    b2 = p["b"] * 1.01
    for sv in (a, twin):
        sv.update_device(b=dev(b2))
    ra, rt = a.solve_device(warm_start=True), twin.solve_device(warm_start=True)
    for key in ("x", "y", "s"):
        assert torch.equal(ra[key], rt[key]), key
    assert ra["info"]["iter"] == rt["info"]["iter"] and ra["info"]["cg_iters"] == rt["info"]["cg_iters"]
    # a clone starts from the constructor's b, c: solved cold it holds the parent's first solution, and differentiates to its bits
    cl = a.clone()
    sc = cl.solve(warm_start=False)
    assert np.array_equal(sc["x"], sa["x"]) and np.array_equal(sc["y"], sa["y"]) and np.array_equal(sc["s"], sa["s"])
    same_bits(got, cl.adjoint(dx=gx, dy=gy, ds=gs, want=("b", "c", "A", "P")))


# ---- 6. column-sorted pass layout, split A' included ---------------------------------------------------------------------------------
def pass_problem():
    """20000 x 16400 (>= 16384 rows in each orientation), 6000 tight rows each pinned to a column of its own, P diagonally dominant:
    a regular, well-conditioned J (LSQR: ~150 iterations to 1e-12)"""
    rng = np.random.default_rng(71)
    m, n, tight = 20000, 16400, 6000
    v = np.concatenate([-rng.uniform(0.5, 1.5, tight), rng.uniform(0.5, 1.5, m - tight)])[rng.permutation(m)]
    rows = np.flatnonzero(v < 0)
    pin = sparse.csc_matrix((np.full(tight, 3.0), (rows, rng.choice(n, tight, replace=False))), shape=(m, n))
    A = (0.5 * pg.random_sparse(m, n, 4, rng) + pin).tocsc()
    A.sort_indices()
    s = np.maximum(v, 0)
    y = s - v
    x = rng.standard_normal(n)
    off = sparse.csc_matrix((0.1 * rng.standard_normal(50), (rng.integers(0, n, 50), rng.integers(0, n, 50))), shape=(n, n))
    P = sparse.csc_matrix(sparse.diags(1.0 + rng.random(n)) + off + off.T)
    return {"A": A, "P": P, "b": A @ x + s, "c": -(P @ x) - A.T @ y}, {"l": m}


@pytest.mark.parametrize("split", ["0", "1"])
def test_pass_layout_agrees_with_the_csr_stream_workspace(monkeypatch, split):
    data, K = pass_problem()
    stg = dict(STG, eps_abs=1e-8, eps_rel=1e-8, max_iters=5000)
    rng = np.random.default_rng(4)
    gx, gy, gs = rng.standard_normal(16400), rng.standard_normal(20000), rng.standard_normal(20000)
    plain = scs.SCS(data, K, linear_solver=IND, **stg)
    s0 = plain.solve(warm_start=False)
    assert "CSR-stream" in s0["info"]["lin_sys_solver"] and s0["info"]["status"] == "solved", s0["info"]
    monkeypatch.setenv("SCS_HIP_CS", "2")
    monkeypatch.setenv("SCS_HIP_CS_SPLIT", split)
    forced = scs.SCS(data, K, linear_solver=IND, **stg)
    s1 = forced.solve(warm_start=False)
    assert "column-sorted pass" in s1["info"]["lin_sys_solver"] and s1["info"]["status"] == "solved", s1["info"]
    want = ("b", "c", "A", "P")
    g0 = plain.adjoint(dx=gx, dy=gy, ds=gs, want=want, tol=TOL)
    g1 = forced.adjoint(dx=gx, dy=gy, ds=gs, want=want, tol=TOL)
    print("pass layout split=%s: LSQR %s / %s" % (split, g0["info"], g1["info"]))
    assert g0["info"]["stop"] in (1, 2) and g1["info"]["stop"] in (1, 2)
    for key in ("db", "dc", "dA", "dP"):
        err = rel(g1[key], g0[key])
        print("pass layout split=%s %s: relative difference %.3e" % (split, key, err))
        assert err <= 1e-10, (key, err)
    f0, f1 = plain.derivative(db=gy, dc=gx, tol=TOL), forced.derivative(db=gy, dc=gx, tol=TOL)
    for key in ("dx", "dy", "ds"):
        assert rel(f1[key], f0[key]) <= 1e-10, key


# ---- 7. a degenerate solution ----------------------------------------------------------------------------------------------------------
def test_degenerate_lp_gives_the_minimum_norm_least_squares_answer():
    """two identical tight rows: J is singular and the right-hand side inconsistent.  Without `normalize` the solver's coordinates are
    the caller's, so LSQR's answer is numpy's lstsq answer (with it, it is the minimum-norm answer of the equilibrated system)."""
    p = ar.problem_degenerate()
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, normalize=False, **STG)
    sol = sv.solve(warm_start=False)
    assert sol["info"]["status"] == "solved"
    i = p["cone"]["z"]
    assert sol["y"][i] > 1e-3 and sol["y"][i + 1] > 1e-3  # both copies of the row carry a multiplier: away from the kink
    gx, gy, gs = cotangents(p)
    ref = ar.adjoint(p["A"], None, p["cone"], sol["x"], sol["y"], sol["s"], gx, gy, gs)
    sing = np.linalg.svd(ref["J"], compute_uv=False)
    assert sing[-1] < 1e-12 * sing[0]
    got = sv.adjoint(dx=gx, dy=gy, ds=gs, want=("b", "c", "A"), tol=1e-10)
    print("degenerate LP: LSQR %s" % (got["info"],))
    assert got["info"]["stop"] == 2
    for key, r in (("db", ref["db"]), ("dc", ref["dc"]), ("dA", ar.stored_values(ref["dA"], p["A"]))):
        assert np.isfinite(got[key]).all()
        assert rel(got[key], r) <= 1e-6, (key, rel(got[key], r))


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def still_solves(sv, ref_x=None):
    """(a later cold solve starts from the scale the earlier one adapted: the same optimum, not the same bits)"""
    r = sv.solve(warm_start=False)
    assert r["info"]["status"] == "solved"
    if ref_x is not None:
        assert np.abs(r["x"] - ref_x).max() <= 1e-4 * max(1.0, np.abs(ref_x).max())
    return r


def test_refusals_leave_the_workspace_usable():
    p = problem("qp_soc12")
    m, n = p["A"].shape
    stg = dict(STG, eps_abs=1e-7, eps_rel=1e-7)
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **stg)
    for call in (sv.adjoint, sv.derivative):
        with pytest.raises(ValueError, match="no solve yet"):
            call()
    first = still_solves(sv)
    assert sv.adjoint(dx=np.ones(n))["info"]["stop"] in (1, 2)
    # stale after every kind of update; a new solve makes it fresh
    for update in (lambda: sv.update(b=p["b"].copy()), lambda: sv.update_device(c=dev(p["c"])),
                   lambda: sv.update_matrix(A=p["A"].data.copy()), lambda: sv.update_matrix_device(P=dev(p["P"].data))):
        update()
        for call in (sv.adjoint, sv.adjoint_device, sv.derivative, sv.derivative_device):
            with pytest.raises(ValueError, match="stale"):
                call()
        still_solves(sv, first["x"])
        assert sv.derivative(db=np.ones(m))["info"]["stop"] in (1, 2)
    # the last solve did not end solved
    bad = scs.SCS({"A": sparse.csc_matrix(np.array([[-1.0], [1.0]])), "b": np.array([-1.0, 0.0]), "c": np.array([1.0])}, {"l": 2},
                  linear_solver=IND, **stg)
    assert bad.solve(warm_start=False)["info"]["status"] == "infeasible"
    with pytest.raises(ValueError, match="did not end solved"):
        bad.adjoint()
    bad.update(b=np.array([1.0, 0.0]))  # x <= 1, x >= 0 ... feasible now
    still_solves(bad)
    assert bad.adjoint(dx=np.ones(1))["info"]["stop"] in (1, 2)
    # a cone without a derivative is named
    rng = np.random.default_rng(0)
    Ke = {"l": 2, "ep": 1}
    de, _, _ = pg.gen_feasible(Ke, 3, 2, 5, lambda z, K: _scs_hip.proj_cone(z, K, dual=True))
    ex = scs.SCS(de, Ke, linear_solver=IND, **stg)
    re = still_solves(ex)
    with pytest.raises(ValueError, match=r"exponential \(ep\) cone"):
        ex.adjoint()
    still_solves(ex, re["x"])
    # dP for a solver without P (Python) and for a P whose columns are not sorted (the library, as update_matrix)
    lp = solved("lp3")[0]
    with pytest.raises(ValueError, match="created without P"):
        lp.adjoint(want=("P",))
    A = sparse.csc_matrix(np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]]))
    raw = _scs_hip.SCS((4, 2), A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), np.array([2.0, 1.0, 0.5]),
                       np.array([0, 1, 0], dtype=np.int32), np.array([0, 1, 3], dtype=np.int32), np.ones(4), np.array([-1.0, 1.0]), {"l": 4},
                       eps_abs=1e-7, eps_rel=1e-7, verbose=False)
    r0 = raw.solve(warm_start=False)
    assert r0["info"]["status"] == "solved"
    with pytest.raises(ValueError, match="ascend"):
        raw.adjoint(want=("b", "P"))
    assert raw.adjoint(want=("b", "c", "A"), dx=np.ones(2))["info"]["stop"] in (1, 2)
    assert np.abs(raw.solve(warm_start=False)["x"] - r0["x"]).max() <= 1e-4
    # a tensor that is not on the workspace's GPU never reaches the library
    with pytest.raises(ValueError, match="must live on the workspace's GPU"):
        sv.adjoint_device(dx=torch.zeros(n, dtype=torch.float64))


# ---- 9. the torch layer ------------------------------------------------------------------------------------------------------------------
def test_autograd_solve():
    import scs.autograd
    p = problem("qp_soc12")
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    sv.autograd_tol = 1e-11
    b = dev(p["b"]).requires_grad_(True)
    c = dev(p["c"]).requires_grad_(True)
    x, y, s = scs.autograd.solve(sv, b, c)
    cold_iters = sv.autograd_info["iter"]
    gx, gy, gs = (dev(g) for g in cotangents(p))
    (x @ gx + y @ gy + s @ gs).backward()
    direct = sv.adjoint_device(dx=gx, dy=gy, ds=gs, tol=1e-11)
    assert torch.equal(b.grad, direct["db"]) and torch.equal(c.grad, direct["dc"])
    ref, cond, _ = reference(p, {"x": x.detach().cpu().numpy(), "y": y.detach().cpu().numpy(), "s": s.detach().cpu().numpy()},
                             *(g.cpu().numpy() for g in (gx, gy, gs)))
    assert rel(b.grad.cpu().numpy(), ref["db"]) <= 100 * cond * 1e-11
    # a second forward after b changed starts from the resident solution
    b2 = (b.detach() * 1.001).requires_grad_(True)
    x2, _, _ = scs.autograd.solve(sv, b2, c)
    assert sv.autograd_info["status"] == "solved" and sv.autograd_info["iter"] < cold_iters, (sv.autograd_info["iter"], cold_iters)
    with pytest.raises(RuntimeError, match="solved again"):
        (x @ gx).backward()  # (the first graph's solution is gone)
    x2.sum().backward()
    assert b2.grad is not None and torch.isfinite(b2.grad).all()
