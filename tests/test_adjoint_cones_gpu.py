"""Derivatives of a solve with a box cone and power cones on the device (csrc/dproj_box_pow.hpp through SCS.adjoint / derivative, their
device twins and scs.autograd) against the dense numpy reference of tests/dproj_cones_ref.py at the GPU solve's own (x, y, s).

The error bound is the one of tests/test_adjoint_gpu.py: LSQR stops at a relative residual `tol`, so the relative l2 error of its answer
is at most cond2(J) tol; a factor 100 covers the norm equivalences between lambda and the gradients formed from it.  The problems keep
cond2(J) <= 1e4 (asserted) and the tests assert 100 cond tol with tol = 1e-12.  (With `normalize` LSQR runs on the equilibrated system,
whose condition number is another one: the bound is exact without it.)"""
import gc

import numpy as np
import pytest
from scipy import sparse

import torch

import adjoint_ref as ar
import dproj_cones_ref as dr

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

IND, DEN = scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE
STG = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=False, max_iters=100000)
TOL = 1e-12
NAMES = sorted(dr.PROBLEMS)
_problems, _solved = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _finish_cached_solvers():
    """the solvers this module solves once and shares are finished with it (the block pool's account is an invariant of
    tests/test_pool_lifecycle_gpu.py)"""
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
        _problems[name] = dr.PROBLEMS[name]()
    return _problems[name]


def solved(name, normalize=True, solver=IND):
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


def directions(p, seed=9):
    """db, dc and value arrays dA, dP with their dense images"""
    rng = np.random.default_rng(seed)
    A, P = p["A"], p["P"]
    m, n = A.shape
    dAv, dPv = rng.standard_normal(A.nnz), rng.standard_normal(P.nnz)
    dA = sparse.csc_matrix((dAv, A.indices, A.indptr), shape=A.shape).toarray()
    dPu = sparse.csc_matrix((dPv, P.indices, P.indptr), shape=P.shape).toarray()
    return rng.standard_normal(m), rng.standard_normal(n), dAv, dPv, dA, dPu + dPu.T - np.diag(np.diag(dPu))


def rel(got, ref):
    return np.linalg.norm(got - ref) / np.linalg.norm(ref)


def reference(p, sol, gx, gy, gs):
    ref = dr.adjoint(p["A"], p["P"], p["cone"], sol["x"], sol["y"], sol["s"], gx, gy, gs)
    cond = float(np.linalg.cond(ref["J"]))
    assert cond <= dr.COND_CAP, cond  # (a condition on the test's inputs)
    return {"db": ref["db"], "dc": ref["dc"], "dA": ar.stored_values(ref["dA"], p["A"]), "dP": ar.stored_values(ref["dP"], p["P"])}, cond


def same_bits(a, b):
    assert set(a) == set(b)
    for key in a:
        if key == "info":
            assert {k: v for k, v in a[key].items() if k != "time_ms"} == {k: v for k, v in b[key].items() if k != "time_ms"}
        else:
            ga = a[key].cpu().numpy() if isinstance(a[key], torch.Tensor) else a[key]
            gb = b[key].cpu().numpy() if isinstance(b[key], torch.Tensor) else b[key]
            assert np.array_equal(ga, gb), key


# ---- 1. adjoint and forward against the reference, their duality ------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [IND, DEN], ids=["indirect", "dense"])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("name", NAMES)
def test_adjoint_and_derivative_match_the_reference_and_are_dual(name, normalize, solver):
    sv, sol, p = solved(name, normalize, solver)
    gx, gy, gs = cotangents(p)
    ad = sv.adjoint(dx=gx, dy=gy, ds=gs, want=("b", "c", "A", "P"), tol=TOL)
    ref, cond = reference(p, sol, gx, gy, gs)
    bound = 100 * cond * TOL
    for key in ref:
        err = rel(ad[key], ref[key])
        print("%s normalize=%s %s %s: relative error %.3e, bound %.3e, cond(J) %.3e, LSQR %s" % (name, normalize, solver.name, key, err, bound,
                                                                                                 cond, ad["info"]))
        assert ad[key].shape == ref[key].shape
        assert err <= bound, (name, normalize, key, err, bound, ad["info"])
    assert ad["info"]["stop"] in (1, 2, 3) and ad["info"]["iters"] >= 1
    db, dc, dAv, dPv, dA, dP = directions(p)
    g = np.concatenate([gx, gy, gs])
    for with_matrices in (False, True):
        kw = dict(dA=dAv, dP=dPv) if with_matrices else {}
        fw = sv.derivative(db=db, dc=dc, tol=TOL, **kw)
        fref = dr.derivative(p["A"], p["P"], p["cone"], sol["x"], sol["y"], sol["s"], db, dc, **(dict(dA=dA, dP=dP) if with_matrices else {}))
        for key in ("dx", "dy", "ds"):
            err = rel(fw[key], fref[key])
            print("%s normalize=%s %s forward%s %s: relative error %.3e, bound %.3e" % (name, normalize, solver.name,
                                                                                       " (dA, dP)" if with_matrices else "", key, err, bound))
            assert err <= bound, (key, with_matrices, err, bound)
        # <adjoint(g), d> = <g, derivative(d)>: each side is an inner product of an exact vector with one whose relative error is <= bound
        lhs = gx @ fw["dx"] + gy @ fw["dy"] + gs @ fw["ds"]
        grads, dirs = [ad["db"], ad["dc"]], [db, dc]
        if with_matrices:
            grads += [ad["dA"], ad["dP"]]
            dirs += [dAv, dPv]
        rhs = sum(a @ b for a, b in zip(grads, dirs))
        d = np.concatenate([fw["dx"], fw["dy"], fw["ds"]])
        scale = np.linalg.norm(g) * np.linalg.norm(d) + np.linalg.norm(np.concatenate(grads)) * np.linalg.norm(np.concatenate(dirs))
        print("duality %s: lhs %.15e rhs %.15e, difference / scale %.3e" % (name, lhs, rhs, abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= bound * scale


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_two_calls_and_both_entries_give_the_same_bits(name):
    sv, sol, p = solved(name)
    gx, gy, gs = cotangents(p)
    want = ("b", "c", "A", "P")
    first = sv.adjoint(dx=gx, dy=gy, ds=gs, want=want)
    same_bits(first, sv.adjoint(dx=gx, dy=gy, ds=gs, want=want))
    same_bits(first, sv.adjoint_device(dx=dev(gx), dy=dev(gy), ds=dev(gs), want=want))
    db, dc, dAv, dPv, _, _ = directions(p)
    for kw, kwd in (({}, {}), (dict(dA=dAv, dP=dPv), dict(dA=dev(dAv), dP=dev(dPv)))):
        fw = sv.derivative(db=db, dc=dc, **kw)
        same_bits(fw, sv.derivative(db=db, dc=dc, **kw))
        same_bits(fw, sv.derivative_device(db=dev(db), dc=dev(dc), **kwd))


@pytest.mark.parametrize("name", NAMES)
def test_a_call_leaves_the_state_of_the_next_solve_alone(name):
    """a warm-started solve after differentiating equals the same solve on a twin that never differentiated, bit for bit: the box
    cone's preparation runs the projection on a copy and never touches the solve's warm-start scalar"""
    p = problem(name)
    gx, gy, gs = cotangents(p)
    stg = dict(STG, eps_abs=1e-7, eps_rel=1e-7)
    a, twin = (scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **stg) for _ in range(2))
    sa, st = a.solve(warm_start=False), twin.solve(warm_start=False)
    assert sa["info"]["status"] == "solved" and np.array_equal(sa["x"], st["x"])
    assert a.adjoint(dx=gx, dy=gy, ds=gs, want=("b", "c", "A", "P"))["info"]["iters"] >= 1
    a.derivative(db=gy, dc=gx)
    b2 = p["b"] * 1.01  # (the cone is a cone: still feasible, t of the box QP becomes 1.01)
    for sv in (a, twin):
        sv.update_device(b=dev(b2))
    ra, rt = a.solve_device(warm_start=True), twin.solve_device(warm_start=True)
    for key in ("x", "y", "s"):
        assert torch.equal(ra[key], rt[key]), key
    assert ra["info"]["iter"] == rt["info"]["iter"] and ra["info"]["cg_iters"] == rt["info"]["cg_iters"]


# ---- 3. the torch layer -----------------------------------------------------------------------------------------------------------------
def test_autograd_solve_on_the_box_qp():
    import scs.autograd
    p = problem("box_qp")
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    sv.autograd_tol = TOL
    b = dev(p["b"]).requires_grad_(True)
    c = dev(p["c"]).requires_grad_(True)
    x, y, s = scs.autograd.solve(sv, b, c)
    gx, gy, gs = cotangents(p)
    (x @ dev(gx) + y @ dev(gy) + s @ dev(gs)).backward()
    sol = {"x": x.detach().cpu().numpy(), "y": y.detach().cpu().numpy(), "s": s.detach().cpu().numpy()}
    ref, cond = reference(p, sol, gx, gy, gs)
    bound = 100 * cond * TOL
    assert rel(b.grad.cpu().numpy(), ref["db"]) <= bound and rel(c.grad.cpu().numpy(), ref["dc"]) <= bound


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def feasible_qp(K, seed):
    """a strictly convex QP with a feasible point: P = I, s0 = Pi_K(random), b = A x0 + s0"""
    rng = np.random.default_rng(seed)
    m = (K.get("z", 0) + K.get("l", 0) + 3 * (K.get("ep", 0) + K.get("ed", 0)) + sum(k * k for k in K.get("cs", [])) +
         sum(k + 1 for k in K.get("ell1", [])))
    n = 3
    s0 = _scs_hip.proj_cone(rng.standard_normal(m), K, dual=False)
    A = sparse.csc_matrix(rng.standard_normal((m, n)))
    return {"P": sparse.identity(n, format="csc"), "A": A, "b": A @ rng.standard_normal(n) + s0, "c": rng.standard_normal(n)}


@pytest.mark.parametrize("K,pattern", [({"l": 2, "ep": 1}, r"exponential \(ep\) cone"), ({"l": 2, "ed": 1}, r"dual exponential \(ed\) cone"),
                                       ({"l": 2, "cs": [2]}, r"complex PSD \(cs\) cone.*z, l, q and s cones only"),
                                       ({"l": 2, "ell1": [3]}, r"ell1 cone")], ids=["ep", "ed", "cs", "ell1"])
def test_cones_without_a_derivative_are_refused_by_name_and_the_workspace_still_solves(K, pattern):
    data = feasible_qp(K, 5)
    sv = scs.SCS(data, K, linear_solver=IND, **dict(STG, eps_abs=1e-7, eps_rel=1e-7))
    first = sv.solve(warm_start=False)
    assert first["info"]["status"] == "solved", first["info"]
    for call in (sv.adjoint, sv.derivative):
        with pytest.raises(ValueError, match=pattern):
            call()
    again = sv.solve(warm_start=False)
    assert again["info"]["status"] == "solved"
    assert np.abs(again["x"] - first["x"]).max() <= 1e-4 * max(1.0, np.abs(first["x"]).max())
