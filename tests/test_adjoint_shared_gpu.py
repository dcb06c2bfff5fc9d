"""The matrix gradients of solve_many's members summed over the batch (`reduce="sum"`: include/scs_hip.h scs_hip_adjoint_shared, and the
layer scs.autograd.solve_many(solver, B, C, A=, P=)), through the solver.

What is compared with equal bits: db, dc and every member's LSQR figures against the call without the matrix gradients; host against
device; explicit clones against solve_many's members; the layer against the direct call.  The sums themselves are held to the bound of
tests/test_grad_shared_gpu.py — (2K + 2) 2^-52 sum|products| per entry against math.fsum of the products, built from the X, Y, db, dc
the calls return: the per-member formula is tied to finite differences by tests/test_adjoint_gpu.py and its siblings, and the sum is
linear, so nothing else needs a tolerance.

Problems: the generators of the adjoint tests — an LP, a QP with P, one with SOC and PSD blocks, one with box and power cones (n <= 40) —
with K = 5 perturbed (b, c) each.  Every member below ends "solved" at STG."""
import gc

import numpy as np
import pytest

import torch

import adjoint_ref as ar
import adjoint_psd_ref as apr
import dproj_cones_ref as dr
from test_grad_shared_gpu import reference

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

IND = scs.LinearSolver.HIP_INDIRECT
STG = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=False, max_iters=100000)
TOL = 1e-12
K = 5
ALL = ("b", "c", "A", "P")
FIGURES = ("iters", "stop", "residual", "normal_residual")


def problem_soc_psd():  # 1 zero row + 2 tight rows + a boundary SOC (1) + 3 + 3 directions of the PSD blocks = 10 <= n
    return apr.gen_problem(41, n=14, z=1, l=4, tight_l=2, s=(3, 5), ranks=(1, 3), q=(3, 4), q_case=("bd", "in"), with_P=True)


PROBLEMS = {"lp": ar.problem_lp, "qp": ar.problem_qp, "soc_psd": problem_soc_psd, "box_pow": dr.PROBLEMS["mixed"]}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _finish_cached_solvers():
    """the solvers this module solves once and shares are finished with it (tests/test_pool_lifecycle_gpu.py counts the pool's blocks)"""
    yield
    _cache.clear()
    gc.collect()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def host(t):
    return t.detach().cpu().numpy()


def batch_data(p, count=K, seed=3):
    """`count` (b, c) near the problem's own: the zero rows' b as it is"""
    rng = np.random.default_rng(seed)
    m, n = p["A"].shape
    z = p["cone"].get("z", 0)
    B = p["b"][None, :] + 0.01 * rng.standard_normal((count, m)) * np.r_[np.zeros(z), np.ones(m - z)]
    C = p["c"][None, :] + 0.01 * rng.standard_normal((count, n))
    G = (rng.standard_normal((count, n)), rng.standard_normal((count, m)), rng.standard_normal((count, m)))
    return B, C, G


def many_solved(name, count=K):
    """(solver, problem, the device solutions of its `count` members, cotangents): solved once per module"""
    key = (name, count)
    if key not in _cache:
        p = PROBLEMS[name]()
        B, C, G = batch_data(p, count)
        sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
        out = sv.solve_many_device(b=dev(B), c=dev(C))
        assert all(i["status"] == "solved" for i in out["info"]), (name, [i["status"] for i in out["info"]])
        _cache[key] = (sv, p, out, G)
    return _cache[key]


def within_bound(p, X, Y, DB, DC, dA, dP):
    (ref_a, bound_a), p_side = reference(p["A"], p["P"], X, Y, DB, DC)
    if dA is not None:
        err = np.abs(dA - ref_a)
        assert dA.shape == ref_a.shape and (err <= bound_a).all(), float((err / np.maximum(bound_a, 1e-300)).max())
        assert np.abs(dA).max() > 0
    if dP is not None:
        ref_p, bound_p = p_side
        err = np.abs(dP - ref_p)
        assert dP.shape == ref_p.shape and (err <= bound_p).all(), float((err / np.maximum(bound_p, 1e-300)).max())
        assert np.abs(dP).max() > 0


def same_figures(a, b):
    for k in FIGURES:
        assert a[k] == b[k], (k, a[k], b[k])


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_summed_gradients_of_solve_many(name):
    sv, p, out, (GX, GY, GS) = many_solved(name)
    want = ALL if p["P"] is not None else ("b", "c", "A")
    plain = sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=("b", "c"), tol=TOL)
    got = sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=want, tol=TOL, reduce="sum")
    assert list(got) == ["d" + k for k in want] + ["info"]
    # the members are differentiated as ever: db, dc and the LSQR figures, bit for bit
    assert torch.equal(got["db"], plain["db"]) and torch.equal(got["dc"], plain["dc"])
    assert all(i["iters"] > 0 for i in got["info"])
    for a, b in zip(got["info"], plain["info"]):
        same_figures(a, b)
    # the sums: one vector each, within the bound of the exact sum of the members' products
    assert got["dA"].shape == (p["A"].nnz,)
    dP = None
    if p["P"] is not None:
        assert got["dP"].shape == (p["P"].nnz,)
        dP = host(got["dP"])
    within_bound(p, host(out["x"]), host(out["y"]), host(got["db"]), host(got["dc"]), host(got["dA"]), dP)
    # two calls on the same state: the same bits
    again = sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=want, tol=TOL, reduce="sum")
    for k in want:
        assert torch.equal(again["d" + k], got["d" + k]), k
    # the host functions give the bits of the device ones
    res, grads = sv.adjoint_many(GX, GY, GS, want=want, tol=TOL, reduce="sum")
    assert len(res) == K and sorted(grads) == sorted("d" + k for k in want if k in "AP")
    for i, r in enumerate(res):
        assert sorted(r) == ["db", "dc", "info"]
        assert np.array_equal(r["db"], host(got["db"][i])) and np.array_equal(r["dc"], host(got["dc"][i]))
        same_figures(r["info"], got["info"][i])
    for k in grads:
        assert np.array_equal(grads[k], host(got[k])), k


def test_explicit_clones_and_a_alone():
    sv, p, out, (GX, GY, GS) = many_solved("qp")
    got = sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=ALL, tol=TOL, reduce="sum")
    # the same K problems on clones the caller made: adjoint_batch(reduce="sum") does the same
    B, C, _ = batch_data(p)
    base = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    members = [base] + [base.clone() for _ in range(K - 1)]
    for i, mv in enumerate(members):
        mv.update(b=B[i], c=C[i])
    assert all(r["info"]["status"] == "solved" for r in scs.solve_batch(members))
    res, grads = scs.adjoint_batch(members, GX, GY, GS, want=ALL, tol=TOL, reduce="sum")
    for i, r in enumerate(res):
        assert np.array_equal(r["db"], host(got["db"][i])) and np.array_equal(r["dc"], host(got["dc"][i]))
    assert np.array_equal(grads["dA"], host(got["dA"])) and np.array_equal(grads["dP"], host(got["dP"]))
    res_d, grads_d = scs.adjoint_batch_device(members, list(dev(GX)), list(dev(GY)), list(dev(GS)), want=("c", "P"), tol=TOL, reduce="sum")
    assert [sorted(r) for r in res_d] == [["dc", "info"]] * K and list(grads_d) == ["dP"]
    assert torch.equal(grads_d["dP"], got["dP"])
    # A alone: no db, dc come back, the sum is the same
    only = sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=("A",), tol=TOL, reduce="sum")
    assert list(only) == ["dA", "info"] and torch.equal(only["dA"], got["dA"])
    res, grads = sv.adjoint_many(GX, GY, GS, want=("A",), tol=TOL, reduce="sum")
    assert [list(r) for r in res] == [["info"]] * K and np.array_equal(grads["dA"], host(got["dA"]))


def test_one_member():
    sv, p, out, (GX, GY, GS) = many_solved("qp", count=1)
    got = sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=ALL, tol=TOL, reduce="sum")
    solo = sv.adjoint_device(dx=dev(GX[0]), dy=dev(GY[0]), ds=dev(GS[0]), want=ALL, tol=TOL)
    assert torch.equal(got["db"][0], solo["db"]) and torch.equal(got["dc"][0], solo["dc"])
    within_bound(p, host(out["x"]), host(out["y"]), host(got["db"]), host(got["dc"]), host(got["dA"]), host(got["dP"]))


def test_refusals_leave_the_solvers_usable():
    p = PROBLEMS["qp"]()
    B, C, (GX, GY, GS) = batch_data(p, 3)
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    other = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)

    def still_fine():
        out = sv.solve_many_device(b=dev(B), c=dev(C))
        assert all(i["status"] == "solved" for i in out["info"])
        assert other.solve(warm_start=False)["info"]["status"] == "solved"
        got = sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=ALL, tol=TOL, reduce="sum")
        within_bound(p, host(out["x"]), host(out["y"]), host(got["db"]), host(got["dc"]), host(got["dA"]), host(got["dP"]))

    # no solve yet: the member is named
    with pytest.raises(ValueError, match=r"member 0.*no solve yet"):
        sv.adjoint_many(want=("A",), reduce="sum")
    still_fine()
    # members that do not share one matrix: two separately built solvers
    with pytest.raises(ValueError, match=r"member 1.*does not share the matrix set"):
        scs.adjoint_batch([sv, other], GX[:2], GY[:2], GS[:2], want=("A",), tol=TOL, reduce="sum")
    with pytest.raises(ValueError, match=r"member 1.*does not share the matrix set"):
        scs.adjoint_batch_device([sv, other], list(dev(GX[:2])), want=("b", "P"), tol=TOL, reduce="sum")
    still_fine()
    # reduce="sum" without a matrix in `want`; another value
    with pytest.raises(ValueError, match="want must hold 'A' or 'P'"):
        sv.adjoint_many_device(dev(GX), want=("b", "c"), reduce="sum")
    with pytest.raises(ValueError, match="reduce must be None or 'sum'"):
        sv.adjoint_many_device(dev(GX), want=("A",), reduce="mean")
    # stale after an update: the member is named
    sv.update(b=B[0].copy())
    with pytest.raises(ValueError, match=r"member 0.*stale"):
        sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=ALL, tol=TOL, reduce="sum")
    still_fine()
    # dP for a solver without P: before the library (the binding knows the pattern), and by the library's own ladder
    lp = PROBLEMS["lp"]()
    Bl, Cl, (GXl, _, _) = batch_data(lp, 2)
    noP = scs.SCS(ar.data_of(lp), lp["cone"], linear_solver=IND, **STG)
    assert all(i["status"] == "solved" for i in noP.solve_many_device(b=dev(Bl), c=dev(Cl))["info"])
    with pytest.raises(ValueError, match="dP wanted, but the solver was created without P"):
        noP.adjoint_many_device(dev(GXl), want=("A", "P"), tol=TOL, reduce="sum")
    raw = [noP._solver] + noP._solver._many
    with _scs_hip._locked(raw) as works:
        dummy = np.zeros(4)
        rc = _scs_hip._lib.scs_hip_adjoint_shared(works, None, None, None, None, None, None, dummy.ctypes.data, None, None, 2)
        err = _scs_hip.last_error()
        rc_none = _scs_hip._lib.scs_hip_adjoint_shared(works, None, None, None, None, None, None, None, None, None, 2)
        err_none = _scs_hip.last_error()
    assert rc == -1 and "member 0" in err and "dPx for a workspace created without P" in err
    assert rc_none == -1 and "both NULL" in err_none
    out = noP.solve_many_device(b=dev(Bl), c=dev(Cl))
    assert all(i["status"] == "solved" for i in out["info"])
    got = noP.adjoint_many_device(dev(GXl), want=("b", "c", "A"), tol=TOL, reduce="sum")
    within_bound(lp, host(out["x"]), host(out["y"]), host(got["db"]), host(got["dc"]), host(got["dA"]), None)


def test_the_layer_with_shared_matrices():
    import scs.autograd
    p = PROBLEMS["qp"]()
    m, n = p["A"].shape
    B0, C0, (GX, GY, GS) = batch_data(p)
    GX, GY, GS = dev(GX), dev(GY), dev(GS)
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    sv.autograd_tol = 1e-11
    B, C, Ax, Px = (dev(v).requires_grad_(True) for v in (B0, C0, p["A"].data, p["P"].data))
    X, Y, S = scs.autograd.solve_many(sv, B, C, A=Ax, P=Px)
    assert X.shape == (K, n) and all(i["status"] == "solved" for i in sv.autograd_info)
    ((X * GX).sum() + (Y * GY).sum() + (S * GS).sum()).backward()
    direct = sv.adjoint_many_device(GX, GY, GS, want=ALL, tol=1e-11, reduce="sum")
    assert Ax.grad.shape == (p["A"].nnz,) and Px.grad.shape == (p["P"].nnz,)
    assert torch.equal(Ax.grad, direct["dA"]) and torch.equal(Px.grad, direct["dP"])
    assert torch.equal(B.grad, direct["db"]) and torch.equal(C.grad, direct["dc"])
    assert len(sv.autograd_adjoint_info) == K
    # the gradients of B, C: the bits of the layer without matrices on the same data
    tw = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    tw.autograd_tol = 1e-11
    Bt, Ct = dev(B0).requires_grad_(True), dev(C0).requires_grad_(True)
    Xt, Yt, St = scs.autograd.solve_many(tw, Bt, Ct)
    ((Xt * GX).sum() + (Yt * GY).sum() + (St * GS).sum()).backward()
    assert torch.equal(Xt, X) and torch.equal(Bt.grad, B.grad) and torch.equal(Ct.grad, C.grad)
    # only the inputs that need a gradient are asked for: A alone
    A_only = dev(p["A"].data).requires_grad_(True)
    X1, _, _ = scs.autograd.solve_many(sv, B.detach(), C.detach(), A=A_only)
    (X1 * GX).sum().backward()
    assert torch.equal(A_only.grad, sv.adjoint_many_device(GX, want=("A",), tol=1e-11, reduce="sum")["dA"])
    # an optimiser-style step on A: the second forward solves the new matrix
    A2 = p["A"].copy()
    A2.data = p["A"].data * (1.0 + 0.01 * np.random.default_rng(8).standard_normal(p["A"].nnz))
    X2, _, _ = scs.autograd.solve_many(sv, B.detach(), C.detach(), A=dev(A2.data).requires_grad_(True), P=Px.detach())
    assert all(i["status"] == "solved" for i in sv.autograd_info)
    new = scs.SCS(dict(ar.data_of(p), A=A2), p["cone"], linear_solver=IND, **STG).solve_many(b=B0, c=C0)
    for i, r in enumerate(new):
        assert r["info"]["status"] == "solved"
        assert np.abs(host(X2[i]) - r["x"]).max() <= 1e-4 * max(1.0, np.abs(r["x"]).max())  # (both ends stop at STG's eps: as the layer of one problem)
    # backward after a later solve: the existing error
    with pytest.raises(RuntimeError, match="solved again"):
        (X1 * GX).sum().backward()
    X2.sum().backward()
