"""Forward derivatives with respect to the stored values of A and P (include/scs_hip.h: scs_hip_derivative_full ...; csrc/perturb.hpp):
the perturbation products on their own, `derivative(db, dc, dA=, dP=)` against the dense numpy reference
(tests/derivative_matrix_ref.py), its duality with the adjoint's dL/dA and dL/dP, bits, a finite difference of the GPU solver through
`update_matrix`, the pass layout, the refusals, batches, and the torch layer with A and P as inputs.

Every bound is a priori.  Products: (row length + 2) 2^-53 (|dM| |vec|)_i per component.  Derivatives: LSQR stops at
|J q - rhs| <= TOL (|J| |q| + |rhs|), so the relative error is at most about cond(J) TOL; the tests assert 100 cond(J) TOL with cond(J)
computed by numpy for the problem at hand and asserted <= 1e4."""
import gc
import json
import os

import numpy as np
import pytest
from scipy import sparse

import torch

import adjoint_psd_ref as apr
import adjoint_ref as ar
import derivative_matrix_ref as dr
import problem_gen as pg

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "derivative_matrix_fd.json")))
IND, DEN = scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE
STG = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=False, max_iters=100000)
TOL = 1e-12
PROBLEMS = {"lp3": ar.problem_lp3, "qp_soc12": ar.problem_qp_soc, "big300": ar.problem_big, "qp_sdp": apr.problem_qp_sdp}
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
        _problems[name] = PROBLEMS[name]()
    return _problems[name]


def solved(name, normalize=True, solver=IND):
    """(solver, its solution, the problem), solved once per module; the tests only differentiate them"""
    key = (name, normalize, solver)
    if key not in _solved:
        p = problem(name)
        sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=solver, normalize=normalize, **STG)
        sol = sv.solve(warm_start=False)
        assert sol["info"]["status"] == "solved", sol["info"]
        assert np.abs(sol["x"] - p["x"]).max() < 1e-5, name  # the generator's pair: every row and cone is in the case it was built in
        _solved[key] = (sv, sol, p)
    return _solved[key]


def rel(got, ref):
    return np.linalg.norm(got - ref) / np.linalg.norm(ref)


def forward_of(name):
    return apr.derivative if name == "qp_sdp" else ar.derivative


def reference(name, p, sol, db=None, dc=None, dAv=None, dPv=None):
    ref = dr.derivative(p["A"], p["P"], p["cone"], sol["x"], sol["y"], sol["s"], db, dc, dAv, dPv, forward=forward_of(name))
    cond = float(np.linalg.cond(ref["J"]))
    assert cond <= 1e4, cond  # (a condition on the test's inputs)
    return ref, cond


def same_bits(a, b):
    for key in a:
        if key == "info":
            assert {k: v for k, v in a[key].items() if k != "time_ms"} == {k: v for k, v in b[key].items() if k != "time_ms"}
        else:
            ga = a[key].cpu().numpy() if isinstance(a[key], torch.Tensor) else a[key]
            gb = b[key].cpu().numpy() if isinstance(b[key], torch.Tensor) else b[key]
            assert np.array_equal(ga, gb), key


# ---- 1. the products alone ------------------------------------------------------------------------------------------------------------
PROD_N, PROD_M = 151, 40


def product_problem():
    """An l-cone problem with m = 40 rows and n = 151 columns built around a chosen optimal pair (as adjoint_ref.gen_problem builds its
    problems).  (A row of 150 nonzeros and an empty column need 151 columns.)
    A: row 0 has 150 nonzeros — every column but the empty one; more than kPertLongIters = 16 strides of the 8 lanes its mean row length
    gives a row (csrc/perturb.hpp), so the whole workgroup sums it —, row 1 is empty, row 2 has 1 nonzero, row 3 has 3, row 4 has 20
    (three strides of a lane group), the others 2 to 4; column 9 is empty.
    P (upper triangle): column 5 is empty (so is row 5), column 6 holds its diagonal only, the others a diagonal and some off-diagonals."""
    rng = np.random.default_rng(81)
    n, m, empty_col = PROD_N, PROD_M, 9
    cols = np.array([j for j in range(n) if j != empty_col])
    A = np.zeros((m, n))
    A[0, cols] = rng.standard_normal(n - 1) / np.sqrt(n)
    A[2, rng.choice(cols, 1, replace=False)] = rng.standard_normal(1)
    A[3, rng.choice(cols, 3, replace=False)] = rng.standard_normal(3)
    A[4, rng.choice(cols, 20, replace=False)] = rng.standard_normal(20) / 4
    for i in range(5, m):
        k = int(rng.integers(2, 5))
        A[i, rng.choice(cols, k, replace=False)] = rng.standard_normal(k)
    assert not A[1].any() and not A[:, empty_col].any() and np.count_nonzero(A[0]) == 150
    assert sorted(np.count_nonzero(A[2:4], axis=1)) == [1, 3]
    U = np.zeros((n, n))
    for j in range(n):
        if j == 5:
            continue
        U[j, j] = rng.uniform(1.0, 2.0)
    for _ in range(60):
        i, j = sorted(rng.choice([k for k in range(n) if k not in (5, 6)], 2, replace=False))
        U[i, j] = 0.1 * rng.standard_normal()
    assert not U[:, 5].any() and not U[5].any() and np.count_nonzero(U[:, 6]) == 1 and U[6, 6] != 0
    P = sparse.csc_matrix(U)
    P.sort_indices()
    Pd = U + U.T - np.diag(np.diag(U))  # (diagonally dominant where it is not zero: PSD)
    v = rng.uniform(0.5, 1.5, m) * np.where(np.arange(m) % 3 == 0, -1.0, 1.0)
    v[1] = 1.0  # (the empty row: s = b > 0)
    s = np.maximum(v, 0.0)
    y = s - v
    x = rng.standard_normal(n)
    A = sparse.csc_matrix(A)
    A.sort_indices()
    assert A.nnz <= 8 * m and 150 > 16 * 8  # (mean row length <= 8: 8 lanes per row, and row 0 is past 16 strides of them)
    return {"A": A, "P": P, "b": A @ x + s, "c": -Pd @ x - A.T @ y, "cone": {"l": m}, "x": x, "y": y, "s": s}


def test_products_match_a_host_product_componentwise():
    p = product_problem()
    A, P = p["A"], p["P"]
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **dict(STG, eps_abs=1e-7, eps_rel=1e-7))
    sol = sv.solve(warm_start=False)
    assert sol["info"]["status"] == "solved", sol["info"]
    raw = sv._solver
    rng = np.random.default_rng(3)
    dAv, dPv = rng.standard_normal(A.nnz), rng.standard_normal(P.nnz)
    x, y = sol["x"].astype(np.longdouble), sol["y"].astype(np.longdouble)
    u = 2.0 ** -53

    def host(dAv, dPv):
        """the products in extended precision, their componentwise magnitudes |dM| |vec| and the row lengths"""
        n, m = PROD_N, PROD_M
        out_c, out_b, mag_c, mag_b = (np.zeros(k, dtype=np.longdouble) for k in (n, m, n, m))
        len_c, len_b = np.zeros(n), np.zeros(m)
        if dAv is not None:
            dA = dr.dense_dA(A, dAv).astype(np.longdouble)
            out_c += dA.T @ y
            out_b += dA @ x
            mag_c += np.abs(dA).T @ np.abs(y)
            mag_b += np.abs(dA) @ np.abs(x)
            len_c += np.diff(A.indptr)
            len_b += np.bincount(A.indices, minlength=m)
        if dPv is not None:
            dP = dr.dense_dP(P, dPv).astype(np.longdouble)
            out_c += dP @ x
            mag_c += np.abs(dP) @ np.abs(x)
            Pfull = sparse.csr_matrix(dr.dense_dP(P, np.ones(P.nnz)))
            len_c += np.diff(Pfull.indptr)
        return out_c, out_b, (len_c + 2) * u * mag_c, (len_b + 2) * u * mag_b

    for a, q in ((dAv, dPv), (dAv, None), (None, dPv)):
        got_c, got_b = _scs_hip.data_perturbation(raw, dA=a, dP=q)
        ref_c, ref_b, bound_c, bound_b = host(a, q)
        err_c, err_b = np.abs(got_c - ref_c).astype(float), np.abs(got_b - ref_b).astype(float)
        worst = max(float((err_c / np.maximum(bound_c, 1e-300)).max()), float((err_b / np.maximum(bound_b, 1e-300)).max()))
        print("products dA=%s dP=%s: worst error / bound %.3f" % (a is not None, q is not None, worst))
        assert (err_c <= bound_c).all(), (np.argmax(err_c - bound_c), err_c.max())
        assert (err_b <= bound_b).all(), (np.argmax(err_b - bound_b), err_b.max())
        if a is not None:
            assert got_b[1] == 0.0 and got_c[9] == (0.0 if q is None else got_c[9])  # the empty row; the empty column without dP
        # the same bits from a second call and from the device entry
        again = _scs_hip.data_perturbation(raw, dA=a, dP=q)
        assert np.array_equal(again[0], got_c) and np.array_equal(again[1], got_b)
        on_dev = raw.data_perturbation_device(dA=dev(a) if a is not None else None, dP=dev(q) if q is not None else None)
        assert on_dev[0].is_cuda and np.array_equal(on_dev[0].cpu().numpy(), got_c) and np.array_equal(on_dev[1].cpu().numpy(), got_b)
    zero_c, zero_b = _scs_hip.data_perturbation(raw)
    assert not zero_c.any() and not zero_b.any()


# ---- 2. derivative(db, dc, dA, dP) against the reference --------------------------------------------------------------------------------
def check_against_the_reference(name, normalize, solver):
    sv, sol, p = solved(name, normalize, solver)
    db, dc, dAv, dPv = dr.directions(p, 18)
    db2, dc2, dAv2, dPv2 = dr.directions(p, 19)
    has_P = p["P"] is not None
    cases = {"all": (db, dc, dAv, dPv), "dA alone": (None, None, dAv, None), "second": (db2, dc2, dAv2, dPv2)}
    if has_P:
        cases["dP alone"] = (None, None, None, dPv)
    got = {}
    for label, (b_, c_, a_, q_) in cases.items():
        got[label] = sv.derivative(db=b_, dc=c_, tol=TOL, dA=a_, dP=q_)
        ref, cond = reference(name, p, sol, b_, c_, a_, q_)
        bound = 100 * cond * TOL
        for key in ("dx", "dy", "ds"):
            err = rel(got[label][key], ref[key])
            print("%s normalize=%s %s %s %s: relative error %.3e, bound %.3e, cond(J) %.3e, LSQR %s" % (
                name, normalize, solver.name, label, key, err, bound, cond, got[label]["info"]))
            assert got[label][key].shape == ref[key].shape
            assert err <= bound, (name, normalize, label, key, err, bound, got[label]["info"])
        assert got[label]["info"]["stop"] in (1, 2, 3) and got[label]["info"]["iters"] >= 1
    # linearity: the derivative in the sum of two directions is the sum of the derivatives, each known to `bound`
    both = sv.derivative(db=db + db2, dc=dc + dc2, tol=TOL, dA=dAv + dAv2, dP=dPv + dPv2 if has_P else None)
    for key in ("dx", "dy", "ds"):
        total = got["all"][key] + got["second"][key]
        err = np.linalg.norm(both[key] - total) / (np.linalg.norm(got["all"][key]) + np.linalg.norm(got["second"][key]))
        print("%s linearity %s: %.3e (bound %.3e)" % (name, key, err, bound))
        assert err <= bound, (key, err, bound)


@pytest.mark.parametrize("solver", [IND, DEN], ids=["indirect", "dense"])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("name", ["lp3", "qp_soc12", "big300"])
def test_derivative_matches_the_reference(name, normalize, solver):
    check_against_the_reference(name, normalize, solver)


def test_derivative_matches_the_reference_on_an_sdp():
    check_against_the_reference("qp_sdp", True, IND)


# ---- 3. duality with the adjoint's matrix gradients ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp_soc12", "big300"])
def test_forward_and_adjoint_are_dual_in_all_four_inputs(name):
    sv, sol, p = solved(name)
    m, n = p["A"].shape
    rng = np.random.default_rng(5)
    gx, gy, gs = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    db, dc, dAv, dPv = dr.directions(p, 9)
    fw = sv.derivative(db=db, dc=dc, tol=TOL, dA=dAv, dP=dPv)
    ad = sv.adjoint(dx=gx, dy=gy, ds=gs, want=("b", "c", "A", "P"), tol=TOL)
    _, cond = reference(name, p, sol, db, dc, dAv, dPv)
    bound = 100 * cond * TOL
    lhs = gx @ fw["dx"] + gy @ fw["dy"] + gs @ fw["ds"]
    rhs = ad["db"] @ db + ad["dc"] @ dc + ad["dA"] @ dAv + ad["dP"] @ dPv
    # each side is an inner product of an exact vector with one whose relative error is at most `bound`
    g, d = np.concatenate([gx, gy, gs]), np.concatenate([fw["dx"], fw["dy"], fw["ds"]])
    bar, move = np.concatenate([ad["db"], ad["dc"], ad["dA"], ad["dP"]]), np.concatenate([db, dc, dAv, dPv])
    scale = np.linalg.norm(g) * np.linalg.norm(d) + np.linalg.norm(bar) * np.linalg.norm(move)
    print("duality %s: lhs %.15e rhs %.15e, difference / scale %.3e, bound %.3e" % (name, lhs, rhs, abs(lhs - rhs) / scale, bound))
    assert abs(lhs - rhs) <= bound * scale


# ---- 4. zeros, bits and the pool ----------------------------------------------------------------------------------------------------------
def test_zero_perturbations_change_nothing_and_plain_calls_allocate_nothing():
    p = problem("qp_soc12")
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    assert sv.solve(warm_start=False)["info"]["status"] == "solved"
    db, dc, dAv, dPv = dr.directions(p, 2)
    plain = sv.derivative(db=db, dc=dc)
    d_db, d_dc, d_dA, d_dP = dev(db), dev(dc), dev(dAv), dev(dPv)
    sv.derivative_device(db=d_db, dc=d_dc)
    torch.cuda.synchronize()
    before = _scs_hip.pool_stats()["misses"]
    same_bits(plain, sv.derivative_device(db=d_db, dc=d_dc))  # (the device entry: the host entry stages its vectors in new blocks)
    assert _scs_hip.pool_stats()["misses"] == before  # (a call without dA / dP takes nothing new)
    zeros = sv.derivative(db=db, dc=dc, dA=np.zeros_like(dAv), dP=np.zeros_like(dPv))
    for key in ("dx", "dy", "ds"):
        assert np.array_equal(zeros[key], plain[key]), key
    # with perturbations: two calls and both entries give the same bits, and repeated calls take their blocks from the pool
    full = sv.derivative(db=db, dc=dc, dA=dAv, dP=dPv)
    same_bits(full, sv.derivative(db=db, dc=dc, dA=dAv, dP=dPv))
    on_device = sv.derivative_device(db=d_db, dc=d_dc, dA=d_dA, dP=d_dP)
    assert all(on_device[k].is_cuda for k in ("dx", "dy", "ds"))
    same_bits(full, on_device)
    torch.cuda.synchronize()
    before = _scs_hip.pool_stats()["misses"]
    same_bits(full, sv.derivative_device(db=d_db, dc=d_dc, dA=d_dA, dP=d_dP))
    assert _scs_hip.pool_stats()["misses"] == before  # (the scratch and the maps were taken by the first such call)
    # the front end takes a scipy matrix of the constructor's pattern, as update_matrix does
    dA_m = sparse.csc_matrix((dAv, p["A"].indices, p["A"].indptr), shape=p["A"].shape)
    dP_m = sparse.csc_matrix((dPv, p["P"].indices, p["P"].indptr), shape=p["P"].shape)
    same_bits(full, sv.derivative(db=db, dc=dc, dA=dA_m, dP=dP_m))
    # a workspace whose matrix was updated reuses the maps of the update, and a clone is served
    sv.update_matrix(A=p["A"].data.copy(), P=p["P"].data.copy())
    assert sv.solve(warm_start=False)["info"]["status"] == "solved"
    after = sv.derivative(db=db, dc=dc, tol=TOL, dA=dAv, dP=dPv)
    ref = sv.derivative(db=db, dc=dc, tol=TOL)
    assert rel(after["dx"], full["dx"]) < 1e-5 and rel(after["dx"], ref["dx"]) > 1e-3
    cl = sv.clone()
    assert cl.solve(warm_start=False)["info"]["status"] == "solved"
    got = cl.derivative(db=db, dc=dc, tol=TOL, dA=dAv, dP=dPv)
    assert rel(got["dx"], after["dx"]) < 1e-5
    del cl


# ---- 5. one end-to-end central difference of the GPU solver ---------------------------------------------------------------------------------
def test_finite_differences_of_the_gpu_solver_through_update_matrix():
    p = ar.problem_qp_soc()
    rec = GOLD["qp_soc"]
    bound = 10 * max(v for k, v in rec.items() if k != "cond")
    A0, P0 = p["A"].data.copy(), p["P"].data.copy()
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)

    def solve(data):
        sv.update_matrix(A=data["A"].data.copy(), P=data["P"].data.copy())
        r = sv.solve(warm_start=False)
        assert r["info"]["status"] == "solved"
        return r

    def predict(dAv, dPv):
        return sv.derivative(tol=TOL, dA=dAv, dP=dPv)

    got = dr.fd_compare(p, solve, dr.FD_SEED, GOLD["h"], predict=predict)
    print("finite differences through update_matrix: %s, bound %.3e (CPU reference recorded %s)" % (got, bound, rec))
    for key in ("dx", "dy", "ds"):
        assert got[key] <= bound, (key, got[key], bound)
    assert np.array_equal(A0, p["A"].data) and np.array_equal(P0, p["P"].data)


# ---- 6. the pass layout ------------------------------------------------------------------------------------------------------------------
def pass_problem():
    """the problem of tests/test_adjoint_gpu.py's pass-layout test: 20000 x 16400 (>= 16384 rows in each orientation), 6000 tight rows
    each pinned to a column of its own, P diagonally dominant"""
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


def test_pass_layout_agrees_with_the_csr_stream_workspace(monkeypatch):
    data, K = pass_problem()
    stg = dict(STG, eps_abs=1e-8, eps_rel=1e-8, max_iters=5000)
    rng = np.random.default_rng(4)
    db, dc = rng.standard_normal(20000), rng.standard_normal(16400)
    Pu = sparse.triu(data["P"], format="csc")
    dAv, dPv = rng.standard_normal(data["A"].nnz), rng.standard_normal(Pu.nnz)
    plain = scs.SCS(data, K, linear_solver=IND, **stg)
    s0 = plain.solve(warm_start=False)
    assert "CSR-stream" in s0["info"]["lin_sys_solver"] and s0["info"]["status"] == "solved", s0["info"]
    monkeypatch.setenv("SCS_HIP_CS", "2")
    monkeypatch.setenv("SCS_HIP_CS_SPLIT", "1")
    forced = scs.SCS(data, K, linear_solver=IND, **stg)
    s1 = forced.solve(warm_start=False)
    assert "column-sorted pass" in s1["info"]["lin_sys_solver"] and s1["info"]["status"] == "solved", s1["info"]
    f0 = plain.derivative(db=db, dc=dc, tol=TOL, dA=dAv, dP=dPv)
    f1 = forced.derivative(db=db, dc=dc, tol=TOL, dA=dAv, dP=dPv)
    print("pass layout: LSQR %s / %s" % (f0["info"], f1["info"]))
    assert f0["info"]["stop"] in (1, 2) and f1["info"]["stop"] in (1, 2)
    for key in ("dx", "dy", "ds"):
        err = rel(f1[key], f0[key])
        print("pass layout %s: relative difference %.3e" % (key, err))
        assert err <= 1e-10, (key, err)
    # (the perturbation matters: the products are not lost in the comparison)
    assert rel(plain.derivative(db=db, dc=dc, tol=TOL)["dx"], f0["dx"]) > 1e-3


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
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
    _, _, dAv, dPv = dr.directions(p, 1)
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **stg)
    with pytest.raises(ValueError, match="no solve yet"):
        sv.derivative(dA=dAv)
    first = still_solves(sv)
    assert sv.derivative(dA=dAv, dP=dPv)["info"]["stop"] in (1, 2)
    # stale after an update; a new solve makes it fresh
    sv.update_matrix(A=p["A"].data.copy())
    for call in (lambda: sv.derivative(dA=dAv), lambda: sv.derivative_device(dP=dev(dPv)), lambda: sv._solver.data_perturbation(dA=dAv)):
        with pytest.raises(ValueError, match="stale"):
            call()
    still_solves(sv, first["x"])
    assert sv.derivative(dA=dAv, dP=dPv)["info"]["stop"] in (1, 2)
    # dP for a solver without P (Python)
    lp, _, plp = solved("lp3")
    with pytest.raises(ValueError, match="created without P"):
        lp.derivative(dP=np.zeros(3))
    assert lp.derivative(dA=np.ones(plp["A"].nnz))["info"]["stop"] in (1, 2)
    # dP for a P whose columns are not sorted (the library, as update_matrix); dA is served
    A = sparse.csc_matrix(np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]]))
    raw = _scs_hip.SCS((4, 2), A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), np.array([2.0, 1.0, 0.5]),
                       np.array([0, 1, 0], dtype=np.int32), np.array([0, 1, 3], dtype=np.int32), np.ones(4), np.array([-1.0, 1.0]), {"l": 4},
                       eps_abs=1e-7, eps_rel=1e-7, verbose=False)
    r0 = raw.solve(warm_start=False)
    assert r0["info"]["status"] == "solved"
    with pytest.raises(ValueError, match="ascend"):
        raw.derivative(dP=np.ones(3))
    with pytest.raises(ValueError, match="ascend"):
        raw.data_perturbation(dP=np.ones(3))
    assert raw.derivative(db=np.ones(4), dA=np.ones(4))["info"]["stop"] in (1, 2)
    assert np.abs(raw.solve(warm_start=False)["x"] - r0["x"]).max() <= 1e-4
    # a tensor that is not on the workspace's GPU never reaches the library; a host address handed to the device entry is refused by it
    with pytest.raises(ValueError, match="must live on the workspace's GPU"):
        sv.derivative_device(dA=torch.zeros(p["A"].nnz, dtype=torch.float64))
    host = np.zeros(p["A"].nnz)
    out = [torch.zeros(k, dtype=torch.float64, device="cuda") for k in (n, m, m)]
    rc = _scs_hip._lib.scs_hip_derivative_full_device(sv._solver._work, None, None, host.ctypes.data, None, out[0].data_ptr(), out[1].data_ptr(),
                                                      out[2].data_ptr(), None, None)
    assert rc == -1 and "dAx_dev" in _scs_hip.last_error(), _scs_hip.last_error()
    assert sv.derivative(dA=dAv, dP=dPv)["info"]["stop"] in (1, 2)
    still_solves(sv, first["x"])


# ---- 8. batches ----------------------------------------------------------------------------------------------------------------------------
def make_qp(seed):
    return ar.gen_problem(seed, n=12, z=2, l=5, tight_l=2, q=(3, 4, 6), q_case=("polar", "bd", "in"), with_P=True)


def fresh_qp(seed):
    p = make_qp(seed)
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    assert sv.solve(warm_start=False)["info"]["status"] == "solved"
    return sv, p


def test_derivative_batch_with_matrix_perturbations_has_the_solo_bits():
    members = [fresh_qp(seed) for seed in (13, 14, 15, 16)]
    svs = [sv for sv, _ in members]
    d = [dr.directions(p, 40 + i) for i, (_, p) in enumerate(members)]
    solo = [sv.derivative(db=d[i][0], dc=d[i][1], tol=TOL, dA=d[i][2], dP=d[i][3]) for i, sv in enumerate(svs)]
    deltas = []
    for K in (2, 4):
        before = scs.diff_group_launches()
        got = scs.derivative_batch(svs[:K], [v[0] for v in d[:K]], [v[1] for v in d[:K]], tol=TOL, dA=[v[2] for v in d[:K]], dP=[v[3] for v in d[:K]])
        deltas.append(scs.diff_group_launches() - before)
        for a, b in zip(got, solo):
            same_bits(a, b)
    print("grouped launches for K = 2, 4:", deltas, "iterations:", [r["info"]["iters"] for r in solo])
    assert deltas[0] > 0  # (equal counts for members that stop together: the next test)
    on_dev = scs.derivative_batch_device(svs, [dev(v[0]) for v in d], [dev(v[1]) for v in d], tol=TOL, dA=[dev(v[2]) for v in d],
                                         dP=[dev(v[3]) for v in d])
    for a, b in zip(on_dev, solo):
        same_bits(a, b)
    # members that differ in what they pass are grouped apart and keep the caller's order
    mixed = scs.derivative_batch(svs, [v[0] for v in d], [v[1] for v in d], tol=TOL, dA=[d[0][2], None, d[2][2], None],
                                 dP=[None, d[1][3], None, d[3][3]])
    for i, r in enumerate(mixed):
        same_bits(r, svs[i].derivative(db=d[i][0], dc=d[i][1], tol=TOL, dA=d[i][2] if i % 2 == 0 else None, dP=d[i][3] if i % 2 else None))


def test_the_launch_count_of_a_grouped_call_does_not_depend_on_K():
    copies = [fresh_qp(13) for _ in range(4)]
    db, dc, dAv, dPv = dr.directions(copies[0][1], 7)
    deltas, iters = [], []
    for K in (2, 4):
        svs = [sv for sv, _ in copies[:K]]
        before = scs.diff_group_launches()
        res = scs.derivative_batch(svs, [db] * K, [dc] * K, tol=TOL, dA=[dAv] * K, dP=[dPv] * K)
        deltas.append(scs.diff_group_launches() - before)
        iters.append([r["info"]["iters"] for r in res])
    plain_before = scs.diff_group_launches()
    scs.derivative_batch([sv for sv, _ in copies[:2]], [db] * 2, [dc] * 2, tol=TOL)
    plain = scs.diff_group_launches() - plain_before
    print("grouped launches for K = 2, 4:", deltas, "without dA / dP:", plain, "iterations:", iters)
    assert len(set(iters[0] + iters[1])) == 1
    assert deltas[0] == deltas[1] and deltas[0] > 0, deltas


def test_derivative_many_over_clones():
    K = 4
    p = make_qp(13)
    rng = np.random.default_rng(13)
    m, n = p["A"].shape
    B = p["b"][None, :] + 0.01 * rng.standard_normal((K, m)) * np.r_[np.zeros(2), np.ones(m - 2)]  # (the zero rows' b as it is)
    Cc = p["c"][None, :] + 0.01 * rng.standard_normal((K, n))
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    assert all(r["info"]["status"] == "solved" for r in sv.solve_many(b=B, c=Cc))
    DB, DC = rng.standard_normal((K, m)), rng.standard_normal((K, n))
    DA, DP = rng.standard_normal((K, p["A"].nnz)), rng.standard_normal((K, p["P"].nnz))
    raw = [sv._solver] + sv._solver._many
    assert len(raw) == K
    solo = [r.derivative(db=DB[i], dc=DC[i], tol=TOL, dA=DA[i], dP=DP[i]) for i, r in enumerate(raw)]
    for a, b in zip(sv.derivative_many(DB, DC, tol=TOL, dA=DA, dP=DP), solo):
        same_bits(a, b)
    fdev = sv.derivative_many_device(dev(DB), dev(DC), tol=TOL, dA=dev(DA), dP=dev(DP))
    for i in range(K):
        same_bits({"dx": fdev["dx"][i], "dy": fdev["dy"][i], "ds": fdev["ds"][i], "info": fdev["info"][i]}, solo[i])


# ---- 9. the torch layer --------------------------------------------------------------------------------------------------------------------
def test_autograd_solve_with_matrix_inputs():
    import scs.autograd
    p = problem("qp_soc12")
    m, n = p["A"].shape
    rng = np.random.default_rng(5)
    gx, gy, gs = dev(rng.standard_normal(n)), dev(rng.standard_normal(m)), dev(rng.standard_normal(m))
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    sv.autograd_tol = 1e-11
    b, c, Ax, Px = (dev(v).requires_grad_(True) for v in (p["b"], p["c"], p["A"].data, p["P"].data))
    x, y, s = scs.autograd.solve(sv, b, c, A=Ax, P=Px)
    assert sv.autograd_info["status"] == "solved"
    (x @ gx + y @ gy + s @ gs).backward()
    direct = sv.adjoint_device(dx=gx, dy=gy, ds=gs, want=("b", "c", "A", "P"), tol=1e-11)
    assert torch.equal(b.grad, direct["db"]) and torch.equal(c.grad, direct["dc"])
    assert torch.equal(Ax.grad, direct["dA"]) and torch.equal(Px.grad, direct["dP"])
    # only the inputs that need a gradient are asked for
    A_only = dev(p["A"].data).requires_grad_(True)
    x1, _, _ = scs.autograd.solve(sv, b.detach(), c.detach(), A=A_only)
    (x1 @ gx).backward()
    assert A_only.grad is not None and torch.equal(A_only.grad, sv.adjoint_device(dx=gx, want=("A",), tol=1e-11)["dA"])
    # a second forward with perturbed A reaches the solution of a new solver on those values
    A2 = p["A"].copy()
    A2.data = p["A"].data * (1.0 + 0.01 * rng.standard_normal(p["A"].nnz))
    x2, _, _ = scs.autograd.solve(sv, b.detach(), c.detach(), A=dev(A2.data).requires_grad_(True), P=Px.detach())
    assert sv.autograd_info["status"] == "solved"
    new = scs.SCS(dict(ar.data_of(p), A=A2), p["cone"], linear_solver=IND, **STG).solve(warm_start=False)
    assert new["info"]["status"] == "solved"
    assert np.abs(x2.detach().cpu().numpy() - new["x"]).max() <= 1e-4 * max(1.0, np.abs(new["x"]).max())
    with pytest.raises(RuntimeError, match="solved again"):
        (x @ gx).backward()  # (the first graph's solution is gone)
    x2.sum().backward()
    # with A = P = None the layer is the two-argument layer, bit for bit
    one, two = (scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG) for _ in range(2))
    outs = []
    for sv_k, call in ((one, lambda s_, b_, c_: scs.autograd.solve(s_, b_, c_)), (two, lambda s_, b_, c_: scs.autograd.solve(s_, b_, c_, A=None, P=None))):
        sv_k.autograd_tol = 1e-11
        bk, ck = dev(p["b"]).requires_grad_(True), dev(p["c"]).requires_grad_(True)
        xk, yk, sk = call(sv_k, bk, ck)
        (xk @ gx + yk @ gy + sk @ gs).backward()
        outs.append((xk.detach(), yk.detach(), sk.detach(), bk.grad, ck.grad))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)
    # live clones hold the matrix: update_matrix refuses, and the layer lets that through
    cl = one.clone()
    with pytest.raises(ValueError, match="clones"):
        scs.autograd.solve(one, dev(p["b"]), dev(p["c"]), A=dev(p["A"].data))
    del cl
