"""SCS.refine / refine_device (csrc/refine.hpp): Newton polish of a loosely solved point on the device, against the dense numpy reference
of tests/refine_ref.py and the generators' exact primal-dual pairs.

Every problem is solved at LOOSE (1e-4) and refined to TOL = 1e-10, three decades above the 1e-13 level the preparation's PSD
decomposition stops at.  The bounds:
  * the stop rule recomputed in numpy holds at 10 TOL (the factor covers the other summation order of the recomputation);
  * |Pi(s - y) - s|_inf <= 1e-11 (1 + |s|_inf): s in K, y in K*, s'y = 0 in one;
  * steps <= k_ref + 2, k_ref = the steps of refine_ref.newton (exact inner solves) from the same start: the inexact inner solve cost at
    most one step more on the CPU, the second is margin;
  * |z - z*|_2 <= 10 |J^-1|_2 |F(z)|_2 + 1e-12 |z*|_2 against the generator's pair z* = (x*, s* - y*), J at z*: the first-order bound, 10
    for the curvature over that distance;
  * derivatives at the polished point: the bound of tests/test_adjoint_gpu.py, 100 cond(J) tol with tol = 1e-12."""
import gc

import numpy as np
import pytest
from scipy import sparse

import torch

import adjoint_ref as ar
import adjoint_psd_ref as pr
import dproj_cones_ref as dr
import refine_ref as rr

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

IND, DEN = scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE
LOOSE = dict(eps_abs=1e-4, eps_rel=1e-4, verbose=False, max_iters=100000)
TOL = 1e-10
DTOL = 1e-12
COND_CAP = dr.COND_CAP
GENERATORS = {}
for _mod in (ar, dr, pr):
    for _name, _gen in _mod.PROBLEMS.items():
        GENERATORS[_name] = (_mod, _gen)
GENERATORS["big"] = (ar, ar.problem_big)
SMALL = sorted(n for n in GENERATORS if n != "big")
CASES = [(name, normalize, solver) for name in SMALL for normalize in (True, False) for solver in (IND, DEN)] + [("big", True, IND)]
CASE_IDS = ["%s-%s-%s" % (name, "normalized" if nz else "raw", "indirect" if sv == IND else "dense") for name, nz, sv in CASES]
_problems, _refined = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _finish_cached_solvers():
    """the solvers this module refines once and shares are finished with it (the block pool's account is an invariant of
    tests/test_pool_lifecycle_gpu.py)"""
    def in_use():
        st = _scs_hip.pool_stats()
        return st["live_bytes"] - st["held_bytes"]
    before = in_use()
    yield
    _refined.clear()
    gc.collect()
    assert in_use() <= before, (in_use(), before)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def problem(name):
    if name not in _problems:
        mod, gen = GENERATORS[name]
        _problems[name] = (mod, gen())
    return _problems[name]


def new_solver(name, normalize=True, solver=IND, **over):
    mod, p = problem(name)
    return scs.SCS(ar.data_of(p), p["cone"], linear_solver=solver, normalize=normalize, **dict(LOOSE, **over))


def cotangents(p, seed=5):
    rng = np.random.default_rng(seed)
    m, n = p["A"].shape
    return rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)


def rel(got, ref):
    return np.linalg.norm(got - ref) / np.linalg.norm(ref)


def want_of(p):
    return ("b", "c", "A", "P") if p["P"] is not None else ("b", "c", "A")


def refined(name, normalize=True, solver=IND):
    """one LOOSE solve and one refine(tol=TOL) per case, shared by the tests: (solver, loose solution, refine result, dc of the adjoint
    at the loose solution — for the record test 2 prints)"""
    key = (name, normalize, solver)
    if key not in _refined:
        mod, p = problem(name)
        sv = new_solver(name, normalize, solver)
        loose = sv.solve(warm_start=False)
        assert loose["info"]["status"] == "solved", loose["info"]
        gx, gy, gs = cotangents(p)
        before = sv.adjoint(dx=gx, dy=gy, ds=gs, tol=DTOL)
        res = sv.refine(tol=TOL)
        _refined[key] = (sv, loose, res, before)
    return _refined[key]


def same_bits(a, b):
    assert set(a) == set(b)
    for key in a:
        if key == "info":
            assert {k: v for k, v in a[key].items() if k != "time_ms"} == {k: v for k, v in b[key].items() if k != "time_ms"}
        else:
            ga = a[key].cpu().numpy() if isinstance(a[key], torch.Tensor) else a[key]
            gb = b[key].cpu().numpy() if isinstance(b[key], torch.Tensor) else b[key]
            assert np.array_equal(ga, gb), key


def distance_bound(mod, p, x, y, s):
    """(|z - z*|_2, 10 |J^-1|_2 |F(z)|_2 + 1e-12 |z*|_2) for z = (x, s - y) against the generator's pair"""
    zs = np.concatenate([p["x"], p["s"] - p["y"]])
    z = np.concatenate([x, s - y])
    sing = np.linalg.svd(rr.jacobian(p, mod, p["s"] - p["y"]), compute_uv=False)
    f = np.linalg.norm(rr.F(p, mod, x, s - y))
    return np.linalg.norm(z - zs), 10.0 * f / sing[-1] + 1e-12 * np.linalg.norm(zs)


# ---- 1. reaches the tolerance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,normalize,solver", CASES, ids=CASE_IDS)
def test_refine_reaches_the_tolerance(name, normalize, solver):
    mod, p = problem(name)
    sv, loose, res, _ = refined(name, normalize, solver)
    info = res["info"]
    x, y, s = res["x"], res["y"], res["s"]
    rec = rr.residuals(p, x, y, s)
    k_ref, _, _ = rr.newton(p, mod, loose["x"], loose["s"] - loose["y"], tol=TOL)
    member = np.abs(mod.project(s - y, p["cone"]) - s).max()
    dist, bound = distance_bound(mod, p, x, y, s)
    print("%s normalize=%s %s: %s" % (name, normalize, solver.name, info))
    print("  recomputed %s" % (rec,))
    print("  steps %d (reference %d), |Pi(s - y) - s| %.3e, |z - z*| %.3e (bound %.3e)" % (info["steps"], k_ref, member, dist, bound))
    assert info["stop"] == 1 and info["stop_reason"] == "converged", info
    assert rr.meets(rec, 10 * TOL), rec
    assert member <= 1e-11 * (1.0 + np.abs(s).max()), member
    for key in ("pri", "dual", "gap"):
        got = info["res_" + key] if key != "gap" else info["gap"]
        assert abs(got - rec[key]) <= 1e-12 * (1.0 + rec[key + "_scale"]) + 1e-6 * rec[key], (key, got, rec[key])
    assert info["merit_after"] < info["merit_before"]
    assert 1 <= info["steps"] <= k_ref + 2, (info["steps"], k_ref)
    assert dist <= bound, (dist, bound)


# ---- 2. derivatives at the polished point -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,normalize,solver", CASES, ids=CASE_IDS)
def test_derivatives_at_the_polished_point(name, normalize, solver):
    mod, p = problem(name)
    sv, loose, res, before = refined(name, normalize, solver)
    gx, gy, gs = cotangents(p)
    want = want_of(p)
    ad = sv.adjoint(dx=gx, dy=gy, ds=gs, want=want, tol=DTOL)
    ref = mod.adjoint(p["A"], p["P"], p["cone"], res["x"], res["y"], res["s"], gx, gy, gs)
    cond = float(np.linalg.cond(ref["J"]))
    assert cond <= COND_CAP, cond  # (a condition on the test's inputs)
    bound = 100 * cond * DTOL
    refs = {"db": ref["db"], "dc": ref["dc"], "dA": ar.stored_values(ref["dA"], p["A"])}
    if p["P"] is not None:
        refs["dP"] = ar.stored_values(ref["dP"], p["P"])
    for key, r in refs.items():
        err = rel(ad[key], r)
        print("%s normalize=%s %s %s: relative error %.3e, bound %.3e, cond(J) %.3e" % (name, normalize, solver.name, key, err, bound, cond))
        assert err <= bound, (key, err, bound, ad["info"])
    rng = np.random.default_rng(9)
    m, n = p["A"].shape
    db, dc = rng.standard_normal(m), rng.standard_normal(n)
    fw = sv.derivative(db=db, dc=dc, tol=DTOL)
    fref = mod.derivative(p["A"], p["P"], p["cone"], res["x"], res["y"], res["s"], db, dc)
    for key in ("dx", "dy", "ds"):
        err = rel(fw[key], fref[key])
        print("%s normalize=%s %s forward %s: relative error %.3e, bound %.3e" % (name, normalize, solver.name, key, err, bound))
        assert err <= bound, (key, err, bound)
    # for the record (profiles/refine_first_numbers.txt): the distance to the gradient at the generator's exact pair, before and after
    exact = mod.adjoint(p["A"], p["P"], p["cone"], p["x"], p["y"], p["s"], gx, gy, gs)
    for key in ("db", "dc"):
        print("RECORD %s normalize=%s %s %s: relative distance to the exact pair's gradient %.3e at eps 1e-4, %.3e refined" %
              (name, normalize, solver.name, key, rel(before[key], exact[key]), rel(ad[key], exact[key])))


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp_soc", "mixed", "qp_sdp", "big"])
def test_twins_and_both_entries_give_the_same_bits(name):
    mod, p = problem(name)
    a, b, c = (new_solver(name) for _ in range(3))
    for sv in (a, b, c):
        assert sv.solve(warm_start=False)["info"]["status"] == "solved"
    ra, rb = a.refine(tol=TOL), b.refine(tol=TOL)
    assert ra["info"]["steps"] >= 1
    same_bits(ra, rb)
    same_bits(ra, c.refine_device(tol=TOL))
    gx, gy, gs = cotangents(p)
    want = want_of(p)
    first = a.adjoint(dx=gx, dy=gy, ds=gs, want=want)
    same_bits(first, b.adjoint(dx=gx, dy=gy, ds=gs, want=want))
    same_bits(first, c.adjoint(dx=gx, dy=gy, ds=gs, want=want))


# ---- 4. the solve's state is left alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "qp_sdp"])
def test_refine_leaves_the_state_of_the_next_solve_alone(name):
    a, twin = new_solver(name), new_solver(name)
    sa, st = a.solve(warm_start=False), twin.solve(warm_start=False)
    assert sa["info"]["status"] == "solved" and np.array_equal(sa["x"], st["x"])
    assert a.refine(tol=TOL)["info"]["steps"] >= 1
    ca, ct = a.solve(warm_start=False), twin.solve(warm_start=False)
    for key in ("x", "y", "s"):
        assert np.array_equal(ca[key], ct[key]), key
    assert ca["info"]["iter"] == ct["info"]["iter"] and ca["info"]["cg_iters"] == ct["info"]["cg_iters"]
    # ... and a warm start reads the polished point
    polished = a.refine(tol=TOL)
    assert polished["info"]["stop"] == 1
    warm = a.solve(warm_start=True)
    print("%s: cold %d iterations, warm from the polished point %d" % (name, ca["info"]["iter"], warm["info"]["iter"]))
    assert warm["info"]["status"] == "solved" and warm["info"]["iter"] <= ca["info"]["iter"]


# ---- 5. nothing to do / nothing gained --------------------------------------------------------------------------------------------------
def test_a_point_that_meets_the_rule_is_left_bit_for_bit():
    sv = new_solver("qp_soc", eps_abs=1e-9, eps_rel=1e-9)
    sol = sv.solve(warm_start=False)
    assert sol["info"]["status"] == "solved"
    res = sv.refine(tol=1e-6)
    assert res["info"]["steps"] == 0 and res["info"]["stop"] == 1 and res["info"]["lsqr_iters"] == 0, res["info"]
    assert res["info"]["merit_after"] == res["info"]["merit_before"]
    for key in ("x", "y", "s"):
        assert np.array_equal(res[key], sol[key]), key
    back = {k: torch.zeros(len(sol[k]), dtype=torch.float64, device="cuda") for k in ("x", "y", "s")}  # ... and so is the resident copy
    sv._solver.solution_to_device(back["x"].data_ptr(), back["y"].data_ptr(), back["s"].data_ptr())
    torch.cuda.synchronize()
    for key in ("x", "y", "s"):
        assert np.array_equal(back[key].cpu().numpy(), sol[key]), key


def test_max_steps_stops_and_the_next_call_goes_on():
    sv = new_solver("pow")
    assert sv.solve(warm_start=False)["info"]["status"] == "solved"
    one = sv.refine(tol=1e-14, max_steps=1)
    assert one["info"]["stop"] == 2 and one["info"]["stop_reason"] == "max_steps" and one["info"]["steps"] == 1, one["info"]
    assert one["info"]["merit_after"] < one["info"]["merit_before"]
    two = sv.refine(tol=1e-14, max_steps=1)
    print("pow: first call %s\n     second call %s" % (one["info"], two["info"]))
    assert abs(two["info"]["merit_before"] - one["info"]["merit_after"]) <= 1e-9 * one["info"]["merit_after"]


# ---- 6. refusals, and the workspace survives them ---------------------------------------------------------------------------------------
def feasible_qp(K, seed):
    """a strictly convex QP with a feasible point (as tests/test_adjoint_cones_gpu.py): P = I, s0 = Pi_K(random), b = A x0 + s0"""
    rng = np.random.default_rng(seed)
    m = K.get("z", 0) + K.get("l", 0) + 3 * (K.get("ep", 0) + K.get("ed", 0))
    n = 3
    s0 = _scs_hip.proj_cone(rng.standard_normal(m), K, dual=False)
    A = sparse.csc_matrix(rng.standard_normal((m, n)))
    return {"P": sparse.identity(n, format="csc"), "A": A, "b": A @ rng.standard_normal(n) + s0, "c": rng.standard_normal(n)}


def still_solves(sv):
    assert sv.solve(warm_start=False)["info"]["status"] == "solved"


def test_refusals_leave_the_workspace_usable():
    mod, p = problem("qp_soc")
    sv = new_solver("qp_soc")
    for call in (sv.refine, sv.refine_device):
        with pytest.raises(ValueError, match="libscs_hip: scs_hip_refine.*no solve yet"):
            call()
    still_solves(sv)
    assert sv.refine(tol=TOL)["info"]["stop"] == 1
    sv.update(b=p["b"].copy())
    for call in (sv.refine, sv.refine_device):
        with pytest.raises(ValueError, match="stale"):
            call()
    still_solves(sv)
    assert sv.refine(tol=TOL)["info"]["stop"] == 1
    # the last solve did not end solved (the infeasible LP of tests/test_adjoint_gpu.py)
    bad = scs.SCS({"A": sparse.csc_matrix(np.array([[-1.0], [1.0]])), "b": np.array([-1.0, 0.0]), "c": np.array([1.0])}, {"l": 2},
                  linear_solver=IND, **LOOSE)
    assert bad.solve(warm_start=False)["info"]["status"] == "infeasible"
    with pytest.raises(ValueError, match="did not end solved"):
        bad.refine()
    bad.update(b=np.array([1.0, 0.0]))
    still_solves(bad)
    assert bad.refine(tol=TOL)["info"]["stop"] in (1, 2, 3)
    # a cone without a derivative is named
    K = {"l": 2, "ep": 1}
    ex = scs.SCS(feasible_qp(K, 5), K, linear_solver=IND, **LOOSE)
    still_solves(ex)
    with pytest.raises(ValueError, match=r"exponential \(ep\) cone"):
        ex.refine()
    still_solves(ex)
    # arguments: refused in Python, before the library
    for kw in (dict(tol=0), dict(tol=float("nan")), dict(max_steps=0)):
        for call in (sv.refine, sv.refine_device):
            with pytest.raises(ValueError):
                call(**kw)
    still_solves(sv)


def test_a_nan_tol_is_refused_by_the_library_too():
    import ctypes as C
    sv = new_solver("lp")
    still_solves(sv)
    raw = sv._solver
    opts = _scs_hip._ScsHipRefineOpts(float("nan"), 0, 0.0, 0)
    info = _scs_hip._ScsHipRefineInfo()
    assert _scs_hip._lib.scs_hip_refine(raw._work, None, C.byref(opts), C.byref(info)) == -1
    assert "tol is NaN" in _scs_hip.last_error()
    assert _scs_hip._lib.scs_hip_refine(raw._work, None, None, C.byref(info)) == 0  # NULL sol and opts: the defaults, nothing copied out
    assert info.stop in (1, 2, 3)
    still_solves(sv)


# ---- 7. the identity the design rests on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "pow", "box_qp", "qp_sdp", "lp_sdp", "qp_soc"])
def test_W_v_is_the_projection_of_v(name):
    """Pi_K is positively homogeneous, so Pi_K(v) = W(v) v: the apply of the derivative at u = v is the projection"""
    mod, p = problem(name)
    v = p["s"] - p["y"]
    Wu, WmIu = _scs_hip.dproj_cone(v, v, p["cone"])
    want = mod.project(v, p["cone"])
    err = np.abs(Wu - want).max()
    print("%s: |W v - Pi(v)|_inf = %.3e" % (name, err))
    assert err <= 1e-12 * (1.0 + np.abs(v).max())
    assert np.abs(WmIu - (Wu - v)).max() <= 1e-15 * (1.0 + np.abs(v).max())


# ---- 8. the layer -----------------------------------------------------------------------------------------------------------------------
def test_autograd_solve_refines_when_asked():
    import scs.autograd
    mod, p = problem("box_qp")
    gx, gy, gs = cotangents(p)
    sv = new_solver("box_qp")
    sv.autograd_tol = DTOL
    sv.autograd_refine_tol = TOL
    b = dev(p["b"]).requires_grad_(True)
    c = dev(p["c"]).requires_grad_(True)
    x, y, s = scs.autograd.solve(sv, b, c)
    (x @ dev(gx) + y @ dev(gy) + s @ dev(gs)).backward()
    sol = {k: t.detach().cpu().numpy() for k, t in (("x", x), ("y", y), ("s", s))}
    assert sv.autograd_refine_info["stop"] == 1 and sv.autograd_info["status"] == "solved"
    dist, bound = distance_bound(mod, p, sol["x"], sol["y"], sol["s"])
    print("box_qp layer: |z - z*| %.3e (bound %.3e), refine %s" % (dist, bound, sv.autograd_refine_info))
    assert dist <= bound
    ref = mod.adjoint(p["A"], p["P"], p["cone"], sol["x"], sol["y"], sol["s"], gx, gy, gs)
    cond = float(np.linalg.cond(ref["J"]))
    assert cond <= COND_CAP
    assert rel(b.grad.cpu().numpy(), ref["db"]) <= 100 * cond * DTOL and rel(c.grad.cpu().numpy(), ref["dc"]) <= 100 * cond * DTOL
    # None: the layer is the one it always was
    plain, twin = new_solver("box_qp"), new_solver("box_qp")
    assert getattr(plain, "autograd_refine_tol", None) is None
    xp, yp, sp = scs.autograd.solve(plain, dev(p["b"]), dev(p["c"]))
    twin.update_device(dev(p["b"]), dev(p["c"]))
    direct = twin.solve_device(warm_start=False)
    for got, key in ((xp, "x"), (yp, "y"), (sp, "s")):
        assert torch.equal(got, direct[key]), key
