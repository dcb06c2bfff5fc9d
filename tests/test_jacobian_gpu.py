"""SCS.jacobian: the dense block d of[rows] / d wrt of a solve, computed by adjoint_multi with unit cotangents, against the rows the dense
numpy references (tests/adjoint_ref.py, tests/dproj_cones_ref.py) give for the same cotangents at the GPU solve's own (x, y, s).

The bound is the one of tests/test_adjoint_gpu.py applied to the block: every row is an LSQR answer of relative residual `tol`, so its
relative l2 error is at most cond2(J) tol, J the Jacobian of the optimality conditions; a factor 100 covers the norm equivalences.  The
problems keep cond2(J) <= COND_CAP (asserted) and the tests assert 100 cond tol in the Frobenius norm with tol = 1e-12."""
import gc

import numpy as np
import pytest

import torch

import adjoint_ref as ar
import dproj_cones_ref as dr

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

IND = scs.LinearSolver.HIP_INDIRECT
STG = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=False, max_iters=100000)
TOL = 1e-12
COND_CAP = dr.COND_CAP
CASES = {"qp_soc": (ar.PROBLEMS["qp_soc"], ar.adjoint), "box_qp": (dr.PROBLEMS["box_qp"], dr.adjoint)}
_solved, _refs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _finish_cached_solvers():
    def in_use():
        st = _scs_hip.pool_stats()
        return st["live_bytes"] - st["held_bytes"]
    before = in_use()
    yield
    _solved.clear()
    gc.collect()
    assert in_use() <= before, (in_use(), before)


def solved(name):
    if name not in _solved:
        p = CASES[name][0]()
        sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
        sol = sv.solve(warm_start=False)
        assert sol["info"]["status"] == "solved", sol["info"]
        _solved[name] = (sv, sol, p)
    return _solved[name]


def reference(name, of):
    """({"b": d of / d b, "c": d of / d c}, cond2(J)): the rows the dense reference's adjoint gives for the unit cotangents of `of`,
    computed once and shared"""
    if (name, of) not in _refs:
        sv, sol, p = solved(name)
        size = p["A"].shape[1] if of == "x" else p["A"].shape[0]
        rows = {"b": [], "c": []}
        cond = None
        for r in range(size):
            e = np.zeros(size)
            e[r] = 1.0
            ref = CASES[name][1](p["A"], p["P"], p["cone"], sol["x"], sol["y"], sol["s"], **{"g" + of: e})
            rows["b"].append(ref["db"])
            rows["c"].append(ref["dc"])
            if cond is None:
                cond = float(np.linalg.cond(ref["J"]))
        assert cond <= COND_CAP, cond  # (a condition on the test's inputs)
        _refs[(name, of)] = ({k: np.array(v) for k, v in rows.items()}, cond)
    return _refs[(name, of)]


def rel_fro(got, ref):
    return np.linalg.norm(got - ref) / np.linalg.norm(ref)


@pytest.mark.parametrize("wrt", ["b", "c"])
@pytest.mark.parametrize("of", ["x", "y", "s"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_jacobian_matches_the_dense_reference(name, of, wrt):
    sv, sol, p = solved(name)
    ref, cond = reference(name, of)
    J, infos = sv.jacobian(of=of, wrt=wrt, tol=TOL)
    bound = 100 * cond * TOL
    err = rel_fro(J, ref[wrt])
    print("%s d%s/d%s: shape %s, relative Frobenius error %.3e, bound %.3e, cond(J) %.3e, LSQR iterations %s" % (
        name, of, wrt, J.shape, err, bound, cond, [i["iters"] for i in infos]))
    assert J.shape == ref[wrt].shape and len(infos) == J.shape[0]
    assert err <= bound, (name, of, wrt, err, bound)


@pytest.mark.parametrize("name", sorted(CASES))
def test_chosen_rows_are_those_rows_of_the_full_block(name):
    sv, sol, p = solved(name)
    for of, wrt in (("x", "b"), ("s", "c")):
        full, _ = sv.jacobian(of=of, wrt=wrt, tol=TOL)
        part, infos = sv.jacobian(of=of, wrt=wrt, rows=[0, 3], tol=TOL)
        assert part.shape == (2, full.shape[1]) and len(infos) == 2
        assert np.array_equal(part, full[[0, 3]]), (of, wrt)
        partd, _ = sv.jacobian_device(of=of, wrt=wrt, rows=[0, 3], tol=TOL)
        assert isinstance(partd, torch.Tensor) and partd.is_cuda and np.array_equal(partd.cpu().numpy(), part)
    with pytest.raises(ValueError, match="rows holds"):
        sv.jacobian(rows=[0, p["A"].shape[1]])


@pytest.mark.parametrize("name", sorted(CASES))
def test_jacobian_times_a_direction_is_the_forward_derivative(name):
    sv, sol, p = solved(name)
    _, cond = reference(name, "x")
    bound = 100 * cond * TOL
    m = p["A"].shape[0]
    db = np.random.default_rng(17).standard_normal(m)
    J, _ = sv.jacobian("x", "b", tol=TOL)
    fw = sv.derivative(db=db, tol=TOL)
    err = np.linalg.norm(J @ db - fw["dx"]) / np.linalg.norm(fw["dx"])
    print("%s duality: |J db - dx| / |dx| = %.3e, bound %.3e" % (name, err, bound))
    assert err <= bound, (err, bound)
