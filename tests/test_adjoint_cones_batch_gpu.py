"""Grouped derivatives of problems with a box cone and power cones (csrc/diff_batch.hpp with the bodies of csrc/dproj_box_pow.hpp):
a batch differentiated in lock step gives, member by member, the BITS of the member's own call — outputs, iteration count, stopping rule
and residual figures.  No tolerance appears below.

Seeds: every member below was checked to end "solved" at STG on the CPU oracle (oracle/scs_oracle.py, direct solver)."""
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
SEEDS = (61, 62, 63, 64, 65)
ALL = ("b", "c", "A", "P")
INF = float("inf")
_solved = {}


def make(seed, k=4, npow=4):
    """z | l | box (k bounds) | p (npow cones): the shape is the same for every seed, the bounds, the exponents, the active sets and
    the cases of the power cones differ from member to member"""
    rng = np.random.default_rng(seed + 5000)
    bl = (-rng.uniform(0.3, 1.5, k)).tolist()
    bu = rng.uniform(0.3, 1.5, k).tolist()
    bl[1] = 0.0
    bu[k - 1] = INF
    sets = [["U", "L", "F"][i] for i in rng.integers(0, 3, k)]
    sets[1], sets[k - 1] = "L", "F"
    box = dict(bl=bl, bu=bu, sets=sets, tstar=float(rng.uniform(0.6, 1.2)))
    p = (rng.uniform(0.15, 0.85, npow) * rng.choice([-1.0, 1.0], npow)).tolist()
    p_case = [["in", "polar", "bd", "bd"][i] for i in rng.integers(0, 4, npow)]
    return dr.gen_problem(seed, n=16, z=1, l=3, tight_l=1, box=box, p=p, p_case=p_case)


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


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def fresh(seed, normalize=True, **shape):
    p = make(seed, **shape)
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, normalize=normalize, **STG)
    sol = sv.solve(warm_start=False)
    assert sol["info"]["status"] == "solved", (seed, sol["info"])
    assert np.abs(sol["x"] - p["x"]).max() < 1e-5, seed
    p["sol"] = sol
    return sv, p


def solved(seed, normalize=True):
    key = (seed, normalize)
    if key not in _solved:
        _solved[key] = fresh(seed, normalize)
    return _solved[key]


def cot(p, seed):
    rng = np.random.default_rng(seed)
    m, n = p["A"].shape
    return rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)


def same_bits(got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k in ref:
        if k == "info":
            for f in ("iters", "stop", "residual", "normal_residual"):
                assert got["info"][f] == ref["info"][f], (f, got["info"], ref["info"])
        else:
            a = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
            b = ref[k].cpu().numpy() if isinstance(ref[k], torch.Tensor) else ref[k]
            assert a.shape == b.shape and np.array_equal(a, b), k


@pytest.mark.parametrize("normalize", [True, False])
def test_box_pow_group_has_the_solo_bits(normalize):
    members = [solved(seed, normalize) for seed in SEEDS]
    svs = [sv for sv, _ in members]
    assert scs.diff_batch_plan(svs, want=ALL) == [0] * 5
    # the members really differ in what the grouped kernels read per member
    assert len({tuple(p["cone"]["bu"]) for _, p in members}) == 5 and len({tuple(p["cone"]["p"]) for _, p in members}) == 5
    g = [cot(p, 100 + i) for i, (_, p) in enumerate(members)]
    solo = [sv.adjoint(dx=gi[0], dy=gi[1], ds=gi[2], want=ALL, tol=TOL) for sv, gi in zip(svs, g)]
    got = scs.adjoint_batch(svs, [gi[0] for gi in g], [gi[1] for gi in g], [gi[2] for gi in g], want=ALL, tol=TOL)
    for a, b in zip(got, solo):
        same_bits(a, b)
    assert all(r["info"]["stop"] in (1, 2) for r in solo)
    solo_f = [sv.derivative(db=gi[1], dc=gi[0], tol=TOL) for sv, gi in zip(svs, g)]
    for a, b in zip(scs.derivative_batch(svs, [gi[1] for gi in g], [gi[0] for gi in g], tol=TOL), solo_f):
        same_bits(a, b)
    # against the reference too: the group computes the right thing, not only the same thing
    sv, p = members[0]
    sol = p["sol"]
    ref = dr.adjoint(p["A"], p["P"], p["cone"], sol["x"], sol["y"], sol["s"], *g[0])
    cond = float(np.linalg.cond(ref["J"]))
    assert cond <= dr.COND_CAP
    again = scs.adjoint_batch(svs, [gi[0] for gi in g], [gi[1] for gi in g], [gi[2] for gi in g], tol=TOL)[0]
    assert np.linalg.norm(again["db"] - ref["db"]) <= 100 * cond * TOL * np.linalg.norm(ref["db"])


def test_one_launch_per_kernel_for_the_group():
    copies = [fresh(61) for _ in range(5)]
    gx, gy, gs = cot(copies[0][1], 7)
    deltas, iters = [], []
    for K in (2, 5):
        svs = [sv for sv, _ in copies[:K]]
        assert scs.diff_batch_plan(svs) == [0] * K
        before = scs.diff_group_launches()
        res = scs.adjoint_batch(svs, [gx] * K, [gy] * K, [gs] * K, tol=TOL)
        deltas.append(scs.diff_group_launches() - before)
        iters.append([r["info"]["iters"] for r in res])
    print("grouped launches for K = 2, 5:", deltas, "iterations:", iters)
    assert len(set(iters[0] + iters[1])) == 1
    assert deltas[0] == deltas[1] and deltas[0] > 0, deltas  # the launch count does not depend on K: one launch per kernel


def test_a_different_box_size_or_power_cone_count_splits_the_batch():
    a, b = solved(61), solved(62)
    other_box, other_pow = fresh(63, k=5), fresh(64, npow=3)
    assert other_box[1]["A"].shape[0] != a[1]["A"].shape[0]
    svs = [a[0], other_box[0], b[0], other_pow[0]]
    assert scs.diff_batch_plan(svs) == [0, -1, 0, -1]
    # the same m with another split between box and p rows: 3 more bounds, one power cone fewer
    same_m = fresh(65, k=7, npow=3)
    assert same_m[1]["A"].shape == a[1]["A"].shape
    assert scs.diff_batch_plan([a[0], same_m[0], b[0]]) == [0, -1, 0]
    members = [a, same_m, b]
    g = [cot(p, 30 + i) for i, (_, p) in enumerate(members)]
    solo = [sv.adjoint(dx=gi[0], dy=gi[1], ds=gi[2], tol=TOL) for (sv, _), gi in zip(members, g)]
    got = scs.adjoint_batch([sv for sv, _ in members], [gi[0] for gi in g], [gi[1] for gi in g], [gi[2] for gi in g], tol=TOL)
    for x, y in zip(got, solo):
        same_bits(x, y)


def test_adjoint_many_over_a_solve_many():
    K = 4
    p = make(61)
    rng = np.random.default_rng(3)
    m, n = p["A"].shape
    free_b = np.r_[0.0, np.ones(m - 1)]  # (the zero row's b as it is)
    B = p["b"][None, :] + 0.01 * rng.standard_normal((K, m)) * free_b
    Cc = p["c"][None, :] + 0.01 * rng.standard_normal((K, n))
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    res = sv.solve_many(b=B, c=Cc)
    assert all(r["info"]["status"] == "solved" for r in res)
    GX, GY, GS = rng.standard_normal((K, n)), rng.standard_normal((K, m)), rng.standard_normal((K, m))
    raw = [sv._solver] + sv._solver._many
    assert len(raw) == K
    solo = [r.adjoint(dx=GX[i], dy=GY[i], ds=GS[i], want=ALL, tol=TOL) for i, r in enumerate(raw)]
    for a, b in zip(sv.adjoint_many(GX, GY, GS, want=ALL, tol=TOL), solo):
        same_bits(a, b)
    on_dev = sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=ALL, tol=TOL)
    for i in range(K):
        same_bits({"db": on_dev["db"][i], "dc": on_dev["dc"][i], "dA": on_dev["dA"][i], "dP": on_dev["dP"][i], "info": on_dev["info"][i]}, solo[i])
    solo_f = [r.derivative(db=GY[i], dc=GX[i], tol=TOL) for i, r in enumerate(raw)]
    for a, b in zip(sv.derivative_many(GY, GX, tol=TOL), solo_f):
        same_bits(a, b)


def test_autograd_solve_many_on_box_and_power_cones():
    import scs.autograd
    K = 3
    p = make(62)
    m, n = p["A"].shape
    rng = np.random.default_rng(5)
    B0 = p["b"][None, :] + 0.01 * rng.standard_normal((K, m)) * np.r_[0.0, np.ones(m - 1)]
    C0 = p["c"][None, :] + 0.01 * rng.standard_normal((K, n))
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    sv.autograd_tol = 1e-11
    B, Cc = dev(B0).requires_grad_(True), dev(C0).requires_grad_(True)
    X, Y, S = scs.autograd.solve_many(sv, B, Cc)
    assert all(i["status"] == "solved" for i in sv.autograd_info)
    GX, GY, GS = dev(rng.standard_normal((K, n))), dev(rng.standard_normal((K, m))), dev(rng.standard_normal((K, m)))
    ((X * GX).sum() + (Y * GY).sum() + (S * GS).sum()).backward()
    direct = sv.adjoint_many_device(GX, GY, GS, tol=1e-11)
    assert torch.equal(B.grad, direct["db"]) and torch.equal(Cc.grad, direct["dc"])
    assert torch.isfinite(B.grad).all() and B.grad.abs().max() > 0
