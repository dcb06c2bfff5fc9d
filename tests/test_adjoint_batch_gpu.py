"""Grouped derivatives (scs.adjoint_batch / derivative_batch, SCS.adjoint_many / derivative_many and their device twins,
scs.autograd.solve_many; csrc/diff_batch.hpp): a batch differentiated in lock step gives, member by member, the BITS of the member's own
`adjoint` / `derivative` call — outputs, iteration count, stopping rule and residual figures.  No tolerance appears below: every
comparison is np.array_equal / ==.

Seeds: every problem below was checked to end "solved" at STG on the CPU oracle (oracle/scs_oracle.py, direct solver) — the
QP + SOC shape for seeds 13 .. 22 (150 .. 225 iterations), the QP + SDP shape for seeds 41 .. 48, the long cone for 62 and 63, the
order-33 block for 71."""
import gc

import numpy as np
import pytest

import torch

import adjoint_ref as ar
import adjoint_psd_ref as apr
import problem_gen as pg

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

IND, DEN = scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE
STG = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=False, max_iters=100000)
TOL = 1e-12
QP_SEEDS = (13, 14, 15, 16, 17, 18)
SDP_SEEDS = (41, 42, 43, 44, 45)
LONG_SEEDS = (62, 63)
ALL = ("b", "c", "A", "P")
_solved = {}


def make_qp(seed):
    return ar.gen_problem(seed, n=12, z=2, l=5, tight_l=2, q=(3, 4, 6), q_case=("polar", "bd", "in"), with_P=True)


def make_sdp(seed):
    return apr.gen_problem(seed, n=14, z=1, l=4, tight_l=2, s=(3, 5), ranks=(1, 3), with_P=True)


def make_long(seed):  # one cone of 4100 entries (> kSocBig: the block bodies) and six l rows
    return ar.gen_problem(seed, n=10, z=0, l=6, tight_l=2, q=(4100,), q_case=("bd",), with_P=True)


def make_sdp33(seed):  # a PSD block of order 33: the five-launch tile path, which is not grouped
    return apr.gen_problem(seed, n=40, z=1, l=4, tight_l=2, s=(33,), ranks=(30,), with_P=True)


MAKERS = {"qp": make_qp, "sdp": make_sdp, "long": make_long, "sdp33": make_sdp33}


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


def fresh(shape, seed, normalize=True, solver=IND, stg=STG):
    p = MAKERS[shape](seed)
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=solver, normalize=normalize, **stg)
    sol = sv.solve(warm_start=False)
    assert sol["info"]["status"] == "solved", (shape, seed, sol["info"])
    return sv, p


def solved(shape, seed, normalize=True, solver=IND):
    """(solver, problem), solved once per module; the tests only differentiate them"""
    key = (shape, seed, normalize, solver)
    if key not in _solved:
        _solved[key] = fresh(shape, seed, normalize, solver)
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


def check_group(members, want=ALL, tol=TOL, max_iters=None, plan=None):
    """adjoint_batch and derivative_batch over `members` ((solver, problem) pairs) against the members' own calls; returns the solo
    adjoint results"""
    svs = [sv for sv, _ in members]
    if plan is not None:
        assert scs.diff_batch_plan(svs, want=want) == plan
    g = [cot(p, 100 + i) for i, (_, p) in enumerate(members)]
    solo = [sv.adjoint(dx=gi[0], dy=gi[1], ds=gi[2], want=want, tol=tol, max_iters=max_iters) for sv, gi in zip(svs, g)]
    got = scs.adjoint_batch(svs, [gi[0] for gi in g], [gi[1] for gi in g], [gi[2] for gi in g], want=want, tol=tol, max_iters=max_iters)
    assert len(got) == len(solo)
    for a, b in zip(got, solo):
        same_bits(a, b)
    solo_f = [sv.derivative(db=gi[1], dc=gi[0], tol=tol, max_iters=max_iters) for sv, gi in zip(svs, g)]
    got_f = scs.derivative_batch(svs, [gi[1] for gi in g], [gi[0] for gi in g], tol=tol, max_iters=max_iters)
    for a, b in zip(got_f, solo_f):
        same_bits(a, b)
    return solo


# ---- 1. independent members, z / l / q ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("solver", [IND, DEN], ids=["ind", "den"])
def test_qp_soc_group_has_the_solo_bits(normalize, solver):
    members = [solved("qp", seed, normalize, solver) for seed in QP_SEEDS]
    solo = check_group(members, plan=[0] * 6)
    assert all(r["info"]["stop"] in (1, 2) for r in solo)


# ---- 2. PSD members: the grouped decomposition, the gather, the fused apply -----------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("solver", [IND, DEN], ids=["ind", "den"])
def test_sdp_group_has_the_solo_bits(normalize, solver):
    members = [solved("sdp", seed, normalize, solver) for seed in SDP_SEEDS]
    check_group(members, plan=[0] * 5)


# ---- 3. a long SOC: the block bodies -----------------------------------------------------------------------------------------------------
def test_long_soc_group_has_the_solo_bits():
    members = [solved("long", seed) for seed in LONG_SEEDS]
    check_group(members, plan=[0, 0], tol=1e-10)


# ---- 4. members that finish at different iterations, and the cap ------------------------------------------------------------------------
def test_members_finish_apart_and_the_cap():
    members = [solved("qp", seed) for seed in QP_SEEDS]
    svs = [sv for sv, _ in members]
    g = [cot(p, 100 + i) for i, (_, p) in enumerate(members)]
    iters = [sv.adjoint(dx=gi[0], dy=gi[1], ds=gi[2], tol=TOL)["info"]["iters"] for sv, gi in zip(svs, g)]
    print("solo LSQR iterations:", iters)
    assert len(set(iters)) >= 2, iters
    cap = int(np.median(iters))
    solo = check_group(members, max_iters=cap)
    stops = [r["info"]["stop"] for r in solo]
    print("stops at max_iters = %d:" % cap, stops)
    assert 3 in stops and any(s in (1, 2) for s in stops), stops


# ---- 5. a mixed batch --------------------------------------------------------------------------------------------------------------------
def test_mixed_batch_keeps_the_callers_order():
    members = [solved("qp", 13), solved("sdp", 41), solved("qp", 14), solved("sdp33", 71), solved("sdp", 42), solved("qp", 15)]
    check_group(members, plan=[0, 1, 0, -1, 1, 0])


# ---- 6. the launch count does not depend on K ------------------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_K():
    copies = [fresh("qp", 13) for _ in range(6)]
    gx, gy, gs = cot(copies[0][1], 7)
    deltas, iters = [], []
    for K in (2, 6):
        svs = [sv for sv, _ in copies[:K]]
        assert scs.diff_batch_plan(svs) == [0] * K
        before = scs.diff_group_launches()
        res = scs.adjoint_batch(svs, [gx] * K, [gy] * K, [gs] * K, tol=TOL)
        deltas.append(scs.diff_group_launches() - before)
        iters.append([r["info"]["iters"] for r in res])
    print("grouped launches for K = 2, 6:", deltas, "iterations:", iters)
    assert len(set(iters[0] + iters[1])) == 1
    assert deltas[0] == deltas[1] and deltas[0] > 0, deltas
    # a member served alone issues no grouped launch
    before = scs.diff_group_launches()
    scs.adjoint_batch([copies[0][0]], [gx], [gy], [gs], tol=TOL)
    assert scs.diff_group_launches() == before


# ---- 7. clones ---------------------------------------------------------------------------------------------------------------------------
def many_solved(K, seed=13):
    p = make_qp(seed)
    rng = np.random.default_rng(seed)
    m, n = p["A"].shape
    B = p["b"][None, :] + 0.01 * rng.standard_normal((K, m)) * np.r_[np.zeros(2), np.ones(m - 2)]  # (the zero rows' b as it is)
    Cc = p["c"][None, :] + 0.01 * rng.standard_normal((K, n))
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    res = sv.solve_many(b=B, c=Cc)
    assert all(r["info"]["status"] == "solved" for r in res)
    return sv, p, B, Cc


def test_adjoint_many_over_clones():
    K = 4
    sv, p, _, _ = many_solved(K)
    m, n = p["A"].shape
    rng = np.random.default_rng(3)
    GX, GY, GS = rng.standard_normal((K, n)), rng.standard_normal((K, m)), rng.standard_normal((K, m))
    raw = [sv._solver] + sv._solver._many
    assert len(raw) == K
    solo = [r.adjoint(dx=GX[i], dy=GY[i], ds=GS[i], want=ALL, tol=TOL) for i, r in enumerate(raw)]
    got = sv.adjoint_many(GX, GY, GS, want=ALL, tol=TOL)
    for a, b in zip(got, solo):
        same_bits(a, b)
    on_dev = sv.adjoint_many_device(dev(GX), dev(GY), dev(GS), want=ALL, tol=TOL)
    for k in ("db", "dc", "dA", "dP"):
        assert on_dev[k].shape[0] == K
    for i in range(K):
        same_bits({"db": on_dev["db"][i], "dc": on_dev["dc"][i], "dA": on_dev["dA"][i], "dP": on_dev["dP"][i], "info": on_dev["info"][i]}, solo[i])
    solo_f = [r.derivative(db=GY[i], dc=GX[i], tol=TOL) for i, r in enumerate(raw)]
    for a, b in zip(sv.derivative_many(GY, GX, tol=TOL), solo_f):
        same_bits(a, b)
    fdev = sv.derivative_many_device(dev(GY), dev(GX), tol=TOL)
    for i in range(K):
        same_bits({"dx": fdev["dx"][i], "dy": fdev["dy"][i], "ds": fdev["ds"][i], "info": fdev["info"][i]}, solo_f[i])
    with pytest.raises(ValueError, match="solved 4 members"):
        sv.adjoint_many(np.zeros((K + 1, n)))


# ---- 8. nothing a solve reads is written -------------------------------------------------------------------------------------------------
def test_a_grouped_adjoint_leaves_the_next_solve_alone():
    seeds = QP_SEEDS[:3]
    a = [fresh("qp", seed) for seed in seeds] + [fresh("sdp", 41), fresh("sdp", 42)]
    b = [fresh("qp", seed) for seed in seeds] + [fresh("sdp", 41), fresh("sdp", 42)]
    g = [cot(p, 9) for _, p in a]
    res = scs.adjoint_batch([sv for sv, _ in a], [x[0] for x in g], [x[1] for x in g], [x[2] for x in g], want=ALL, tol=TOL)
    assert scs.diff_batch_plan([sv for sv, _ in a]) == [0, 0, 0, 1, 1] and all(r["info"]["iters"] > 0 for r in res)
    for (sa, _), (sb, _) in zip(a, b):
        ra, rb = sa.solve(warm_start=True), sb.solve(warm_start=True)
        assert ra["info"]["iter"] == rb["info"]["iter"]
        for k in ("x", "y", "s"):
            assert np.array_equal(ra[k], rb[k]), k


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_member_and_leave_every_workspace_usable():
    members = [fresh("qp", seed) for seed in QP_SEEDS[:4]]
    svs = [sv for sv, _ in members]
    g = [cot(p, 21) for _, p in members]
    args = lambda idx: ([svs[i] for i in idx], [g[i][0] for i in idx], [g[i][1] for i in idx], [g[i][2] for i in idx])

    def all_still_solve():
        for sv in svs:
            assert sv.solve(warm_start=False)["info"]["status"] == "solved"
        good = [0, 1, 3]
        solo = [svs[i].adjoint(dx=g[i][0], dy=g[i][1], ds=g[i][2], tol=TOL) for i in good]
        for x, y in zip(scs.adjoint_batch(*args(good), tol=TOL), solo):
            same_bits(x, y)

    svs[2].update(b=members[2][1]["b"].copy())
    with pytest.raises(ValueError, match=r"member 2.*stale"):
        scs.adjoint_batch(*args(range(4)), tol=TOL)
    with pytest.raises(ValueError, match=r"member 2.*stale"):
        scs.derivative_batch(svs, tol=TOL)
    all_still_solve()
    # a cone without a derivative is named, with its member
    Ke = {"l": 2, "ep": 1}
    de, _, _ = pg.gen_feasible(Ke, 3, 2, 5, lambda z, K: _scs_hip.proj_cone(z, K, dual=True))
    ex = scs.SCS(de, Ke, linear_solver=IND, **dict(STG, eps_abs=1e-7, eps_rel=1e-7))
    assert ex.solve(warm_start=False)["info"]["status"] == "solved"
    with pytest.raises(ValueError, match=r"member 1.*exponential \(ep\) cone"):
        scs.adjoint_batch([svs[0], ex, svs[1]], tol=TOL)
    assert ex.solve(warm_start=False)["info"]["status"] == "solved"
    all_still_solve()
    with pytest.raises(ValueError, match="twice"):
        scs.adjoint_batch([svs[0], svs[1], svs[0]], tol=TOL)
    all_still_solve()


# ---- 10. the pool ------------------------------------------------------------------------------------------------------------------------
def test_repeated_calls_take_their_blocks_from_the_pool():
    K = 4
    sv, p, _, _ = many_solved(K, seed=14)
    m, n = p["A"].shape
    GX = dev(np.random.default_rng(1).standard_normal((K, n)))
    sv.adjoint_many_device(GX, tol=TOL)
    sv.adjoint_many_device(GX, tol=TOL)
    torch.cuda.synchronize()
    before = _scs_hip.pool_stats()["misses"]
    sv.adjoint_many_device(GX, tol=TOL)
    assert _scs_hip.pool_stats()["misses"] == before


# ---- 11. the torch layer -----------------------------------------------------------------------------------------------------------------
def test_autograd_solve_many():
    import scs.autograd
    K = 3
    p = make_qp(13)
    m, n = p["A"].shape
    rng = np.random.default_rng(5)
    B0 = p["b"][None, :] + 0.01 * rng.standard_normal((K, m)) * np.r_[np.zeros(2), np.ones(m - 2)]
    C0 = p["c"][None, :] + 0.01 * rng.standard_normal((K, n))
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    sv.autograd_tol = 1e-11
    B, Cc = dev(B0).requires_grad_(True), dev(C0).requires_grad_(True)
    X, Y, S = scs.autograd.solve_many(sv, B, Cc)
    assert X.shape == (K, n) and Y.shape == (K, m) and S.shape == (K, m)
    assert all(i["status"] == "solved" for i in sv.autograd_info)
    GX, GY, GS = dev(rng.standard_normal((K, n))), dev(rng.standard_normal((K, m))), dev(rng.standard_normal((K, m)))
    ((X * GX).sum() + (Y * GY).sum() + (S * GS).sum()).backward()
    direct = sv.adjoint_many_device(GX, GY, GS, tol=1e-11)
    assert torch.equal(B.grad, direct["db"]) and torch.equal(Cc.grad, direct["dc"])
    assert torch.isfinite(B.grad).all() and B.grad.abs().max() > 0
    B2 = (B.detach() * 1.0001).requires_grad_(True)
    X2, _, _ = scs.autograd.solve_many(sv, B2, Cc)
    with pytest.raises(RuntimeError, match="solved again"):
        (X * GX).sum().backward()
    X2.sum().backward()
    assert B2.grad is not None and torch.isfinite(B2.grad).all()
