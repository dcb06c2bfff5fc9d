"""K directions at ONE solution (SCS.adjoint_multi / derivative_multi, include/scs_hip.h: scs_hip_adjoint_multi): every direction has the
bits — outputs and info apart from time_ms — of the solver's own adjoint / derivative on that direction alone, whatever the tile of
lanes it rides in (csrc/spmv_lanes.hpp), whichever lanes leave the tile before it, and on the fallback path too.

Problems come from tests/adjoint_ref.py, tests/dproj_cones_ref.py and tests/adjoint_psd_ref.py; solves use the settings of
tests/test_adjoint_cones_gpu.py."""
import ctypes as C
import gc

import numpy as np
import pytest

import torch

import adjoint_ref as ar
import adjoint_psd_ref as apr
import dproj_cones_ref as dr

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

IND, DEN = scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE
STG = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=False, max_iters=100000)
WANT = ("b", "c", "A", "P")
KS = (1, 7, 8, 9, 17)  # 7, 8, 9: a partial lane tile, a full one and one over it
KMAX = max(KS)


def problem_long_rows():
    """a vertex LP as adjoint_ref.problem_lp, n = 4 and 2100 dense inequality rows: every row of A' holds 2100 > kNnzPerWg = 2048
    nonzeros, a row block of its own that takes the long-row branch of the product"""
    return ar.gen_problem(21, n=4, z=0, l=2100, tight_l=4)


def problem_sdp33():
    """one PSD block of order 33 > kDprojPsdFusedMax = 32: the five-launch tile apply, which the lock-step path does not cover.
    Rank 30: 1 zero row + 2 tight rows + 3 * 4 / 2 = 9 <= n, P positive definite."""
    return apr.gen_problem(44, n=20, z=1, l=4, tight_l=2, s=(33,), ranks=(30,), with_P=True)


PROBLEMS = {"lp": ar.PROBLEMS["lp"], "qp": ar.PROBLEMS["qp"], "qp_soc": ar.PROBLEMS["qp_soc"], "box_qp": dr.PROBLEMS["box_qp"],
            "pow": dr.PROBLEMS["pow"], "lp_sdp": apr.PROBLEMS["lp_sdp"], "long_rows": problem_long_rows, "sdp33": problem_sdp33}
_problems, _solved, _solo = {}, {}, {}


def in_use():
    st = _scs_hip.pool_stats()
    return st["live_bytes"] - st["held_bytes"]


@pytest.fixture(scope="module", autouse=True)
def _finish_cached_solvers():
    """the solvers this module solves once and shares are finished with it (the block pool's account is an invariant of
    tests/test_pool_lifecycle_gpu.py)"""
    before = in_use()
    yield
    _solved.clear()
    _solo.clear()
    gc.collect()
    assert in_use() <= before, (in_use(), before)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def problem(name):
    if name not in _problems:
        _problems[name] = PROBLEMS[name]()
    return _problems[name]


def want_of(p):
    return WANT if p["P"] is not None else WANT[:3]


def solved(name, normalize=True, solver=IND):
    key = (name, normalize, solver)
    if key not in _solved:
        p = problem(name)
        sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=solver, normalize=normalize, **STG)
        sol = sv.solve(warm_start=False)
        assert sol["info"]["status"] == "solved", sol["info"]
        _solved[key] = (sv, p)
    return _solved[key]


def direction_set(p, count=KMAX, seed=3):
    """(GX, GY, GS) with `count` rows: row 0 random, row 1 ZERO (its LSQR stops at once), row 2 a DUPLICATE of row 0, then directions of
    different kinds — one cotangent only, unit vectors, scaled ones — so their LSQR iteration counts differ.  A shorter set is a prefix of
    a longer one (up to KMAX rows)."""
    rng = np.random.default_rng(seed)
    m, n = p["A"].shape
    total = max(count, KMAX)
    GX, GY, GS = rng.standard_normal((total, n)), rng.standard_normal((total, m)), rng.standard_normal((total, m))
    GX, GY, GS = GX[:count].copy(), GY[:count].copy(), GS[:count].copy()
    for k in range(count):
        if k == 1:
            GX[k] = GY[k] = GS[k] = 0.0
        elif k == 2:
            GX[k], GY[k], GS[k] = GX[0], GY[0], GS[0]
        elif k % 4 == 3:  # dL/dx alone, a unit vector
            GX[k] = 0.0
            GX[k, k % n] = 1.0
            GY[k] = GS[k] = 0.0
        elif k % 4 == 0 and k > 0:  # dL/ds alone
            GX[k] = GY[k] = 0.0
        elif k % 4 == 1:  # dL/dy alone, scaled
            GX[k] = GS[k] = 0.0
            GY[k] *= 1e3
    return GX, GY, GS


def strip(info):
    return {k: v for k, v in info.items() if k != "time_ms"}


def solo(name, normalize=True, solver=IND, count=KMAX):
    """the solver's own adjoint and derivative on every direction of the set, one call each: computed once per solver and shared"""
    key = (name, normalize, solver)
    if key not in _solo or len(_solo[key][0]) < count:
        sv, p = solved(name, normalize, solver)
        GX, GY, GS = direction_set(p, count)
        adj = [sv.adjoint(dx=GX[k], dy=GY[k], ds=GS[k], want=want_of(p)) for k in range(count)]
        fwd = [sv.derivative(db=GY[k], dc=GX[k]) for k in range(count)]
        _solo[key] = (adj, fwd)
    return _solo[key]


def assert_rows_equal_solo(res, ref_rows, keys, what):
    """row k of every (K, .) output and info k equal the solo call's, bit for bit"""
    K = len(ref_rows)
    assert len(res["info"]) == K, what
    for key in keys:
        got = res[key].cpu().numpy() if isinstance(res[key], torch.Tensor) else res[key]
        assert got.shape == (K,) + ref_rows[0][key].shape, (what, key, got.shape)
        for k in range(K):
            assert np.array_equal(got[k], ref_rows[k][key]), (what, key, k, np.abs(got[k] - ref_rows[k][key]).max())
    for k in range(K):
        assert strip(res["info"][k]) == strip(ref_rows[k]["info"]), (what, k, res["info"][k], ref_rows[k]["info"])


def check_solo_bits(name, normalize, solver, Ks, device_twins=True):
    sv, p = solved(name, normalize, solver)
    adj, fwd = solo(name, normalize, solver, max(Ks))
    GX, GY, GS = direction_set(p, max(Ks))
    want = want_of(p)
    akeys, fkeys = ["d" + k for k in want], ["dx", "dy", "ds"]
    print("%s normalize=%s %s: solo LSQR iterations, adjoint %s, derivative %s" % (
        name, normalize, solver.name, [r["info"]["iters"] for r in adj], [r["info"]["iters"] for r in fwd]))
    if max(Ks) >= 3:
        assert len(set(r["info"]["iters"] for r in adj[:max(Ks)])) >= 2  # (the zero direction at least leaves early)
        assert adj[1]["info"]["iters"] <= 1 and not adj[1]["db"].any()
    for K in Ks:
        what = "%s normalize=%s %s K=%d" % (name, normalize, solver.name, K)
        am = sv.adjoint_multi(dx=GX[:K], dy=GY[:K], ds=GS[:K], want=want)
        assert_rows_equal_solo(am, adj[:K], akeys, what + " adjoint_multi")
        fm = sv.derivative_multi(db=GY[:K], dc=GX[:K])
        assert_rows_equal_solo(fm, fwd[:K], fkeys, what + " derivative_multi")
        if device_twins:
            amd = sv.adjoint_multi_device(dx=dev(GX[:K]), dy=dev(GY[:K]), ds=dev(GS[:K]), want=want)
            assert all(isinstance(amd[k], torch.Tensor) and amd[k].is_cuda for k in akeys)
            assert_rows_equal_solo(amd, adj[:K], akeys, what + " adjoint_multi_device")
            fmd = sv.derivative_multi_device(db=dev(GY[:K]), dc=dev(GX[:K]))
            assert_rows_equal_solo(fmd, fwd[:K], fkeys, what + " derivative_multi_device")


# ---- 1. solo bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [IND, DEN], ids=["indirect", "dense"])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("name", ["lp", "qp", "qp_soc", "box_qp", "pow", "lp_sdp"])
def test_every_direction_has_the_bits_of_a_call_of_its_own(name, normalize, solver):
    check_solo_bits(name, normalize, solver, KS)


# ---- 2. permutation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp_soc", "lp_sdp"])
def test_permuting_the_directions_permutes_the_outputs(name):
    sv, p = solved(name)
    K = 9
    GX, GY, GS = direction_set(p, K)
    perm = np.random.default_rng(7).permutation(K)
    assert not np.array_equal(perm, np.arange(K))
    want = want_of(p)
    a0 = sv.adjoint_multi(dx=GX, dy=GY, ds=GS, want=want)
    a1 = sv.adjoint_multi(dx=GX[perm], dy=GY[perm], ds=GS[perm], want=want)
    for key in ["d" + k for k in want]:
        assert np.array_equal(a0[key][perm], a1[key]), key
    assert [strip(a0["info"][i]) for i in perm] == [strip(i) for i in a1["info"]]
    f0 = sv.derivative_multi(db=GY, dc=GX)
    f1 = sv.derivative_multi(db=GY[perm], dc=GX[perm])
    for key in ("dx", "dy", "ds"):
        assert np.array_equal(f0[key][perm], f1[key]), key
    assert [strip(f0["info"][i]) for i in perm] == [strip(i) for i in f1["info"]]


# ---- 3. long rows -----------------------------------------------------------------------------------------------------------------------
def test_rows_longer_than_a_row_block_keep_solo_bits():
    p = problem("long_rows")
    assert p["A"].shape == (2100, 4) and p["A"].nnz == 2100 * 4  # every row of A' is one long-row block
    check_solo_bits("long_rows", True, IND, (3, 9), device_twins=False)


# ---- 4. one launch per kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp_soc", "lp_sdp"])
def test_eight_lanes_cost_the_launches_of_one(name):
    sv, p = solved(name)
    GX, GY, GS = direction_set(p, 1)

    def launches(K):
        before = _scs_hip.diff_group_launches()
        res = sv.adjoint_multi(dx=np.repeat(GX, K, axis=0), dy=np.repeat(GY, K, axis=0), ds=np.repeat(GS, K, axis=0))
        return _scs_hip.diff_group_launches() - before, res

    one, r1 = launches(1)
    eight, r8 = launches(8)
    print("%s: grouped launches K=1 %d, K=8 %d, LSQR iterations %d" % (name, one, eight, r1["info"][0]["iters"]))
    assert one > 0 and eight == one
    for k in range(8):
        assert np.array_equal(r8["db"][k], r1["db"][0]) and strip(r8["info"][k]) == strip(r1["info"][0])


# ---- 5. fallback ------------------------------------------------------------------------------------------------------------------------
def test_a_workspace_outside_the_lock_step_path_is_served_in_turn_with_the_same_bits():
    before = _scs_hip.diff_group_launches()
    check_solo_bits("sdp33", True, IND, (3,), device_twins=False)
    assert _scs_hip.diff_group_launches() == before  # nothing went through the grouped tables


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["qp_soc", "box_qp", "lp_sdp"])
def test_multi_calls_leave_the_solver_and_the_pool_as_they_were(name):
    p = problem(name)
    K = 9
    GX, GY, GS = direction_set(p, K)
    base = in_use()
    stg = dict(STG, eps_abs=1e-7, eps_rel=1e-7)
    a, twin = (scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **stg) for _ in range(2))
    sa, st = a.solve(warm_start=False), twin.solve(warm_start=False)
    assert sa["info"]["status"] == "solved" and np.array_equal(sa["x"], st["x"])
    want = want_of(p)
    first = a.adjoint(dx=GX[0], dy=GY[0], ds=GS[0], want=want)
    am = a.adjoint_multi(dx=GX, dy=GY, ds=GS, want=want)
    fm = a.derivative_multi(db=GY, dc=GX)
    assert len(am["info"]) == K and len(fm["info"]) == K
    later = a.adjoint(dx=GX[0], dy=GY[0], ds=GS[0], want=want)
    for key in ["d" + k for k in want]:
        assert np.array_equal(first[key], later[key]) and np.array_equal(first[key], am[key][0]), key
    assert strip(first["info"]) == strip(later["info"])
    b2 = p["b"] * 1.01
    for sv in (a, twin):
        sv.update_device(b=dev(b2))
    ra, rt = a.solve_device(warm_start=True), twin.solve_device(warm_start=True)
    for key in ("x", "y", "s"):
        assert torch.equal(ra[key], rt[key]), key
    assert ra["info"]["iter"] == rt["info"]["iter"] and ra["info"]["cg_iters"] == rt["info"]["cg_iters"]
    del a, twin, sv, ra, rt
    gc.collect()
    assert in_use() == base, (in_use(), base)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_workspace_that_still_solves():
    p = problem("qp_soc")
    m, n = p["A"].shape
    K = 3
    GX, GY, GS = direction_set(p, K)
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    for call in (lambda: sv.adjoint_multi(dx=GX), lambda: sv.derivative_multi(dc=GX), lambda: sv.jacobian()):
        with pytest.raises(ValueError, match="no solve yet"):
            call()
    first = sv.solve(warm_start=False)
    assert first["info"]["status"] == "solved"
    ok = sv.adjoint_multi(dx=GX, dy=GY, ds=GS)
    sv.update(b=p["b"] * 1.01)
    for call in (lambda: sv.adjoint_multi(dx=GX), lambda: sv.derivative_multi(db=GY), lambda: sv.jacobian(rows=[0])):
        with pytest.raises(ValueError, match="stale"):
            call()
    sv.update(b=p["b"])
    again = sv.solve(warm_start=False)
    assert again["info"]["status"] == "solved"
    with pytest.raises(ValueError, match="incompatible dimension"):
        sv.adjoint_multi(dx=np.ones((K, n + 1)))
    with pytest.raises(ValueError, match="incompatible dimension"):
        sv.derivative_multi(db=np.ones((K, m - 1)))
    with pytest.raises(ValueError, match="2-D"):
        sv.adjoint_multi(dx=np.ones(n))
    with pytest.raises(ValueError, match="dy holds 2 directions where the arguments before it hold 3"):
        sv.adjoint_multi(dx=GX, dy=GY[:2])
    with pytest.raises(ValueError, match="dc holds 2 directions"):
        sv.derivative_multi(db=GY, dc=GX[:2])
    with pytest.raises(ValueError, match="no direction given"):
        sv.adjoint_multi()
    with pytest.raises(ValueError, match="no direction given"):
        sv.derivative_multi()
    with pytest.raises(ValueError, match="no direction given"):
        sv.adjoint_multi_device()
    with pytest.raises(ValueError, match="of must be"):
        sv.jacobian(of="z")
    with pytest.raises(ValueError, match="wrt must be"):
        sv.jacobian(wrt="A")
    # through the C entry: K = 0 and K = 33
    raw = sv._solver
    lib = _scs_hip._lib
    big = np.zeros((33, max(m, n)))
    opts = _scs_hip._ScsHipDiffOpts(1e-8, 0)
    infos = (_scs_hip._ScsHipDiffInfo * 33)()
    for k_bad, text in ((0, "K = 0"), (33, "limit of 32")):
        out = np.full((33, m), 7.0)
        assert lib.scs_hip_adjoint_multi(raw._work, k_bad, big.ctypes.data, None, None, out.ctypes.data, None, None, None, C.byref(opts), infos) == -1
        assert text in _scs_hip.last_error(), _scs_hip.last_error()
        assert lib.scs_hip_derivative_multi(raw._work, k_bad, big.ctypes.data, None, out.ctypes.data, None, None, C.byref(opts), infos) == -1
        assert text in _scs_hip.last_error(), _scs_hip.last_error()
        assert (out == 7.0).all()
    after = sv.adjoint_multi(dx=GX, dy=GY, ds=GS)
    for key in ("db", "dc"):
        assert np.array_equal(ok[key], after[key]), key
    last = sv.solve(warm_start=False)
    assert last["info"]["status"] == "solved" and np.array_equal(last["x"], again["x"])


def test_the_exponential_cone_is_refused_by_name_and_the_workspace_still_solves():
    from scipy import sparse
    K = {"l": 2, "ep": 1}
    rng = np.random.default_rng(5)
    m, n = 5, 3
    s0 = _scs_hip.proj_cone(rng.standard_normal(m), K, dual=False)
    A = sparse.csc_matrix(rng.standard_normal((m, n)))
    data = {"P": sparse.identity(n, format="csc"), "A": A, "b": A @ rng.standard_normal(n) + s0, "c": rng.standard_normal(n)}
    sv = scs.SCS(data, K, linear_solver=IND, **dict(STG, eps_abs=1e-7, eps_rel=1e-7))
    first = sv.solve(warm_start=False)
    assert first["info"]["status"] == "solved", first["info"]
    for call in (lambda: sv.adjoint_multi(dx=np.ones((2, n))), lambda: sv.derivative_multi(db=np.ones((2, m))), lambda: sv.jacobian()):
        with pytest.raises(ValueError, match=r"exponential \(ep\) cone"):
            call()
    again = sv.solve(warm_start=False)
    assert again["info"]["status"] == "solved"
    assert np.abs(again["x"] - first["x"]).max() <= 1e-4 * max(1.0, np.abs(first["x"]).max())


# ---- 8. chunking ------------------------------------------------------------------------------------------------------------------------
def test_forty_directions_are_served_in_chunks_with_solo_bits():
    sv, p = solved("lp")
    K = 40
    GX, GY, GS = direction_set(p, K, seed=8)
    want = want_of(p)
    am = sv.adjoint_multi(dx=GX, dy=GY, ds=GS, want=want)
    fm = sv.derivative_multi(db=GY, dc=GX)
    amd = sv.adjoint_multi_device(dx=dev(GX), dy=dev(GY), ds=dev(GS), want=want)
    assert am["db"].shape == (K, p["A"].shape[0]) and len(am["info"]) == K and len(fm["info"]) == K
    for k in (0, 31, 32, 39):
        one = sv.adjoint(dx=GX[k], dy=GY[k], ds=GS[k], want=want)
        for key in ["d" + w for w in want]:
            assert np.array_equal(am[key][k], one[key]), (key, k)
            assert np.array_equal(amd[key][k].cpu().numpy(), one[key]), (key, k)
        assert strip(am["info"][k]) == strip(one["info"]) == strip(amd["info"][k]), k
        fone = sv.derivative(db=GY[k], dc=GX[k])
        for key in ("dx", "dy", "ds"):
            assert np.array_equal(fm[key][k], fone[key]), (key, k)
        assert strip(fm["info"][k]) == strip(fone["info"]), k
