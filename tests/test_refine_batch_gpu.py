"""scs.refine_batch / SCS.refine_many / the layer's polish (csrc/refine_batch.hpp): a batch refined in lock step against the solo
`refine` of every member.

The contract is bit identity, so the reference is `SCS.refine` itself, run on TWIN solvers: built from the same data and solved the
same way (solves are deterministic).  Members of one shape are one generated problem (the generators of tests/test_refine_gpu.py,
n between 10 and 20) whose b and c are moved by a seeded relative 1e-2, solved at eps 1e-4: their Newton trajectories differ.
Results are compared with np.array_equal, infos without time_ms (the group's).  The one bound is that of tests/test_refine_gpu.py:
the stop rule recomputed in numpy holds at 10 tol."""
import ctypes as C
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
TIGHT = dict(LOOSE, eps_abs=1e-9, eps_rel=1e-9)
TOL = 1e-10
MOVE = 1e-2
G = 4
GENERATORS = {}
for _mod in (ar, dr, pr):
    for _name, _gen in _mod.PROBLEMS.items():
        GENERATORS[_name] = (_mod, _gen)
NAMES = sorted(GENERATORS)
CASES = [(name, normalize, solver) for name in NAMES for normalize in (True, False) for solver in (IND, DEN)]
CASE_IDS = ["%s-%s-%s" % (name, "normalized" if nz else "raw", "indirect" if sv == IND else "dense") for name, nz, sv in CASES]
_problems = {}


@pytest.fixture(scope="module", autouse=True)
def _pool_account():
    """8. every solver of this module is finished with it: live-minus-held bytes of the block pool are not above their value before
    (the invariant of tests/test_pool_lifecycle_gpu.py), the groups' tables, lists and borrowed scratch included"""
    def in_use():
        st = _scs_hip.pool_stats()
        return st["live_bytes"] - st["held_bytes"]
    gc.collect()
    before = in_use()
    yield
    gc.collect()
    assert in_use() <= before, (in_use(), before)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def problem(name):
    if name not in _problems:
        mod, gen = GENERATORS[name]
        _problems[name] = (mod, gen())
    return _problems[name]


def member_problem(name, i):
    """member i of the shape `name`: the generated problem with b and c moved by a seeded relative MOVE (member 0 included)"""
    mod, p = problem(name)
    rng = np.random.default_rng(1000 * NAMES.index(name) + i)
    q = dict(p)
    q["b"] = p["b"] * (1.0 + MOVE * rng.standard_normal(p["b"].shape[0]))
    q["c"] = p["c"] * (1.0 + MOVE * rng.standard_normal(p["c"].shape[0]))
    return q


def solved(p, normalize=True, solver=IND, stg=LOOSE):
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=solver, normalize=normalize, **stg)
    sol = sv.solve(warm_start=False)
    assert sol["info"]["status"] == "solved", sol["info"]
    return sv


def group(name, count=G, normalize=True, solver=IND):
    """(problems, solvers): `count` solved members of one shape"""
    ps = [member_problem(name, i) for i in range(count)]
    return ps, [solved(p, normalize, solver) for p in ps]


def without_time(info):
    return {k: v for k, v in info.items() if k != "time_ms"}


def same_bits(got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for key in ref:
        if key == "info":
            assert without_time(got[key]) == without_time(ref[key]), (got[key], ref[key])
        else:
            a = got[key].cpu().numpy() if isinstance(got[key], torch.Tensor) else got[key]
            b = ref[key].cpu().numpy() if isinstance(ref[key], torch.Tensor) else ref[key]
            assert a.shape == b.shape and np.array_equal(a, b), key


def cot(sv, seed):
    rng = np.random.default_rng(seed)
    n, m = sv._solver.n, sv._solver.m
    return rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)


# ---- 1. bit identity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,normalize,solver", CASES, ids=CASE_IDS)
def test_every_member_has_the_bits_of_its_own_refine(name, normalize, solver):
    ps, members = group(name, G, normalize, solver)
    _, twins = group(name, G, normalize, solver)
    _, third = group(name, G, normalize, solver)
    assert scs.diff_batch_plan(members) == [0] * G  # (the members do share their launches)
    before = scs.diff_group_launches()
    got = scs.refine_batch(members, tol=TOL)
    assert scs.diff_group_launches() > before
    solo = [sv.refine(tol=TOL) for sv in twins]
    on_device = scs.refine_batch_device(third, tol=TOL)
    assert len(got) == len(on_device) == G
    print("%s normalize=%s %s: steps %s halvings %s lsqr_iters %s" % (name, normalize, solver.name, [r["info"]["steps"] for r in got],
                                                                     [r["info"]["halvings"] for r in got], [r["info"]["lsqr_iters"] for r in got]))
    for p, a, b, d in zip(ps, got, solo, on_device):
        same_bits(a, b)
        same_bits(d, b)
        assert a["info"]["stop"] == 1, a["info"]
        rec = rr.residuals(p, a["x"], a["y"], a["s"])
        print("  recomputed %s" % (rec,))
        assert rr.meets(rec, 10 * TOL), rec
    # ... and what is resident afterwards is the polished point: the members differentiate like their twins
    gs = [cot(sv, 50 + i) for i, sv in enumerate(members)]
    batch = scs.adjoint_batch(members, [g[0] for g in gs], [g[1] for g in gs], [g[2] for g in gs])
    for sv, g, r in zip(twins, gs, batch):
        same_bits(r, sv.adjoint(dx=g[0], dy=g[1], ds=g[2]))


# ---- 2. divergent members in one group ---------------------------------------------------------------------------------------------------
def divergent(name="qp_soc"):
    """member 0 solved at eps 1e-9, members 1 .. 3 at 1e-4: (problems, solvers, the solutions `solve` returned)"""
    ps = [member_problem(name, i) for i in range(G)]
    svs, sols = [], []
    for i, p in enumerate(ps):
        sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **(TIGHT if i == 0 else LOOSE))
        sol = sv.solve(warm_start=False)
        assert sol["info"]["status"] == "solved", sol["info"]
        svs.append(sv)
        sols.append(sol)
    return ps, svs, sols


@pytest.mark.parametrize("name", ["qp_soc", "mixed"])
def test_members_of_one_group_go_their_own_ways(name):
    # (a) one member has nothing to do
    _, members, sols = divergent(name)
    _, twins, _ = divergent(name)
    assert scs.diff_batch_plan(members) == [0] * G
    got = scs.refine_batch(members, tol=1e-6)
    steps = [r["info"]["steps"] for r in got]
    print("%s (a) tol 1e-6: steps %s stops %s" % (name, steps, [r["info"]["stop"] for r in got]))
    assert got[0]["info"]["steps"] == 0 and got[0]["info"]["stop"] == 1 and got[0]["info"]["lsqr_iters"] == 0, got[0]["info"]
    for key in ("x", "y", "s"):
        assert np.array_equal(got[0][key], sols[0][key]), key
    assert len(set(steps)) >= 2, steps  # (else the inputs are wrong: nothing diverged)
    for a, sv in zip(got, twins):
        same_bits(a, sv.refine(tol=1e-6))
    # (b) one step each, then the cap
    _, members, _ = divergent(name)
    _, twins, _ = divergent(name)
    got = scs.refine_batch(members, tol=1e-13, max_steps=1)
    print("%s (b) tol 1e-13, max_steps 1: stops %s" % (name, [r["info"]["stop"] for r in got]))
    for a in got[1:]:
        assert a["info"]["stop"] == 2 and a["info"]["steps"] == 1 and a["info"]["stop_reason"] == "max_steps", a["info"]
    for a, sv in zip(got, twins):
        same_bits(a, sv.refine(tol=1e-13, max_steps=1))
    # (c) the loose members to 1e-10 beside the tight one
    _, members, _ = divergent(name)
    _, twins, _ = divergent(name)
    got = scs.refine_batch(members, tol=TOL)
    print("%s (c) tol 1e-10: steps %s halvings %s stops %s" % (name, [r["info"]["steps"] for r in got], [r["info"]["halvings"] for r in got],
                                                              [r["info"]["stop"] for r in got]))
    for a in got[1:]:
        assert a["info"]["stop"] == 1 and a["info"]["steps"] >= 1, a["info"]
    assert len(set(r["info"]["steps"] for r in got)) >= 2, got  # (members that all step: some leave the stepping list before others)
    for a, sv in zip(got, twins):
        same_bits(a, sv.refine(tol=TOL))


# Starts far from the solution (solves at eps 0.1 .. 0.3) make the line search work: members of one group accept at different halving
# rounds, so the searching list is compacted inside a step, and on "lp" some run out of halvings (stop 3) beside members that converge.
# A stop of 3 could not be built from a start at eps 1e-4 (a capped LSQR solve still gives a descent direction at t = 1), and the test
# does not depend on one: it asks for different halving counts in the group — else its inputs are wrong — and for the twins' bits.
@pytest.mark.parametrize("name,eps", [("box_qp", 0.3), ("lp", 0.1), ("pow", 0.3)])
def test_members_halve_and_give_up_apart(name, eps):
    far = dict(LOOSE, eps_abs=eps, eps_rel=eps)
    ps = [member_problem(name, i) for i in range(G)]
    members, twins = ([solved(p, stg=far) for p in ps] for _ in range(2))
    assert scs.diff_batch_plan(members) == [0] * G
    got = scs.refine_batch(members, tol=TOL)
    halvings = [r["info"]["halvings"] for r in got]
    print("%s from eps %g: steps %s halvings %s stops %s" % (name, eps, [r["info"]["steps"] for r in got], halvings,
                                                           [r["info"]["stop"] for r in got]))
    assert len(set(halvings)) >= 2, halvings
    for a, sv in zip(got, twins):
        same_bits(a, sv.refine(tol=TOL))


# ---- 3. a mixed call ------------------------------------------------------------------------------------------------------------------------
def make_sdp40():  # a PSD block of order 40: above the fused apply (kDprojPsdFusedMax = 32), which the group does not take
    return pr.gen_problem(71, n=50, z=1, l=4, tight_l=2, s=(40,), ranks=(37,), with_P=True)


def mixed_call():
    ps = [member_problem("qp_soc", 0), member_problem("qp_sdp", 0), make_sdp40(), member_problem("qp_soc", 1), member_problem("qp_sdp", 1),
          member_problem("qp_soc", 2)]
    return ps, [solved(p) for p in ps]


def test_a_mixed_call_keeps_the_callers_order():
    ps, members = mixed_call()
    _, twins = mixed_call()
    assert scs.diff_batch_plan(members) == [0, 1, -1, 0, 1, 0]
    got = scs.refine_batch(members, tol=TOL)
    print("mixed call: steps %s stops %s" % ([r["info"]["steps"] for r in got], [r["info"]["stop"] for r in got]))
    for a, sv in zip(got, twins):
        same_bits(a, sv.refine(tol=TOL))
        assert a["info"]["steps"] >= 1


# ---- 4. the launch count does not grow with G ---------------------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_G():
    p = member_problem("mixed", 0)
    deltas = {}
    for count in (2, 8):
        copies = [solved(p) for _ in range(count)]
        before = scs.diff_group_launches()
        got = scs.refine_batch(copies, tol=TOL)
        deltas[count] = scs.diff_group_launches() - before
        for a in got[1:]:
            same_bits(a, got[0])
        assert got[0]["info"]["steps"] >= 1
    print("grouped launches of one refine_batch: %s" % (deltas,))
    assert deltas[2] == deltas[8] and deltas[2] > 0, deltas


# ---- 5. refine_many -------------------------------------------------------------------------------------------------------------------------
def many_rows(name, K):
    ps = [member_problem(name, i) for i in range(K)]
    return np.stack([p["b"] for p in ps]), np.stack([p["c"] for p in ps])


@pytest.mark.parametrize("name", ["qp_soc", "qp_sdp"])
def test_refine_many_is_refine_batch_over_the_members(name):
    K = 5
    mod, p = problem(name)
    m, n = p["A"].shape
    B, Cc = many_rows(name, K)
    sv, twin = (scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **LOOSE) for _ in range(2))
    for s in (sv, twin):
        assert all(r["info"]["status"] == "solved" for r in s.solve_many(b=B, c=Cc))
    got = sv.refine_many(tol=TOL)
    ref = _scs_hip.refine_batch(twin._solver._many_members(K), tol=TOL)
    assert got["x"].shape == (K, n) and got["y"].shape == got["s"].shape == (K, m) and len(got["info"]) == K
    for i in range(K):
        same_bits({k: got[k][i] for k in ("x", "y", "s", "info")}, ref[i])
        assert got["info"][i]["stop"] == 1
    rng = np.random.default_rng(3)
    GX, GY, GS = rng.standard_normal((K, n)), rng.standard_normal((K, m)), rng.standard_normal((K, m))
    after = sv.adjoint_many(GX, GY, GS)
    direct = _scs_hip.adjoint_batch(twin._solver._many_members(K), GX, GY, GS)
    for a, b in zip(after, direct):
        same_bits(a, b)
    # the device entry, and a warm-started solve_many from the polished points
    third = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **LOOSE)
    third.solve_many(b=B, c=Cc)
    on_device = third.refine_many_device(tol=TOL)
    for key in ("x", "y", "s"):
        assert np.array_equal(on_device[key].cpu().numpy(), got[key]), key
    assert [without_time(i) for i in on_device["info"]] == [without_time(i) for i in got["info"]]
    warm = sv.solve_many(b=B, c=Cc, warm_start=True)
    assert all(r["info"]["status"] == "solved" for r in warm)
    # K above what solve_many solved, and a solver nothing was solved on: the errors of the member list and of the library
    with pytest.raises(ValueError, match="7 rows, but solve_many has solved 5 members"):
        sv.refine_many(K=7)
    new = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **LOOSE)
    with pytest.raises(ValueError, match="3 rows, but solve_many has solved 1 member of this solver"):
        new.refine_many(K=3)
    with pytest.raises(ValueError, match="member 0.*no solve yet"):
        new.refine_many()


# ---- 6. the layer ---------------------------------------------------------------------------------------------------------------------------
def test_the_batched_layer_refines_when_asked():
    import scs.autograd
    name, K = "box_qp", 4
    mod, p = problem(name)
    B, Cc = many_rows(name, K)
    rng = np.random.default_rng(11)
    m, n = p["A"].shape
    GX, GY, GS = rng.standard_normal((K, n)), rng.standard_normal((K, m)), rng.standard_normal((K, m))
    new = lambda: scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **LOOSE)
    sv, twin = new(), new()
    sv.autograd_refine_tol = TOL
    Bt, Ct = dev(B).requires_grad_(True), dev(Cc).requires_grad_(True)
    X, Y, S = scs.autograd.solve_many(sv, Bt, Ct)
    twin.solve_many_device(b=dev(B), c=dev(Cc), warm_start=False)
    direct = twin.refine_many_device(tol=TOL)
    for got, key in ((X, "x"), (Y, "y"), (S, "s")):
        assert torch.equal(got.detach(), direct[key]), key
    assert [without_time(i) for i in sv.autograd_refine_info] == [without_time(i) for i in direct["info"]]
    assert all(i["stop"] == 1 for i in sv.autograd_refine_info) and all(i["status"] == "solved" for i in sv.autograd_info)
    ((X * dev(GX)).sum() + (Y * dev(GY)).sum() + (S * dev(GS)).sum()).backward()
    for i in range(K):  # row i: the solo layer with the same switch on a twin
        one = new()
        one.autograd_refine_tol = TOL
        b, c = dev(B[i]).requires_grad_(True), dev(Cc[i]).requires_grad_(True)
        x, y, s = scs.autograd.solve(one, b, c)
        assert torch.equal(x.detach(), X[i].detach()) and torch.equal(y.detach(), Y[i].detach()) and torch.equal(s.detach(), S[i].detach())
        (x @ dev(GX[i]) + y @ dev(GY[i]) + s @ dev(GS[i])).backward()
        assert torch.equal(b.grad, Bt.grad[i]) and torch.equal(c.grad, Ct.grad[i]), i
    # unset: the layer is the one it always was
    plain, twin = new(), new()
    assert getattr(plain, "autograd_refine_tol", None) is None
    Xp, Yp, Sp = scs.autograd.solve_many(plain, dev(B), dev(Cc))
    direct = twin.solve_many_device(b=dev(B), c=dev(Cc), warm_start=False)
    for got, key in ((Xp, "x"), (Yp, "y"), (Sp, "s")):
        assert torch.equal(got, direct[key]), key
    assert getattr(plain, "autograd_refine_info", None) is None


# ---- 7. refusals, and every workspace survives them ----------------------------------------------------------------------------------------
def feasible_qp(K, seed):
    """a strictly convex QP with a feasible point (as tests/test_refine_gpu.py): P = I, s0 = Pi_K(random), b = A x0 + s0"""
    rng = np.random.default_rng(seed)
    m = K.get("z", 0) + K.get("l", 0) + 3 * (K.get("ep", 0) + K.get("ed", 0))
    n = 3
    s0 = _scs_hip.proj_cone(rng.standard_normal(m), K, dual=False)
    A = sparse.csc_matrix(rng.standard_normal((m, n)))
    return {"P": sparse.identity(n, format="csc"), "A": A, "b": A @ rng.standard_normal(n) + s0, "c": rng.standard_normal(n)}


def test_refusals_name_the_member_and_leave_every_workspace_usable():
    ps, good = group("qp_soc", 3)
    gs = [cot(sv, 70 + i) for i, sv in enumerate(good)]
    resident = [sv.adjoint(dx=g[0], dy=g[1], ds=g[2]) for sv, g in zip(good, gs)]

    def still_resident():
        for sv, g, ref in zip(good, gs, resident):
            same_bits(sv.adjoint(dx=g[0], dy=g[1], ds=g[2]), ref)

    def refused(members, match, **kw):
        for call in (scs.refine_batch, scs.refine_batch_device):
            with pytest.raises(ValueError, match=match):
                call(members, **kw)
        still_resident()

    # a member never solved
    unsolved = scs.SCS(ar.data_of(ps[0]), ps[0]["cone"], linear_solver=IND, **LOOSE)
    refused([good[0], unsolved, good[1], good[2]], "libscs_hip: scs_hip_refine_batch.*member 1.*no solve yet")
    # a member whose solve did not end solved (the infeasible LP of tests/test_adjoint_gpu.py)
    bad = scs.SCS({"A": sparse.csc_matrix(np.array([[-1.0], [1.0]])), "b": np.array([-1.0, 0.0]), "c": np.array([1.0])}, {"l": 2},
                  linear_solver=IND, **LOOSE)
    assert bad.solve(warm_start=False)["info"]["status"] == "infeasible"
    refused([good[0], good[1], bad, good[2]], "member 2.*did not end solved")
    # a stale member
    stale = solved(ps[0])
    stale.update(b=ps[0]["b"].copy())
    refused([stale, good[0], good[1], good[2]], "member 0.*stale")
    # a cone without a derivative, by name
    K = {"l": 2, "ep": 1}
    ex = scs.SCS(feasible_qp(K, 5), K, linear_solver=IND, **LOOSE)
    assert ex.solve(warm_start=False)["info"]["status"] == "solved"
    refused([good[0], ex, good[1]], r"member 1.*exponential \(ep\) cone")
    # a duplicate member, an empty list
    refused([good[0], good[1], good[0]], "member 2.*appears twice")
    refused([], "member 0")
    # a NaN tol: Python refuses it by name, the library by member
    refused(good, "tol must be a positive finite number", tol=float("nan"))
    raw = [sv._solver for sv in good]
    works = (C.c_void_p * 3)(*[sv._work for sv in raw])
    opts = _scs_hip._ScsHipRefineOpts(float("nan"), 0, 0.0, 0)
    for fn in (_scs_hip._lib.scs_hip_refine_batch, _scs_hip._lib.scs_hip_refine_batch_device):
        assert fn(works, None, C.byref(opts), None, 3) == -1
        assert "member 0: tol is NaN" in _scs_hip.last_error(), _scs_hip.last_error()
        assert fn(works, None, None, None, 0) == -1 and "count must be positive" in _scs_hip.last_error()
        dup = (C.c_void_p * 3)(raw[0]._work, raw[1]._work, raw[0]._work)
        assert fn(dup, None, None, None, 3) == -1 and "member 2: a workspace appears twice" in _scs_hip.last_error()
        hole = (C.c_void_p * 3)(raw[0]._work, None, raw[2]._work)
        assert fn(hole, None, None, None, 3) == -1 and "member 1: null workspace" in _scs_hip.last_error()
    still_resident()
    # ... and a good call works, on the members and on those that were refused beside them
    _, twins = group("qp_soc", 3)
    for a, sv in zip(scs.refine_batch(good, tol=TOL), twins):
        same_bits(a, sv.refine(tol=TOL))
        assert a["info"]["stop"] == 1
    assert stale.solve(warm_start=False)["info"]["status"] == "solved" and unsolved.solve(warm_start=False)["info"]["status"] == "solved"
    assert all(r["info"]["stop"] == 1 for r in scs.refine_batch([stale, unsolved], tol=TOL))
