"""Derivatives of a solve with real PSD blocks on the device (csrc/dproj_psd.hpp behind SCS.adjoint / derivative, their device twins,
scs.autograd and scs_hip_dproj_cone) against the dense numpy reference of tests/adjoint_psd_ref.py.

Bounds.  The device decomposes every block of v to a relative off-diagonal norm TAU (kDprojPsdTau; 8 NP 2^-52 beyond order ~56), so its
eigenvectors are off by at most ~TAU / g for a relative sign gap g, and so is W u relative to |u|: the generator keeps g >= GAP = 0.1 and
the tests assert 100 TAU / g |u| per block.  A wrong sqrt(2) or a wrong entry of B gives O(0.1).  For the solved systems LSQR adds its
own cond2(J) tol (tests/test_adjoint_gpu.py): 100 cond(J) max(tol, TAU / g) with tol = 1e-12."""
import gc
import json
import os

import numpy as np
import pytest

import torch

import adjoint_ref as ar
import adjoint_psd_ref as pr
import problem_gen as pg

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "adjoint_psd_fd.json")))
IND, DEN = scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE
STG = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=False, max_iters=100000)
TOL = 1e-12
LEVEL = max(TOL, pr.TAU / pr.GAP)
PROBLEMS = {"qp_sdp": pr.problem_qp_sdp, "lp_sdp": pr.problem_lp_sdp, "mixed_sdp": pr.problem_mixed_sdp}
_problems, _solved, _refs = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _finish_cached_solvers():
    """the solvers this module solves once and shares are finished with it: no device block of theirs — the PSD frames included —
    outlives the module (the block pool's account is an invariant of tests/test_pool_lifecycle_gpu.py)"""
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
    key = (name, normalize, solver)
    if key not in _solved:
        p = problem(name)
        sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=solver, normalize=normalize, **STG)
        sol = sv.solve(warm_start=False)
        assert sol["info"]["status"] == "solved", sol["info"]
        assert np.abs(sol["x"] - p["x"]).max() < 1e-5, name  # the generator's pair: every block has the rank it was built with
        _solved[key] = (sv, sol, p)
    return _solved[key]


def cotangents(p, seed=5):
    rng = np.random.default_rng(seed)
    m, n = p["A"].shape
    return rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)


def rel(got, ref):
    return np.linalg.norm(got - ref) / np.linalg.norm(ref)


def reference(name, normalize, solver):
    """adjoint and forward references at the GPU solve's own (x, y, s), once per solved workspace"""
    key = (name, normalize, solver)
    if key not in _refs:
        sv, sol, p = solved(name, normalize, solver)
        gx, gy, gs = cotangents(p)
        rng = np.random.default_rng(9)
        m, n = p["A"].shape
        db, dc = rng.standard_normal(m), rng.standard_normal(n)
        ref = pr.adjoint(p["A"], p["P"], p["cone"], sol["x"], sol["y"], sol["s"], gx, gy, gs)
        cond = float(np.linalg.cond(ref["J"]))
        assert cond <= 1e4, cond  # (a condition on the test's inputs)
        q = np.linalg.lstsq(ref["J"], np.concatenate([-dc, db]), rcond=None)[0]
        W = ref["W"]
        out = {"db": ref["db"], "dc": ref["dc"], "dA": ar.stored_values(ref["dA"], p["A"])}
        if p["P"] is not None:
            out["dP"] = ar.stored_values(ref["dP"], p["P"])
        fwd = {"dx": q[:n], "ds": W @ q[n:], "dy": W @ q[n:] - q[n:]}
        _refs[key] = (out, fwd, cond, (gx, gy, gs), (db, dc))
    return _refs[key]


# ---- 1. W applied to a vector ------------------------------------------------------------------------------------------------
FUSED_ORDERS = (1, 2, 3, 8, 15, 16, 17, 31, 32)  # both edges of the one-wavefront kernel's lane loops
TILE_ORDERS = (33, 48, 100, 264)                 # an odd and a full tile count; 264: more pivots than wavefronts in the decomposition
SPECTRA = ("positive", "negative", "mixed", "repeated", "mixed_small", "mixed_large")


def spectrum(rng, p, kind):
    lam = rng.uniform(0.5, 1.5, p)
    if kind == "positive":
        return lam
    if kind == "negative":
        return -lam
    if kind == "repeated":
        return np.where(np.arange(p) < (p + 1) // 2, 1.0, -1.0)
    lam[(p + 1) // 2:] *= -1.0
    return lam * {"mixed": 1.0, "mixed_small": 1e-6, "mixed_large": 1e6}[kind]


def dproj_vector(orders, seed=7):
    """z = 3, l = 20, q = [5, 1, 70], then every order with every spectrum"""
    rng = np.random.default_rng(seed)
    q = [5, 1, 70]
    parts = [rng.standard_normal(3), np.where(rng.random(20) < 0.5, -1.0, 1.0) * rng.uniform(0.1, 2.0, 20)] + [rng.standard_normal(k) for k in q]
    s, kinds = [], []
    for p in orders:
        for kind in SPECTRA:
            Q = np.linalg.qr(rng.standard_normal((p, p)))[0]
            parts.append(pr.svec((Q * spectrum(rng, p, kind)) @ Q.T))
            s.append(p)
            kinds.append(kind)
    v = np.concatenate(parts)
    return v, rng.standard_normal(v.size), {"z": 3, "l": 20, "q": q, "s": s}, kinds


_dproj = {}


def dproj_case():
    if not _dproj:
        v, u, cone, kinds = dproj_vector(FUSED_ORDERS + TILE_ORDERS)
        wu, wmiu = _scs_hip.dproj_cone(v, u, cone)
        _dproj.update(v=v, u=u, cone=cone, kinds=kinds, wu=wu, wmiu=wmiu)
    return _dproj


def test_dproj_matches_numpy():
    c = dproj_case()
    v, u, cone, wu = c["v"], c["u"], c["cone"], c["wu"]
    assert np.array_equal(c["wmiu"], wu - u)
    head = 23 + sum(cone["q"])
    zlq = {"z": 3, "l": 20, "q": cone["q"]}
    assert np.abs(wu[:head] - ar.cone_W(v[:head], zlq) @ u[:head]).max() <= 1e-13 * np.linalg.norm(u[:head])
    bound = 100 * pr.TAU / pr.GAP
    worst, o = {}, head
    for p, kind in zip(cone["s"], c["kinds"]):
        d = pr.sd_size(p)
        vb, ub, got = v[o:o + d], u[o:o + d], wu[o:o + d]
        err = np.linalg.norm(got - pr.psd_W_apply(vb, ub, p)) / np.linalg.norm(ub)
        worst[p] = max(worst.get(p, 0.0), err)
        assert err <= bound, (p, kind, err, bound)
        if kind == "negative":
            assert not got.any(), (p, kind)
        if kind == "positive":
            assert np.linalg.norm(got - ub) <= bound * np.linalg.norm(ub), (p, kind)
        elif p > 1 and kind != "negative":
            assert np.linalg.norm(got - ub) > 1e-3 * np.linalg.norm(ub) and got.any(), (p, kind)
        o += d
    assert o == v.size
    print("dproj PSD: worst |W u - ref| / |u| per order (bound %.1e): %s" % (bound, ", ".join("%d: %.1e" % kv for kv in sorted(worst.items()))))


def test_dproj_is_scale_invariant_and_repeatable():
    c = dproj_case()
    again = _scs_hip.dproj_cone(c["v"], c["u"], c["cone"])[0]
    assert np.array_equal(again, c["wu"])  # every reduction has a fixed order
    # (the three mixed cases of an order have different eigenvectors: compare each with the reference above, and here only that a
    #  scaled copy of ONE matrix gives the same W u to the bound)
    rng = np.random.default_rng(1)
    for p in (5, 32, 48):
        Q = np.linalg.qr(rng.standard_normal((p, p)))[0]
        lam = spectrum(rng, p, "mixed")
        ub = rng.standard_normal(pr.sd_size(p))
        outs = [_scs_hip.dproj_cone(pr.svec((Q * (f * lam)) @ Q.T), ub, {"s": [p]})[0] for f in (1.0, 1e-6, 1e6)]
        for other in outs[1:]:
            assert np.linalg.norm(other - outs[0]) <= 100 * pr.TAU / pr.GAP * np.linalg.norm(ub), p


def test_W_is_symmetric():
    c = dproj_case()
    rng = np.random.default_rng(3)
    a, b = c["u"], rng.standard_normal(c["u"].size)
    Wa, Wb = c["wu"], _scs_hip.dproj_cone(c["v"], b, c["cone"])[0]
    o = 23 + sum(c["cone"]["q"])
    worst = 0.0
    for p in c["cone"]["s"]:
        d = pr.sd_size(p)
        gap = abs(a[o:o + d] @ Wb[o:o + d] - Wa[o:o + d] @ b[o:o + d]) / (np.linalg.norm(a[o:o + d]) * np.linalg.norm(b[o:o + d]))
        worst = max(worst, gap)
        assert gap <= 1e-12, (p, gap)
        o += d
    print("symmetry: worst |<a, W b> - <W a, b>| / (|a| |b|) %.2e" % worst)


# ---- 3. adjoint and forward mode against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [IND, DEN], ids=["indirect", "dense"])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("name", ["qp_sdp", "lp_sdp", "mixed_sdp"])
def test_adjoint_and_forward_match_the_reference(name, normalize, solver):
    sv, sol, p = solved(name, normalize, solver)
    ref, fref, cond, (gx, gy, gs), (db, dc) = reference(name, normalize, solver)
    want = ("b", "c", "A") + (("P",) if p["P"] is not None else ())
    got = sv.adjoint(dx=gx, dy=gy, ds=gs, want=want, tol=TOL)
    fw = sv.derivative(db=db, dc=dc, tol=TOL)
    bound = 100 * cond * LEVEL
    errs = {key: rel(got[key], ref[key]) for key in ref}
    errs.update({key: rel(fw[key], fref[key]) for key in fref})
    print("%s normalize=%s %s: relative errors %s, bound %.3e, cond(J) %.3e, LSQR %s / %s" % (
        name, normalize, solver.name, ", ".join("%s %.2e" % kv for kv in errs.items()), bound, cond, got["info"], fw["info"]))
    lhs = gx @ fw["dx"] + gy @ fw["dy"] + gs @ fw["ds"]
    rhs = got["db"] @ db + got["dc"] @ dc
    g, d = np.concatenate([gx, gy, gs]), np.concatenate([fw["dx"], fw["dy"], fw["ds"]])
    scale = np.linalg.norm(g) * np.linalg.norm(d) + np.linalg.norm(np.concatenate([got["db"], got["dc"]])) * np.linalg.norm(np.concatenate([db, dc]))
    print("duality %s: lhs %.15e rhs %.15e, difference / scale %.3e" % (name, lhs, rhs, abs(lhs - rhs) / scale))
    for key, err in errs.items():
        assert err <= bound, (name, normalize, key, err, bound)
    assert abs(lhs - rhs) <= bound * scale
    assert got["info"]["stop"] in (1, 2, 3) and got["info"]["iters"] >= 1


# ---- 4. one end-to-end finite difference on the GPU solver ---------------------------------------------------------------------------
def test_finite_differences_of_the_gpu_solver():
    p = pr.problem_qp_sdp()
    rec = GOLD["qp_sdp"]
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
        err, cond = pr.fd_compare(p, solve, pr.FD_SEEDS[which], which, h=GOLD["h"], grad=grad)
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


@pytest.mark.parametrize("name", ["qp_sdp", "mixed_sdp"])
def test_two_calls_and_both_entries_give_the_same_bits(name):
    sv, sol, p = solved(name)
    gx, gy, gs = cotangents(p)
    want = ("b", "c", "A", "P")
    first = sv.adjoint(dx=gx, dy=gy, ds=gs, want=want)
    same_bits(first, sv.adjoint(dx=gx, dy=gy, ds=gs, want=want))
    same_bits(first, sv.adjoint_device(dx=dev(gx), dy=dev(gy), ds=dev(gs), want=want))
    rng = np.random.default_rng(2)
    db, dc = rng.standard_normal(p["b"].size), rng.standard_normal(p["c"].size)
    fw = sv.derivative(db=db, dc=dc)
    same_bits(fw, sv.derivative(db=db, dc=dc))
    same_bits(fw, sv.derivative_device(db=dev(db), dc=dev(dc)))


def test_a_call_leaves_the_state_of_the_next_solve_alone_and_clones_agree():
    """the decomposition runs over scratch of its own: a warm-started solve after a call is the twin's, bit for bit (the PSD
    projection's warm-start eigenvectors live in the workspace's psd_scratch)"""
    p = problem("mixed_sdp")
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
    cl = a.clone()
    sc = cl.solve(warm_start=False)
    assert np.array_equal(sc["x"], sa["x"]) and np.array_equal(sc["y"], sa["y"]) and np.array_equal(sc["s"], sa["s"])
    same_bits(got, cl.adjoint(dx=gx, dy=gy, ds=gs, want=("b", "c", "A", "P")))


# ---- 6. the block pool -----------------------------------------------------------------------------------------------------------------
def test_the_second_call_adds_no_pool_miss():
    sv, sol, p = solved("mixed_sdp")
    gx, gy, gs = (dev(g) for g in cotangents(p))
    sv.adjoint_device(dx=gx, dy=gy, ds=gs)
    torch.cuda.synchronize()
    before = _scs_hip.pool_stats()
    sv.adjoint_device(dx=gx, dy=gy, ds=gs)
    sv.derivative_device(db=gy, dc=gx)
    after = _scs_hip.pool_stats()
    assert after["misses"] == before["misses"], (before, after)
    assert after["hits"] >= before["hits"] + 2  # the decomposition's scratch came back from the pool both times


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_complex_psd_is_refused_by_name_and_the_workspace_still_solves():
    K = {"l": 2, "cs": [2]}
    data, _, _ = pg.gen_feasible(K, 3, 2, 5, lambda z, K: _scs_hip.proj_cone(z, K, dual=True))
    sv = scs.SCS(data, K, linear_solver=IND, **dict(STG, eps_abs=1e-7, eps_rel=1e-7))
    first = sv.solve(warm_start=False)
    assert first["info"]["status"] == "solved"
    for call in (sv.adjoint, sv.derivative):
        with pytest.raises(ValueError, match=r"complex PSD \(cs\) cone.*z, l, q and s cones only"):
            call()
    again = sv.solve(warm_start=False)
    assert again["info"]["status"] == "solved"
    assert np.abs(again["x"] - first["x"]).max() <= 1e-4 * max(1.0, np.abs(first["x"]).max())
    with pytest.raises(RuntimeError, match=r"complex PSD \(cs\)"):  # (the one-shot parity entry reports through _check)
        _scs_hip.dproj_cone(np.ones(6), np.ones(6), K)


# ---- 8. the torch layer ------------------------------------------------------------------------------------------------------------------
def test_autograd_solve():
    import scs.autograd
    p = problem("qp_sdp")
    sv = scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG)
    sv.autograd_tol = TOL
    b = dev(p["b"]).requires_grad_(True)
    c = dev(p["c"]).requires_grad_(True)
    x, y, s = scs.autograd.solve(sv, b, c)
    gx, gy, gs = cotangents(p)
    (x @ dev(gx) + y @ dev(gy) + s @ dev(gs)).backward()
    ref = pr.adjoint(p["A"], p["P"], p["cone"], x.detach().cpu().numpy(), y.detach().cpu().numpy(), s.detach().cpu().numpy(), gx, gy, gs)
    cond = float(np.linalg.cond(ref["J"]))
    bound = 100 * cond * LEVEL
    eb, ec = rel(b.grad.cpu().numpy(), ref["db"]), rel(c.grad.cpu().numpy(), ref["dc"])
    print("autograd qp_sdp: relative errors db %.3e dc %.3e, bound %.3e" % (eb, ec, bound))
    assert eb <= bound and ec <= bound
