"""Device-resident endpoints (SCS.update_device / solve_device / solve_many_device; include/scs_hip.h scs_hip_*_device): the arithmetic is
the host path's, so every comparison with a twin workspace that went through update / solve / solve_many is exact (np.array_equal).

Shape A (m = 2051, n = 1027, z = 5): a vector workgroup covers 1024 elements, so the kernels run 2-4 workgroups with ragged tails (the
last-arriver fold of k_bc_load has several partials to fold) and the zero-cone / other-rows split of r_y in k_warm_v falls inside a block.
Shape B (m = 7, n = 3): one partial workgroup."""
import numpy as np
import pytest
from scipy import sparse

import torch

import helpers
import problem_gen as pg

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

STG = dict(eps_abs=1e-6, eps_rel=1e-6, max_iters=250, verbose=False)  # (perturbed b, c may run to the cap: the comparison is of bits, not of optima)
K_A = {"z": 5, "l": 1026, "q": [10] * 102}  # m = 2051
K_B = {"z": 1, "l": 3, "q": [3]}            # m = 7
TIMES = ("solve_time", "setup_time", "lin_sys_time", "cone_time", "accel_time")
_cache = {}


def problem(tag):
    if tag not in _cache:
        K, n, k, seed = {"A": (K_A, 1027, 8, 21), "B": (K_B, 3, 2, 22)}[tag]
        data, _, _ = pg.gen_feasible(K, n, k, seed, lambda z, K: _scs_hip.proj_cone(z, K, dual=True))
        assert data["A"].shape == {"A": (2051, 1027), "B": (7, 3)}[tag]
        _cache[tag] = (data, K)
    data, K = _cache[tag]
    return {"A": data["A"], "b": data["b"].copy(), "c": data["c"].copy()}, K


def golden_qp():
    d = np.load(helpers.GOLDEN + "/warm_start_qp.npz")
    P = sparse.csc_matrix((d["P_data"], d["P_indices"], d["P_indptr"]), shape=(15, 15))
    G = sparse.csc_matrix((d["G_data"], d["G_indices"], d["G_indptr"]), shape=(60, 15))
    return {"P": P, "A": G, "b": d["h"].copy(), "c": d["q"].copy()}, {"l": 60}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def host(t):
    return t.cpu().numpy()


def same_vectors(got, ref, what=""):
    for key in ("x", "y", "s"):
        g = host(got[key]) if isinstance(got[key], torch.Tensor) else got[key]
        assert np.array_equal(g, ref[key], equal_nan=True), (what, key, np.abs(g - ref[key]).max())


def same_info(gi, ri, what=""):
    for key, rv in ri.items():
        if key in TIMES:
            continue
        gv = gi[key]
        if isinstance(rv, float):
            assert gv == rv or (np.isnan(gv) and np.isnan(rv)), (what, key, gv, rv)
        else:
            assert gv == rv, (what, key, gv, rv)


def same_result(got, ref, what=""):
    same_vectors(got, ref, what)
    same_info(got["info"], ref["info"], what)


def new_bc(data, rng):
    return data["b"] * 1.1 + 0.01 * rng.standard_normal(data["b"].size), data["c"] * 0.9 + 0.01 * rng.standard_normal(data["c"].size)


# ---- 1. update ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solved_before", [False, True], ids=["deferred_setup", "after_a_solve"])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("which", ["b", "c", "both"])
@pytest.mark.parametrize("solver", [scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE], ids=["indirect", "dense"])
def test_update_device_then_host_solve_matches_host_update(solver, which, normalize, solved_before):
    data, K = problem("A")
    b2, c2 = new_bc(data, np.random.default_rng(1))
    bn, cn = (b2 if which != "c" else None), (c2 if which != "b" else None)
    d, h = (scs.SCS(data, K, linear_solver=solver, normalize=normalize, **STG) for _ in range(2))
    if solved_before:
        same_result(d.solve(warm_start=False), h.solve(warm_start=False), "first solve")
    d.update_device(dev(bn) if bn is not None else None, dev(cn) if cn is not None else None)
    h.update(bn, cn)
    got, ref = d.solve(warm_start=False), h.solve(warm_start=False)
    same_result(got, ref)
    assert got["info"]["iter"] == ref["info"]["iter"] and got["info"]["pobj"] == ref["info"]["pobj"]
    assert got["info"]["iter"] > 0


def test_update_device_with_quadratic_objective():
    data, K = golden_qp()
    b2, c2 = new_bc(data, np.random.default_rng(2))
    d, h = (scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG) for _ in range(2))
    d.update_device(dev(b2), dev(c2))
    h.update(b2, c2)
    same_result(d.solve(warm_start=False), h.solve(warm_start=False))
    same_result(d.solve_device(warm_start=True), h.solve(warm_start=True), "warm re-solve")


# ---- 2. mixed calls -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["A", "B"])
def test_device_update_then_host_update_refreshes_the_stale_mirror(tag):
    data, K = problem(tag)
    b2, c2 = new_bc(data, np.random.default_rng(3))
    d, h = (scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG) for _ in range(2))
    d.update_device(b=dev(b2))
    d.update(c=c2)  # b is None here: the host mirror of b is stale and must be refreshed from the device
    h.update(b=b2)
    h.update(c=c2)
    same_result(d.solve(warm_start=False), h.solve(warm_start=False))
    # ... and the other way round: a host update, then a device update that keeps the vector the host wrote
    b3, c3 = new_bc(data, np.random.default_rng(4))
    d.update(b=b3)
    d.update_device(c=dev(c3))
    h.update(b=b3)
    h.update(c=c3)
    same_result(d.solve(warm_start=False), h.solve(warm_start=False), "host then device")


# ---- 3. cold solve ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["A", "B"])
@pytest.mark.parametrize("solver", [scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE], ids=["indirect", "dense"])
def test_cold_solve_device_equals_host_solve(solver, tag):
    data, K = problem(tag)
    d, h = (scs.SCS(data, K, linear_solver=solver, **dict(STG, max_iters=5000)) for _ in range(2))
    got, ref = d.solve_device(), h.solve(warm_start=False)
    for key, length in (("x", data["c"].size), ("y", data["b"].size), ("s", data["b"].size)):
        t = got[key]
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.is_cuda and tuple(t.shape) == (length,)
    same_result(got, ref)
    assert ref["info"]["status"] == "solved"


# ---- 4. warm start ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
def test_warm_start_from_device_tensors_equals_host_warm_start(normalize):
    data, K = problem("A")
    rng = np.random.default_rng(5)
    n, m = data["c"].size, data["b"].size
    x0, y0, s0 = rng.standard_normal(n), rng.standard_normal(m), np.abs(rng.standard_normal(m))
    y0[2] = np.inf   # a zero-cone row (z = 5)
    y0[700] = np.nan
    x0[1026] = np.nan
    s0[2050] = -np.inf
    d, h = (scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, normalize=normalize, **STG) for _ in range(2))
    got = d.solve_device(warm_start=True, x=dev(x0), y=dev(y0), s=dev(s0))
    ref = h.solve(warm_start=True, x=x0, y=y0, s=s0)
    same_result(got, ref)
    assert np.isfinite(ref["x"]).all() and ref["info"]["iter"] > 0


# ---- 5. previous solution -----------------------------------------------------------------------------------------------------
def test_warm_start_from_the_previous_device_solution():
    data, K = problem("A")
    b2, c2 = new_bc(data, np.random.default_rng(6))
    d, h = (scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG) for _ in range(2))
    same_result(d.solve_device(warm_start=True), h.solve(warm_start=True), "before any solve: zeros")
    d.update_device(dev(b2), dev(c2))
    h.update(b2, c2)
    got, ref = d.solve_device(warm_start=True), h.solve(warm_start=True)
    same_result(got, ref, "from the previous solution")
    # one vector given, two taken from the previous solution
    x1 = ref["x"] * 0.5
    same_result(d.solve_device(warm_start=True, x=dev(x1)), h.solve(warm_start=True, x=x1), "x given")


# ---- 6. undefined vectors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix, status, nan_keys", [("std_infeas_", "infeasible", ("x", "s")), ("std_unbdd_", "unbounded", ("y",))])
def test_certificates_and_nan_pattern(prefix, status, nan_keys):
    data, K, _ = helpers.load_problem("problems_std.npz", prefix)
    stg = dict(eps_abs=1e-6, eps_rel=1e-6, verbose=False)
    d, h = (scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **stg) for _ in range(2))
    got, ref = d.solve_device(), h.solve(warm_start=False)
    assert ref["info"]["status"] == status
    same_result(got, ref)
    for key in ("x", "y", "s"):
        assert bool(torch.isnan(got[key]).all()) == (key in nan_keys)


# ---- 7. solve_many_device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag, count", [("B", 3), ("A", 2)])
def test_solve_many_device_equals_host_solve_many(tag, count):
    data, K = problem(tag)
    rng = np.random.default_rng(7)
    n, m = data["c"].size, data["b"].size
    bs = np.stack([new_bc(data, rng)[0] for _ in range(count)])
    cs = np.stack([new_bc(data, rng)[1] for _ in range(count)])
    d, h = (scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG) for _ in range(2))
    ref = h.solve_many(bs, cs)
    plan_ref = _scs_hip.batch_plan([h._solver] + h._solver._many[:count - 1])
    got = d.solve_many_device(dev(bs), dev(cs))
    assert _scs_hip.batch_plan([d._solver] + d._solver._many[:count - 1]) == plan_ref
    for key, width in (("x", n), ("y", m), ("s", m)):
        t = got[key]
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.is_cuda and tuple(t.shape) == (count, width)
    assert len(got["info"]) == count
    for i in range(count):
        same_result({"x": got["x"][i], "y": got["y"][i], "s": got["s"][i], "info": got["info"][i]}, ref[i], "member %d" % i)
    # a warm-started second sweep: rows of x given, y and s from every member's previous solution
    bs2, x0 = bs * 1.05, np.stack([r["x"] for r in ref]) * 0.9
    ref2 = h.solve_many(bs2, None, warm_start=True, x=x0)
    got2 = d.solve_many_device(dev(bs2), None, warm_start=True, x=dev(x0))
    for i in range(count):
        same_result({"x": got2["x"][i], "y": got2["y"][i], "s": got2["s"][i], "info": got2["info"][i]}, ref2[i], "warm member %d" % i)


# ---- 8. stream ordering -------------------------------------------------------------------------------------------------------
def test_inputs_produced_on_torchs_stream_just_before_the_call():
    data, K = problem("A")
    base_b, base_c = dev(data["b"]), dev(data["c"])
    d, h = (scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG) for _ in range(2))
    b = base_b * 1.1  # enqueued on torch's stream; no synchronisation here
    c = base_c * 0.9
    d.update_device(b, c)
    h.update(host(b), host(c))
    got = d.solve_device()
    y0 = got["y"] * 0.5  # again: produced right before it is consumed
    same_result(got, h.solve(warm_start=False))
    same_result(d.solve_device(warm_start=True, y=y0), h.solve(warm_start=True, y=host(y0)), "warm")


# ---- 9. clones ----------------------------------------------------------------------------------------------------------------
def test_clone_of_a_device_updated_parent_starts_from_the_original_data():
    data, K = problem("B")
    b2, c2 = new_bc(data, np.random.default_rng(9))
    parent = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG)
    parent.update_device(dev(b2), dev(c2))
    child = parent.clone()
    fresh = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG)
    same_result(child.solve(warm_start=False), fresh.solve(warm_start=False))


# ---- 10. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_workspace_usable():
    data, K = problem("B")
    m, n = data["b"].size, data["c"].size
    d, h = (scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG) for _ in range(2))
    good = dev(data["b"])
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        d.update_device(b=data["b"])
    with pytest.raises(TypeError, match="float64"):
        d.update_device(b=good.to(torch.float32))
    with pytest.raises(ValueError, match="workspace's GPU"):
        d.update_device(b=torch.as_tensor(data["b"]))
    with pytest.raises(ValueError, match="length %d" % m):
        d.update_device(b=dev(np.zeros(m + 1)))
    with pytest.raises(ValueError, match="contiguous"):
        d.update_device(b=dev(np.zeros(2 * m))[::2])
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        d.solve_device(warm_start=True, x=np.zeros(n))
    with pytest.raises(ValueError, match="length %d" % n):
        d.solve_device(warm_start=True, x=dev(np.zeros(n + 2)))
    with pytest.raises(ValueError, match="2-D"):
        d.solve_many_device(b=good)
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        d.solve_many_device(b=np.zeros((2, m)))
    same_result(d.solve_device(), h.solve(warm_start=False))
