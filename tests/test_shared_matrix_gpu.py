"""GPU tests of SCS.clone / SCS.solve_many: many (b, c) over ONE device copy of the matrix (include/scs_hip.h scs_hip_clone;
csrc/work.hpp MatrixSet; csrc/batch.hpp d_spmv_stream_tiled).

The oracle of every test: for member i an INDEPENDENT full workspace scs.SCS(data, cone, **settings), update(b_i, c_i), solve().
The shared path — clones on one matrix set, grouped by solve_batch into runs whose CSR-stream products read the matrix once per
tile of four members in the labs build (SCS_HIP_SHARED_TILE=1), member by member in the product — must return the same iteration / CG-step / Anderson counters and bit-identical x, y, s."""
import gc
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
from scipy import sparse

import problem_gen as pg

pytestmark = pytest.mark.gpu

EXACT_INFO = ("status_val", "iter", "cg_iters", "scale_updates", "scale", "pobj", "dobj", "res_pri", "res_dual", "gap",
              "comp_slack", "rejected_accel_steps", "accepted_accel_steps")
STG = dict(verbose=False, max_iters=400)
KMAX = 9


def _proj(z, K):
    from scs import _scs_hip
    return _scs_hip.proj_cone(z, K, dual=True)


def _assert_same(a, b, tag):
    for key in ("x", "y", "s"):
        assert np.array_equal(a[key], b[key], equal_nan=True), "%s: %s differs (max |d| = %g)" % (tag, key, np.nanmax(np.abs(a[key] - b[key])))
    for key in EXACT_INFO:
        va, vb = a["info"][key], b["info"][key]
        assert va == vb or (va != va and vb != vb), (tag, key, va, vb)
    assert a["info"]["aa_stats"] == b["info"]["aa_stats"], (tag, a["info"]["aa_stats"], b["info"]["aa_stats"])
    assert a["info"]["status"] == b["info"]["status"]


def _feasible_bc(A, K, rng, P=None, scale=1.0):
    """(b, c) of a feasible, bounded program over the given A (problem_gen's construction, A fixed)"""
    m, n = A.shape
    z = rng.standard_normal(m)
    y = np.asarray(_proj(z, K), dtype=np.float64)
    s = y - z
    x = rng.standard_normal(n)
    c = -(A.T @ y) - (P @ x if P is not None else 0.0)
    return scale * (A @ x + s), scale * c


def _dense_row_matrix(rng):
    """40 x 2100, ~2 nonzeros per column, row 7 fully dense: one row of more than kNnzPerWg = 2048 nonzeros among sparse ones"""
    A = pg.random_sparse(40, 2100, 2, rng).tolil()
    A[7, :] = rng.standard_normal(2100)
    A = A.tocsc()
    A.sort_indices()
    return A


def _shape_case(name):
    rng = np.random.default_rng({"blocks": 11, "rows_per_lane": 12, "long_row": 13, "long_row_t": 14}[name])
    if name == "blocks":  # ~3600 nonzeros: two row blocks in CSR(A) and in CSR(A')
        A = sparse.random(120, 60, density=0.5, random_state=np.random.RandomState(11), format="csc", data_rvs=rng.standard_normal)
    elif name == "rows_per_lane":  # 1500 rows in ONE block of CSR(A): lanes own several rows (kRowsPerLane loop)
        rows = np.arange(1500)
        A = sparse.csc_matrix((rng.standard_normal(1500), (rows, rng.integers(0, 40, 1500))), shape=(1500, 40))
    elif name == "long_row":
        A = _dense_row_matrix(rng)
    else:
        A = _dense_row_matrix(rng).T.tocsc()
    A.sort_indices()
    K = {"l": A.shape[0]}
    bc = [_feasible_bc(A, K, rng) for _ in range(KMAX)]
    return A, K, bc


_CASES = {}


def _case(name):
    """the matrix, the KMAX (b, c) pairs and the oracle's answers for them — computed once, shared by the K-parametrised tests"""
    import scs
    if name not in _CASES:
        A, K, bc = _shape_case(name)
        data = {"A": A, "b": bc[0][0], "c": bc[0][1]}
        ref = []
        for b, c in bc:
            sv = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG)
            sv.update(b, c)
            ref.append(sv.solve(warm_start=False))
        _CASES[name] = (data, K, bc, ref)
    return _CASES[name]


@pytest.mark.parametrize("count", [1, 2, 4, 5, 9])
@pytest.mark.parametrize("name", ["blocks", "rows_per_lane", "long_row", "long_row_t"])
def test_runs_match_independent_workspaces_bit_for_bit(name, count):
    """the product: shared storage, per-member launches (the tiled kernel is a labs switch until it is measured to win)"""
    _check_runs(name, count, tiled_expected=False)


@pytest.mark.labs
@pytest.mark.parametrize("count", [1, 2, 4, 5, 9])
@pytest.mark.parametrize("name", ["blocks", "rows_per_lane", "long_row", "long_row_t"])
def test_tiled_runs_match_independent_workspaces_bit_for_bit(name, count, monkeypatch):
    """labs build, SCS_HIP_SHARED_TILE=1: the same runs through k_spmv_stream_tiled (full tiles, a remainder, K = 1 on the old path)"""
    monkeypatch.setenv("SCS_HIP_SHARED_TILE", "1")
    _check_runs(name, count, tiled_expected=count > 1)


def _check_runs(name, count, tiled_expected):
    import scs
    data, K, bc, ref = _case(name)
    parent = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG)
    members = [parent] + [parent.clone() for _ in range(count - 1)]
    for sv in members[1:]:
        assert parent.shares_matrix(sv) and sv.shares_matrix(members[-1])
    for sv, (b, c) in zip(members, bc):
        sv.update(b, c)
    plan = scs.batch_plan(members)
    assert plan == ([-1] if count == 1 else [0] * count), plan
    from scs import _scs_hip
    tiled = _scs_hip.tiled_launches()
    got = scs.solve_batch(members)
    tiled = _scs_hip.tiled_launches() - tiled
    assert (tiled > 0) == tiled_expected, tiled  # which kernel the run's products really went through
    for i in range(count):
        _assert_same(ref[i], got[i], "%s member %d of %d" % (name, i, count))


def test_init_then_update_agrees_with_init_at_solver_tolerance():
    """A fresh SCS(dict(data, b=b_i, c=c_i)) scales b, c on the device, update() on the host: bits may differ, the answers may not.
    Both runs end with gap <= eps_abs + eps_rel max(|pobj|, |dobj|) (eps = 1e-4), and the optimum lies between a run's objectives up to
    its residuals, so two solved runs differ by at most twice that; a factor two on top for the residual terms."""
    import scs
    data, K, bc, _ = _case("blocks")
    stg = dict(verbose=False, max_iters=20000, linear_solver=scs.LinearSolver.HIP_INDIRECT)  # (to convergence: STG's cap ends these runs early)
    parent = scs.SCS(data, K, **stg)
    got = parent.solve_many(b=np.stack([bc[i][0] for i in (1, 4, 8)]), c=np.stack([bc[i][1] for i in (1, 4, 8)]))
    for k, i in enumerate((1, 4, 8)):
        fresh = scs.SCS(dict(data, b=bc[i][0], c=bc[i][1]), K, **stg).solve()
        assert fresh["info"]["status"] == got[k]["info"]["status"] == "solved", (fresh["info"], got[k]["info"])
        tol = 4 * (1e-4 + 1e-4 * max(abs(fresh["info"]["pobj"]), abs(got[k]["info"]["pobj"])))
        assert abs(fresh["info"]["pobj"] - got[k]["info"]["pobj"]) <= tol


def test_members_that_diverge_in_one_batch():
    """different b, c and scalings of them (CG-step counts and adaptive-scale updates fall differently), one member made primal
    infeasible by its b, and — same A, a workspace of its own, so alone on its matrix set inside the group — one stopped by max_iters"""
    import scs
    rng = np.random.default_rng(21)
    A0 = sparse.random(118, 60, density=0.5, random_state=np.random.RandomState(21), format="csc", data_rvs=rng.standard_normal)
    r = rng.standard_normal((1, 60))
    A = sparse.vstack([A0, sparse.csc_matrix(r), sparse.csc_matrix(-r)]).tocsc()  # rows 118, 119: r x <= b_118, -r x <= b_119
    A.sort_indices()
    K = {"l": 120}
    bc = [_feasible_bc(A, K, rng, scale=sc) for sc in (1.0, 30.0, 0.02, 1.0, 400.0, 1.0, 5.0)]
    bc[3][0][118:] = -1.0  # r x <= -1 and r x >= 1
    stg = dict(verbose=False, max_iters=2000)
    data = {"A": A, "b": bc[0][0], "c": bc[0][1]}
    ref = []
    for i, (b, c) in enumerate(bc):
        sv = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **dict(stg, max_iters=30 if i == 6 else 2000))
        sv.update(b, c)
        ref.append(sv.solve(warm_start=False))
    assert ref[3]["info"]["status_val"] == -2, ref[3]["info"]
    assert ref[6]["info"]["iter"] == 30
    assert len({o["info"]["scale_updates"] for o in ref[:6]}) >= 2, [o["info"]["scale_updates"] for o in ref]
    assert len({o["info"]["cg_iters"] for o in ref[:6]}) >= 2
    parent = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **stg)
    members = [parent] + [parent.clone() for _ in range(5)]
    members.append(scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **dict(stg, max_iters=30)))
    for sv, (b, c) in zip(members, bc):
        sv.update(b, c)
    assert scs.batch_plan(members) == [0] * 7
    got = scs.solve_batch(members)
    for i in range(7):
        _assert_same(ref[i], got[i], "member %d" % i)


def _mixed_cone_problem(rng):
    K = dict(z=3, l=10, q=[5, 4], s=[3], ep=1, p=[0.4], ell1=[5])
    m = 3 + 10 + 9 + 6 + 3 + 3 + 6
    A = sparse.random(m, 25, density=0.4, random_state=np.random.RandomState(5), format="csc", data_rvs=rng.standard_normal)
    A.sort_indices()
    return A, K


@pytest.mark.parametrize("variant", ["qp", "aa1", "aa2", "aa_off", "dense", "mixed_cones"])
def test_solve_many_variants_match_the_oracle(variant):
    import scs
    rng = np.random.default_rng(31)
    stg = dict(STG)
    solver = scs.LinearSolver.HIP_DENSE if variant == "dense" else scs.LinearSolver.HIP_INDIRECT
    P = None
    if variant == "mixed_cones":  # (random b, c: bit identity needs no feasible instance; the iteration cap ends the run)
        A, K = _mixed_cone_problem(rng)
        bc = [(rng.standard_normal(A.shape[0]), rng.standard_normal(A.shape[1])) for _ in range(5)]
        stg["max_iters"] = 150
    else:
        K = {"z": 10, "l": 80, "q": [10, 10, 10]}
        A = sparse.random(120, 60, density=0.5, random_state=np.random.RandomState(31), format="csc", data_rvs=rng.standard_normal)
        A.sort_indices()
        if variant == "qp":
            B = pg.random_sparse(15, 60, 3, rng)
            P = (B.T @ B + sparse.eye(60)).tocsc()
        bc = [_feasible_bc(A, K, rng, P=P) for _ in range(5)]
    if variant == "aa2":
        stg.update(acceleration_type_1=False, acceleration_interval=1)
    if variant == "aa_off":
        stg["acceleration_lookback"] = 0
    data = {"A": A, "b": bc[0][0], "c": bc[0][1]}
    if P is not None:
        data["P"] = P
    ref = []
    for b, c in bc:
        sv = scs.SCS(data, K, linear_solver=solver, **stg)
        sv.update(b, c)
        ref.append(sv.solve(warm_start=False))
    parent = scs.SCS(data, K, linear_solver=solver, **stg)
    got = parent.solve_many(b=np.stack([b for b, _ in bc]), c=np.stack([c for _, c in bc]))
    assert len(got) == 5
    for i in range(5):
        _assert_same(ref[i], got[i], "%s member %d" % (variant, i))
    if variant == "dense":
        assert got[0]["info"]["lin_sys_solver"].startswith("dense-direct")
    if variant in ("aa1", "aa2"):
        assert any(o["info"]["accepted_accel_steps"] + o["info"]["rejected_accel_steps"] > 0 for o in got)


def test_mixed_batch_two_runs_and_a_lone_member():
    import scs
    K = {"l": 120}
    mats, bcs = [], []
    for seed in (41, 42, 43):
        rng = np.random.default_rng(seed)
        A = sparse.random(120, 60, density=0.5, random_state=np.random.RandomState(seed), format="csc", data_rvs=rng.standard_normal)
        A.sort_indices()
        mats.append(A)
        bcs.append([_feasible_bc(A, K, rng) for _ in range(3)])
    hip = scs.LinearSolver.HIP_INDIRECT

    def fresh(j):
        return scs.SCS({"A": mats[j], "b": bcs[j][0][0], "c": bcs[j][0][1]}, K, linear_solver=hip, **STG)

    X, Y, Z = fresh(0), fresh(1), fresh(2)
    batch = [X, X.clone(), Y, Y.clone(), Y.clone(), Z]
    owner = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 0)]
    ref = []
    for sv, (j, i) in zip(batch, owner):
        sv.update(*bcs[j][i])
        o = fresh(j)
        o.update(*bcs[j][i])
        ref.append(o.solve(warm_start=False))
    assert scs.batch_plan(batch) == [0] * 6
    assert batch[0].shares_matrix(batch[1]) and batch[2].shares_matrix(batch[4]) and not batch[1].shares_matrix(batch[2])
    assert not Z.shares_matrix(X)
    got = scs.solve_batch(batch)
    for i in range(6):
        _assert_same(ref[i], got[i], "mixed batch member %d" % i)


def test_lifetime_parent_first_clone_of_clone_and_pristine_state():
    import scs
    from scs import _scs_hip
    data, K, bc, ref = _case("blocks")
    hip = scs.LinearSolver.HIP_INDIRECT
    first = scs.SCS(data, K, linear_solver=hip, **STG).solve(warm_start=False)  # a fresh workspace's first solve
    parent = scs.SCS(data, K, linear_solver=hip, **STG)
    parent.update(*bc[2])
    parent.solve()
    c0 = parent.clone()  # of a parent that has solved and been updated: still the constructor's state
    c1 = parent.clone()
    c2 = c1.clone()
    assert c2.shares_matrix(parent) and c2.shares_matrix(c1) and c0.shares_matrix(c2)
    _assert_same(first, c0.solve(warm_start=False), "clone of a used parent")
    del c0
    del parent
    gc.collect()
    c1.update(*bc[3])
    c2.update(*bc[4])
    got = scs.solve_batch([c1, c2])
    _assert_same(ref[3], got[0], "clone after its parent is gone")
    _assert_same(ref[4], got[1], "clone of a clone after the parent is gone")
    del c1, c2, got
    gc.collect()
    st = _scs_hip.pool_stats()
    assert st["live_bytes"] == st["held_bytes"], st
    _scs_hip.trim_pool()
    st = _scs_hip.pool_stats()
    assert st["live_bytes"] == 0 and st["held_bytes"] == 0, st


def test_a_clone_allocates_no_matrix():
    """matrix-dominated instance: the two stored forms of A alone are 12 bytes per nonzero each, and a clone allocates neither"""
    import scs
    from scs import _scs_hip
    rng = np.random.default_rng(51)
    A = sparse.random(2000, 1000, density=0.5, random_state=np.random.RandomState(51), format="csc", data_rvs=rng.standard_normal)
    A.sort_indices()
    data = {"A": A, "b": rng.standard_normal(2000), "c": rng.standard_normal(1000)}
    hip = scs.LinearSolver.HIP_INDIRECT
    _scs_hip.trim_pool()
    live0 = _scs_hip.pool_stats()["live_bytes"]
    parent = scs.SCS(data, {"l": 2000}, linear_solver=hip, **STG)
    live1 = _scs_hip.pool_stats()["live_bytes"]
    clone = parent.clone()
    live2 = _scs_hip.pool_stats()["live_bytes"]
    delta_fresh, delta_clone = live1 - live0, live2 - live1
    print("live bytes: fresh workspace %d, clone %d, nnz %d" % (delta_fresh, delta_clone, A.nnz))
    assert clone.shares_matrix(parent)
    assert delta_clone <= delta_fresh - 24 * A.nnz, (delta_clone, delta_fresh, A.nnz)


def test_four_threads_each_solve_their_own_clone():
    import scs
    data, K, bc, ref = _case("blocks")
    parent = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG)
    clones = [parent.clone() for _ in range(4)]
    out, errs = [None] * 4, []

    def work(i):
        try:
            clones[i].update(*bc[i + 1])
            out[i] = clones[i].solve(warm_start=False)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(4):
        _assert_same(ref[i + 1], out[i], "thread %d" % i)


def test_solve_many_warm_sweep_and_clone_cache():
    import scs
    from scs import _scs_hip
    data, K, bc, ref = _case("blocks")
    parent = scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **STG)
    B, Cm = np.stack([b for b, _ in bc[:5]]), np.stack([c for _, c in bc[:5]])
    first = parent.solve_many(b=B, c=Cm)
    for i in range(5):
        _assert_same(ref[i], first[i], "solve_many member %d" % i)
    misses = _scs_hip.pool_stats()["misses"]
    second = parent.solve_many(b=B, c=Cm, warm_start=True, x=np.stack([o["x"] for o in first]), y=np.stack([o["y"] for o in first]),
                               s=np.stack([o["s"] for o in first]))
    assert _scs_hip.pool_stats()["misses"] == misses  # the cached clones were reused: nothing new from hipMalloc
    for a, b in zip(first, second):
        assert b["info"]["iter"] <= a["info"]["iter"], (a["info"]["iter"], b["info"]["iter"])


def test_solve_many_b_none_keeps_b():
    """second call with new c only, against independent workspaces with the same history (update, solve, update(c), solve)"""
    import scs
    data, K, bc, ref = _case("blocks")
    hip = scs.LinearSolver.HIP_INDIRECT
    B, Cm = np.stack([b for b, _ in bc[:3]]), np.stack([c for _, c in bc[:3]])
    C2 = np.stack([c for _, c in bc[4:7]])
    want = []
    for i in range(3):
        sv = scs.SCS(data, K, linear_solver=hip, **STG)
        sv.update(B[i], Cm[i])
        sv.solve(warm_start=False)
        sv.update(None, C2[i])
        want.append(sv.solve(warm_start=False))
    parent = scs.SCS(data, K, linear_solver=hip, **STG)
    parent.solve_many(b=B, c=Cm)
    got = parent.solve_many(c=C2)
    for i in range(3):
        _assert_same(want[i], got[i], "b=None member %d" % i)


_CS_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(pkg)r]
import numpy as np
import scs, problem_gen as pg
rng = np.random.default_rng(61)
A = pg.random_sparse(20000, 16500, 3, rng)
K = {"l": 20000}
bc = [(rng.standard_normal(20000), rng.standard_normal(16500)) for _ in range(3)]
stg = dict(verbose=False, max_iters=40, linear_solver=scs.LinearSolver.HIP_INDIRECT)
data = {"A": A, "b": bc[0][0], "c": bc[0][1]}
ref = []
for b, c in bc:
    sv = scs.SCS(data, K, **stg); sv.update(b, c); ref.append(sv.solve(warm_start=False))
parent = scs.SCS(data, K, **stg)
kt = parent._solver._kernel_times()
members = [parent, parent.clone(), parent.clone()]
assert all(parent.shares_matrix(sv) for sv in members[1:])
for sv, (b, c) in zip(members, bc):
    sv.update(b, c)
plan = scs.batch_plan(members)
got = scs.solve_batch(members)
for i, (r, g) in enumerate(zip(ref, got)):
    print("MEMBER", i, r["info"]["iter"], g["info"]["iter"], r["info"]["cg_iters"], g["info"]["cg_iters"], r["info"]["status"], "|", g["info"]["status"],
          float(np.nanmax(np.abs(r["x"] - g["x"]))), file=sys.stderr)
same = all(np.array_equal(r[k], g[k], equal_nan=True) for r, g in zip(ref, got) for k in "xys") and all(r["info"]["iter"] == g["info"]["iter"] and r["info"]["cg_iters"] == g["info"]["cg_iters"] for r, g in zip(ref, got))
print("RESULT", plan, same, kt["k1_wgs"], kt["k2_wgs"])
"""


def test_large_layout_clones_are_solved_alone_on_shared_storage():
    """SCS_HIP_CS=2: the column-sorted pass layout on a small matrix (both orientations have >= 16384 rows).  Such members are not
    grouped (batch_plan: -1): the clones are solved one after the other by the one-problem loop, on the parent's layouts."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SCS_HIP_CS="2")
    r = subprocess.run([sys.executable, "-c", _CS_CHILD % {"root": root, "pkg": os.path.join(root, "scs-python_amd")}], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1]
    assert line.startswith("RESULT [-1, -1, -1] True"), line + "\n" + r.stderr[-1500:]
