"""SCS.update_matrix / update_matrix_device (include/scs_hip.h scs_hip_update_matrix*): new values of A and P on the resident layouts.

The contract is one sentence — afterwards the workspace is in the state the constructor leaves a NEW solver in, given the new values
on the old pattern and the current b, c — so every comparison is np.array_equal on x, y, s plus the non-timing info fields against a
twin `scs.SCS` constructed from the new matrices.  The comparison is of bits, not of optima: max_iters is 20 to 250.

Shapes are the smallest that reach each path: shapes A (2051 x 1027) and B (7 x 3) of test_device_io_gpu.py for the CSR-stream
forms, the golden 15-variable QP and a 400-variable one with SOC and PSD cones for P, 20000 x 16400 under SCS_HIP_CS=2 for the
column-sorted pass layout (>= 16384 rows in each orientation), 300000 x 270000 under SCS_HIP_CS=0 for the slab layout."""
import re

import numpy as np
import pytest
from scipy import sparse

import torch

import problem_gen as pg
import test_device_io_gpu as dio

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

STG = dio.STG
IND, DEN = scs.LinearSolver.HIP_INDIRECT, scs.LinearSolver.HIP_DENSE
same_result, dev = dio.same_result, dio.dev


def new_values(M, seed, zero_at=1):
    """M's pattern with data * (1 + 0.1 r) + 0.01 r' and one stored entry set to exactly 0.0"""
    rng = np.random.default_rng(seed)
    N = M.copy()
    N.data = M.data * (1 + 0.1 * rng.standard_normal(M.nnz)) + 0.01 * rng.standard_normal(M.nnz)
    N.data[zero_at % M.nnz] = 0.0
    return N


def new_psd_values(P, seed):
    """new values for P, as the upper triangle the constructor takes as well: entries scaled by 1 + 0.1 r, r in [0, 1) (the diagonal
    grows with the rest), one off-diagonal entry set to exactly 0.0; the stored pattern is kept"""
    rng = np.random.default_rng(seed)
    U = sparse.triu(P, format="csc")
    U.sort_indices()
    U.data = U.data * (1 + 0.1 * rng.random(U.nnz))
    off = np.flatnonzero(U.indices != np.repeat(np.arange(U.shape[1]), np.diff(U.indptr)))
    if off.size:
        U.data[off[0]] = 0.0
    return U


def fresh(data, K, solver=IND, **kw):
    stg = dict(STG)
    stg.update(kw)
    return scs.SCS(data, K, linear_solver=solver, **stg)


def same_grouped(got, ref, what=""):
    """same_result for a member of a grouped solve: its `lin_sys_solver` string names the group ("...; grouped solve of 3"), everything
    else — vectors, counts, residuals — is compared as in same_result"""
    dio.same_vectors(got, ref, what)
    skip = ("lin_sys_solver",)
    dio.same_info({k: v for k, v in got["info"].items() if k not in skip}, {k: v for k, v in ref["info"].items() if k not in skip}, what)


def with_(data, **new):
    d = dict(data)
    d.update(new)
    return d


# ---- 1. CSR-stream forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solved_before", [False, True], ids=["deferred_setup", "after_a_solve"])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("solver", [IND, DEN], ids=["indirect", "dense"])
@pytest.mark.parametrize("tag", ["B", "A"])
def test_new_values_of_A_equal_a_new_solver(tag, solver, normalize, solved_before):
    data, K = dio.problem(tag)
    A2 = new_values(data["A"], 31)
    sv = fresh(data, K, solver, normalize=normalize)
    if solved_before:
        same_result(sv.solve(warm_start=False), fresh(data, K, solver, normalize=normalize).solve(warm_start=False), "first solve")
    sv.update_matrix(A=A2)
    ref = fresh(with_(data, A=A2), K, solver, normalize=normalize).solve(warm_start=False)
    got = sv.solve(warm_start=False)
    same_result(got, ref)
    assert got["info"]["iter"] > 0
    if solved_before:  # the old matrix is really gone
        assert not np.array_equal(got["x"], fresh(data, K, solver, normalize=normalize).solve(warm_start=False)["x"])


# ---- 2. P ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [IND, DEN], ids=["indirect", "dense"])
@pytest.mark.parametrize("which", ["P", "A", "both"])
def test_golden_qp_P_and_A(which, solver):
    data, K = dio.golden_qp()
    A2 = new_values(data["A"], 32) if which != "P" else data["A"]
    P2 = new_psd_values(data["P"], 33) if which != "A" else data["P"]
    sv = fresh(data, K, solver)
    sv.solve(warm_start=False)
    sv.update_matrix(A=A2 if which != "P" else None, P=P2 if which != "A" else None)
    same_result(sv.solve(warm_start=False), fresh(with_(data, A=A2, P=P2), K, solver).solve(warm_start=False))
    # ... and once more with the other argument kept: the kept matrix is re-equilibrated from its raw values
    A3 = new_values(A2, 34)
    sv.update_matrix(A=A3)
    same_result(sv.solve(warm_start=False), fresh(with_(data, A=A3, P=P2), K, solver).solve(warm_start=False), "second update")


def test_qp_with_soc_and_psd_cones_resets_their_state():
    K = {"z": 10, "l": 600, "q": [30, 12, 5], "s": [6, 3]}
    data, _, _ = pg.gen_feasible_qp(K, 400, 4, 41, lambda z, K: _scs_hip.proj_cone(z, K, dual=True))
    A2, P2 = new_values(data["A"], 42), new_psd_values(data["P"], 43)
    sv = fresh(data, K, max_iters=120)
    sv.solve(warm_start=False)  # (leaves warm eigenvectors, an adapted scale and an Anderson history behind)
    sv.update_matrix(A=A2, P=P2)
    same_result(sv.solve(warm_start=False), fresh(with_(data, A=A2, P=P2), K, max_iters=120).solve(warm_start=False))


# ---- 3. box cone ---------------------------------------------------------------------------------------------------------------
def test_box_bounds_follow_the_new_row_scaling():
    rng = np.random.default_rng(51)
    n, nb = 12, 6
    K = {"z": 2, "l": 8, "bl": list(-1.0 - rng.random(nb)), "bu": list(1.0 + rng.random(nb))}
    m = 2 + 8 + nb + 1
    A = sparse.random(m, n, 0.5, format="csc", random_state=7) + sparse.vstack([sparse.csc_matrix((m - n, n)), sparse.eye(n)]).tocsc()
    A = sparse.csc_matrix(A)
    A.sort_indices()
    data = {"A": A, "b": np.abs(rng.standard_normal(m)) + 0.5, "c": rng.standard_normal(n)}
    A2 = new_values(A, 52)
    A2.data[::3] *= 40.0  # the row norms — hence D and the scaled bounds — move a lot
    sv = fresh(data, K)
    sv.solve(warm_start=False)
    sv.update_matrix(A=A2)
    same_result(sv.solve(warm_start=False), fresh(with_(data, A=A2), K).solve(warm_start=False))


# ---- 4. pass layout ------------------------------------------------------------------------------------------------------------
LONG = 6000  # nonzeros of the dense row / column of the `long_lines` variants (see pass_problem)


def pass_problem(long_lines, with_P):
    """20000 x 16400, about 4 nonzeros per column.  long_lines: `long_lines` more nonzeros in row 7 and in column 11.  At this size a
    workgroup owns 128 rows of A (192 of A', split in two: spmv_cs.hpp cs_pick_geometry) with one row per lane, so its few hundred
    nonzeros are ONE pass and the count field of a row holds 2048 per pass (cs_peel_threshold(1)): the line of 70 nonzeros the issue
    names fits that field and is laid out like any other row, while 6000 nonzeros (3000 in each half of a split chunk) overflow it in
    both orientations — the builder then cuts the line into virtual-row pieces (or, SCS_HIP_CS_VIRT=0 in the labs build, peels it)."""
    rng = np.random.default_rng(61)
    m, n = 20000, 16400
    A = pg.random_sparse(m, n, 4, rng).tolil()
    if long_lines:
        A[7, rng.choice(n, long_lines, replace=False)] = rng.standard_normal(long_lines)
        A[rng.choice(m, long_lines, replace=False), 11] = rng.standard_normal((long_lines, 1))
    A = A.tocsc()
    A.sort_indices()
    data = {"A": A, "b": np.abs(rng.standard_normal(m)) + 0.5, "c": rng.standard_normal(n)}
    if with_P:
        off = sparse.csc_matrix((0.1 * rng.standard_normal(50), (rng.integers(0, n, 50), rng.integers(0, n, 50))), shape=(n, n))
        P = sparse.diags(1.0 + rng.random(n)) + off + off.T
        data["P"] = sparse.csc_matrix(P)
    return data, {"l": m}


MAPPED = re.compile(r"value maps: CSR\(A\) (\d+), CSR\(P\) (\d+); pass layouts A' (\d+), A (\d+), P (\d+) slots "
                    r"\(peeled rows (\d+), (\d+), (\d+); pieces (\d+), (\d+), (\d+)\)")


def mapped_layouts(capfd):
    """what the first update_matrix mapped, off the line the library prints under SCS_HIP_DEBUG=setup (matrix_update.hpp)"""
    found = MAPPED.findall(capfd.readouterr().err)
    assert len(found) == 1, found
    v = [int(x) for x in found[0]]
    return {"csr": v[0:2], "pass": v[2:5], "peeled": v[5:8], "pieces": v[8:11]}  # (pass / peeled / pieces: A', A, P)


def pass_layout_case(monkeypatch, capfd, variant, split):
    monkeypatch.setenv("SCS_HIP_CS", "2")
    monkeypatch.setenv("SCS_HIP_CS_SPLIT", split)
    monkeypatch.setenv("SCS_HIP_DEBUG", "setup")
    data, K = pass_problem({"long_lines": 70, "dense_lines": LONG}.get(variant, 0), variant == "with_P")
    A2 = new_values(data["A"], 62)
    new = {"A": A2}
    if variant == "with_P":
        new["P"] = new_psd_values(data["P"], 63)
    sv = fresh(data, K, max_iters=40)
    first = sv.solve(warm_start=False)
    assert "column-sorted pass" in first["info"]["lin_sys_solver"], first["info"]["lin_sys_solver"]
    capfd.readouterr()
    sv.update_matrix(**new)
    mapped = mapped_layouts(capfd)
    got = sv.solve(warm_start=False)
    same_result(got, fresh(with_(data, **new), K, max_iters=40).solve(warm_start=False))
    assert not np.array_equal(got["x"], first["x"])
    return sv, data, K, A2, got, mapped


@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("variant", ["plain", "long_lines", "dense_lines", "with_P"])
def test_pass_layout(monkeypatch, capfd, variant, split):
    sv, data, K, A2, got, mapped = pass_layout_case(monkeypatch, capfd, variant, split)
    assert mapped["pass"][0] > 0 and mapped["pass"][1] > 0, mapped  # both orientations of A have a pass copy, and it was mapped
    if variant == "with_P":  # ... and so has P
        assert mapped["pass"][2] > 0 and mapped["csr"][1] > 0, mapped
    if variant == "dense_lines":  # the lines really are in virtual-row pieces, in both orientations: that branch of the map builder ran
        assert "long rows in pieces" in got["info"]["lin_sys_solver"], got["info"]["lin_sys_solver"]
        assert mapped["pieces"][0] > 0 and mapped["pieces"][1] > 0, mapped
    else:
        assert mapped["pieces"] == [0, 0, 0] and mapped["peeled"] == [0, 0, 0], mapped
    if variant != "long_lines" and split == "1":  # the device entry on these layouts
        tw = fresh(data, K, max_iters=40)
        tw.update_matrix_device(A=dev(A2.data), **({"P": dev(new_psd_values(data["P"], 63).data)} if variant == "with_P" else {}))
        same_result(tw.solve(warm_start=False), got, "device entry")


@pytest.mark.labs
@pytest.mark.parametrize("split", ["0", "1"])
def test_pass_layout_with_peeled_rows(monkeypatch, capfd, split):
    """SCS_HIP_CS_VIRT=0 (a switch of the labs build): the dense lines are peeled off the passes instead of cut into pieces — the peel-mask
    branch of the map builder, which the product reaches only where the virtual-row plan fails"""
    monkeypatch.setenv("SCS_HIP_CS_VIRT", "0")
    sv, data, K, A2, got, mapped = pass_layout_case(monkeypatch, capfd, "dense_lines", split)
    assert "long rows peeled" in got["info"]["lin_sys_solver"], got["info"]["lin_sys_solver"]
    assert mapped["peeled"][0] > 0 and mapped["peeled"][1] > 0 and mapped["pieces"] == [0, 0, 0], mapped


# ---- 5. slab -------------------------------------------------------------------------------------------------------------------
def test_slab_layout(monkeypatch):
    monkeypatch.setenv("SCS_HIP_CS", "0")
    rng = np.random.default_rng(5)
    A = pg.random_sparse(300000, 270000, 7, rng)
    data = {"A": A, "b": np.abs(rng.standard_normal(300000)) + 0.5, "c": rng.standard_normal(270000)}
    K = {"l": 300000}
    A2 = new_values(A, 71)
    sv = fresh(data, K, max_iters=20)
    first = sv.solve(warm_start=False)
    assert "L2-blocked slab" in first["info"]["lin_sys_solver"], first["info"]["lin_sys_solver"]
    sv.update_matrix(A=A2)
    same_result(sv.solve(warm_start=False), fresh(with_(data, A=A2), K, max_iters=20).solve(warm_start=False))


# ---- 6. sequence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qp", [False, True], ids=["lp", "qp"])
def test_sequence_reuses_maps_and_staging(qp):
    data, K = dio.golden_qp() if qp else dio.problem("A")
    A2, A3, A4 = (new_values(data["A"], s) for s in (81, 82, 83))
    b2, c2 = dio.new_bc(data, np.random.default_rng(84))
    sv = fresh(data, K)
    sv.update_matrix(A=A2)
    sv.update(b2, c2)
    sv.update_matrix(A=A3)
    before = _scs_hip.pool_stats()["misses"]
    sv.update_matrix(A=A4)
    assert _scs_hip.pool_stats()["misses"] == before, "the third update allocated new device blocks"
    same_result(sv.solve(warm_start=False), fresh(with_(data, A=A4, b=b2, c=c2), K).solve(warm_start=False))
    # b, c that arrived on the device (the host mirror is stale) are the current ones too
    sv.update_device(dev(data["b"]), dev(data["c"]))
    sv.update_matrix(A=A2)
    same_result(sv.solve(warm_start=False), fresh(with_(data, A=A2), K).solve(warm_start=False), "after update_device")


# ---- 7. device entry -----------------------------------------------------------------------------------------------------------
def test_device_entry_equals_host_entry():
    data, K = dio.problem("A")
    A2 = new_values(data["A"], 91)
    d, h = fresh(data, K), fresh(data, K)
    d.update_matrix_device(A=dev(A2.data))
    h.update_matrix(A=A2.data)  # (values alone: the second form of the argument)
    ref = h.solve(warm_start=False)
    same_result(d.solve(warm_start=False), ref)
    # inputs produced on torch's stream right before the call
    src = dev(A2.data)
    big = torch.ones(1 << 22, dtype=torch.float64, device=src.device)
    for _ in range(8):  # work queued in front of the copy on torch's current stream
        big = big * 1.0000001
    vals = src.clone()
    d.update_matrix_device(A=vals)
    same_result(d.solve(warm_start=False), ref, "stream-ordered input")
    dq, Kq = dio.golden_qp()
    P2 = new_psd_values(dq["P"], 92)
    q = fresh(dq, Kq)
    q.update_matrix_device(P=dev(P2.data))
    same_result(q.solve(warm_start=False), fresh(with_(dq, P=P2), Kq).solve(warm_start=False), "P on the device")


# ---- 8. interplay --------------------------------------------------------------------------------------------------------------
def test_solve_many_clones_and_batches():
    data, K = dio.problem("A")
    A2 = new_values(data["A"], 101)
    rng = np.random.default_rng(102)
    bs = np.stack([data["b"] * (1 + 0.05 * k) for k in range(3)])
    sv = fresh(data, K)
    sv.solve_many(b=bs)  # (caches two clones on the solver)
    sv.update_matrix(A=A2)
    many = sv.solve_many(b=bs)
    for k in range(3):
        same_grouped(many[k], fresh(with_(data, A=A2, b=bs[k]), K).solve(warm_start=False), "solve_many member %d" % k)
    # a clone the USER holds: refused, and the solver still solves with its old matrix
    sv, twin = fresh(data, K), fresh(data, K)  # (the twin solves as often as sv, and nothing else)
    same_result(sv.solve(warm_start=False), twin.solve(warm_start=False), "before the refusal")
    cl = sv.clone()
    with pytest.raises(ValueError, match="shared by 2 workspaces"):
        sv.update_matrix(A=A2)
    same_result(sv.solve(warm_start=False), twin.solve(warm_start=False), "after the refusal")
    del cl
    # a clone taken AFTER an update: the new matrices, the original b, c
    b2, c2 = dio.new_bc(data, rng)
    sv.update(b2, c2)
    sv.update_matrix(A=A2)
    same_result(sv.clone().solve(warm_start=False), fresh(with_(data, A=A2), K).solve(warm_start=False), "clone after update")
    # solve_batch of three updated workspaces = their solo solves
    mats = [new_values(data["A"], 110 + k) for k in range(3)]
    grp = [fresh(data, K) for _ in range(3)]
    for g, M in zip(grp, mats):
        g.update_matrix(A=M)
    for got, M in zip(scs.solve_batch(grp), mats):
        same_grouped(got, fresh(with_(data, A=M), K).solve(warm_start=False), "solve_batch")


# ---- 9. refusals leave the workspace usable ------------------------------------------------------------------------------------
def test_refusals_leave_the_workspace_unchanged():
    data, K = dio.problem("B")
    A = data["A"]
    sv, twin = fresh(data, K), fresh(data, K)  # the twin solves as often as sv and is never asked for anything else
    same_result(sv.solve(warm_start=False), twin.solve(warm_start=False), "first solve")
    moved = A.tolil()
    r, c = next((r, c) for r in range(A.shape[0]) for c in range(A.shape[1]) if A[r, c] == 0)
    moved[r, c] = 1.0
    cases = [
        (ValueError, lambda: sv.update_matrix(A=A.data[:-1])),                       # wrong length
        (ValueError, lambda: sv.update_matrix(A=moved.tocsc())),                     # changed pattern
        (ValueError, lambda: sv.update_matrix(P=sparse.eye(A.shape[1], format="csc"))),  # P without P
        (ValueError, lambda: sv.update_matrix_device(A=torch.zeros(A.nnz, dtype=torch.float64))),  # tensor on the CPU
        (TypeError, lambda: sv.update_matrix_device(A=torch.zeros(A.nnz, dtype=torch.float32).cuda())),  # float32 tensor
    ]
    for exc, call in cases:
        with pytest.raises(exc):
            call()
        same_result(sv.solve(warm_start=False), twin.solve(warm_start=False), "after a refusal")
    sv.update_matrix()  # both None: a no-op
    same_result(sv.solve(warm_start=False), twin.solve(warm_start=False), "after the no-op")
