"""GPU parity tests (run with -m gpu on an MI355X): every hot-path kernel and the
whole ADMM loop against the CPU oracle, through the C-ABI (ctypes -> libscs_hip.so).

Tolerances: SpMV bit-exact (same per-row summation order as the oracle);
SOC / PSD / box / power / exp projections 1e-9 .. 1e-7 absolute; KKT solve 1e-8
relative; full solves: x, y, s within rtol 1e-4 of the oracle's direct-LDL answer
at eps = 1e-9 (the notion of cross-backend agreement the reference itself tests,
R:test/test_scs_coverage.py:2060-2080), objective within 1e-6 of p*.
"""
import numpy as np
import pytest
from scipy import sparse

import helpers
import problem_gen as pg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from scs import _scs_hip
    assert _scs_hip.device_count() > 0, "GPU tests need a HIP device (no CPU fallback exists)"
    return _scs_hip


@pytest.fixture(scope="module")
def oracle():
    from oracle import scs_oracle
    return scs_oracle


def _rand_csc(m, n, density, seed, long_rows=False):
    rng = np.random.RandomState(seed)
    A = sparse.rand(m, n, density, format="csc", random_state=rng)
    A.data = rng.randn(A.nnz)
    if long_rows:  # a few dense rows / columns exercise the long-row path (> 2048 nnz)
        A = A.tolil()
        A[3, :] = rng.randn(n)
        A[:, 5] = rng.randn(m).reshape(-1, 1)
        A = A.tocsc()
    A.sort_indices()
    return A


@pytest.mark.parametrize("m,n,density,long_rows", [
    (50, 30, 0.2, False), (1000, 700, 0.01, False), (5000, 4000, 0.002, True),
    (300, 1, 0.5, False), (1, 300, 0.5, False), (4000, 3000, 0.0, False),
])
def test_spmv_bit_exact(hip, oracle, m, n, density, long_rows):
    A = _rand_csc(m, n, density, 11, long_rows)
    rng = np.random.RandomState(5)
    x, y = rng.randn(n), rng.randn(m)
    for trans, vec in ((False, x), (True, y)):
        got, ref = hip.spmv(A, vec, transpose=trans), oracle.spmv(A, vec, trans=trans)
        # rows longer than one LDS stage (2048 nnz) are reduced by a whole workgroup in a fixed
        # tree order (still run-to-run deterministic, but not the oracle's sequential order)
        counts = np.diff((A.tocsr() if not trans else A.T.tocsr()).indptr)
        short = counts <= 2048
        np.testing.assert_array_equal(got[short], ref[short])
        np.testing.assert_allclose(got[~short], ref[~short], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cs", ["1", "0"], ids=["column-sorted", "slab"])
def test_spmv_slab_layout_bit_exact(hip, oracle, monkeypatch, cs):
    monkeypatch.setenv("SCS_HIP_CS_SPLIT", "0")  # one workgroup per row chunk: sequential per-row sums (see below for the split)
    """large gather vector (> 2 MiB) + many rows => the column-sorted pass kernel (or, SCS_HIP_CS=0, the L2-blocked
    slab kernel) is selected; it must reproduce the CSR-stream / oracle summation order bit for bit (incl. a
    dense-ish row and column)."""
    monkeypatch.setenv("SCS_HIP_CS", cs)
    rng = np.random.default_rng(17)
    m, n = 70000, 300000
    A = pg.random_sparse(m, n, 4, rng).tolil()
    A[123, :5000] = rng.standard_normal(5000)      # long row: spans one slab densely
    A = A.tocsc()
    A.sort_indices()
    x, y = rng.standard_normal(n), rng.standard_normal(m)
    got, ref = hip.spmv(A, x), oracle.spmv(A, x)          # CSR(A): rows=m, cols=n
    if cs == "1":  # the 5000-nonzero row is peeled off the passes and reduced by a whole workgroup (fixed tree)
        long_row = np.zeros(m, dtype=bool)
        long_row[123] = True
        np.testing.assert_array_equal(got[~long_row], ref[~long_row])
        np.testing.assert_allclose(got[long_row], ref[long_row], rtol=1e-12, atol=1e-12)
    else:
        np.testing.assert_array_equal(got, ref)
    At = A.T.tocsc()
    At.sort_indices()
    np.testing.assert_array_equal(hip.spmv(At, x, transpose=True)[np.arange(m) != 123], oracle.spmv(At, x, trans=True)[np.arange(m) != 123])
    np.testing.assert_allclose(hip.spmv(At, x, transpose=True)[123], oracle.spmv(At, x, trans=True)[123], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", helpers.load_projection_cases(), ids=lambda c: c[0])
def test_cone_projection_vs_oracle_and_golden(hip, oracle, case):
    tag, K, z, gproj, gdual = case
    if z.size == 0:
        return
    for dual, gold in ((False, gproj), (True, gdual)):
        got = hip.proj_cone(z, K, dual=dual)
        ref = oracle.proj_cone(z, K, dual=dual)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-8 * max(1.0, np.abs(z).max()))
        # goldens: the reference's Python exp bisection stops at 1e-9 on rho with an inner
        # Newton tolerance of 1e-6 (R:test/gen_random_cone_prob.py:259-313) => 1e-4 there
        np.testing.assert_allclose(got, gold, rtol=0, atol=1e-4 * max(1.0, np.abs(z).max()))


def test_cone_projection_large_mixed(hip, oracle):
    rng = np.random.RandomState(3)
    K = {"z": 100, "l": 300, "bu": (rng.rand(99) + 0.1).tolist(), "bl": (-rng.rand(99) - 0.1).tolist(),
         "q": [20] * 50 + [5000, 1, 0, 2], "s": [1, 2, 7, 16, 33], "ep": 500, "ed": 500,
         "p": (rng.uniform(0.1, 0.9, 400) * rng.choice([-1, 1], 400)).tolist()}
    m = pg.cone_dims(K)
    for scl in (1.0, 25.0):
        z = scl * rng.randn(m)
        for dual in (False, True):
            got = hip.proj_cone(z, K, dual=dual)
            ref = oracle.proj_cone(z, K, dual=dual)
            np.testing.assert_allclose(got, ref, rtol=0, atol=2e-8 * scl)


@pytest.mark.parametrize("qmax", [2, 9, 10, 17, 18, 33, 34, 200])
def test_soc_lane_groups_vs_oracle(hip, oracle, qmax):
    """short second-order cones share a wavefront in lane groups of 8/16/32/64 (cones.hpp soc_group, chosen from the
    longest cone): every group width against the oracle, with ragged counts (a last wave partly empty), q = 0/1/2
    members, interior / polar / boundary points — and the SAME bits whichever width the other cones forced."""
    rng = np.random.RandomState(qmax)
    q = [int(v) for v in rng.randint(0, qmax + 1, 203)] + [qmax, 1, 0, 2][: 1 + (qmax % 4)]
    K = {"l": 3, "q": q}
    m = pg.cone_dims(K)
    z = rng.randn(m)
    o = 3
    for i, d in enumerate(q):           # a third inside, a third in the polar cone, the rest outside
        if d > 0 and i % 3 == 0:
            z[o] = np.linalg.norm(z[o + 1:o + d]) + 0.5
        elif d > 0 and i % 3 == 1:
            z[o] = -np.linalg.norm(z[o + 1:o + d]) - 0.5
        o += d
    for dual in (False, True):
        got, ref = hip.proj_cone(z, K, dual=dual), oracle.proj_cone(z, K, dual=dual)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13 * max(1.0, np.abs(z).max()))
    K64 = {"l": 3, "q": q + [300]}      # one long cone forces full-wave groups for all of them
    z64 = np.concatenate([z, rng.randn(300)])
    np.testing.assert_array_equal(hip.proj_cone(z64, K64)[:m], hip.proj_cone(z, K))


@pytest.mark.parametrize("nb,scl,shift", [(20000, 1.0, 0.0), (50001, 10.0, 5.0), (17000, 1.0, -1e5), (100000, 0.3, 2.0)])
def test_box_cone_many_workgroups_vs_oracle(hip, oracle, nb, scl, shift):
    """box cones beyond 16384 bounds run the Newton iteration on t as one launch per round over many workgroups
    (last-arriver reduction); same answer as the oracle's sequential Newton, primal and dual, incl. t* = 0
    (shift << 0) and a repeated call (device-side warm start of t)"""
    rng = np.random.RandomState(nb % 97)
    K = {"l": 7, "bu": (rng.rand(nb) * 2 + 0.1).tolist(), "bl": (-rng.rand(nb) * 2 - 0.1).tolist(), "q": [5]}
    z = scl * rng.randn(pg.cone_dims(K))
    z[7] += shift  # the t entry
    for dual in (False, True):
        ref = oracle.proj_cone(z, K, dual=dual)
        got = hip.proj_cone(z, K, dual=dual)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-8 * max(1.0, np.abs(z).max()))
        np.testing.assert_array_equal(hip.proj_cone(z, K, dual=dual), got)  # run-to-run: fixed-order reduction
    if shift < -10:
        assert hip.proj_cone(z, K)[7] == 0.0 and oracle.proj_cone(z, K)[7] == 0.0


@pytest.mark.parametrize("with_P", [False, True])
def test_kkt_solve_vs_direct_ldl(hip, oracle, with_P):
    m, n = 600, 250
    A = _rand_csc(m, n, 0.03, 21)
    rng = np.random.RandomState(8)
    P = None
    if with_P:
        B = sparse.rand(n, n, 0.02, format="csc", random_state=rng)
        P = sparse.triu(B.T @ B + sparse.eye(n) * 0.1, format="csc")
        P.sort_indices()
    diag_r = np.concatenate([np.full(n, 1e-3), np.full(50, 0.01), np.full(m - 50, 10.0)])
    rhs = rng.randn(n + m)
    ref, _ = oracle.kkt_solve(A, P, diag_r, rhs, indirect=False)
    got, its = hip.kkt_solve(A, P, diag_r, rhs, tol=1e-13)
    assert its > 0
    np.testing.assert_allclose(got, ref, rtol=1e-7, atol=1e-8 * np.abs(ref).max())


def test_kkt_solve_large_layouts_agree(hip, monkeypatch):
    """the fused CG epilogues (K1/K2/K1'/K2' + P) on the three matrix layouts: column-sorted passes, L2-blocked
    slabs and plain CSR-stream solve the same KKT system to the same answer (the CSR-stream path is the one
    checked against the oracle's LDL above; partial sums are partitioned differently => tolerance, not bits)"""
    rng = np.random.default_rng(31)
    m, n = 330000, 280000
    A = pg.random_sparse(m, n, 6, rng)
    B = pg.random_sparse(n, n, 2, rng)
    P = sparse.triu(B + B.T + sparse.eye(n) * 12.0, format="csc")  # diagonally dominant => PSD
    P.sort_indices()
    diag_r = np.concatenate([np.full(n, 1e-2), np.full(1000, 0.05), np.full(m - 1000, 8.0)])
    rhs = rng.standard_normal(n + m)
    sols = {}
    for name, env in (("cs", {}), ("slab", {"SCS_HIP_CS": "0"}), ("stream", {"SCS_HIP_SLAB": "0"})):
        for k in ("SCS_HIP_CS", "SCS_HIP_SLAB"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sols[name], its = hip.kkt_solve(A, P, diag_r, rhs, tol=1e-12)
        assert its > 0
    scl = np.abs(sols["stream"]).max()
    np.testing.assert_allclose(sols["cs"], sols["stream"], rtol=0, atol=1e-9 * scl)
    np.testing.assert_allclose(sols["slab"], sols["stream"], rtol=0, atol=1e-9 * scl)


STG = dict(eps_abs=1e-9, eps_rel=1e-9, eps_infeas=1e-9, verbose=False)


def _solve_both(hip, oracle, data, K, **kw):
    stg = dict(STG)
    stg.update(kw)
    args = helpers.raw_args(data, K)
    got = hip.SCS(*args, **stg).solve(False, None, None, None)
    ref = oracle.OracleSCS(*args, indirect=False, **stg).solve(False)
    return got, ref


def _assert_xys(got, ref, rtol=1e-4, keys=("x", "y", "s")):
    for key in keys:
        scale = np.abs(ref[key]).max()
        np.testing.assert_allclose(got[key], ref[key], rtol=rtol, atol=rtol * scale, err_msg=key)


@pytest.mark.parametrize("fname,prefix", [
    ("problems_std.npz", "std_feas_"), ("problems_rand.npz", "feas0_"), ("problems_rand.npz", "feas1_"),
    ("problems_sdp.npz", "feas0_"), ("problems_sdp.npz", "feas2_"),
])
def test_solve_feasible_golden(hip, oracle, fname, prefix):
    data, K, p_star = helpers.load_problem(fname, prefix)
    got, ref = _solve_both(hip, oracle, data, K)
    assert got["info"]["status"] == "solved" and ref["info"]["status"] == "solved"
    assert abs(got["info"]["pobj"] - p_star) < 1e-5 * max(1, abs(p_star))
    assert abs(-data["b"] @ got["y"] - p_star) < 1e-5 * max(1, abs(p_star))
    # These generator instances have m ~ 3n: about m/2 constraints are active at the optimum, more
    # than n, so the primal is degenerate and the DUAL solution is not unique (the oracle's own LDL
    # and CG variants land on different y with identical 1e-9 certificates).  x and s are unique and
    # are compared entry-wise; y is pinned by its certificate, as the reference's tests do
    # (R:test/test_solve_random_cone_prob.py:55-65).  Unique-dual instances: test_*_generated_parity.
    if prefix == "std_feas_":
        _assert_xys(got, ref, keys=("x", "s"))
    assert abs(got["info"]["pobj"] - ref["info"]["pobj"]) < 1e-6 * max(1, abs(p_star))
    pri, dual, gap = helpers.kkt_certificate(data, got)
    assert pri < 1e-6 and dual < 1e-6 and gap < 1e-6
    # cone membership through the oracle's projections (R:test/test_solve_random_cone_prob.py:63-65)
    np.testing.assert_allclose(got["s"], oracle.proj_cone(got["s"], K), atol=1e-6)
    np.testing.assert_allclose(got["y"], oracle.proj_cone(got["y"], K, dual=True), atol=1e-6)


@pytest.mark.parametrize("fname,prefix", [("problems_std.npz", "std_infeas_"), ("problems_rand.npz", "infeas0_"),
                                          ("problems_sdp.npz", "infeas1_")])
def test_solve_infeasible_golden(hip, oracle, fname, prefix):
    data, K, _ = helpers.load_problem(fname, prefix)
    got, ref = _solve_both(hip, oracle, data, K, eps_infeas=1e-7)
    assert got["info"]["status"] == "infeasible" and ref["info"]["status"] == "infeasible"
    y = got["y"]
    assert np.linalg.norm(data["A"].T @ y) < 1e-3 and data["b"] @ y < -0.1
    np.testing.assert_allclose(y, oracle.proj_cone(y, K, dual=True), atol=1e-4)
    assert np.isnan(got["x"]).all() and np.isnan(got["s"]).all()


@pytest.mark.parametrize("fname,prefix", [("problems_std.npz", "std_unbdd_"), ("problems_rand.npz", "unbdd0_"),
                                          ("problems_sdp.npz", "unbdd1_")])
def test_solve_unbounded_golden(hip, oracle, fname, prefix):
    """reference-generated unbounded instances (R:test/gen_random_cone_prob.py gen_unbounded): the HIP path next to
    the oracle's LDL' — status, the certificate (R:test/test_solve_random_cone_prob.py:82-91) checked in numpy, and
    the normalisation c'x = -1 both produce"""
    data, K, _ = helpers.load_problem(fname, prefix)
    got, ref = _solve_both(hip, oracle, data, K, eps_infeas=1e-7)
    assert got["info"]["status"] == "unbounded" and ref["info"]["status"] == "unbounded"
    for sol in (got, ref):
        x, s = sol["x"], sol["s"]
        assert np.linalg.norm(data["A"] @ x + s) < 1e-3 and data["c"] @ x < -0.1
        assert abs(data["c"] @ x + 1.0) < 1e-9
        np.testing.assert_allclose(s, oracle.proj_cone(s, K), atol=1e-4)
        assert np.isnan(sol["y"]).all()
    assert got["info"]["pobj"] == -np.inf and got["info"]["dobj"] == -np.inf
    assert got["info"]["res_unbdd_a"] < 1e-6 and ref["info"]["res_unbdd_a"] < 1e-6


def test_config1_lp_golden_against_stored_optimum_and_oracle(hip, oracle):
    """BASELINE.json configs[0]: the reference-generated LP (K = {l: 4000}, n = 2000; tests/golden/make_golden.py, p*
    cross-checked with HiGHS there) through the HIP path: stored optimum, the oracle's LDL' answer, certificate"""
    data, K, p_star = helpers.load_problem("problem_config1_lp.npz", "lp_")
    # (eps = 1e-6: at 1e-8 the indirect path needs more than the default 1e5 iterations on this degenerate LP)
    got = hip.SCS(*helpers.raw_args(data, K), **dict(STG, eps_abs=1e-6, eps_rel=1e-6)).solve(False, None, None, None)
    ref = helpers.oracle_result("config1_ldl_1e-6")   # oracle.OracleSCS(*args, indirect=False, same settings).solve(False), started when the collection was done
    assert got["info"]["status"] == "solved" and ref["info"]["status"] == "solved"
    assert abs(got["info"]["pobj"] - p_star) <= 1e-5 * max(1.0, abs(p_star))
    assert abs(got["info"]["pobj"] - ref["info"]["pobj"]) <= 1e-5 * max(1.0, abs(p_star))
    # m = 2n: about n constraints are active at the optimum, so x sits on a nearly singular active set (two 1e-6
    # certificates differ by 2e-4 of the largest entry) and the dual is not unique: x, s at 1e-3, y by its certificate
    _assert_xys(got, ref, rtol=1e-3, keys=("x", "s"))
    pri, dual, gap = helpers.kkt_certificate(data, got)
    scale = max(1.0, np.abs(data["b"]).max(), np.abs(data["c"]).max(), abs(p_star))
    assert pri < 1e-5 * scale and dual < 1e-5 * scale and gap < 1e-5 * scale
    assert got["y"].min() > -1e-7 and got["s"].min() > -1e-7


def test_psd_every_small_order_against_lapack(hip):
    """orders 1..32 run in the four-wavefront kernel (psd.hpp d_proj_psd_small4: rows / columns move between fixed positions, odd orders
    padded to even): every order, several matrices per launch, against numpy's eigh — random spectra, a matrix that is already PSD,
    one that is negative definite and one of rank 1"""
    rng = np.random.default_rng(2)
    for order in range(1, 33):
        mats = []
        for kind in range(5):
            G = rng.standard_normal((order, order))
            X = (G + G.T) / 2
            if kind == 2:
                X = G @ G.T + 0.1 * np.eye(order)
            elif kind == 3:
                X = -(G @ G.T) - 0.1 * np.eye(order)
            elif kind == 4:
                v = rng.standard_normal(order)
                X = np.outer(v, v) - 0.5 * np.eye(order)
            mats.append(X)
        z = np.concatenate([helpers.sym_to_svec(X) for X in mats])
        K = {"s": [order] * len(mats)}
        want = helpers.proj_dual_l_s_numpy(z, K)
        got = hip.proj_cone(z, K, dual=True)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()), err_msg="order %d" % order)
        np.testing.assert_allclose(hip.proj_cone(z, K, dual=True), got, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))   # again


@pytest.mark.parametrize("cone,order", [("s", 1500), ("cs", 600)])
def test_psd_orders_beyond_1024(hip, cone, order):
    """PSD order 1500 / complex PSD order 600 (embedding 1200): refused by this backend in rounds 1-2 (pivots per step
    of the block-Jacobi kernels), valid for the reference (R:scs/scsobject.h:726-737).  Against LAPACK's eigh."""
    rng = np.random.default_rng(order)
    if cone == "s":
        G = rng.standard_normal((order, order))
        X = (G + G.T) / 2
        z = helpers.sym_to_svec(X)
        want = helpers.proj_dual_l_s_numpy(z, {"s": [order]})
        got = hip.proj_cone(z, {"s": [order]}, dual=True)
    else:
        G = rng.standard_normal((order, order)) + 1j * rng.standard_normal((order, order))
        z = helpers.herm_to_cvec((G + G.conj().T) / 2)
        want = helpers.proj_hermitian_psd(z, order)
        got = hip.proj_cone(z, {"cs": [order]}, dual=True)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(want).max())


def test_lp_soc_generated_parity(hip, oracle):
    K, n, k, seed = pg.workload("small_lp_soc")
    data, p_star, (x0, y0, s0) = pg.gen_feasible(K, n, k, seed, lambda z, K: oracle.proj_cone(z, K, dual=True))
    got, ref = _solve_both(hip, oracle, data, K)
    assert got["info"]["status"] == "solved"
    assert abs(got["info"]["pobj"] - p_star) < 1e-6 * max(1, abs(p_star))
    _assert_xys(got, ref)


@pytest.mark.parametrize("K,n,k,seed", [
    ({"z": 50, "l": 400, "q": [3, 10, 25, 1], "ep": 20, "ed": 20, "p": [0.3, -0.6, 0.5, -0.2] * 5}, 420, 12, 31),
    ({"l": 300, "q": [8] * 10, "s": [6, 9, 12]}, 380, 10, 32),
    ({"z": 20, "l": 200, "bu": [1.0] * 30, "bl": [-0.5] * 30, "q": [12] * 5}, 250, 10, 33),
])
def test_mixed_cones_generated_parity(hip, oracle, K, n, k, seed):
    """Strictly convex QP (P > 0) with n above the number of active rows: the primal AND the dual
    solution are unique, so x, y, s are all compared entry-wise — against the oracle's direct-LDL
    answer and against the (x, y, s) the instance was constructed from."""
    data, p_star, (x0, y0, s0) = pg.gen_feasible_qp(K, n, k, seed, lambda z, K: oracle.proj_cone(z, K, dual=True))
    got, ref = _solve_both(hip, oracle, data, K)
    assert got["info"]["status"] == "solved" and ref["info"]["status"] == "solved"
    assert abs(got["info"]["pobj"] - p_star) < 1e-6 * max(1, abs(p_star))
    _assert_xys(got, ref)
    _assert_xys(got, {"x": x0, "y": y0, "s": s0})


def test_iteration_counts_track_oracle_cg(hip, oracle):
    """Same algorithm => the ADMM iteration count follows the oracle's CPU-CG variant closely once the
    two chaotic amplifiers are off: Anderson acceleration and the adaptive-scale branch (a scale update
    fires when a running geometric mean crosses sqrt(10); a 1e-13 difference in a projection can flip
    that decision and send the two runs down different, equally valid, paths)."""
    data, K, _ = helpers.load_problem("problems_std.npz", "std_feas_")
    args = helpers.raw_args(data, K)
    stg = dict(STG, acceleration_lookback=0, adaptive_scale=False, eps_abs=1e-6, eps_rel=1e-6)
    got = hip.SCS(*args, **stg).solve(False, None, None, None)
    ref = helpers.oracle_result("std_feas_cg_plain_1e-6")   # oracle.OracleSCS(*args, indirect=True, **stg).solve(False), started when the collection was done
    assert got["info"]["status"] == ref["info"]["status"] == "solved"
    gi, ri = got["info"], ref["info"]
    assert abs(gi["iter"] - ri["iter"]) <= 0.05 * ri["iter"] + 25, (gi["iter"], ri["iter"])
    assert abs(gi["cg_iters"] - ri["cg_iters"]) <= 0.05 * ri["cg_iters"] + 50, (gi["cg_iters"], ri["cg_iters"])


def test_qp_with_P_parity(hip, oracle):
    d = np.load(helpers.GOLDEN + "/warm_start_qp.npz")
    P = sparse.csc_matrix((d["P_data"], d["P_indices"], d["P_indptr"]), shape=(15, 15))
    G = sparse.csc_matrix((d["G_data"], d["G_indices"], d["G_indptr"]), shape=(60, 15))
    data = {"P": P, "A": G, "b": d["h"].copy(), "c": d["q"].copy()}
    # The reference runs this regression QP (R:test/test_warm_start_consistency.py:228-241) on its
    # direct backend only.  Its adaptive scale falls to 1e-4, where the reduced system
    # R_x + P + A'R_y^{-1}A has eigenvalues ~1e-6 and an absolute CG residual floor of 1e-12 caps
    # the attainable accuracy near 1e-6 (the oracle's CPU-CG variant stalls identically), so the
    # indirect path is compared at eps = 1e-5.
    got, ref = _solve_both(hip, oracle, data, {"l": 60}, eps_abs=1e-5, eps_rel=1e-5, eps_infeas=1e-7)
    assert got["info"]["status"] == "solved" and ref["info"]["status"] == "solved"
    assert abs(got["info"]["pobj"] - ref["info"]["pobj"]) < 1e-6
    # |x*| ~ 1e-5 here, below eps_abs: entry-wise comparison is meaningless; certificates instead
    Pu = sparse.triu(P)
    Pf = Pu + sparse.triu(Pu, 1).T
    pri, dual, gap = helpers.kkt_certificate(data, got, P=Pf)
    assert pri < 1e-4 and dual < 1e-4 and gap < 1e-4


def test_determinism_bit_exact(hip):
    # R:test/test_scs_coverage.py:2283-2301 — two fresh instances give identical bits
    data, K, _ = helpers.load_problem("problems_std.npz", "std_feas_")
    args = helpers.raw_args(data, K)
    a = hip.SCS(*args, verbose=False).solve(False, None, None, None)
    b = hip.SCS(*args, verbose=False).solve(False, None, None, None)
    for key in ("x", "y", "s"):
        np.testing.assert_array_equal(a[key], b[key])
    assert a["info"]["iter"] == b["info"]["iter"]


@pytest.mark.parametrize("n", [400, 40000])
def test_determinism_bit_exact_with_P(hip, oracle, n):
    """the QP path (K3: Gp = P p on the full symmetric CSR of P, csrc/work.hpp Pf) under the same rule
    (R:test/test_scs_coverage.py:2283-2301): no float atomics, fixed summation order — two fresh instances give identical bits.
    n = 40000: nnz(Pf) > 2^20, so K3 runs on the column-sorted pass layout the large-matrix kernels read; and the product P x of
    the solver's layout is checked entry for entry against scipy through the kernel-level entry point."""
    K = {"l": n, "q": [10] * (n // 10)}
    data, p_star, _ = pg.gen_feasible_qp(K, n, 8, 17, lambda z, K: oracle.proj_cone(z, K, dual=True), b_per_col=4 if n > 1000 else 3)
    args = helpers.raw_args(data, K)
    stg = dict(verbose=False, max_iters=60 if n > 1000 else 2000)
    a = hip.SCS(*args, **stg).solve(False, None, None, None)
    b = hip.SCS(*args, **stg).solve(False, None, None, None)
    for key in ("x", "y", "s"):
        np.testing.assert_array_equal(a[key], b[key])
    assert a["info"]["iter"] == b["info"]["iter"] and a["info"]["cg_iters"] == b["info"]["cg_iters"]
    if n <= 1000:
        assert a["info"]["status"] == "solved" and abs(a["info"]["pobj"] - p_star) <= 1e-3 * max(1.0, abs(p_star))
    Pu = data["P"]
    Pf = (Pu + sparse.triu(Pu, 1).T).tocsc()
    Pf.sort_indices()
    x = np.random.RandomState(3).randn(n)
    got = hip.spmv(Pf, x)
    np.testing.assert_allclose(got, Pf @ x, rtol=1e-12, atol=1e-12 * np.abs(Pf @ x).max())
    np.testing.assert_array_equal(got, hip.spmv(Pf, x))


@pytest.mark.parametrize("with_P", [False, True])
def test_equilibration_matches_oracle(hip, oracle, with_P):
    """K12 runs on the device; D, E, sigma and the scaled data must match the oracle's restatement to a
    few ulp (same pass structure and summation order; device sqrt / the l2-pass order of P's
    contribution may differ in the last bit, compounded over 26 passes)."""
    data, K, _ = helpers.load_problem("problems_sdp.npz", "feas0_")
    A = data["A"]
    n = A.shape[1]
    P = None
    if with_P:
        rng = np.random.RandomState(4)
        B = sparse.rand(n, n, 0.05, format="csc", random_state=rng)
        P = sparse.triu(B.T @ B + sparse.eye(n), format="csc")
        P.sort_indices()
    got = hip.normalize(A, P, data["b"], data["c"], K)
    ref = oracle.normalize(A, P, data["b"], data["c"], K)
    names = ["A", "P", "b", "c", "D", "E"]
    for name, g, r in zip(names, got[:6], ref[:6]):
        if g is None:
            continue
        np.testing.assert_allclose(g, r, rtol=1e-13, atol=0, err_msg=name)
    assert abs(got[6] - ref[6]) <= 1e-13 * ref[6]


@pytest.mark.labs
def test_equilibration_fused_pass_finish_bit_identical(hip, oracle, monkeypatch):
    """round 5: the square roots of the l2 pass, the cone-block rule and both 1/sqrt sweeps of an equilibration pass are ONE launch
    (normalize_dev.hpp k_pass_finish; scs_init of a small problem is bound by the number of runtime calls).  Same operations on the same
    values in the same order: every output must keep its bits — on a cone with one-row blocks (SOC of size 1, PSD of order 1), blocks
    beyond one wavefront's 64 rows (reduced by the shuffle tree), exp / power triples and a box"""
    rng = np.random.RandomState(11)
    K = {"z": 3, "l": 40, "bu": [1.0, 2.0, 0.5], "bl": [-1.0, 0.0, -0.5], "q": [1, 7, 100, 1, 65], "s": [1, 12, 3], "ep": 2, "ed": 1, "p": [0.3, -0.6]}
    m = pg.cone_dims(K)
    n = 60
    A = sparse.rand(m, n, 0.15, format="csc", random_state=rng)
    A.data = rng.randn(A.nnz)
    A.sort_indices()
    B = sparse.rand(n, n, 0.05, format="csc", random_state=rng)
    P = sparse.triu(B.T @ B + sparse.eye(n), format="csc")
    P.sort_indices()
    b, c = rng.randn(m), rng.randn(n)
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SCS_HIP_NORM_FUSE", mode)
        outs[mode] = (hip.normalize(A, None, b, c, K), hip.normalize(A, P, b, c, K))
    for u, v in zip(outs["0"], outs["1"]):
        for x, y in zip(u, v):
            if x is None:
                assert y is None
            else:
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    ref = oracle.normalize(A, P, b, c, K)
    for name, g, r in zip(["A", "P", "b", "c", "D", "E"], outs["1"][1][:6], ref[:6]):
        np.testing.assert_allclose(g, r, rtol=1e-12, atol=0, err_msg=name)


def _random_cone(rng):
    """small random mixed cone (every cone type of the path can appear)"""
    K = {}
    if rng.rand() < 0.5:
        K["z"] = int(rng.randint(1, 6))
    K["l"] = int(rng.randint(3, 25))
    if rng.rand() < 0.4:
        nb = int(rng.randint(1, 6))
        K["bu"] = (rng.rand(nb) + 0.2).tolist()
        K["bl"] = (-rng.rand(nb) - 0.2).tolist()
    if rng.rand() < 0.7:
        K["q"] = [int(t) for t in rng.randint(1, 9, size=rng.randint(1, 4))]
    if rng.rand() < 0.5:
        K["s"] = [int(t) for t in rng.randint(1, 7, size=rng.randint(1, 3))]
    if rng.rand() < 0.4:
        K["ep"] = int(rng.randint(1, 4))
    if rng.rand() < 0.4:
        K["ed"] = int(rng.randint(1, 4))
    if rng.rand() < 0.4:
        K["p"] = (rng.uniform(0.15, 0.85, size=rng.randint(1, 4)) * rng.choice([-1.0, 1.0])).tolist()
    return K


@pytest.mark.parametrize("seed", range(12))
def test_random_mixed_cone_qp_sweep(hip, oracle, seed):
    """Randomised parity sweep: strictly convex QPs over random cone mixes; x, y, s against the oracle's
    direct-LDL solve and against the constructed optimum (rtol 1e-4 of the north star)."""
    rng = np.random.RandomState(1000 + seed)
    K = _random_cone(rng)
    m = pg.cone_dims(K)
    n = m + 2  # n >= m: the active constraint gradients are independent, so y is unique (P > 0 makes x, s unique)
    data, p_star, (x0, y0, s0) = pg.gen_feasible_qp(K, n, min(6, m), 2000 + seed, lambda z, K: oracle.proj_cone(z, K, dual=True))
    got, ref = _solve_both(hip, oracle, data, K)
    assert got["info"]["status"] == "solved" and ref["info"]["status"] == "solved", (K, got["info"], ref["info"])
    assert abs(got["info"]["pobj"] - p_star) < 1e-6 * max(1, abs(p_star))
    _assert_xys(got, ref)
    _assert_xys(got, {"x": x0, "y": y0, "s": s0})


def test_psd_heavy_parity(hip, oracle):
    """config-4 shaped instance at oracle-friendly size: several PSD cones + l, QP for uniqueness."""
    K = {"l": 40, "s": [24, 17, 30, 9]}
    m = pg.cone_dims(K)
    data, p_star, (x0, y0, s0) = pg.gen_feasible_qp(K, int(0.6 * m), 8, 77, lambda z, K: oracle.proj_cone(z, K, dual=True))
    got, ref = _solve_both(hip, oracle, data, K)
    assert got["info"]["status"] == "solved" and ref["info"]["status"] == "solved"
    _assert_xys(got, ref)
    _assert_xys(got, {"x": x0, "y": y0, "s": s0})


@pytest.mark.parametrize("orders,split", [([40, 64, 100], "1"), ([40, 64, 100], "0"), ([200] * 3, "1"), ([33, 128], "0")])
def test_psd_large_orders_warm_path_in_solve(hip, monkeypatch, orders, split):
    """The order > 32 kernel INSIDE a solve: MFMA block Jacobi warm-started from the previous call's eigenvectors,
    Newton-Schulz re-orthogonalisation every 32 calls, second-order reconstruction, split mode (config 4 lives here).
    Strictly convex QP with n >= m: x, y, s are unique, so the answer is compared entry-wise with the optimum the
    instance was constructed from (numpy/LAPACK projections — no oracle, no HIP kernel in the construction)."""
    monkeypatch.setenv("SCS_HIP_PSD_SPLIT", split)
    K = {"l": 50, "s": orders}
    m = pg.cone_dims(K)
    data, p_star, (x0, y0, s0) = pg.gen_feasible_qp(K, m + 2, 6, 40 + len(orders), helpers.proj_dual_l_s_numpy)
    got = hip.SCS(*helpers.raw_args(data, K), **STG).solve(False, None, None, None)
    assert got["info"]["status"] == "solved", got["info"]
    assert got["info"]["iter"] > 64  # past the first re-orthogonalisation
    assert abs(got["info"]["pobj"] - p_star) < 1e-6 * max(1, abs(p_star))
    _assert_xys(got, {"x": x0, "y": y0, "s": s0})
    o = K["l"]
    for k in orders:  # membership: eigenvalues of the s and y blocks
        d = k * (k + 1) // 2
        for vec in (got["s"], got["y"]):
            assert np.linalg.eigvalsh(helpers.svec_to_sym(vec[o:o + d], k)).min() > -1e-7 * max(1.0, np.abs(vec[o:o + d]).max())
        o += d


@pytest.mark.parametrize("split", ["0", "1"])
def test_psd_projection_special_spectra(hip, monkeypatch, split):
    """The block Jacobi (cross-pair pivots, intra-block pairs once per sweep) on spectra that stress a Jacobi method: multiple and
    clustered eigenvalues, low rank, already diagonal, zero, identity multiples, tiny and huge scales, one order per kernel family
    (one wavefront <= 32 < block kernel; 200 = config 4).  Checked against numpy's eigensolver."""
    monkeypatch.setenv("SCS_HIP_PSD_SPLIT", split)
    rng = np.random.RandomState(5)

    def sym_with(eigs):
        k = len(eigs)
        Q, _ = np.linalg.qr(rng.randn(k, k))
        return (Q * np.asarray(eigs)) @ Q.T

    mats = []
    for k in (7, 32, 33, 48, 100, 200):
        mats += [
            sym_with(np.r_[np.ones(k // 2), -np.ones(k - k // 2)]),                      # two eigenvalues, both highly multiple
            sym_with(np.r_[rng.rand(3) + 1, np.zeros(k - 3)]),                           # rank 3, PSD already
            sym_with(np.r_[-(rng.rand(3) + 1), np.zeros(k - 3)]),                        # rank 3, NSD: projection is 0
            sym_with(1.0 + 1e-9 * rng.randn(k)),                                          # cluster at 1
            sym_with(1e-7 * rng.randn(k)),                                                # cluster around 0, both signs
            np.diag(rng.randn(k)),                                                        # diagonal
            np.zeros((k, k)),
            -3.0 * np.eye(k),
            1e-12 * sym_with(rng.randn(k)),                                               # tiny scale
            1e9 * sym_with(rng.randn(k)),                                                 # huge scale
            sym_with(np.sign(rng.randn(k)) * 10.0 ** rng.uniform(-6, 2, k)),              # eight decades
        ]
    K = {"s": [M.shape[0] for M in mats]}
    z = np.concatenate([helpers.sym_to_svec(M) for M in mats])
    got = hip.proj_cone(z, K)
    o = 0
    for M in mats:
        k = M.shape[0]
        d = k * (k + 1) // 2
        w, V = np.linalg.eigh(M)
        want = helpers.sym_to_svec((V * np.maximum(w, 0)) @ V.T)
        scale = max(np.abs(M).max(), 1e-300)
        np.testing.assert_allclose(got[o:o + d], want, rtol=0, atol=2e-11 * k * scale, err_msg="order %d" % k)
        o += d


# ---- complex PSD cone `cs` ---------------------------------------------------------------------
@pytest.mark.parametrize("orders", [[1], [2], [3], [5, 4], [8, 1, 0, 13], [40], [100]])
def test_cs_projection_vs_oracle_and_complex_eigh(hip, oracle, orders):
    rng = np.random.RandomState(sum(orders))
    K = {"l": 3, "cs": orders}
    m = pg.cone_dims(K)
    for scl in (1.0, 30.0):
        z = scl * rng.randn(m)
        for dual in (False, True):
            got = hip.proj_cone(z, K, dual=dual)
            if max(orders) <= 40:  # the oracle's cyclic Jacobi on the 2k x 2k embedding is slow beyond that
                np.testing.assert_allclose(got, oracle.proj_cone(z, K, dual=dual), rtol=0, atol=1e-9 * scl * max(orders))
            o = 3
            for k in orders:  # independent check: numpy's complex Hermitian eigensolver
                np.testing.assert_allclose(got[o:o + k * k], helpers.proj_hermitian_psd(z[o:o + k * k], k), rtol=0,
                                           atol=1e-9 * scl * max(k, 1))
                o += k * k


def _cs_qp(cone, seed, density, p_scale):
    """instance construction of the reference's cs tests (R:test/test_spectral_and_complex_cones.py:55-71)"""
    rng = np.random.RandomState(seed)
    m = pg.cone_dims(cone)
    P = p_scale * sparse.eye(m, format="csc")
    A = sparse.random(m, m, density=density, format="csc", random_state=rng)
    A.data = rng.randn(A.nnz)
    c = rng.randn(m)
    b = A @ rng.randn(m) + np.abs(rng.randn(m))
    return dict(P=P, A=A, b=b, c=c)


@pytest.mark.parametrize("cone,seed", [({"cs": [3]}, 42), ({"cs": [2, 3]}, 123), (dict(z=1, l=2, s=[3], cs=[3]), 456),
                                       (dict(z=1, l=2, s=[3, 4], cs=[5, 4]), 1234)])
def test_cs_solves_reference_cases(hip, oracle, cone, seed):
    """R:test/test_spectral_and_complex_cones.py:121-152, R:test/test_mix_sd_csd_cone.py:31-40 ask for 'solved';
    here additionally x, y, s against the oracle's direct solve (P = I and n = m make them unique)."""
    data = _cs_qp(cone, seed, 0.5, 1.0)
    got, ref = _solve_both(hip, oracle, data, cone)
    assert got["info"]["status"] == "solved" and ref["info"]["status"] == "solved"
    _assert_xys(got, ref)
    pri, dual, gap = helpers.kkt_certificate(data, got, P=data["P"])
    assert pri < 1e-6 and dual < 1e-6 and gap < 1e-6
    o = pg.cone_dims({k: v for k, v in cone.items() if k != "cs"})
    for k in cone["cs"]:
        for vec in (got["s"], got["y"]):
            assert np.linalg.eigvalsh(helpers.cvec_to_herm(vec[o:o + k * k], k)).min() > -1e-7
        o += k * k


def test_cs_generated_parity_larger(hip, oracle):
    K = {"l": 20, "s": [6], "cs": [12, 7]}
    m = pg.cone_dims(K)
    data, p_star, (x0, y0, s0) = pg.gen_feasible_qp(K, m + 2, 6, 91, lambda z, K: oracle.proj_cone(z, K, dual=True))
    got, ref = _solve_both(hip, oracle, data, K)
    assert got["info"]["status"] == "solved" and ref["info"]["status"] == "solved"
    _assert_xys(got, ref)
    _assert_xys(got, {"x": x0, "y": y0, "s": s0})


# ---- K9 split mode (sweeps on one CU + V updates / reconstruction on the others) vs the one-launch kernel ----
def test_psd_split_mode_bit_identical(hip, oracle, monkeypatch):
    monkeypatch.setenv("SCS_HIP_PSD_REFINE", "0")  # strict sweeps (the refinement stage of round 5 exists in split mode only: tests/test_psd_refine_gpu.py)
    rng = np.random.RandomState(11)
    K = {"l": 5, "s": [40, 64, 33, 100], "cs": [20]}
    z = rng.randn(pg.cone_dims(K))
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SCS_HIP_PSD_SPLIT", mode)
        out[mode] = hip.proj_cone(z, K)
    np.testing.assert_array_equal(out["0"], out["1"])
    # and through a full solve (warm-started calls, re-orthogonalisation, several [sweep, apply] rounds)
    K = {"l": 30, "s": [40, 35]}
    data, _, _ = pg.gen_feasible_qp(K, 500, 6, 21, lambda z, K: oracle.proj_cone(z, K, dual=True))
    args = helpers.raw_args(data, K)
    sols = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SCS_HIP_PSD_SPLIT", mode)
        sols[mode] = hip.SCS(*args, eps_abs=1e-7, eps_rel=1e-7, verbose=False, max_iters=5000).solve(False, None, None, None)
    assert sols["0"]["info"]["iter"] == sols["1"]["info"]["iter"]
    assert sols["0"]["info"]["status"] == sols["1"]["info"]["status"] == "solved", sols["0"]["info"]
    for key in ("x", "y", "s"):
        np.testing.assert_array_equal(sols["0"][key], sols["1"][key], err_msg=key)


# ---- K9 split mode, sweeps of one matrix spread over G CUs (k_psd_sweep_mc) vs the one-workgroup sweep kernel ----
@pytest.mark.labs
@pytest.mark.parametrize("coop,look_ahead", [("1", "1"), ("1", "0"), ("0", "0")])
def test_psd_sweeps_over_several_cus_labs_variants(hip, oracle, monkeypatch, coop, look_ahead):
    """the lab switches of the multi-CU sweep kernel (labs build): cooperative launch, two barriers per step instead of the look-ahead"""
    monkeypatch.setenv("SCS_HIP_PSD_COOP", coop)  # 0: ordinary launch (the product)
    monkeypatch.setenv("SCS_HIP_PSD_LA", look_ahead)  # 1 (the product): one barrier per step, the next pivots solved beside the A tasks (A double-buffered)
    test_psd_sweeps_over_several_cus_bit_identical(hip, oracle, monkeypatch)


def test_psd_sweeps_over_several_cus_bit_identical(hip, oracle, monkeypatch):
    """Same rotations, same MFMA sequences, spinning barriers between the members of a matrix's group: every bit of the
    projection — and of a whole solve with warm starts, re-orthogonalisation and several [sweep, apply] rounds — must
    be the one the single-workgroup sweeps give.  G = 3 leaves members without a pivot at order 40; G = 8 is the cap."""
    monkeypatch.setenv("SCS_HIP_PSD_SPLIT", "1")
    rng = np.random.RandomState(12)
    K = {"l": 5, "s": [200, 130, 40, 96, 64, 33, 177, 50, 150], "cs": [60, 20]}
    z = rng.randn(pg.cone_dims(K))
    out = {}
    for G in ("1", "2", "3", "4", "8"):
        monkeypatch.setenv("SCS_HIP_PSD_MC", G)
        out[G] = hip.proj_cone(z, K)
    for G in ("2", "3", "4", "8"):
        np.testing.assert_array_equal(out["1"], out[G], err_msg="G=" + G)
    o = 5
    for k in K["s"]:  # and it is the projection: numpy's eigensolver
        d = k * (k + 1) // 2
        S = helpers.svec_to_sym(z[o:o + d], k)
        w, V = np.linalg.eigh(S)
        np.testing.assert_allclose(out["4"][o:o + d], helpers.sym_to_svec((V * np.maximum(w, 0)) @ V.T), rtol=0, atol=1e-10 * k)
        o += d
    K = {"l": 30, "s": [100, 128, 40]}
    data, _, _ = pg.gen_feasible_qp(K, pg.cone_dims(K) + 2, 6, 23, helpers.proj_dual_l_s_numpy)
    args = helpers.raw_args(data, K)
    sols = {}
    for G in ("1", "4"):
        monkeypatch.setenv("SCS_HIP_PSD_MC", G)
        sols[G] = hip.SCS(*args, eps_abs=1e-7, eps_rel=1e-7, verbose=False, max_iters=5000).solve(False, None, None, None)
    assert sols["1"]["info"]["iter"] == sols["4"]["info"]["iter"] and sols["1"]["info"]["iter"] > 64
    assert sols["1"]["info"]["status"] == sols["4"]["info"]["status"] == "solved", sols["1"]["info"]
    for key in ("x", "y", "s"):
        np.testing.assert_array_equal(sols["1"][key], sols["4"][key], err_msg=key)


@pytest.mark.labs
def test_psd_refused_cooperative_launch_falls_back(hip, monkeypatch):
    """A grid the runtime cannot co-schedule (320 workgroups of 1024 lanes on 256 CUs): hipLaunchCooperativeKernel refuses it,
    nothing has run, and the projection is done by the one-workgroup sweeps — same bits, no error."""
    monkeypatch.setenv("SCS_HIP_PSD_SPLIT", "1")
    rng = np.random.RandomState(3)
    K = {"l": 2, "s": [40] * 40}
    z = rng.randn(pg.cone_dims(K))
    monkeypatch.setenv("SCS_HIP_PSD_MC", "1")
    ref = hip.proj_cone(z, K)
    monkeypatch.setenv("SCS_HIP_PSD_MC", "8")
    monkeypatch.setenv("SCS_HIP_PSD_MC_NOCHECK", "1")
    np.testing.assert_array_equal(hip.proj_cone(z, K), ref)


# ---- run-ahead ADMM loop (whole iterations enqueued ahead of the host) vs one host look per iteration ----
@pytest.mark.parametrize("case", ["lp_soc", "qp_mixed", "sdp", "long_cg"])
def test_run_ahead_loop_bit_identical(hip, oracle, monkeypatch, case):
    """Same kernels in the same order; a too-short CG chunk stalls the queue and is finished synchronously.
    Iterates, iteration counts and CG step counts must not depend on the mode."""
    proj = lambda z, K: oracle.proj_cone(z, K, dual=True)
    stg = dict(STG)
    stg.update(eps_abs=1e-7, eps_rel=1e-7, max_iters=600)
    if case == "lp_soc":
        K, n, k, seed = pg.workload("small_lp_soc")
        data, _, _ = pg.gen_feasible(K, n, k, seed, proj)
    elif case == "qp_mixed":
        K = {"z": 10, "l": 600, "q": [30, 12, 5], "s": [6, 3], "ep": 4, "ed": 3, "p": [0.4, -0.7], "bu": [1.0] * 5, "bl": [-1.0] * 5}
        data, _, _ = pg.gen_feasible_qp(K, 420, 7, 5, proj)
    elif case == "sdp":
        K = {"l": 30, "s": [40, 12], "cs": [5]}
        data, _, _ = pg.gen_feasible_qp(K, pg.cone_dims(K) + 2, 6, 21, proj)
    else:  # a badly scaled problem: CG step counts jump around, chunks are often too short (stall + recovery path)
        K = {"z": 150, "l": 300}
        data, _, _ = pg.gen_feasible(K, 200, 12, 9, proj)
        stg.update(scale=25.0, adaptive_scale=False, acceleration_lookback=0)
    args = helpers.raw_args(data, K)
    sols = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SCS_HIP_PIPELINE", mode)
        sols[mode] = hip.SCS(*args, **stg).solve(False, None, None, None)
    a, b = sols["0"]["info"], sols["1"]["info"]
    assert (a["iter"], a["cg_iters"], a["status"]) == (b["iter"], b["cg_iters"], b["status"])
    assert a["accepted_accel_steps"] == b["accepted_accel_steps"] and a["rejected_accel_steps"] == b["rejected_accel_steps"]
    for key in ("x", "y", "s"):
        np.testing.assert_array_equal(sols["0"][key], sols["1"][key], err_msg=key)


# ---- small systems: CG update + direction as one launch (vec.hpp k_cg_update_dir) vs the two kernels ----
@pytest.mark.labs
@pytest.mark.parametrize("case", ["lp_soc", "qp_mixed", "long_cg", "tall"])
@pytest.mark.parametrize("pipeline", ["1", "0"], ids=["run-ahead", "host-sync"])
def test_fused_cg_update_dir_bit_identical(hip, oracle, monkeypatch, case, pipeline):
    """n <= 32768: the last workgroup to finish the CG update forms beta from everybody's partials (agent-scope release /
    acquire around a ticket) and updates the whole direction vector.  Same partials, same order, same elementwise
    arithmetic: iterates, CG step counts and solutions must not depend on the switch — incl. a tall problem whose update
    grid (sized by m) is many workgroups on several XCDs."""
    proj = lambda z, K: oracle.proj_cone(z, K, dual=True)
    stg = dict(STG)
    stg.update(eps_abs=1e-7, eps_rel=1e-7, max_iters=600)
    if case == "lp_soc":
        K, n, k, seed = pg.workload("small_lp_soc")
        data, _, _ = pg.gen_feasible(K, n, k, seed, proj)
    elif case == "qp_mixed":
        K = {"z": 10, "l": 600, "q": [30, 12, 5], "s": [6, 3], "ep": 4, "ed": 3, "p": [0.4, -0.7], "bu": [1.0] * 5, "bl": [-1.0] * 5}
        data, _, _ = pg.gen_feasible_qp(K, 420, 7, 5, proj)
    elif case == "long_cg":
        K = {"z": 150, "l": 300}
        data, _, _ = pg.gen_feasible(K, 200, 12, 9, proj)
        stg.update(scale=25.0, adaptive_scale=False, acceleration_lookback=0)
    else:  # 120 000 rows, 3000 columns: 118 update workgroups, one direction vector of 3000
        K = {"l": 100000, "q": [20] * 1000}
        data, _, _ = pg.gen_feasible(K, 3000, 6, 3, proj)
        stg.update(max_iters=150)
    args = helpers.raw_args(data, K)
    monkeypatch.setenv("SCS_HIP_PIPELINE", pipeline)
    sols = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SCS_HIP_CG_FUSE", mode)
        sols[mode] = hip.SCS(*args, **stg).solve(False, None, None, None)
    a, b = sols["0"]["info"], sols["1"]["info"]
    assert (a["iter"], a["cg_iters"], a["status"]) == (b["iter"], b["cg_iters"], b["status"])
    assert a["cg_iters"] > 0
    for key in ("x", "y", "s"):
        np.testing.assert_array_equal(sols["0"][key], sols["1"][key], err_msg=key)


# ---- short SOCs + small PSD matrices in one launch (psd.hpp k_proj_soc_psd_small) vs two ----
@pytest.mark.labs
@pytest.mark.parametrize("linsys", ["indirect", "dense"])
def test_soc_and_small_psd_in_one_launch_bit_identical(hip, oracle, monkeypatch, linsys):
    """the same two bodies, selected by the workgroup index: iterates, counts and solutions must not depend on the switch
    (config-5-shaped cone: l + 20 SOCs of 50 + 5 PSD matrices of order 20, plus ragged small ones)"""
    import scs
    proj = lambda z, K: oracle.proj_cone(z, K, dual=True)
    K = {"l": 200, "q": [50] * 20 + [3, 1, 7], "s": [20] * 5 + [2, 1, 9]}
    data, _, _ = pg.gen_feasible(K, 300, 6, 17, proj)
    ls = scs.LinearSolver.HIP_DENSE if linsys == "dense" else scs.LinearSolver.HIP_INDIRECT
    sols = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SCS_HIP_SOC_PSD_FUSE", mode)
        sols[mode] = scs.SCS(data, K, linear_solver=ls, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iters=800).solve()
    a, b = sols["0"]["info"], sols["1"]["info"]
    assert (a["iter"], a["cg_iters"], a["status"]) == (b["iter"], b["cg_iters"], b["status"]) and a["iter"] > 50
    for key in ("x", "y", "s"):
        np.testing.assert_array_equal(sols["0"][key], sols["1"][key], err_msg=key)


# ---- scs_init's matrix work on the device (setup_dev.hpp) vs the host builders ----
@pytest.mark.parametrize("cs", ["1", "0"], ids=["column-sorted", "slab"])
def test_device_setup_matches_host_setup(hip, oracle, monkeypatch, cs):
    """CSC -> CSR transposition and the large-matrix layouts (column-sorted passes; SCS_HIP_CS=0: L2-blocked slabs)
    built on the device must give the same matrices, entry for entry, as the host builders: identical SpMV bits and
    identical solves."""
    monkeypatch.setenv("SCS_HIP_CS", cs)
    rng = np.random.default_rng(5)
    A = pg.random_sparse(300000, 270000, 7, rng)  # wide enough for the slab layout in both orientations
    x = rng.standard_normal(A.shape[1])
    y = rng.standard_normal(A.shape[0])
    res = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("SCS_HIP_SETUP", mode)
        res[mode] = (hip.spmv(A, x), hip.spmv(A, y, transpose=True))
    np.testing.assert_array_equal(res["host"][0], res["device"][0])
    np.testing.assert_array_equal(res["host"][1], res["device"][1])
    np.testing.assert_array_equal(res["device"][0], oracle.spmv(A, x))
    # full solves: small (CSR-stream layouts) with P, and one large enough for slabs
    K = {"z": 10, "l": 600, "q": [30, 12, 5], "s": [6, 3]}
    data, _, _ = pg.gen_feasible_qp(K, 400, 7, 5, lambda z, K: oracle.proj_cone(z, K, dual=True))
    K2 = {"l": 400000}
    data2, _, _ = pg.gen_feasible(K2, 300000, 6, 8, lambda z, K: oracle.proj_cone(z, K, dual=True))
    for dat, cone, iters in ((data, K, 200), (data2, K2, 40)):
        sols = {}
        for mode in ("host", "device"):
            monkeypatch.setenv("SCS_HIP_SETUP", mode)
            sols[mode] = hip.SCS(*helpers.raw_args(dat, cone), eps_abs=1e-9, eps_rel=1e-9, verbose=False,
                                 max_iters=iters).solve(False, None, None, None)
        for key in ("x", "y", "s"):
            np.testing.assert_array_equal(sols["host"][key], sols["device"][key], err_msg=key)


@pytest.mark.parametrize("split", ["0", "1"], ids=["one-wg-per-chunk", "split"])
@pytest.mark.parametrize("shape,per_col,rpt,dense", [((300000, 270000), 7, None, False), ((1100000, 400000), 3, None, False),
                                                     ((270000, 300000), 9, "2", False), ((400000, 300000), 5, "16", False),
                                                     ((400000, 300000), 5, "16", True)])
def test_spmv_column_sorted_layout(hip, oracle, monkeypatch, shape, per_col, rpt, dense, split):
    """spmv_cs.hpp: every chunk size (rows per lane 1 .. 16), both orientations, device and host builders, against the
    oracle's sequential loops — bit for bit.  A pattern that does not fit the format's count fields (8 / 16 rows per
    lane: 6-bit counts; here a dense block) has the offending rows peeled off and keeps the same bits.
    split: A' products use two workgroups per row chunk (each sums its half of the chunk's column-sorted stream, the
    two partial sums are added) — still deterministic and identical between the builders, but (a + b) + (c + d) is not
    the oracle's sequential order: 1e-13 relative instead of bits."""
    monkeypatch.setenv("SCS_HIP_CS_SPLIT", split)
    rng = np.random.default_rng(23)
    A = pg.random_sparse(*shape, per_col, rng)
    if dense:  # 70 nonzeros of one row inside one pass: more than a 6-bit count holds
        ii, jj = np.meshgrid(np.arange(70), np.arange(70), indexing="ij")
        A = (A + sparse.csc_matrix((rng.standard_normal(4900), (ii.ravel(), jj.ravel())), shape=shape)).tocsc()
        A.sort_indices()
    if rpt:
        if not hip.labs_build():
            pytest.skip("forcing the rows per lane (SCS_HIP_CS_RPT) is a switch of the labs build; the product picks the geometry")
        monkeypatch.setenv("SCS_HIP_CS_RPT", rpt)
    x, y = rng.standard_normal(shape[1]), rng.standard_normal(shape[0])
    ref = (oracle.spmv(A, x), oracle.spmv(A, y, trans=True))
    keep = (np.diff(A.tocsr().indptr) <= 63, np.diff(A.indptr) <= 63)  # rows the passes keep (longer ones are peeled: wave tree)
    got = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("SCS_HIP_SETUP", mode)
        got[mode] = (hip.spmv(A, x), hip.spmv(A, y, transpose=True))
        np.testing.assert_array_equal(got[mode][0][keep[0]], ref[0][keep[0]], err_msg=mode)
        if split == "0":
            np.testing.assert_array_equal(got[mode][1][keep[1]], ref[1][keep[1]], err_msg=mode)
        for k in (0, 1):
            np.testing.assert_allclose(got[mode][k], ref[k], rtol=0, atol=1e-13 * np.abs(ref[k]).max(), err_msg=mode)
    np.testing.assert_array_equal(got["device"][1], got["host"][1])
    np.testing.assert_array_equal(hip.spmv(A, y, transpose=True), got["host"][1])  # run-to-run


@pytest.mark.labs
@pytest.mark.parametrize("split_a,split_at", [("2", "4"), ("4", "2")])
def test_spmv_in_kernel_combine(hip, oracle, monkeypatch, split_a, split_at):
    """SCS_HIP_CS_COMBINE=1: every workgroup of a row chunk publishes its partial row sums and the LAST one to arrive adds
    them (fixed part order) and runs the epilogue — no combine pass, no spinning.  Against the oracle at 1e-13 (the parts
    are summed separately), device and host builders identical, run-to-run identical bits whichever workgroup arrived
    last, and a full solve through the fused CG epilogues agreeing with the default layout's."""
    monkeypatch.setenv("SCS_HIP_CS_COMBINE", "1")
    monkeypatch.setenv("SCS_HIP_CS_SPLIT_A", split_a)
    monkeypatch.setenv("SCS_HIP_CS_SPLIT_AT", split_at)
    rng = np.random.default_rng(29)
    A = pg.random_sparse(600000, 450000, 6, rng)
    x, y = rng.standard_normal(A.shape[1]), rng.standard_normal(A.shape[0])
    ref = (oracle.spmv(A, x), oracle.spmv(A, y, trans=True))
    got = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("SCS_HIP_SETUP", mode)
        got[mode] = (hip.spmv(A, x), hip.spmv(A, y, transpose=True))
        for k in (0, 1):
            np.testing.assert_allclose(got[mode][k], ref[k], rtol=0, atol=1e-13 * np.abs(ref[k]).max(), err_msg=mode)
    for k in (0, 1):
        np.testing.assert_array_equal(got["device"][k], got["host"][k])
    for rep in range(5):  # arrival order varies from launch to launch; the bits must not
        np.testing.assert_array_equal(hip.spmv(A, x), got["host"][0])
        np.testing.assert_array_equal(hip.spmv(A, y, transpose=True), got["host"][1])
    monkeypatch.delenv("SCS_HIP_SETUP")
    K, n, k, seed = pg.workload("config2_lp_soc")
    data, p_star, _ = pg.gen_feasible(K, n, k, seed, lambda z, K: oracle.proj_cone(z, K, dual=True))
    stg = dict(eps_abs=1e-7, eps_rel=1e-7, verbose=False)
    a = hip.SCS(*helpers.raw_args(data, K), **stg).solve(False, None, None, None)
    monkeypatch.delenv("SCS_HIP_CS_COMBINE")
    b = hip.SCS(*helpers.raw_args(data, K), **stg).solve(False, None, None, None)
    assert a["info"]["status"] == "solved" and b["info"]["status"] == "solved", (a["info"], b["info"])
    assert abs(a["info"]["pobj"] - p_star) <= 1e-5 * max(1.0, abs(p_star))
    for key in ("x", "y", "s"):
        np.testing.assert_allclose(a[key], b[key], rtol=0, atol=2e-4 * np.abs(b[key]).max(), err_msg=key)


@pytest.mark.parametrize("pattern", ["powerlaw", "banded", "dense_rows"])
@pytest.mark.parametrize("split", ["0", "1"], ids=["one-wg-per-chunk", "split"])
def test_spmv_skewed_patterns_keep_the_layout(hip, oracle, monkeypatch, pattern, split):
    """Heavy-tailed row lengths, a banded matrix, a few fully dense rows and columns: the column-sorted layout is kept
    — rows longer than a count field holds are peeled off it and done by a CSR-stream side launch over the plain CSR —
    with the oracle's bits for every row the passes keep (up to 63 nonzeros at 8 / 16 rows per lane); a peeled row is
    reduced by one wavefront in a fixed tree (1e-12).  Identical between the device and host builders, both orientations."""
    monkeypatch.setenv("SCS_HIP_CS_SPLIT", split)
    rng = np.random.default_rng(77)
    m, n = 400000, 300000
    if pattern == "powerlaw":
        A = pg.powerlaw_sparse(m, n, 8, rng)
    elif pattern == "banded":
        A = pg.banded_sparse(m, n, 9, rng)
    else:
        A = pg.random_sparse(m, n, 6, rng).tolil()
        A[7, :] = rng.standard_normal(n)            # a budget row: every variable
        A[123456, :40000] = rng.standard_normal(40000)
        A[:, 11] = rng.standard_normal(m).reshape(-1, 1)   # and a variable in every constraint
        A = A.tocsc()
        A.sort_indices()
    x, y = rng.standard_normal(n), rng.standard_normal(m)
    ref = (oracle.spmv(A, x), oracle.spmv(A, y, trans=True))
    lens = (np.diff(A.tocsr().indptr), np.diff(A.indptr))
    got = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("SCS_HIP_SETUP", mode)
        got[mode] = (hip.spmv(A, x), hip.spmv(A, y, transpose=True))
        for k in (0, 1):
            short = lens[k] <= 63
            if split == "0" or k == 0:
                np.testing.assert_array_equal(got[mode][k][short], ref[k][short], err_msg="%s %d" % (mode, k))
            else:
                np.testing.assert_allclose(got[mode][k][short], ref[k][short], rtol=0, atol=1e-13 * np.abs(ref[k]).max())
            np.testing.assert_allclose(got[mode][k][~short], ref[k][~short], rtol=1e-12, atol=1e-12 * np.abs(ref[k]).max())
    for k in (0, 1):
        np.testing.assert_array_equal(got["device"][k], got["host"][k])
    # the device product IS the host walk of the virtual-row layout (one of the piece lengths the builder tries), bit for bit
    if pattern != "banded":
        npass_est = max(1, A.nnz // 256 // 8192)
        walks = [hip.cs_layout_host_spmv_pieces(A, x, piece_len=pp * npass_est) for pp in (24, 12, 6)]
        assert any(w is not None and np.array_equal(w, got["device"][0]) for w in walks)
    # round 3: the long rows ride in the passes as pieces (default); SCS_HIP_CS_VIRT=0 = the side launch of round 2 sums them
    # whole from the plain CSR.  Rows the passes keep whole have the same bits either way; long rows agree to the tree's rounding.
    if not hip.labs_build():
        return  # (the side launch of round 2 lives in the labs build)
    monkeypatch.setenv("SCS_HIP_CS_VIRT", "0")
    old = (hip.spmv(A, x), hip.spmv(A, y, transpose=True))
    for k in (0, 1):
        short = lens[k] <= 63
        if split == "0" or k == 0:  # (A' with peeled rows keeps two workgroups per chunk: partial sums; with pieces it is one)
            np.testing.assert_array_equal(old[k][short], got["host"][k][short])
        np.testing.assert_allclose(old[k], got["host"][k], rtol=0, atol=1e-12 * np.abs(ref[k]).max())


def test_solve_with_dense_rows_stays_on_the_column_sorted_layout(hip, oracle, monkeypatch):
    """an LP with a budget row (all variables) and a dense column: round 1 threw the whole matrix back to the slab /
    CSR-stream layouts; now it keeps the column-sorted passes (info says so) and solves to the same answer as the
    CSR-stream path, with the fused CG epilogues running on the peeled rows too"""
    K = {"l": 120000, "q": [10] * 2000}
    data, p_star, _ = pg.gen_feasible(K, 70000, 16, 5, lambda z, K: oracle.proj_cone(z, K, dual=True))
    rng = np.random.default_rng(3)
    A = data["A"].tolil()
    A[5, :] = 0.05 * rng.standard_normal(A.shape[1])
    A[:, 9] = 0.05 * rng.standard_normal(A.shape[0]).reshape(-1, 1)
    A = A.tocsc()
    A.sort_indices()
    x0 = rng.standard_normal(A.shape[1])
    z = rng.standard_normal(A.shape[0])
    y0 = oracle.proj_cone(z, K, dual=True)
    s0 = y0 - z
    dat = {"A": A, "b": A @ x0 + s0, "c": -(A.T @ y0)}
    stg = dict(eps_abs=1e-7, eps_rel=1e-7, verbose=False)
    got = hip.SCS(*helpers.raw_args(dat, K), **stg).solve(False, None, None, None)
    assert "column-sorted" in got["info"]["lin_sys_solver"], got["info"]["lin_sys_solver"]
    assert "long rows in pieces" in got["info"]["lin_sys_solver"], got["info"]["lin_sys_solver"]  # (round 2: "peeled")
    # a budget row left WHOLE in the passes (one lane adding its 8191 products of every pass one after the other) made this solve
    # take 87 s instead of ~1 s for a while in round 3: rows with more than 2048 nonzeros in a pass never ride whole
    assert got["info"]["solve_time"] < 30e3, got["info"]["solve_time"]
    if hip.labs_build():  # (the side launch of round 2 lives in the labs build)
        monkeypatch.setenv("SCS_HIP_CS_VIRT", "0")
        old = hip.SCS(*helpers.raw_args(dat, K), **stg).solve(False, None, None, None)
        assert "long rows peeled" in old["info"]["lin_sys_solver"], old["info"]["lin_sys_solver"]
        # (long rows are summed in another order: an accelerated solve to 1e-7 lands a few per cent of iterations away — 3450 / 3600 / 3575
        # with pieces / peeled / CSR-stream)
        assert old["info"]["status"] == "solved" and abs(old["info"]["iter"] - got["info"]["iter"]) <= 0.15 * got["info"]["iter"]
        monkeypatch.delenv("SCS_HIP_CS_VIRT")
    monkeypatch.setenv("SCS_HIP_SLAB", "0")
    ref = hip.SCS(*helpers.raw_args(dat, K), **stg).solve(False, None, None, None)
    assert "CSR-stream" in ref["info"]["lin_sys_solver"]
    assert got["info"]["status"] == "solved" and ref["info"]["status"] == "solved"
    p_opt = float(dat["c"] @ x0)
    assert abs(got["info"]["pobj"] - p_opt) <= 1e-5 * max(1.0, abs(p_opt))
    pri, dual, gap = helpers.kkt_certificate(dat, got)
    assert pri < 1e-5 and dual < 1e-5 and gap < 1e-4 * max(1.0, abs(p_opt))
    # (the dense column's variable is only weakly determined, and two accelerated solves whose mat-vecs round differently do
    # not end on the same iterate: a handful of the 140 000 entries are loose — 3 with round 2's Anderson kernels, 4 with
    # round 3's; the certificate above is the parity statement)
    for key in ("x", "s"):
        bad = np.abs(got[key] - ref[key]) > 2e-4 * np.abs(ref[key]).max()
        assert bad.sum() <= 8, (key, int(bad.sum()))


def test_device_setup_long_rows_fall_back(hip, oracle):
    A = _rand_csc(3000, 2500, 0.002, 3, long_rows=True).tolil()  # a dense row: longer than the one-lane sort takes
    A = sparse.csc_matrix(A)
    A.sort_indices()
    x = np.random.RandomState(1).randn(A.shape[1])
    np.testing.assert_allclose(hip.spmv(A, x), oracle.spmv(A, x), rtol=1e-12, atol=1e-12)
    rng = np.random.RandomState(2)
    data = {"A": A, "b": np.abs(rng.randn(A.shape[0])) + 1.0, "c": rng.randn(A.shape[1])}
    sol = hip.SCS(*helpers.raw_args(data, {"l": A.shape[0]}), verbose=False, max_iters=50).solve(False, None, None, None)
    assert sol["info"]["iter"] == 50 and np.isfinite(sol["x"]).all()


def test_full_solve_on_column_sorted_layouts(hip, oracle, monkeypatch):
    """the whole ADMM path on the large-matrix layouts (column-sorted passes for A, the split layout for A'), forced on
    at a mid size by lowering their threshold, against the same solve on the plain CSR-stream layout (whose parity with
    the oracle the tests above pin): x, y, s at the cross-backend tolerance (rtol 1e-4 of the vector's scale).
    SCS_TEST_LONG=1 additionally runs the oracle's CPU-CG variant on the instance (0.5-2 minutes of host time;
    checked by hand: x 6e-7, y 9e-5, s 1e-6 relative, 2600 vs 2575 iterations)."""
    import os
    K = {"z": 500, "l": 20000, "q": [10] * 1500, "ep": 300, "p": [0.3, -0.6] * 100}
    data, p_star, _ = pg.gen_feasible(K, 17000, 12, 77, lambda z, K: oracle.proj_cone(z, K, dual=True))
    stg = dict(eps_abs=1e-8, eps_rel=1e-8, verbose=False)
    monkeypatch.setenv("SCS_HIP_CS", "1000")  # the pass layout from 1000 nonzeros on
    got = hip.SCS(*helpers.raw_args(data, K), **stg).solve(False, None, None, None)
    assert "column-sorted" in got["info"]["lin_sys_solver"]
    monkeypatch.setenv("SCS_HIP_SLAB", "0")
    ref = hip.SCS(*helpers.raw_args(data, K), **stg).solve(False, None, None, None)
    assert "CSR-stream" in ref["info"]["lin_sys_solver"]
    refs = [ref]
    if os.environ.get("SCS_TEST_LONG") == "1":
        refs.append(oracle.solve(data, K, indirect=True, **stg))
    for r in refs:
        assert got["info"]["status"] == "solved" and r["info"]["status"] == "solved"
        # (iteration counts are not compared: 2600 / 2125 / 2575 for the three — Anderson acceleration amplifies the
        # last-bit differences of differently partitioned reductions; the answers agree)
        for key in ("x", "y", "s"):
            np.testing.assert_allclose(got[key], r[key], rtol=0, atol=2e-4 * np.abs(r[key]).max(), err_msg=key)
    assert abs(got["info"]["pobj"] - p_star) <= 1e-6 * max(1.0, abs(p_star))
