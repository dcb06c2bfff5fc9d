"""Spectral cones on the device (scs-python_amd/csrc/spectral.hpp): kernel-level projections against the numpy reference
(tests/spectral_ref.py), the cross-checks against the existing HIP cone kernels, the reference's spectral tests
(R:test/test_spectral_and_complex_cones.py) restated over the HIP backends, and solve-level properties."""
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

import spectral_ref as sr

pytestmark = pytest.mark.gpu


def _proj(cone, w, dual=False):
    from scs import _scs_hip
    return _scs_hip.proj_cone(w, cone, dual=dual)


def _cone_of(kind, sz):
    return {"d": lambda: {"d": [sz[0]]}, "nuc": lambda: {"nuc_m": [sz[0]], "nuc_n": [sz[1]]}, "ell1": lambda: {"ell1": [sz[0]]},
            "sl": lambda: {"sl_n": [sz[0]], "sl_k": [sz[1]]}}[kind]()


def _inputs(kind, sz, rng):
    L = sr.length(kind, sz)
    out = [rng.standard_normal(L), 1e3 * rng.standard_normal(L), np.zeros(L)]
    p = sr.proj(kind, sz, rng.standard_normal(L))
    out += [p, 2.0 * p, -sr.proj(kind, sz, rng.standard_normal(L), dual=True)]  # boundary, inside, polar
    if kind in ("sl", "d"):
        n, off = sz[0], (2 if kind == "d" else 1)
        for spec in (np.ones(n), np.r_[np.zeros(n // 2), np.ones(n - n // 2)], np.r_[-np.ones(n // 2), 3 * np.ones(n - n // 2)]):
            Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
            w = np.zeros(L)
            w[:off] = rng.standard_normal(off)
            w[off:] = sr.svec((Q * spec) @ Q.T)
            out.append(w)
    if kind == "nuc":
        m, n = sz
        r = max(1, min(m, n) // 2)
        out.append(np.r_[rng.standard_normal(), (rng.standard_normal((m, r)) @ rng.standard_normal((r, n))).reshape(-1, order="F")])
    return out


CASES = ([("ell1", (n,)) for n in (1, 2, 7, 64, 65, 1000, 2048, 2049, 100000)] +
         [("sl", (n, k)) for n, k in ((1, 1), (2, 1), (5, 2), (8, 8), (17, 1), (17, 9), (33, 33), (64, 1), (64, 32), (64, 64))] +
         [("d", (n,)) for n in (1, 2, 3, 8, 17, 33, 64)] +
         [("nuc", sz) for sz in ((1, 1), (3, 2), (2, 3), (4, 4), (1, 9), (9, 1), (64, 64), (128, 64), (20, 64), (64, 128), (8192, 1))])


@pytest.mark.parametrize("kind,sz", CASES)
def test_kernel_projection_matches_reference(kind, sz):
    rng = np.random.default_rng(zlib.crc32(repr((kind, sz)).encode()))
    cone = _cone_of(kind, sz)
    for w in _inputs(kind, sz, rng):
        scale = max(1.0, np.abs(w).max())
        for dual in (False, True):
            got = _proj(cone, w, dual)
            ref = sr.proj(kind, sz, w, dual)
            np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-10 * scale, err_msg="%s %s dual=%s" % (kind, sz, dual))
        # Moreau: w = Pi_K(w) - Pi_{K*}(-w)
        np.testing.assert_allclose(_proj(cone, w) - _proj(cone, -w, dual=True), w, atol=1e-10 * scale)


def test_several_cones_of_every_kind_in_one_vector():
    """one launch per kind covers every cone of that kind, each at its own offset, next to the standard cones"""
    rng = np.random.default_rng(3)
    cone = dict(l=2, q=[3], s=[2], ep=1, d=[3, 1, 5], nuc_m=[2, 4, 3], nuc_n=[3, 4, 1], ell1=[4, 3000, 1, 70, 2500], sl_n=[4, 2, 6],
                sl_k=[2, 2, 1])
    m = sr.m_of(cone)
    w = rng.standard_normal(m)
    for dual in (False, True):
        got = _proj(cone, w, dual)
        at = 2 + 3 + 3 + 3
        for kind, sz in sr.spectral_order(cone):
            L = sr.length(kind, sz)
            np.testing.assert_allclose(got[at:at + L], sr.proj(kind, sz, w[at:at + L], dual), rtol=1e-10, atol=1e-10)
            at += L
        assert at == m
        np.testing.assert_allclose(got[:11], _proj(dict(l=2, q=[3], s=[2], ep=1), w[:11], dual), rtol=0, atol=0)


@pytest.mark.parametrize("dual", [False, True])
def test_cross_check_against_standard_hip_kernels(dual):
    """d=[1] = ep, nuc (m,1) and (1,m) = q=[m+1], ell1=[1] = q=[2], through the existing HIP kernels"""
    rng = np.random.default_rng(17)
    for _ in range(20):
        w = rng.standard_normal(3)
        np.testing.assert_allclose(_proj({"d": [1]}, w, dual), _proj({"ep": 1}, w, dual), rtol=1e-6, atol=1e-7)
        w = rng.standard_normal(6)
        for sz in ((5, 1), (1, 5)):
            np.testing.assert_allclose(_proj({"nuc_m": [sz[0]], "nuc_n": [sz[1]]}, w, dual), _proj({"q": [6]}, w, dual), rtol=1e-10, atol=1e-12)
        w = rng.standard_normal(2)
        np.testing.assert_allclose(_proj({"ell1": [1]}, w, dual), _proj({"q": [2]}, w, dual), rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------- solves
def _gen_feasible_qp(cone, rng):
    """R:test/test_spectral_and_complex_cones.py:54-69"""
    m = sr.m_of(cone)
    n = m
    P = sp.eye(n, format="csc")
    A = sp.random(m, n, density=0.5, format="csc", random_state=rng)
    A.data = rng.randn(A.nnz)
    c = rng.randn(n)
    b = A @ rng.randn(n) + np.abs(rng.randn(m))
    return dict(P=P, A=A, b=b, c=c)


def _solvers():
    import scs
    return [pytest.param({"linear_solver": scs.LinearSolver.HIP_INDIRECT}, id="indirect"),
            pytest.param({"linear_solver": scs.LinearSolver.HIP_DENSE}, id="dense"),
            pytest.param({"linear_solver": scs.LinearSolver.AUTO}, id="auto", marks=pytest.mark.auto_resolution)]


REF_CASES = [  # (seed, cone, max_iters) of the reference's spectral classes
    (10, {"ell1": [4]}, None), (20, {"ell1": [3, 5]}, None), (30, dict(z=1, l=2, q=[3], ell1=[4]), None),
    (40, {"nuc_m": [3], "nuc_n": [2]}, None), (50, {"nuc_m": [3, 4], "nuc_n": [2, 3]}, None), (60, dict(l=3, nuc_m=[3], nuc_n=[2]), None),
    (70, {"d": [3]}, 10000), (80, {"d": [2, 3]}, 10000), (90, dict(l=2, d=[2]), 10000),
    (100, {"sl_n": [4], "sl_k": [2]}, 10000), (110, {"sl_n": [3, 4], "sl_k": [1, 2]}, 10000), (120, dict(z=1, l=2, sl_n=[3], sl_k=[1]), 10000),
    (200, dict(z=1, l=2, q=[3], s=[2], cs=[2], ep=1, ed=1, p=[0.5], d=[2], nuc_m=[3], nuc_n=[2], ell1=[3], sl_n=[3], sl_k=[1]), 10000),
    (210, dict(cs=[3], ell1=[5], nuc_m=[4], nuc_n=[3]), 5000),
    (300, {"ell1": [1]}, None), (310, {"nuc_m": [3], "nuc_n": [3]}, None), (320, {"d": [1]}, 10000), (330, {"sl_n": [3], "sl_k": [1]}, 10000),
]


@pytest.mark.parametrize("solver_opts", _solvers())
@pytest.mark.parametrize("seed,cone,max_iters", REF_CASES, ids=[str(c[0]) for c in REF_CASES])
def test_reference_spectral_cases(solver_opts, seed, cone, max_iters):
    import scs
    data = _gen_feasible_qp(cone, np.random.RandomState(seed))
    kw = {"max_iters": max_iters} if max_iters else {}
    sol = scs.solve(data, cone, **solver_opts, verbose=False, **kw)
    assert sol["info"]["status_val"] in (1, 2), sol["info"]["status"]


def test_norm_bounds():
    """R:test/test_spectral_and_complex_cones.py:180-193, 230-243"""
    import scs
    data = _gen_feasible_qp({"ell1": [5]}, np.random.RandomState(35))
    sol = scs.solve(data, {"ell1": [5]}, verbose=False, eps_abs=1e-9, eps_rel=1e-9)
    assert sol["info"]["status_val"] == 1
    assert sol["s"][0] >= np.abs(sol["s"][1:]).sum() - 1e-4
    data = _gen_feasible_qp({"nuc_m": [4], "nuc_n": [3]}, np.random.RandomState(65))
    sol = scs.solve(data, {"nuc_m": [4], "nuc_n": [3]}, verbose=False, eps_abs=1e-9, eps_rel=1e-9)
    assert sol["info"]["status_val"] == 1
    X = sol["s"][1:].reshape(4, 3, order="F")
    assert sol["s"][0] >= np.linalg.svd(X, compute_uv=False).sum() - 1e-4


def _projection_qp(cone, w):
    """min 1/2 |z - w|^2 s.t. z in K (s = z): the solution is Pi_K(w), the optimal value 1/2 |Pi_K(w) - w|^2 - 1/2 |w|^2"""
    L = w.size
    return dict(P=sp.eye(L, format="csc"), A=-sp.eye(L, format="csc"), b=np.zeros(L), c=-w)


@pytest.mark.parametrize("kind,sz", [("ell1", (6,)), ("nuc", (3, 2)), ("nuc", (2, 4)), ("sl", (4, 2)), ("d", (3,))])
def test_solve_recovers_the_projection(kind, sz):
    import scs
    rng = np.random.default_rng(zlib.crc32(repr((kind, sz)).encode()))
    w = rng.standard_normal(sr.length(kind, sz))
    cone = _cone_of(kind, sz)
    sol = scs.solve(_projection_qp(cone, w), cone, verbose=False, eps_abs=1e-9, eps_rel=1e-9, max_iters=100000)
    assert sol["info"]["status_val"] == 1
    np.testing.assert_allclose(sol["x"], sr.proj(kind, sz, w), atol=1e-5)


def test_ell1_agrees_with_its_lp_reformulation():
    """min 1/2 |z - w|^2 over z = (t, x) in ell1 vs the same objective over (t, x, u) with -u <= x <= u, sum u <= t (an LP cone),
    the latter solved by this backend and by the oracle"""
    import scs
    from oracle import scs_oracle
    rng = np.random.default_rng(8)
    n = 6
    w = rng.standard_normal(n + 1)
    spec = scs.solve(_projection_qp({"ell1": [n]}, w), {"ell1": [n]}, verbose=False, eps_abs=1e-9, eps_rel=1e-9)
    N = 2 * n + 1
    P = sp.diags(np.r_[np.ones(n + 1), np.zeros(n)]).tocsc()
    c = np.r_[-w, np.zeros(n)]
    rows = []
    for i in range(n):  # x_i - u_i <= 0 ; -x_i - u_i <= 0
        r = np.zeros(N); r[1 + i] = 1; r[1 + n + i] = -1; rows.append(r)
        r = np.zeros(N); r[1 + i] = -1; r[1 + n + i] = -1; rows.append(r)
    r = np.zeros(N); r[0] = -1; r[1 + n:] = 1; rows.append(r)  # sum u - t <= 0
    A = sp.csc_matrix(np.array(rows))
    data = dict(P=P, A=A, b=np.zeros(A.shape[0]), c=c)
    lp = scs.solve(data, {"l": A.shape[0]}, verbose=False, eps_abs=1e-9, eps_rel=1e-9)
    ref = scs_oracle.solve(data, {"l": A.shape[0]}, eps_abs=1e-9, eps_rel=1e-9, verbose=False)
    for s in (spec, lp, ref):
        assert s["info"]["status_val"] == 1
    assert abs(spec["info"]["pobj"] - lp["info"]["pobj"]) <= 1e-4
    assert abs(spec["info"]["pobj"] - ref["info"]["pobj"]) <= 1e-4


KITCHEN = dict(z=1, l=2, q=[3], s=[2], ep=1, d=[2], nuc_m=[3], nuc_n=[2], ell1=[3], sl_n=[3], sl_k=[1])


def test_two_solves_are_bit_identical():
    import scs
    data = _gen_feasible_qp(KITCHEN, np.random.RandomState(7))
    a = scs.solve(data, KITCHEN, verbose=False, max_iters=3000)
    b = scs.solve(data, KITCHEN, verbose=False, max_iters=3000)
    assert a["info"]["iter"] == b["info"]["iter"]
    for key in ("x", "y", "s"):
        assert np.array_equal(a[key], b[key]), key


def test_warm_start_and_update():
    """R:test/test_spectral_and_complex_cones.py:376-: warm start and update(b, c)"""
    import scs
    rng = np.random.RandomState(340)
    cone = {"ell1": [4], "sl_n": [3], "sl_k": [2]}
    data = _gen_feasible_qp(cone, rng)
    solver = scs.SCS(data, cone, verbose=False, max_iters=5000)
    s1 = solver.solve()
    assert s1["info"]["status_val"] in (1, 2)
    s2 = solver.solve(warm_start=True, x=s1["x"], y=s1["y"], s=s1["s"])
    assert s2["info"]["status_val"] in (1, 2) and s2["info"]["iter"] <= s1["info"]["iter"]
    solver.update(b=data["b"] * 1.1, c=data["c"] * 0.9)
    s3 = solver.solve()
    assert s3["info"]["status_val"] in (1, 2)
    fresh = scs.solve(dict(data, b=data["b"] * 1.1, c=data["c"] * 0.9), cone, verbose=False, max_iters=5000)
    assert abs(s3["info"]["pobj"] - fresh["info"]["pobj"]) <= 1e-3 * max(1, abs(fresh["info"]["pobj"]))


def test_batch_equals_separate_solves():
    import scs
    solvers, seps = [], []
    for seed in (1, 2, 3):
        data = _gen_feasible_qp(KITCHEN, np.random.RandomState(seed))
        solvers.append(scs.SCS(data, KITCHEN, verbose=False, max_iters=3000))
        seps.append(scs.solve(data, KITCHEN, verbose=False, max_iters=3000))
    for got, ref in zip(scs.solve_batch(solvers), seps):
        assert got["info"]["iter"] == ref["info"]["iter"]
        for key in ("x", "y", "s"):
            assert np.array_equal(got[key], ref[key]), key


@pytest.mark.parametrize("cone,why", [
    ({"d": [65]}, "exceeds the supported order 64"), ({"sl_n": [65], "sl_k": [1]}, "exceeds the supported order 64"),
    ({"sl_n": [4], "sl_k": [5]}, "1 <= k <= n"), ({"sl_n": [4], "sl_k": [0]}, "1 <= k <= n"),
    ({"nuc_m": [65], "nuc_n": [65]}, "min(m, n) exceeds 64"), ({"nuc_m": [8193], "nuc_n": [1]}, "m n exceeds 8192"),
    ({"d": [0]}, "order must be >= 1"), ({"ell1": [0]}, "length must be >= 1"), ({"nuc_m": [0], "nuc_n": [3]}, "sizes must be >= 1"),
])
def test_limits_are_refused_with_a_reason(cone, why):
    import scs
    m = max(1, sr.m_of(cone))
    data = dict(A=sp.eye(m, format="csc"), b=np.ones(m), c=np.ones(m))
    with pytest.raises(ValueError, match="ScsWork allocation error") as e:
        scs.solve(data, cone, verbose=False)
    assert why in str(e.value), str(e.value)


@pytest.mark.parametrize("cone", [{"d": [64]}, {"sl_n": [64], "sl_k": [7]}, {"nuc_m": [128], "nuc_n": [64]}, {"nuc_m": [8192], "nuc_n": [1]}])
def test_largest_accepted_sizes_solve(cone):
    import scs
    kind, sz = sr.spectral_order(cone)[0]
    w = np.random.default_rng(4).standard_normal(sr.length(kind, sz))
    sol = scs.solve(_projection_qp(cone, w), cone, verbose=False, eps_abs=1e-7, eps_rel=1e-7, max_iters=20000)
    assert sol["info"]["status_val"] == 1
    np.testing.assert_allclose(sol["x"], sr.proj(kind, sz, w), atol=1e-4)


def test_row_count_of_the_core():
    """the core counts the spectral rows as the reference's helper does (R:test/test_spectral_and_complex_cones.py:27-51): the
    kitchen sink is accepted with exactly that m and refused with one row more or less"""
    import scs
    m = sr.m_of(KITCHEN)
    assert m == 1 + 2 + 3 + 3 + 3 + (3 + 2) + (6 + 1) + (3 + 1) + (6 + 1)
    for mm in (m - 1, m + 1):
        data = dict(A=sp.eye(mm, format="csc"), b=np.ones(mm), c=np.ones(mm))
        with pytest.raises(ValueError, match="cone dimensions do not match m"):
            scs.SCS(data, KITCHEN, verbose=False)
    data = dict(A=sp.eye(m, format="csc"), b=np.ones(m), c=np.ones(m))
    scs.SCS(data, KITCHEN, verbose=False)


# ---------------------------------------------------------------- standard-cone reformulations
# spectral_ref.reformulation: min 1/2 |z - w|^2 over z plus auxiliary variables whose standard cones (l, s, ep) force z into K.
# Its optimal value equals that of the projection QP over the spectral cone itself.  Both are solved by this backend, the
# reformulation also by the oracle; the three optimal values agree to 1e-4.
@pytest.mark.parametrize("kind,sz", [("nuc", (3, 2)), ("nuc", (2, 4)), ("nuc", (3, 3)), ("sl", (4, 2)), ("sl", (3, 1)), ("sl", (5, 5)),
                                     ("d", (2,)), ("d", (3,))])
def test_spectral_cone_agrees_with_its_standard_reformulation(kind, sz):
    import scs
    from oracle import scs_oracle
    rng = np.random.default_rng(zlib.crc32(repr(("reform", kind, sz)).encode()))
    w = rng.standard_normal(sr.length(kind, sz))
    if kind == "d":
        w[1] = abs(w[1]) + 0.5  # (v > 0: the interior of the log-det cone's projection is reached away from the face v = 0)
    cone = _cone_of(kind, sz)
    data, std = sr.reformulation(kind, sz, w)
    stg = dict(eps_abs=1e-9, eps_rel=1e-9, max_iters=200000, verbose=False)
    spec = scs.solve(_projection_qp(cone, w), cone, **stg)
    hip = scs.solve(data, std, **stg)
    ref = scs_oracle.solve(data, std, **stg)
    for s in (spec, hip, ref):
        assert s["info"]["status_val"] in (1, 2), s["info"]["status"]
    exact = 0.5 * np.sum((sr.proj(kind, sz, w) - w) ** 2) - 0.5 * w @ w
    for s in (spec, hip, ref):
        assert abs(s["info"]["pobj"] - exact) <= 1e-4, (s["info"]["pobj"], exact)
    np.testing.assert_allclose(hip["x"][:w.size], spec["x"], atol=1e-4)
