"""Dense numpy reference for the derivatives of a solve (csrc/diff.hpp) and a generator of small problems with a known solution.

At a solution let v = s - y: s = Pi_K(v), y = Pi_K(v) - v.  In the unknowns (x, v) the optimality conditions are
    F1 = P x + A'(Pi(v) - v) + c = 0,   F2 = A x + Pi(v) - b = 0,   J = [[P, A'(W - I)], [A, W]],   W = D Pi_K(v).
adjoint:  g = (gx ; W gs + (W - I) gy),  J' lam = g,  dc = -lam1,  db = lam2,  dA_ij = -(y_i lam1_j + lam2_i x_j),
          dP_ij = -(lam1_i x_j + lam1_j x_i) for a stored i < j,  dP_ii = -lam1_i x_i
forward:  J (dx ; dv) = (-dc ; db),  ds = W dv,  dy = (W - I) dv
Everything here is dense and uses numpy.linalg.lstsq (minimum-norm least squares when J is singular)."""
import numpy as np
from scipy import sparse


def soc_W(v):
    """derivative of the projection onto the second-order cone at v = (t, z)"""
    q = v.shape[0]
    t, z = v[0], v[1:]
    r = np.linalg.norm(z)
    if r <= t:
        return np.eye(q)
    if r <= -t:
        return np.zeros((q, q))
    W = np.empty((q, q))
    W[0, 0] = r
    W[0, 1:] = z
    W[1:, 0] = z
    W[1:, 1:] = (t + r) * np.eye(q - 1) - t * np.outer(z, z) / r ** 2
    return W / (2 * r)


def cone_W(v, cone):
    """W = D Pi_K(v) as a dense matrix for a cone dict with z, l, q"""
    m = v.shape[0]
    W = np.zeros((m, m))
    z, l = int(cone.get("z", 0)), int(cone.get("l", 0))
    for i in range(z, z + l):
        W[i, i] = 1.0 if v[i] > 0 else 0.0
    o = z + l
    for q in cone.get("q", []):
        W[o:o + q, o:o + q] = soc_W(v[o:o + q]) if q > 1 else (1.0 if v[o] > 0 else 0.0)
        o += q
    assert o == m
    return W


def jacobian(A, P, W):
    A = np.asarray(A.todense()) if sparse.issparse(A) else np.asarray(A)
    m, n = A.shape
    Pd = np.zeros((n, n)) if P is None else full_P(P)
    I = np.eye(m)
    return np.block([[Pd, A.T @ (W - I)], [A, W]])


def full_P(P):
    """dense symmetric matrix from the stored upper triangle"""
    U = np.asarray(sparse.triu(sparse.csc_matrix(P)).todense())
    return U + U.T - np.diag(np.diag(U))


def adjoint(A, P, cone, x, y, s, gx=None, gy=None, gs=None):
    """returns dict(db, dc, dA (dense m x n), dP (dense n x n, read its upper triangle), lam, J, W)"""
    m, n = A.shape
    gx = np.zeros(n) if gx is None else gx
    gy = np.zeros(m) if gy is None else gy
    gs = np.zeros(m) if gs is None else gs
    W = cone_W(s - y, cone)
    J = jacobian(A, P, W)
    g = np.concatenate([gx, W @ gs + (W - np.eye(m)) @ gy])
    lam = np.linalg.lstsq(J.T, g, rcond=None)[0]
    l1, l2 = lam[:n], lam[n:]
    dA = -(np.outer(y, l1) + np.outer(l2, x))
    dP = -(np.outer(l1, x) + np.outer(x, l1))
    dP[np.diag_indices(n)] = -l1 * x
    return {"db": l2, "dc": -l1, "dA": dA, "dP": dP, "lam": lam, "J": J, "W": W}


def derivative(A, P, cone, x, y, s, db=None, dc=None):
    m, n = A.shape
    db = np.zeros(m) if db is None else db
    dc = np.zeros(n) if dc is None else dc
    W = cone_W(s - y, cone)
    J = jacobian(A, P, W)
    q = np.linalg.lstsq(J, np.concatenate([-dc, db]), rcond=None)[0]
    dv = q[n:]
    return {"dx": q[:n], "ds": W @ dv, "dy": (W - np.eye(m)) @ dv, "J": J}


def stored_values(dense, M):
    """the entries of a dense matrix at the stored positions of the CSC matrix M, in its order"""
    M = sparse.csc_matrix(M)
    cols = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
    return dense[M.indices, cols]


# ---------------------------------------------------------------- generator
def gen_problem(seed, n, z, l, tight_l, q=(), q_case=(), with_P=False, density=1.0):
    """A feasible problem built from a chosen primal-dual pair (x, y, s), so which rows and cones are tight is the caller's choice:
    the first `tight_l` of the l nonnegative rows are tight (s = 0 < y), the others slack; q_case[i] in {"in", "polar", "bd"} puts
    SOC i strictly inside (s = v, y = 0), in the polar case (s = 0, y = -v) or on the boundary (both on the boundary).  No v is within
    1e-3 of a kink: |v_i| >= 0.5 on the l rows, | |z| - |t| | >= 0.25 |z| on the cones.
    J is regular only if the tight rows and cones (zero rows and polar cones with all their rows, a boundary cone as one) number at
    most n — with P = 0 (an LP) exactly n: a vertex — so the caller counts.  Returns dict(A, P, b, c, cone, x, y, s)."""
    rng = np.random.default_rng(seed)
    q = list(q)
    m = z + l + sum(q)
    v = np.zeros(m)
    v[:z] = rng.uniform(0.5, 1.5, z) * rng.choice([-1.0, 1.0], z)  # zero rows: s = 0, y = -v free
    v[z:z + tight_l] = -rng.uniform(0.5, 1.5, tight_l)
    v[z + tight_l:z + l] = rng.uniform(0.5, 1.5, l - tight_l)
    o = z + l
    for qi, case in zip(q, q_case):
        zz = rng.standard_normal(qi - 1)
        zz *= rng.uniform(0.8, 1.2) / np.linalg.norm(zz)
        r = np.linalg.norm(zz)
        if case == "in":
            t = r * rng.uniform(1.5, 2.0)
        elif case == "polar":
            t = -r * rng.uniform(1.5, 2.0)
        else:
            t = r * rng.uniform(-0.75, 0.75)
        v[o] = t
        v[o + 1:o + qi] = zz
        o += qi
    cone = {"z": z, "l": l, "q": q}
    s = project(v, cone)
    y = s - v
    x = rng.standard_normal(n)
    if density >= 1.0:
        A = rng.standard_normal((m, n)) / np.sqrt(n)
    else:
        A = sparse.random(m, n, density=density, random_state=np.random.RandomState(seed), data_rvs=rng.standard_normal).toarray()
        A[np.arange(m), rng.integers(0, n, m)] += rng.standard_normal(m)  # no empty row
        A[rng.integers(0, m, n), np.arange(n)] += rng.standard_normal(n)  # no empty column
        A /= np.sqrt(max(1.0, density * n))
    P = None
    Pd = np.zeros((n, n))
    if with_P:
        if density >= 1.0:
            G = rng.standard_normal((n, n)) / np.sqrt(n)
            Pd = G @ G.T + 0.5 * np.eye(n)
        else:
            Gs = sparse.random(n, n, density=density / 2, random_state=np.random.RandomState(seed + 1), data_rvs=rng.standard_normal).toarray()
            Pd = 0.2 * (Gs + Gs.T)
            Pd += np.diag(np.abs(Pd).sum(axis=1) + rng.uniform(0.5, 1.0, n))
        P = sparse.triu(sparse.csc_matrix(Pd), format="csc")
        P.sort_indices()
    b = A @ x + s
    c = -Pd @ x - A.T @ y
    A = sparse.csc_matrix(A)
    A.sort_indices()
    return {"A": A, "P": P, "b": b, "c": c, "cone": cone, "x": x, "y": y, "s": s}


def project(v, cone):
    """Euclidean projection onto K (z, l, q)"""
    out = v.copy()
    z, l = int(cone.get("z", 0)), int(cone.get("l", 0))
    out[:z] = 0.0
    out[z:z + l] = np.maximum(v[z:z + l], 0.0)
    o = z + l
    for q in cone.get("q", []):
        t, zz = v[o], v[o + 1:o + q]
        r = np.linalg.norm(zz)
        if q == 1:
            out[o] = max(t, 0.0)
        elif r <= t:
            pass
        elif r <= -t:
            out[o:o + q] = 0.0
        else:
            a = 0.5 * (r + t)
            out[o] = a
            out[o + 1:o + q] = a * zz / r
        o += q
    return out


def data_of(p):
    d = {"A": p["A"], "b": p["b"], "c": p["c"]}
    if p["P"] is not None:
        d["P"] = p["P"]
    return d


# the three problems of the finite-difference check (tests/test_adjoint_ref_cpu.py, tests/golden/adjoint_fd.json) and of the GPU tests
def problem_lp():  # z = 2, l = 12, n = 7: a vertex — 2 zero rows + 5 tight rows = n
    return gen_problem(11, n=7, z=2, l=12, tight_l=5)


def problem_qp():  # z = 2, l = 12, n = 12: 2 + 6 = 8 <= n - 1 tight rows
    return gen_problem(12, n=12, z=2, l=12, tight_l=6, with_P=True)


def problem_qp_soc():  # z = 2, l = 5, q = [3, 4, 6], n = 12: 2 + 2 tight rows, a polar cone (3 rows), a boundary cone (1): 8 <= n - 1
    return gen_problem(13, n=12, z=2, l=5, tight_l=2, q=(3, 4, 6), q_case=("polar", "bd", "in"), with_P=True)


def fd_compare(p, solve, seed, which, h=1e-4, grad=None):
    """|<grad, direction> - central difference| / |central difference| for L = gx'x + gy'y + gs's with random gx, gy, gs and one
    random direction: which = "bcA" moves b, c and the stored values of A at once, "P" the stored triangle of P.  solve(data) returns
    the dict of a solve; the gradient is the dense reference at the unperturbed solution, or grad(gx, gy, gs) -> {"db", "dc", "dA", "dP"}
    (value arrays in stored order) called right after the unperturbed solve.  Returns (relative difference, cond(J))."""
    rng = np.random.default_rng(seed)
    A, P = p["A"], p["P"]
    m, n = A.shape
    base = solve(data_of(p))
    gx, gy, gs = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    ref = adjoint(A, P, p["cone"], base["x"], base["y"], base["s"], gx, gy, gs)
    if grad is None:
        got = {"db": ref["db"], "dc": ref["dc"], "dA": stored_values(ref["dA"], A), "dP": stored_values(ref["dP"], P) if P is not None else None}
    else:
        got = grad(gx, gy, gs)
    if which == "bcA":
        db, dc, dAv = rng.standard_normal(m), rng.standard_normal(n), rng.standard_normal(A.nnz)
        pred = got["db"] @ db + got["dc"] @ dc + got["dA"] @ dAv
    else:
        dPv = rng.standard_normal(P.nnz)
        pred = got["dP"] @ dPv

    def moved(t):
        d = data_of(p)
        if which == "bcA":
            A2 = A.copy()
            A2.data = A.data + t * dAv
            d["A"], d["b"], d["c"] = A2, p["b"] + t * db, p["c"] + t * dc
        else:
            P2 = P.copy()
            P2.data = P.data + t * dPv
            d["P"] = P2
        return d

    def L(r):
        return gx @ r["x"] + gy @ r["y"] + gs @ r["s"]

    fd = (L(solve(moved(h))) - L(solve(moved(-h)))) / (2 * h)
    return abs(pred - fd) / abs(fd), float(np.linalg.cond(ref["J"]))


PROBLEMS = {"lp": problem_lp, "qp": problem_qp, "qp_soc": problem_qp_soc}
FD_SEEDS = {"bcA": 100, "P": 101}


def problem_lp3():  # n = 3: z = 1, l = 5, 1 + 2 tight rows = n (a vertex)
    return gen_problem(24, n=3, z=1, l=5, tight_l=2)


BIG_Q = [3] * 20 + [10] * 6 + [60]
BIG_Q_CASE = ["in", "polar", "bd", "bd"] * 5 + ["bd", "in", "polar", "bd", "in", "bd"] + ["bd"]


def problem_big():  # n = 300, m = 700: 20 zero + 150 tight rows, 25 polar rows, 14 boundary cones: 209 <= n - 1; sparse A and P
    return gen_problem(31, n=300, z=20, l=500, tight_l=150, q=BIG_Q, q_case=BIG_Q_CASE, with_P=True, density=0.02)


def problem_degenerate():
    """the LP of problem_lp3 with its first tight row stored twice (same row of A, same b; the multiplier shared): J is singular"""
    p = problem_lp3()
    A = p["A"].toarray()
    i = p["cone"]["z"]  # the first tight nonnegative row
    A2 = np.vstack([A[:i + 1], A[i:i + 1], A[i + 1:]])
    ins = lambda v, val: np.concatenate([v[:i + 1], [val], v[i + 1:]])
    y = p["y"].copy()
    y[i] *= 0.5
    y2, s2, b2 = ins(y, y[i]), ins(p["s"], 0.0), ins(p["b"], p["b"][i])
    cone = {"z": p["cone"]["z"], "l": p["cone"]["l"] + 1, "q": []}
    A2 = sparse.csc_matrix(A2)
    A2.sort_indices()
    return {"A": A2, "P": None, "b": b2, "c": p["c"], "cone": cone, "x": p["x"], "y": y2, "s": s2}
