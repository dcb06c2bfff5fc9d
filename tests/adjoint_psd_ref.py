"""Dense numpy reference for the derivatives of a solve with real PSD blocks (csrc/dproj_psd.hpp), extending tests/adjoint_ref.py with
the `s` cones, and a generator of small SDPs with a known solution.

A block of order p is a vector of p (p + 1) / 2 entries: the lower triangle by column, off-diagonals times sqrt(2) (svec).  With
mat(v) = Q diag(lam) Q' the derivative of the projection is  W u = svec(Q (B o (Q' smat(u) Q)) Q'),  B_ij the first divided difference
of max(., 0) at (lam_i, lam_j): 1 / 0 where both are positive / neither is, hi / (hi - lo) across the sign change."""
import numpy as np
from scipy import sparse

import adjoint_ref as ar

SQ2 = np.sqrt(2.0)
TAU = 1e-13   # csrc/dproj_psd.hpp kDprojPsdTau: the relative off-diagonal norm the device's eigen-decomposition stops at
GAP = 0.1     # relative sign gap of every generated spectrum: |lam| in [0.5, 1.5] gives min|lam| / (2 max|lam|) >= 1/6


def sd_size(p):
    return p * (p + 1) // 2


def svec(M):
    p = M.shape[0]
    out = np.empty(sd_size(p))
    k = 0
    for j in range(p):
        out[k] = M[j, j]
        out[k + 1:k + p - j] = SQ2 * M[j + 1:, j]
        k += p - j
    return out


def smat(v, p):
    M = np.zeros((p, p))
    k = 0
    for j in range(p):
        M[j, j] = v[k]
        M[j + 1:, j] = v[k + 1:k + p - j] / SQ2
        M[j, j + 1:] = M[j + 1:, j]
        k += p - j
    return M


def divided_differences(lam):
    lp = np.maximum(lam, 0.0)
    num = lp[:, None] - lp[None, :]
    den = lam[:, None] - lam[None, :]
    B = np.where(lam[:, None] + lam[None, :] > 0, 1.0, 0.0)  # (equal eigenvalues: 1 if positive, else 0)
    ok = den != 0
    B[ok] = num[ok] / den[ok]
    return B


def psd_W(v, p):
    """W = D Pi_{S+}(v) as a dense sd_size(p) x sd_size(p) matrix"""
    d = sd_size(p)
    lam, Q = np.linalg.eigh(smat(v, p))
    B = divided_differences(lam)
    W = np.empty((d, d))
    for k in range(d):
        e = np.zeros(d)
        e[k] = 1.0
        W[:, k] = svec(Q @ (B * (Q.T @ smat(e, p) @ Q)) @ Q.T)
    return W


def psd_W_apply(v, u, p):
    """psd_W(v, p) @ u without forming W (orders whose dense W would not fit)"""
    lam, Q = np.linalg.eigh(smat(v, p))
    return svec(Q @ (divided_differences(lam) * (Q.T @ smat(u, p) @ Q)) @ Q.T)


def psd_project(v, p):
    lam, Q = np.linalg.eigh(smat(v, p))
    return svec((Q * np.maximum(lam, 0.0)) @ Q.T)


def split(cone):
    zlq = {"z": int(cone.get("z", 0)), "l": int(cone.get("l", 0)), "q": list(cone.get("q", []))}
    return zlq, zlq["z"] + zlq["l"] + sum(zlq["q"])


def cone_W(v, cone):
    """W = D Pi_K(v), dense, for a cone dict with z, l, q, s"""
    m = v.shape[0]
    zlq, o = split(cone)
    W = np.zeros((m, m))
    W[:o, :o] = ar.cone_W(v[:o], zlq)
    for p in cone.get("s", []):
        d = sd_size(p)
        W[o:o + d, o:o + d] = psd_W(v[o:o + d], p)
        o += d
    assert o == m
    return W


def project(v, cone):
    zlq, o = split(cone)
    out = v.copy()
    out[:o] = ar.project(v[:o], zlq)
    for p in cone.get("s", []):
        d = sd_size(p)
        out[o:o + d] = psd_project(v[o:o + d], p)
        o += d
    assert o == v.shape[0]
    return out


def adjoint(A, P, cone, x, y, s, gx=None, gy=None, gs=None):
    """as adjoint_ref.adjoint, for a cone dict with z, l, q, s"""
    m, n = A.shape
    gx = np.zeros(n) if gx is None else gx
    gy = np.zeros(m) if gy is None else gy
    gs = np.zeros(m) if gs is None else gs
    W = cone_W(s - y, cone)
    J = ar.jacobian(A, P, W)
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
    J = ar.jacobian(A, P, W)
    q = np.linalg.lstsq(J, np.concatenate([-dc, db]), rcond=None)[0]
    dv = q[n:]
    return {"dx": q[:n], "ds": W @ dv, "dy": (W - np.eye(m)) @ dv, "J": J}


# ---------------------------------------------------------------- generator
def psd_point(rng, p, rank, scale=1.0):
    """svec of Q diag(lam) Q' with `rank` positive eigenvalues and p - rank negative ones, |lam| in [0.5, 1.5]"""
    Q = np.linalg.qr(rng.standard_normal((p, p)))[0]
    lam = rng.uniform(0.5, 1.5, p)
    lam[rank:] *= -1.0
    return svec((Q * (scale * lam)) @ Q.T)


def gen_problem(seed, n, z, l, tight_l, s=(), ranks=(), q=(), q_case=(), with_P=False):
    """adjoint_ref.gen_problem with PSD blocks: block i has v = Q diag(lam) Q' with ranks[i] positive eigenvalues, |lam| in [0.5, 1.5]
    (relative sign gap >= GAP), s = Pi(v), y = s - v; b, c from a random x.  A block of order p and rank r is tight in
    (p - r)(p - r + 1) / 2 directions; the caller counts them against n as in adjoint_ref.gen_problem."""
    base = ar.gen_problem(seed, n=n, z=z, l=l, tight_l=tight_l, q=q, q_case=q_case)
    rng = np.random.default_rng(seed + 1000)
    v0 = base["s"] - base["y"]
    v = np.concatenate([v0] + [psd_point(rng, p, r) for p, r in zip(s, ranks)])
    cone = {"z": z, "l": l, "q": list(q), "s": list(s)}
    m = v.shape[0]
    sv = project(v, cone)
    y = sv - v
    x = rng.standard_normal(n)
    A = rng.standard_normal((m, n)) / np.sqrt(n)
    P = None
    Pd = np.zeros((n, n))
    if with_P:
        G = rng.standard_normal((n, n)) / np.sqrt(n)
        Pd = G @ G.T + 0.5 * np.eye(n)
        P = sparse.triu(sparse.csc_matrix(Pd), format="csc")
        P.sort_indices()
    b = A @ x + sv
    c = -Pd @ x - A.T @ y
    A = sparse.csc_matrix(A)
    A.sort_indices()
    return {"A": A, "P": P, "b": b, "c": c, "cone": cone, "x": x, "y": y, "s": sv}


# J is regular when the multiplier is unique — zero rows + tight rows + (p - r)(p - r + 1) / 2 per block of order p and rank r <= n — and,
# without P, so is x: zero rows + tight rows + p (p + 1) / 2 - r (r + 1) / 2 per block >= n.
def problem_qp_sdp():  # n = 14, with P: 1 + 2 + 3 + 3 = 9 <= n
    return gen_problem(41, n=14, z=1, l=4, tight_l=2, s=(3, 5), ranks=(1, 3), with_P=True)


def problem_lp_sdp():  # n = 9: 1 + 2 + 3 = 6 <= n <= 1 + 2 + 7 = 10
    return gen_problem(42, n=9, z=1, l=4, tight_l=2, s=(4,), ranks=(2,))


MIXED_S = (2, 40, 3, 33, 5, 8, 17, 32, 12, 4, 16, 7)
MIXED_RANKS = (1, 38, 2, 31, 3, 5, 15, 31, 10, 3, 14, 4)


def problem_mixed_sdp():
    """12 PSD blocks of orders 2 .. 40 (both apply paths of dproj_psd.hpp) next to l and q rows.  The multiplier of a block of order p
    and rank r has (p - r)(p - r + 1) / 2 free directions: 34 in all, + 2 zero rows + 3 tight rows + 1 boundary cone = 40 <= n, and P is
    positive definite: J is regular"""
    return gen_problem(43, n=60, z=2, l=8, tight_l=3, s=MIXED_S, ranks=MIXED_RANKS, q=(3, 5), q_case=("bd", "in"), with_P=True)


PROBLEMS = {"qp_sdp": problem_qp_sdp, "lp_sdp": problem_lp_sdp}
FD_SEEDS = {"bcA": 200, "P": 201}


def fd_compare(p, solve, seed, which, h=1e-4, grad=None):
    """adjoint_ref.fd_compare with this module's reference: (relative difference to the central difference, cond(J))"""
    rng = np.random.default_rng(seed)
    A, P = p["A"], p["P"]
    m, n = A.shape
    base = solve(ar.data_of(p))
    gx, gy, gs = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    ref = adjoint(A, P, p["cone"], base["x"], base["y"], base["s"], gx, gy, gs)
    if grad is None:
        got = {"db": ref["db"], "dc": ref["dc"], "dA": ar.stored_values(ref["dA"], A),
               "dP": ar.stored_values(ref["dP"], P) if P is not None else None}
    else:
        got = grad(gx, gy, gs)
    if which == "bcA":
        db, dc, dAv = rng.standard_normal(m), rng.standard_normal(n), rng.standard_normal(A.nnz)
        pred = got["db"] @ db + got["dc"] @ dc + got["dA"] @ dAv
    else:
        dPv = rng.standard_normal(P.nnz)
        pred = got["dP"] @ dPv

    def moved(t):
        d = ar.data_of(p)
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
