"""Dense numpy reference for the forward derivative with perturbations of the matrix VALUES (csrc/perturb.hpp), on top of
tests/adjoint_ref.py.

From F1 = P x + A' y + c = 0 and F2 = A x + s - b = 0 a perturbation (dA, dP, db, dc) of the data gives
    J (dx ; dv) = (-(dc + dP x + dA' y) ; db - dA x),
so the forward reference is called with  dc_eff = dc + dP x + dA' y  and  db_eff = db - dA x.
dA is nnz(A) values in the stored (CSC) order of A; dP is nnz(P) values of the stored upper triangle T, an off-diagonal value standing
for both of its mirror images: the full perturbation is T + T' - diag(T)."""
import numpy as np
from scipy import sparse

import adjoint_ref as ar


def dense_dA(A, dAv):
    """the dense perturbation of A from values in its stored order"""
    A = sparse.csc_matrix(A)
    return sparse.csc_matrix((np.asarray(dAv, dtype=float), A.indices, A.indptr), shape=A.shape).toarray()


def dense_dP(P, dPv):
    """the dense SYMMETRIC perturbation of P from values of its stored upper triangle: T + T' - diag(T)"""
    P = sparse.csc_matrix(P)
    T = sparse.csc_matrix((np.asarray(dPv, dtype=float), P.indices, P.indptr), shape=P.shape).toarray()
    assert not np.tril(T, -1).any(), "P is stored as an upper triangle"
    return T + T.T - np.diag(np.diag(T))


def products(A, P, x, y, dAv=None, dPv=None):
    """(dP x + dA' y, dA x): what scs_hip_data_perturbation writes"""
    m, n = A.shape
    out_c, out_b = np.zeros(n), np.zeros(m)
    if dAv is not None:
        dA = dense_dA(A, dAv)
        out_c += dA.T @ y
        out_b += dA @ x
    if dPv is not None:
        out_c += dense_dP(P, dPv) @ x
    return out_c, out_b


def effective(A, P, x, y, db=None, dc=None, dAv=None, dPv=None):
    """(db_eff, dc_eff)"""
    m, n = A.shape
    out_c, out_b = products(A, P, x, y, dAv, dPv)
    return (np.zeros(m) if db is None else db) - out_b, (np.zeros(n) if dc is None else dc) + out_c


def derivative(A, P, cone, x, y, s, db=None, dc=None, dAv=None, dPv=None, forward=ar.derivative):
    """{"dx", "dy", "ds", "J"}: `forward` (adjoint_ref.derivative, or adjoint_psd_ref.derivative for cones with PSD blocks) at the
    effective right-hand side"""
    db_eff, dc_eff = effective(A, P, x, y, db, dc, dAv, dPv)
    return forward(A, P, cone, x, y, s, db_eff, dc_eff)


def directions(p, seed):
    """one random direction (db, dc, dAv, dPv) for a problem of the generators; dPv is None without P"""
    rng = np.random.default_rng(seed)
    A, P = p["A"], p["P"]
    m, n = A.shape
    return rng.standard_normal(m), rng.standard_normal(n), rng.standard_normal(A.nnz), rng.standard_normal(P.nnz) if P is not None else None


FD_SEED = 300


def fd_compare(p, solve, seed, h, predict=None):
    """Relative differences {"dx", "dy", "ds"} between the forward derivative in a random direction (dA, dP) — b and c stay — and the
    central difference (sol(+h) - sol(-h)) / 2h of solve(data) -> {"x", "y", "s"}, plus "cond" = cond2(J).  The prediction is the dense
    reference at the unperturbed solution, or predict(dAv, dPv) -> {"dx", "dy", "ds"} called right after the unperturbed solve."""
    A, P = p["A"], p["P"]
    _, _, dAv, dPv = directions(p, seed)
    base = solve(ar.data_of(p))
    ref = derivative(A, P, p["cone"], base["x"], base["y"], base["s"], dAv=dAv, dPv=dPv)
    got = ref if predict is None else predict(dAv, dPv)

    def moved(t):
        d = ar.data_of(p)
        A2 = A.copy()
        A2.data = A.data + t * dAv
        d["A"] = A2
        if P is not None:
            P2 = P.copy()
            P2.data = P.data + t * dPv
            d["P"] = P2
        return d

    plus, minus = solve(moved(h)), solve(moved(-h))
    out = {"cond": float(np.linalg.cond(ref["J"]))}
    for key in ("x", "y", "s"):
        fd = (plus[key] - minus[key]) / (2 * h)
        out["d" + key] = float(np.linalg.norm(got["d" + key] - fd) / np.linalg.norm(fd))
    return out
