"""Dense numpy reference for SCS.refine (csrc/refine.hpp): the stop rule's figures and a Newton iteration with exact steps.

In the unknowns z = (x, v) with s = Pi_K(v), y = Pi_K(v) - v the optimality conditions are (tests/adjoint_ref.py)
    F1 = P x + A'(Pi(v) - v) + c,   F2 = A x + Pi(v) - b,   J = [[P, A'(W - I)], [A, W]],   W = D Pi_K(v).
`mod` below is the reference module of the problem's cones — adjoint_ref (z, l, q), dproj_cones_ref (+ box, p), adjoint_psd_ref (+ s):
its `project` and `cone_W` are all that is used."""
import numpy as np

import adjoint_ref as ar


def dense(p):
    A = np.asarray(p["A"].todense())
    n = A.shape[1]
    P = np.zeros((n, n)) if p["P"] is None else ar.full_P(p["P"])
    return A, P


def residuals(p, x, y, s):
    """the three figures of the solver's stop rule in the caller's units and the scale each is compared against:
    {"pri", "dual", "gap"} and {"pri_scale", "dual_scale", "gap_scale"}; the rule is figure <= tol (1 + scale)"""
    A, P = dense(p)
    inf = lambda a: float(np.abs(a).max()) if a.size else 0.0
    Ax, Px, Aty = A @ x, P @ x, A.T @ y
    xPx, ctx, bty = float(x @ Px), float(p["c"] @ x), float(p["b"] @ y)
    return {"pri": inf(Ax + s - p["b"]), "pri_scale": max(inf(Ax), inf(s), inf(p["b"])),
            "dual": inf(Px + Aty + p["c"]), "dual_scale": max(inf(Px), inf(Aty), inf(p["c"])),
            "gap": abs(xPx + ctx + bty), "gap_scale": max(abs(xPx), abs(ctx), abs(bty))}


def meets(res, tol):
    return all(res[k] <= tol * (1.0 + res[k + "_scale"]) for k in ("pri", "dual", "gap"))


def F(p, mod, x, v):
    A, P = dense(p)
    s = mod.project(v, p["cone"])
    return np.concatenate([P @ x + A.T @ (s - v) + p["c"], A @ x + s - p["b"]])


def jacobian(p, mod, v):
    return ar.jacobian(p["A"], p["P"], mod.cone_W(v, p["cone"]))


def newton(p, mod, x, v, max_steps=20, tol=1e-10):
    """Newton on F(x, v) = 0 from (x, v) with exact (lstsq) steps and the line search of csrc/refine.hpp: t = 1, 1/2, ... (at most 10
    halvings), accept |F(z + t d)|_2 < (1 - 1e-4 t) |F(z)|_2; stops when the stop rule holds at `tol`, after max_steps accepted steps, or
    when no t gives a decrease.  Returns (steps, x, v)."""
    n = x.shape[0]
    x, v = x.copy(), v.copy()
    steps = 0

    def done(x, v):
        s = mod.project(v, p["cone"])
        return meets(residuals(p, x, s - v, s), tol)

    while steps < max_steps and not done(x, v):
        f = F(p, mod, x, v)
        phi = np.linalg.norm(f)
        d = np.linalg.lstsq(jacobian(p, mod, v), -f, rcond=None)[0]
        t = 1.0
        for _ in range(11):
            xt, vt = x + t * d[:n], v + t * d[n:]
            if np.linalg.norm(F(p, mod, xt, vt)) < (1.0 - 1e-4 * t) * phi:
                break
            t *= 0.5
        else:
            break
        x, v = xt, vt
        steps += 1
    return steps, x, v
