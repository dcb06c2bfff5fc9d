"""Dense numpy reference for the derivative of the box-cone and power-cone projections (csrc/dproj_box_pow.hpp), a cone_W that extends
tests/adjoint_ref.py / tests/adjoint_psd_ref.py with `bu` / `bl` / `p` in SCS row order (z | l | box | q | s | p), and a generator of
small problems with a known solution in the style of adjoint_ref.gen_problem.

Box cone K = {(t, w): t bl <= w <= t bu, t >= 0} at v = (v0, w): with t* the first entry of Pi_K(v), U = {w_j > t* bu_j},
L = {w_j < t* bl_j}, a_j = bu_j on U, bl_j on L, 0 elsewhere, h = 1 + sum a_j^2:
    W = [[1/h, a'/h], [a/h, diag(free) + a a'/h]]  if t* > 0,   W = diag(0, free)  if t* = 0.
Power cone pow(a) = {(x, y, z): x^a y^(1-a) >= |z|, x, y >= 0}: W = I inside, 0 inside the polar cone, else with p = (x, y, sz r) the
projection, mu = |v_z| - r, g = (a r / x, (1-a) r / y, -sz), H the Hessian of x^a y^(1-a) at p, M = (I - mu H)^{-1}:
    W = M - (M g)(M g)' / (g' M g).
An exponent a < 0 stands for the dual cone pow(|a|)*: W = I - W_pow(|a|)(-v).
The projections here are found by BISECTION (box: on t; power: on r), not by the formulas above: they are the independent side of
the finite-difference checks in tests/test_dproj_cones_ref_cpu.py."""
import numpy as np
from scipy import sparse

import adjoint_ref as ar
import adjoint_psd_ref as pr


# ---------------------------------------------------------------- box cone
def _box_g(t, v0, w, bl, bu):
    """derivative in t of 0.5 |(t, clip(w, t bl, t bu)) - v|^2: increasing in t"""
    with np.errstate(invalid="ignore"):
        hi, lo = w > t * bu, w < t * bl
    g = t - v0
    g += np.sum((t * bu[hi] - w[hi]) * bu[hi]) + np.sum((t * bl[lo] - w[lo]) * bl[lo])
    return g


def box_tstar(v, bl, bu):
    """the first entry of the projection of v onto the box cone, by bisection"""
    v0, w = v[0], v[1:]
    if _box_g(0.0, v0, w, bl, bu) >= 0:
        return 0.0
    lo, hi = 0.0, max(1.0, abs(v0))
    while _box_g(hi, v0, w, bl, bu) < 0:
        hi *= 2
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _box_g(mid, v0, w, bl, bu) < 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def box_sets(v, bl, bu, t=None):
    """(t*, U, L) with the comparisons of the projection: an infinite bound is never active"""
    t = box_tstar(v, bl, bu) if t is None else t
    with np.errstate(invalid="ignore"):
        U, L = v[1:] > t * bu, v[1:] < t * bl
    return t, U, L


def box_project(v, bl, bu):
    t, U, L = box_sets(v, bl, bu)
    out = v.copy()
    out[0] = t
    out[1:][U] = t * bu[U]
    out[1:][L] = t * bl[L]
    return out


def box_coef(v, bl, bu):
    """(t*, a, active, h)"""
    t, U, L = box_sets(v, bl, bu)
    a = np.zeros(v.size - 1)
    a[U] = bu[U]
    a[L] = bl[L]
    return t, a, U | L, 1.0 + a @ a


def box_W(v, bl, bu):
    k = v.size - 1
    bl, bu = np.asarray(bl, float), np.asarray(bu, float)
    t, a, act, h = box_coef(v, bl, bu)
    W = np.zeros((k + 1, k + 1))
    W[1:, 1:] = np.diag((~act).astype(float))
    if t > 0:
        W[0, 0] = 1.0 / h
        W[0, 1:] = a / h
        W[1:, 0] = a / h
        W[1:, 1:] += np.outer(a, a) / h
    return W


# ---------------------------------------------------------------- power cone
def _pow_x(r, xh, rh, a):
    q = a * (rh - r) * r
    d = np.sqrt(xh * xh + 4 * q)
    return 0.5 * (xh + d) if xh >= 0 else 2 * q / (d - xh)


def pow_case(v, a):
    """"in", "polar" or "bd" for the primal cone pow(a), 0 < a < 1"""
    xh, yh, rh = v[0], v[1], abs(v[2])
    if xh >= 0 and yh >= 0 and xh ** a * yh ** (1 - a) >= rh:
        return "in"
    if xh <= 0 and yh <= 0 and (-xh) ** a * (-yh) ** (1 - a) >= rh * a ** a * (1 - a) ** (1 - a):
        return "polar"
    return "bd"


def pow_project_primal(v, a):
    """projection onto pow(a), 0 < a < 1: bisection on r"""
    case = pow_case(v, a)
    if case == "in":
        return v.copy()
    if case == "polar":
        return np.zeros(3)
    xh, yh, rh = v[0], v[1], abs(v[2])
    if rh == 0:
        return np.array([max(xh, 0.0), max(yh, 0.0), 0.0])
    lo, hi = 0.0, rh
    for _ in range(200):
        r = 0.5 * (lo + hi)
        if _pow_x(r, xh, rh, a) ** a * _pow_x(r, yh, rh, 1 - a) ** (1 - a) - r > 0:
            lo = r
        else:
            hi = r
    r = 0.5 * (lo + hi)
    return np.array([_pow_x(r, xh, rh, a), _pow_x(r, yh, rh, 1 - a), np.sign(v[2]) * r])


def pow_project(v, a):
    """projection onto the cone of exponent a: pow(a) for a >= 0, pow(|a|)* for a < 0 (Moreau)"""
    return pow_project_primal(v, a) if a >= 0 else v + pow_project_primal(-v, -a)


def _pow_parts(v, a):
    """(I - mu H, g) at the projection of a boundary-case v onto pow(a)"""
    p = pow_project_primal(v, a)
    x, y, r = p[0], p[1], abs(p[2])
    sz = -1.0 if v[2] < 0 else 1.0
    mu = abs(v[2]) - r
    g = np.array([a * r / x, (1 - a) * r / y, -sz])
    H = np.zeros((3, 3))
    H[0, 0] = a * (a - 1) * r / x ** 2
    H[0, 1] = H[1, 0] = a * (1 - a) * r / (x * y)
    H[1, 1] = -a * (1 - a) * r / y ** 2
    return np.eye(3) - mu * H, g


def pow_W_primal(v, a):
    case = pow_case(v, a)
    if case == "in":
        return np.eye(3)
    if case == "polar":
        return np.zeros((3, 3))
    if v[2] == 0:
        return np.diag([float(v[0] > 0), float(v[1] > 0), 0.0])
    B, g = _pow_parts(v, a)
    M = np.linalg.inv(B)
    Mg = M @ g
    return M - np.outer(Mg, Mg) / (g @ Mg)


def pow_W(v, a):
    return pow_W_primal(v, a) if a >= 0 else np.eye(3) - pow_W_primal(-v, -a)


def pow_cond(v, a):
    """cond2(I - mu H) of the boundary case (1 in the other cases): the factor of the device's error bound"""
    vv, aa = (v, a) if a >= 0 else (-v, -a)
    if pow_case(vv, aa) != "bd" or vv[2] == 0:
        return 1.0
    return float(np.linalg.cond(_pow_parts(vv, aa)[0]))


def pow_case_of(v, a):
    """the case of v for the cone of exponent a (a < 0: the dual cone): "in" = W is I, "polar" = W is 0"""
    if a >= 0:
        return pow_case(v, a)
    return {"in": "polar", "polar": "in", "bd": "bd"}[pow_case(-v, -a)]


# ---------------------------------------------------------------- the whole cone
def offsets(cone):
    """row offsets (box, q, s, p, m) of a cone dict with z, l, bu / bl, q, s, p"""
    z, l = int(cone.get("z", 0)), int(cone.get("l", 0))
    k = len(cone.get("bu", []))
    o_box = z + l
    o_q = o_box + (k + 1 if k else 0)
    o_s = o_q + sum(cone.get("q", []))
    o_p = o_s + sum(pr.sd_size(p) for p in cone.get("s", []))
    return o_box, o_q, o_s, o_p, o_p + 3 * len(cone.get("p", []))


def cone_W(v, cone):
    """W = D Pi_K(v), dense, for a cone dict with z, l, bu / bl, q, s, p"""
    o_box, o_q, o_s, o_p, m = offsets(cone)
    assert v.shape[0] == m
    W = np.zeros((m, m))
    zl = {"z": int(cone.get("z", 0)), "l": int(cone.get("l", 0)), "q": []}
    W[:o_box, :o_box] = ar.cone_W(v[:o_box], zl)
    if o_q > o_box:
        W[o_box:o_q, o_box:o_q] = box_W(v[o_box:o_q], np.asarray(cone["bl"], float), np.asarray(cone["bu"], float))
    W[o_q:o_s, o_q:o_s] = ar.cone_W(v[o_q:o_s], {"q": list(cone.get("q", []))})
    o = o_s
    for p in cone.get("s", []):
        d = pr.sd_size(p)
        W[o:o + d, o:o + d] = pr.psd_W(v[o:o + d], p)
        o += d
    for a in cone.get("p", []):
        W[o:o + 3, o:o + 3] = pow_W(v[o:o + 3], a)
        o += 3
    return W


def project(v, cone):
    o_box, o_q, o_s, o_p, m = offsets(cone)
    out = v.copy()
    zl = {"z": int(cone.get("z", 0)), "l": int(cone.get("l", 0)), "q": []}
    out[:o_box] = ar.project(v[:o_box], zl)
    if o_q > o_box:
        out[o_box:o_q] = box_project(v[o_box:o_q], np.asarray(cone["bl"], float), np.asarray(cone["bu"], float))
    out[o_q:o_s] = ar.project(v[o_q:o_s], {"q": list(cone.get("q", []))})
    o = o_s
    for p in cone.get("s", []):
        d = pr.sd_size(p)
        out[o:o + d] = pr.psd_project(v[o:o + d], p)
        o += d
    for a in cone.get("p", []):
        out[o:o + 3] = pow_project(v[o:o + 3], a)
        o += 3
    return out


def adjoint(A, P, cone, x, y, s, gx=None, gy=None, gs=None):
    """as adjoint_ref.adjoint, with this module's cone_W"""
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


def derivative(A, P, cone, x, y, s, db=None, dc=None, dA=None, dP=None):
    """as adjoint_ref.derivative; dA (dense m x n) and dP (dense symmetric n x n) perturb the matrices:
    dc + dP x + dA' y and db - dA x take the place of dc and db"""
    m, n = A.shape
    db = np.zeros(m) if db is None else db
    dc = np.zeros(n) if dc is None else dc
    if dA is not None:
        dc = dc + dA.T @ y
        db = db - dA @ x
    if dP is not None:
        dc = dc + dP @ x
    W = cone_W(s - y, cone)
    J = ar.jacobian(A, P, W)
    q = np.linalg.lstsq(J, np.concatenate([-dc, db]), rcond=None)[0]
    dv = q[n:]
    return {"dx": q[:n], "ds": W @ dv, "dy": (W - np.eye(m)) @ dv, "J": J}


# ---------------------------------------------------------------- generator
MARGIN = 1e-3  # no generated v lies within this relative distance of a case boundary


def box_point(rng, bl, bu, sets, tstar):
    """v = (v0, w) whose projection has first entry tstar > 0 and row j on its upper bound (sets[j] = "U"), lower bound ("L") or free
    ("F"); active rows overshoot their bound by 0.3 .. 1, free rows keep 20 % of the gap (or 0.3) to either bound"""
    bl, bu = np.asarray(bl, float), np.asarray(bu, float)
    k = bl.size
    w = np.zeros(k)
    v0 = tstar
    for j in range(k):
        lo, hi = tstar * bl[j], tstar * bu[j]
        if sets[j] == "U":
            assert np.isfinite(hi)
            d = rng.uniform(0.3, 1.0)
            w[j] = hi + d
            v0 -= d * bu[j]
        elif sets[j] == "L":
            assert np.isfinite(lo)
            d = rng.uniform(0.3, 1.0)
            w[j] = lo - d
            v0 += d * bl[j]
        else:
            a = lo + 0.2 * (hi - lo) if np.isfinite(lo) and np.isfinite(hi) else (lo + 0.3 if np.isfinite(lo) else
                                                                                  hi - 0.3 if np.isfinite(hi) else -1.0)
            b = hi - 0.2 * (hi - lo) if np.isfinite(lo) and np.isfinite(hi) else a + 1.0
            w[j] = rng.uniform(a, b)
    return np.concatenate([[v0], w])


def box_case(rng, k, tstar, empty=()):
    """(v, bl, bu) for a box cone with k bound rows, vectorised: bounds of magnitude 0.2 .. 2 with about a tenth each of bu = inf,
    bl = -inf and bl = 0; rows on U / L / F at random (a row on an infinite bound is free; "U" or "L" in `empty` leaves that set
    empty).  tstar > 0: active rows overshoot their bound by 0.3 .. 1, free rows keep a distance to it, and the first entry of the
    projection is tstar.  tstar == 0: |w_j| >= 0.1 and v0 is so negative that the projection's first entry is 0."""
    bl, bu = -rng.uniform(0.2, 2.0, k), rng.uniform(0.2, 2.0, k)
    kind = rng.integers(0, 10, k)
    bu[kind == 0] = np.inf
    bl[kind == 1] = -np.inf
    bl[kind == 2] = 0.0
    if k >= 3:  # every kind is present from three rows on
        bu[0], bl[1], bl[2] = np.inf, -np.inf, 0.0
        bl[0], bu[1], bu[2] = -1.0, 1.0, 1.0
    if tstar == 0:
        w = rng.uniform(0.1, 1.0, k) * rng.choice([-1.0, 1.0], k)
        big = np.maximum(np.where(np.isfinite(bl), np.abs(bl), 0.0), np.where(np.isfinite(bu), bu, 0.0))
        return np.concatenate([[-(1.0 + np.sum(np.abs(w) * big))], w]), bl, bu
    sets = rng.integers(0, 3, k)  # 0 = U, 1 = L, 2 = F
    if k >= 3:
        sets[2] = 1  # the zero bound is active
    sets[(sets == 0) & ~np.isfinite(bu)] = 2
    sets[(sets == 1) & ~np.isfinite(bl)] = 2
    if "U" in empty:
        sets[sets == 0] = 2
    if "L" in empty:
        sets[sets == 1] = 2
    d = rng.uniform(0.3, 1.0, k)
    lo = np.where(np.isfinite(bl), tstar * bl, np.where(np.isfinite(bu), tstar * bu - 2.0, -1.0))
    hi = np.where(np.isfinite(bu), tstar * bu, lo + 2.0)
    w = lo + rng.uniform(0.2, 0.8, k) * (hi - lo)
    U, L = sets == 0, sets == 1
    w[U] = tstar * bu[U] + d[U]
    w[L] = tstar * bl[L] - d[L]
    v0 = tstar - np.sum(d[U] * bu[U]) + np.sum(d[L] * bl[L])
    return np.concatenate([[v0], w]), bl, bu


def pow_point(rng, a, case):
    """a 3-vector in the chosen case ("in": W = I, "polar": W = 0, "bd") of the cone of exponent a, at least MARGIN (relative) away
    from the other cases; a boundary point's projection onto the primal cone has x, y >= 0.05 |v|"""
    if a < 0:
        return -pow_point(rng, -a, {"in": "polar", "polar": "in", "bd": "bd"}[case])
    sz = rng.choice([-1.0, 1.0])
    if case == "in":
        x, y = rng.uniform(0.5, 1.5, 2)
        return np.array([x, y, sz * rng.uniform(0.2, 0.7) * x ** a * y ** (1 - a)])
    if case == "polar":
        x, y = rng.uniform(0.5, 1.5, 2)
        return np.array([-x, -y, sz * rng.uniform(0.2, 0.7) * x ** a * y ** (1 - a) / (a ** a * (1 - a) ** (1 - a))])
    while True:
        v = np.array([rng.uniform(-1.0, 1.5), rng.uniform(-1.0, 1.5), sz * rng.uniform(0.5, 2.0)])
        if min(abs(v[0]), abs(v[1])) < 0.05:
            continue
        if any(pow_case(v * np.array([1.0, 1.0, f]), a) != "bd" for f in (1 - 50 * MARGIN, 1.0)):
            continue
        p = pow_project_primal(v, a)
        if min(p[0], p[1]) >= 0.05 * np.linalg.norm(v) and abs(v[2]) - abs(p[2]) >= 0.05:
            return v


def gen_problem(seed, n, z=0, l=0, tight_l=0, box=None, q=(), q_case=(), s=(), ranks=(), p=(), p_case=(), box_rows_identity=False):
    """A feasible QP (P positive definite) built from a chosen primal-dual pair: v per cone in a chosen case, s = Pi_K(v), y = s - v,
    random x, b = A x + s, c = -A'y - P x.  box = dict(bl, bu, sets, tstar, fix_t): fix_t makes the t row of A zero, so b fixes t = tstar
    (the MPC shape: variable bounds); box_rows_identity makes the bound rows of A minus the first k columns of the identity.
    The caller counts tight directions against n as in adjoint_ref.gen_problem."""
    rng = np.random.default_rng(seed)
    parts = []
    vz = rng.uniform(0.5, 1.5, z) * rng.choice([-1.0, 1.0], z)
    vl = np.concatenate([-rng.uniform(0.5, 1.5, tight_l), rng.uniform(0.5, 1.5, l - tight_l)])
    parts += [vz, vl]
    cone = {"z": z, "l": l}
    if box is not None:
        parts.append(box_point(rng, box["bl"], box["bu"], box["sets"], box["tstar"]))
        cone["bl"], cone["bu"] = list(map(float, box["bl"])), list(map(float, box["bu"]))
    for qi, case in zip(q, q_case):
        zz = rng.standard_normal(qi - 1)
        zz *= rng.uniform(0.8, 1.2) / np.linalg.norm(zz)
        r = np.linalg.norm(zz)
        t = r * (rng.uniform(1.5, 2.0) if case == "in" else -rng.uniform(1.5, 2.0) if case == "polar" else rng.uniform(-0.75, 0.75))
        parts.append(np.concatenate([[t], zz]))
    cone["q"] = list(q)
    for order, rank in zip(s, ranks):
        parts.append(pr.psd_point(rng, order, rank))
    cone["s"] = list(s)
    for a, case in zip(p, p_case):
        parts.append(pow_point(rng, a, case))
    cone["p"] = list(map(float, p))
    v = np.concatenate(parts)
    m = v.size
    sv = project(v, cone)
    y = sv - v
    x = rng.standard_normal(n)
    A = rng.standard_normal((m, n)) / np.sqrt(n)
    if box is not None:
        o = z + l
        k = len(box["bl"])
        if box.get("fix_t"):
            A[o] = 0.0
        if box_rows_identity:
            A[o + 1:o + 1 + k] = 0.0
            A[o + 1 + np.arange(k), np.arange(k)] = -1.0
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    Pd = G @ G.T + 0.5 * np.eye(n)
    P = sparse.triu(sparse.csc_matrix(Pd), format="csc")
    P.sort_indices()
    b = A @ x + sv
    c = -Pd @ x - A.T @ y
    A = sparse.csc_matrix(A)
    A.sort_indices()
    return {"A": A, "P": P, "b": b, "c": c, "cone": cone, "x": x, "y": y, "s": sv}


INF = float("inf")


def problem_box_qp():
    """A bounded QP in the MPC shape: n = 10 variables, 3 equality rows, and the box cone (t, x) with t fixed to 1 through a zero row
    of A and the bound rows -I.  Bounds: 3 active above, 3 active below — one of them the zero bound bl = 0 — 4 free, one of those with
    both bounds infinite, one with bu infinite.  3 + 6 tight directions <= n - 1 and P is positive definite: J is regular."""
    bl = [-1.0, -0.5, -2.0, -1.0, 0.0, -1.5, -1.0, -INF, -0.5, -1.0]
    bu = [1.0, 0.8, 1.5, 1.0, 2.0, 0.7, 1.0, INF, INF, 2.0]
    sets = ["U", "U", "U", "L", "L", "L", "F", "F", "F", "F"]
    return gen_problem(51, n=10, z=3, box=dict(bl=bl, bu=bu, sets=sets, tstar=1.0, fix_t=True), box_rows_identity=True)


POW_P = [0.3, 0.3, 0.3, 0.3, -0.3, -0.3, -0.3, -0.3, 0.5, -0.6, 0.9, -0.1]
POW_CASE = ["in", "polar", "bd", "bd", "in", "polar", "bd", "bd", "bd", "bd", "polar", "in"]


def problem_pow():
    """12 power cones, primal and dual exponents in every case: 1 zero row + 3 rows per cone whose s is 0 (the "polar" case: 3 cones)
    + 1 per boundary cone (6) = 16 tight directions <= n - 1 = 19, P positive definite"""
    return gen_problem(52, n=20, z=1, p=POW_P, p_case=POW_CASE)


def problem_mixed():
    """z | l | box | q | s | p together: 1 zero row + 2 tight rows + 2 active bounds (t free) + 1 boundary SOC + 3 directions of the
    rank-1 PSD block of order 3 + 2 boundary power cones + 3 rows of a polar one = 14 <= n - 1"""
    box = dict(bl=[-1.0, 0.0, -0.5, -INF], bu=[1.0, 1.5, 0.5, 2.0], sets=["U", "L", "F", "F"], tstar=0.8)
    return gen_problem(53, n=16, z=1, l=4, tight_l=2, box=box, q=(3, 4), q_case=("bd", "in"), s=(3,), ranks=(1,),
                       p=(0.4, -0.7, 0.5, 0.25), p_case=("bd", "bd", "in", "polar"))


PROBLEMS = {"box_qp": problem_box_qp, "pow": problem_pow, "mixed": problem_mixed}
FD_SEEDS = {"bcA": 300, "P": 301}
COND_CAP = 1e4


def fd_compare(p, solve, seed, which, h=1e-4, grad=None):
    """adjoint_ref.fd_compare with this module's reference: (relative difference to the central difference, cond(J))"""
    rng = np.random.default_rng(seed)
    A, P = p["A"], p["P"]
    m, n = A.shape
    base = solve(ar.data_of(p))
    gx, gy, gs = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(m)
    ref = adjoint(A, P, p["cone"], base["x"], base["y"], base["s"], gx, gy, gs)
    if grad is None:
        got = {"db": ref["db"], "dc": ref["dc"], "dA": ar.stored_values(ref["dA"], A), "dP": ar.stored_values(ref["dP"], P)}
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


def forward_fd_compare(p, solve, seed, h=1e-4):
    """max over x, y, s of |derivative(db, dc) - central difference| / |central difference| for one random direction (db, dc)"""
    rng = np.random.default_rng(seed)
    A, P = p["A"], p["P"]
    m, n = A.shape
    base = solve(ar.data_of(p))
    db, dc = rng.standard_normal(m), rng.standard_normal(n)
    ref = derivative(A, P, p["cone"], base["x"], base["y"], base["s"], db=db, dc=dc)

    def moved(t):
        d = ar.data_of(p)
        d["b"], d["c"] = p["b"] + t * db, p["c"] + t * dc
        return d

    rp, rm = solve(moved(h)), solve(moved(-h))
    worst = 0.0
    for key, name in (("x", "dx"), ("y", "dy"), ("s", "ds")):
        fd = (rp[key] - rm[key]) / (2 * h)
        worst = max(worst, float(np.linalg.norm(ref[name] - fd) / np.linalg.norm(fd)))
    return worst
