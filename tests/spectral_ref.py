"""numpy reference projections onto the spectral cones (scs-python_amd/csrc/spectral.hpp), with membership tests for K and K*.

Slice layouts (as in the m-vector):
    d    : (t, v, svec X)       K = cl{ v > 0, X > 0, t <= v log det(X / v) }
    nuc  : (t, vec X), X m x n column-major     K = { t >= ||X||_* }
    ell1 : (t, x)               K = { t >= ||x||_1 }
    sl   : (t, svec X)          K = { t >= sum of the k largest eigenvalues of X }
svec is the PSD cone's layout: lower triangle by column, off-diagonal entries times sqrt(2), so that <svec X, svec Y> = tr(XY).

Every projection reduces to an eigen- or singular-value decomposition (numpy eigh / svd) and a projection of the value vector,
solved here by algorithms independent of the device kernels (sorting, nested bisection, scalar root brackets).  Dual cones,
derived once for all four from K = { (t, X) : t >= sigma_C(X) } style support-function arguments, are in the docstrings of the
`in_dual_*` functions.  Positive homogeneity (Pi(a w) = a Pi(w), a > 0) is used to scale inputs to unit size.
"""
import numpy as np

SQ2 = np.sqrt(2.0)


# ---------------------------------------------------------------- layouts
def svec(X):
    n = X.shape[0]
    out = []
    for j in range(n):
        for i in range(j, n):
            out.append(X[i, j] if i == j else SQ2 * X[i, j])
    return np.array(out)


def smat(v):
    n = int(round((np.sqrt(8 * len(v) + 1) - 1) / 2))
    X = np.zeros((n, n))
    k = 0
    for j in range(n):
        for i in range(j, n):
            X[i, j] = X[j, i] = v[k] if i == j else v[k] / SQ2
            k += 1
    return X


def sd(n):
    return n * (n + 1) // 2


# ---------------------------------------------------------------- ell1
def proj_ell1_vec(t, a):
    """(t, a) onto {t >= ||a||_1}: a+ = sign(a) max(|a| - lam, 0), t+ = t + lam, lam the root of
    sum max(|a_i| - lam, 0) = t + lam (found by sorting the breakpoints)."""
    a = np.asarray(a, dtype=float)
    u = np.abs(a)
    if u.sum() <= t:
        return float(t), a.copy()
    if u.size == 0 or u.max() <= -t:
        return 0.0, np.zeros_like(a)
    s = np.sort(u)[::-1]
    cs = np.cumsum(s)
    lam = None
    for j in range(1, len(s) + 1):  # j largest entries active
        cand = (cs[j - 1] - t) / (j + 1)
        lo = s[j] if j < len(s) else 0.0
        if cand >= lo - 1e-300 and cand <= s[j - 1]:
            lam = cand
            break
    if lam is None:
        lam = max((cs[-1] - t) / (len(s) + 1), 0.0)
    lam = max(lam, 0.0)
    return float(t + lam), np.sign(a) * np.maximum(u - lam, 0.0)


def proj_ell1(w):
    t, x = proj_ell1_vec(w[0], w[1:])
    return np.concatenate([[t], x])


def in_ell1(p, tol):
    return p[0] >= np.abs(p[1:]).sum() - tol


def in_dual_ell1(p, tol):
    """K* of {t >= ||x||_1} is {s >= ||y||_inf}: st + y.x >= t s - ||y||_inf ||x||_1 >= 0, tight for x = -t sign(y_i) e_i."""
    return p[0] >= (np.abs(p[1:]).max() if p.size > 1 else 0.0) - tol


# ---------------------------------------------------------------- nuclear norm
def unvec_nuc(w, m, n):
    return w[0], np.asarray(w[1:]).reshape((m, n), order="F")


def proj_nuc(w, m, n):
    """Pi(t, X) = (t+, U diag(sigma+) V') with (t+, sigma+) = Pi_ell1(t, sigma): the nuclear norm is the ell1 norm of the
    singular values and the cone is unitarily invariant."""
    t, X = unvec_nuc(w, m, n)
    U, sig, Vt = np.linalg.svd(X, full_matrices=False)
    tp, sp = proj_ell1_vec(t, sig)
    Xp = (U * sp) @ Vt
    return np.concatenate([[tp], Xp.reshape(-1, order="F")])


def in_nuc(p, m, n, tol):
    t, X = unvec_nuc(p, m, n)
    return t >= np.linalg.svd(X, compute_uv=False).sum() - tol


def in_dual_nuc(p, m, n, tol):
    """K* of {t >= ||X||_*} is {s >= ||Y||_2} (dual norms): st + <Y, X> >= s t - ||Y||_2 ||X||_* >= 0."""
    s, Y = unvec_nuc(p, m, n)
    return s >= np.linalg.norm(Y, 2) - tol


# ---------------------------------------------------------------- sum of the k largest eigenvalues
def _topk(lam, k):
    return np.sort(lam)[::-1][:k].sum()


def proj_sl_vec(t, lam, k):
    """(t, lam) onto {t >= f_k(lam)}, f_k = sum of the k largest.  mu_i = lam_i - clip(lam_i - c, 0, theta), t+ = t + theta:
    for a fixed theta the level c solves sum clip(lam_i - c, 0, theta) = k theta (decreasing in c: bisection); then
    h(theta) = f_k(mu(theta)) - t - theta is decreasing and its root is bisected too."""
    lam = np.asarray(lam, dtype=float)
    if _topk(lam, k) <= t:
        return float(t), lam.copy()

    def c_of(th):
        lo, hi = lam.min() - th - 1.0, lam.max() + 1.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if np.clip(lam - mid, 0.0, th).sum() > k * th:
                lo = mid
            else:
                hi = mid
            if hi - lo <= 1e-18 * max(1.0, abs(mid)):
                break
        return 0.5 * (lo + hi)

    def mu_of(th):
        if k == len(lam):
            return lam - th
        return lam - np.clip(lam - c_of(th), 0.0, th)

    def h(th):
        return _topk(mu_of(th), k) - t - th

    lo, hi = 0.0, 1.0
    while h(hi) > 0:
        lo, hi = hi, 2 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if h(mid) > 0:
            lo = mid
        else:
            hi = mid
        if hi - lo <= 1e-17 * hi:
            break
    th = 0.5 * (lo + hi)
    return float(t + th), mu_of(th)


def proj_sl(w, n, k):
    X = smat(w[1:])
    lam, V = np.linalg.eigh(X)
    tp, mu = proj_sl_vec(w[0], lam, k)
    return np.concatenate([[tp], svec((V * mu) @ V.T)])


def in_sl(p, n, k, tol):
    return p[0] >= _topk(np.linalg.eigvalsh(smat(p[1:])), k) - tol


def in_dual_sl(p, n, k, tol):
    """f_k(X) = max{ tr(XZ) : 0 <= Z <= I, tr Z = k } is the support function of that set C, so K = {t >= sigma_C(X)} and
    K* = {(s, Y) : s >= 0, -Y in s C}: the eigenvalues of -Y lie in [0, s] and add up to k s."""
    s = p[0]
    mu = np.linalg.eigvalsh(-smat(p[1:]))
    scale = max(1.0, abs(s), np.abs(mu).max())
    return (s >= -tol and mu.min() >= -tol * scale and mu.max() <= s + tol * scale and abs(mu.sum() - k * s) <= tol * scale * k)


# ---------------------------------------------------------------- log-det
def _brent_increasing(f, lo, hi, it=300):
    """root of an increasing f on [lo, hi] with f(lo) <= 0 < f(hi): bisection to the last bit"""
    for _ in range(it):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if f(mid) > 0:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


def proj_logdet_vec(t, v, x):
    """(t, v, x) onto K_log = cl{ v > 0, x > 0, t <= v sum log(x_i / v) }.  KKT with multiplier rho:
    t+ = t - rho, x+_i = (x_i + sqrt(x_i^2 + 4 rho v+)) / 2, v+ = v + rho (sum log(x+_i / v+) - n), t+ = v+ sum log(x+_i / v+).
    Nested scalar brackets: for v+ fixed, rho solves the (increasing) last equation; the second-last, as a function of v+,
    is increasing (it is the derivative of a strictly convex function) and is bisected.  v+ -> 0 is the face v = 0."""
    x = np.asarray(x, dtype=float)
    n = x.size
    scale = max(abs(t), abs(v), np.abs(x).max())
    if scale == 0:
        return 0.0, 0.0, np.zeros(n)
    t, v, x = t / scale, v / scale, x / scale
    if v > 0 and x.min() > 0 and v * np.log(x / v).sum() >= t:
        return t * scale, v * scale, x * scale

    def xp_of(rho, vp):
        q = np.sqrt(x * x + 4 * rho * vp)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(x >= 0, 0.5 * (x + q), 2 * rho * vp / (q - x))

    def h(rho, vp):
        with np.errstate(divide="ignore"):
            return vp * np.log(xp_of(rho, vp) / vp).sum() + rho - t

    def inner(vp):
        if x.min() > 0 and h(0.0, vp) >= 0:
            return 0.0
        lo, hi = 0.0, 1.0
        while h(hi, vp) <= 0:
            lo, hi = hi, 2 * hi
        return _brent_increasing(lambda r: h(r, vp), lo, hi)

    def G(vp):
        rho = inner(vp)
        if rho == 0:
            return vp - v
        return vp - v + rho * (n - np.log(xp_of(rho, vp) / vp).sum())

    lo, hi = 0.0, max(v, 0.0) + 1.0
    while G(hi) <= 0:
        lo, hi = hi, 2 * hi
    vp = _brent_increasing(G, lo, hi, it=120)
    rho = inner(vp)
    return (t - rho) * scale, vp * scale, xp_of(rho, vp) * scale


def proj_logdet(w, n):
    X = smat(w[2:])
    lam, V = np.linalg.eigh(X)
    tp, vp, mu = proj_logdet_vec(w[0], w[1], lam)
    return np.concatenate([[tp, vp], svec((V * mu) @ V.T)])


def in_logdet(p, n, tol):
    t, v = p[0], p[1]
    lam = np.linalg.eigvalsh(smat(p[2:]))
    if v < -tol or lam.min() < -tol:
        return False
    if v <= tol:  # the face v = 0 of the closure: t <= 0, X >= 0
        return t <= tol
    lam = np.maximum(lam, 1e-300)
    return t <= v * np.log(lam / v).sum() + tol


def in_dual_logdet(p, n, tol):
    """K* = cl{ (s, u, Y) : s < 0, Y > 0, u >= s sum (log(lambda_i(Y) / (-s)) + 1) }.  For s < 0 the worst t is
    v sum log(x_i / v); with z = x / v the condition is s sum log z_i + u + y.z >= 0 for all z > 0, i.e. y > 0 and, at the
    minimiser z_i = -s / y_i, u >= n s - s sum log(-s / y_i).  s > 0 is impossible (t -> -inf), s = 0 leaves u >= 0, Y >= 0."""
    s, u = p[0], p[1]
    lam = np.linalg.eigvalsh(smat(p[2:]))
    if s > tol or lam.min() < -tol:
        return False
    if s >= -tol:
        return u >= -tol
    lam = np.maximum(lam, 1e-300)
    return u >= s * (np.log(lam / (-s)) + 1).sum() - tol


# ---------------------------------------------------------------- whole m-vectors
def spectral_order(cone):
    """(kind, sizes) of every spectral cone in m-vector order: d, nuc, ell1, sl"""
    out = [("d", (n,)) for n in cone.get("d", [])]
    out += [("nuc", (a, b)) for a, b in zip(cone.get("nuc_m", []), cone.get("nuc_n", []))]
    out += [("ell1", (n,)) for n in cone.get("ell1", [])]
    out += [("sl", (n, k)) for n, k in zip(cone.get("sl_n", []), cone.get("sl_k", []))]
    return out


def length(kind, sz):
    return {"d": lambda: sd(sz[0]) + 2, "nuc": lambda: sz[0] * sz[1] + 1, "ell1": lambda: sz[0] + 1,
            "sl": lambda: sd(sz[0]) + 1}[kind]()


def proj(kind, sz, w, dual=False):
    """Pi_K (dual=False) or Pi_{K*} = w + Pi_K(-w) (Moreau) of one cone's slice"""
    f = {"d": lambda z: proj_logdet(z, *sz), "nuc": lambda z: proj_nuc(z, *sz), "ell1": proj_ell1,
         "sl": lambda z: proj_sl(z, *sz)}[kind]
    w = np.asarray(w, dtype=float)
    return w + f(-w) if dual else f(w)


def member(kind, sz, p, tol, dual=False):
    if dual:
        return {"d": lambda: in_dual_logdet(p, sz[0], tol), "nuc": lambda: in_dual_nuc(p, *sz, tol),
                "ell1": lambda: in_dual_ell1(p, tol), "sl": lambda: in_dual_sl(p, *sz, tol)}[kind]()
    return {"d": lambda: in_logdet(p, sz[0], tol), "nuc": lambda: in_nuc(p, *sz, tol), "ell1": lambda: in_ell1(p, tol),
            "sl": lambda: in_sl(p, *sz, tol)}[kind]()


def m_of(cone):
    """rows of a cone dict, spectral cones included (R:test/test_spectral_and_complex_cones.py:27-51)"""
    m = cone.get("z", 0) + cone.get("l", 0)
    m += sum(cone.get("q", [])) + sum(sd(s) for s in cone.get("s", [])) + sum(c * c for c in cone.get("cs", []))
    m += 3 * (cone.get("ep", 0) + cone.get("ed", 0) + len(cone.get("p", [])))
    m += sum(length(kd, sz) for kd, sz in spectral_order(cone))
    if cone.get("bu") is not None and len(cone.get("bu", [])):
        m += len(cone["bu"]) + 1
    return m


# ---------------------------------------------------------------- standard-cone reformulations
# min 1/2 |z - w|^2 over z = one spectral cone's slice plus auxiliary variables, with standard cones (l, s, ep) that force z into K:
# the optimal value and z equal those of the projection of w.  Each builder returns (data, cone) for a standard SCS solve.
def _sparse():
    import scipy.sparse
    return scipy.sparse


class _Rows:
    """s = G u + h, one cone block after the other; A = -G, b = h"""

    def __init__(self, N):
        self.N, self.G, self.h = N, [], []

    def row(self, coef=None, const=0.0):
        g = np.zeros(self.N)
        for j, a in (coef or {}).items():
            g[j] += a
        self.G.append(g)
        self.h.append(const)

    def data(self, w):
        G = np.array(self.G)
        L = w.size
        P = _sparse().diags(np.r_[np.ones(L), np.zeros(self.N - L)]).tocsc()
        return dict(P=P, A=_sparse().csc_matrix(-G), b=np.array(self.h), c=np.r_[-w, np.zeros(self.N - L)])


def _svec_rows(R, order, entry):
    """append the svec rows of a symmetric matrix of `order` whose (i, j) entry (i >= j) is the affine map entry(i, j)"""
    for j in range(order):
        for i in range(j, order):
            coef = entry(i, j)
            R.row({k: (v if i == j else SQ2 * v) for k, v in coef.items()})


def _tri_index(n):
    """index of the (i, j), i >= j, entry of a lower triangle stored by column"""
    idx, k = {}, 0
    for j in range(n):
        for i in range(j, n):
            idx[(i, j)] = k
            k += 1
    return idx


def reform_nuc(m, n, w):
    """t >= ||X||_*  <=>  exists W1, W2: [[W1, X], [X', W2]] >= 0, (tr W1 + tr W2) / 2 <= t"""
    i1, i2 = _tri_index(m), _tri_index(n)
    oX, o1 = 1, 1 + m * n
    o2 = o1 + len(i1)
    R = _Rows(o2 + len(i2))
    R.row({0: 1.0, **{o1 + i1[(i, i)]: -0.5 for i in range(m)}, **{o2 + i2[(i, i)]: -0.5 for i in range(n)}})  # l
    def entry(i, j):
        if i < m:
            return {o1 + i1[(i, j)]: 1.0}
        if j < m:  # (X')_{i-m, j} = X_{j, i-m}
            return {oX + j + m * (i - m): 1.0}
        return {o2 + i2[(i - m, j - m)]: 1.0}
    _svec_rows(R, m + n, entry)
    return R.data(w), {"l": 1, "s": [m + n]}


def reform_sl(n, k, w):
    """sum of the k largest eigenvalues of X <= t  <=>  exists z, Z >= 0: z I + Z - X >= 0, k z + tr Z <= t"""
    it = _tri_index(n)
    oX, oz = 1, 1 + len(it)
    oZ = oz + 1
    R = _Rows(oZ + len(it))
    R.row({0: 1.0, oz: -float(k), **{oZ + it[(i, i)]: -1.0 for i in range(n)}})
    _svec_rows(R, n, lambda i, j: {oZ + it[(i, j)]: 1.0})
    # z I + Z - X: the X part is already an svec entry (off-diagonal values carry sqrt 2), so divide it back out
    _svec_rows(R, n, lambda i, j: {**({oz: 1.0} if i == j else {}), oZ + it[(i, j)]: 1.0, oX + it[(i, j)]: -(1.0 if i == j else 1 / SQ2)})
    return R.data(w), {"l": 1, "s": [n, n]}


def reform_d(n, w):
    """t <= v log det(X / v)  <=>  exists lower-triangular D, r: [[X, D], [D', diag(D)]] >= 0, (r_i, v, D_ii) in K_exp, sum r >= t
    (X = L L' with L lower triangular, D = L diag(L) attains det X = prod D_ii)"""
    it = _tri_index(n)
    oX, oD = 2, 2 + len(it)
    orr = oD + len(it)
    R = _Rows(orr + n)
    R.row({0: -1.0, **{orr + i: 1.0 for i in range(n)}})  # sum r - t >= 0
    def entry(i, j):
        if i < n:  # X block: its svec entry, off-diagonal sqrt 2 divided back out
            return {oX + it[(i, j)]: 1.0 if i == j else 1 / SQ2}
        if j < n:  # (D')_{i-n, j} = D_{j, i-n}, lower triangular: j >= i - n
            return {oD + it[(j, i - n)]: 1.0} if j >= i - n else {}
        return {oD + it[(i - n, i - n)]: 1.0} if i == j else {}
    _svec_rows(R, 2 * n, entry)
    for i in range(n):  # (r_i, v, D_ii) in K_exp
        R.row({orr + i: 1.0})
        R.row({1: 1.0})
        R.row({oD + it[(i, i)]: 1.0})
    return R.data(w), {"l": 1, "s": [2 * n], "ep": n}




def reformulation(kind, sz, w):
    return {"nuc": lambda: reform_nuc(*sz, w), "sl": lambda: reform_sl(*sz, w), "d": lambda: reform_d(*sz, w)}[kind]()
