"""Independent reference of the data equilibration (K12), numpy and scipy only.

Written from the algorithm statement in the header of csrc/normalize_dev.hpp, not from any loop of the product or of the CPU checker:

    26 passes on the symmetric matrix [P A'; A 0]: passes 0..24 take the largest magnitude of every line (Ruiz), pass 25 the root of
    the sum of squares.  The lines are the rows of A (-> D), and the columns of A joined with the lines of the full symmetric P (-> E).
    Row norms behind the separable prefix are made constant on every cone block: the largest one in a Ruiz pass, the mean of the
    roots in the l2 pass.  limit(x) = 1 for x < 1e-4, 1e4 for x > 1e4, x otherwise; the factor of a line is 1 / sqrt(limit(norm)).
    A <- diag(Dt) A diag(Et), P <- diag(Et) P diag(Et), D <- D Dt, E <- E Et after every pass.  At the end
    sigma = 1 / limit(max(|D b|_inf, |E c|_inf)), b_hat = sigma D b, c_hat = sigma E c.

Every reduction is a segmented numpy reduction over index arrays, in the working precision `dtype` (float64, or longdouble for the
floor the tests measure against).  Nothing here is dense, so the largest test case takes well under a second."""
import collections

import numpy as np

LO, HI = 1e-4, 1e4
RUIZ_PASSES, L2_PASSES = 25, 1

Equilibrated = collections.namedtuple(
    "Equilibrated", "A P b c D E sigma blocks clamp_margin passes")
# A, P: the scaled values in the CSC order of the inputs (P: the upper triangle as given; None without P)
# blocks: (prefix, [(offset, length), ...]); clamp_margin: see equilibrate(); passes: per pass (row norms as they enter the limit,
# column norms likewise, row factors, column factors)


def _tri(n):
    return n * (n + 1) // 2


def _ints(cone, key):
    v = cone.get(key, [])
    return [int(t) for t in np.atleast_1d(v)] if v is not None else []


def block_table(cone):
    """(prefix, [(offset, length), ...]) of a cone dict: the z + l + box rows are separable (every row its own scale, the box rows
    too); then one block per q, s, cs, ep, ed, p cone and per d, nuc, ell1, sl cone, in that order.  Blocks of length 0 are dropped
    (their offset still advances by 0)."""
    nbox = len(np.atleast_1d(cone.get("bu", []))) if cone.get("bu") is not None else 0
    prefix = int(cone.get("z", 0)) + int(cone.get("f", 0)) + int(cone.get("l", 0)) + (nbox + 1 if nbox else 0)
    lens = list(_ints(cone, "q"))
    lens += [_tri(s) for s in _ints(cone, "s")]
    lens += [s * s for s in _ints(cone, "cs")]
    npow = len(np.atleast_1d(cone.get("p", []))) if cone.get("p") is not None else 0
    lens += [3] * (int(cone.get("ep", 0)) + int(cone.get("ed", 0)) + npow)
    lens += [_tri(d) + 2 for d in _ints(cone, "d")]
    lens += [a * b + 1 for a, b in zip(_ints(cone, "nuc_m"), _ints(cone, "nuc_n"))]
    lens += [v + 1 for v in _ints(cone, "ell1")]
    lens += [_tri(v) + 1 for v in _ints(cone, "sl_n")]
    blocks, at = [], prefix
    for ln in lens:
        if ln > 0:
            blocks.append((at, ln))
        at += ln
    return prefix, blocks


def table_rows(table):
    prefix, blocks = table
    return prefix + sum(ln for _, ln in blocks)


class _Lines(object):
    """segmented reductions of values over `nlines` lines; `line[k]` is the line of the k-th contribution and `src[k]` the position
    of its value"""

    def __init__(self, line, src, nlines):
        order = np.argsort(line, kind="stable")
        self.src = np.asarray(src)[order]
        counts = np.bincount(line, minlength=nlines)
        self.nonempty = counts > 0
        self.starts = (np.cumsum(counts) - counts)[self.nonempty]
        self.nlines = nlines

    def reduce(self, ufunc, vals):
        out = np.zeros(self.nlines, dtype=vals.dtype)
        if self.starts.size:
            out[self.nonempty] = ufunc.reduceat(vals[self.src], self.starts)
        return out


def _limit(x):
    x = np.where(x < LO, x.dtype.type(1.0), x)
    return np.where(x > HI, x.dtype.type(HI), x)


def _margin(x):
    """smallest |x/t - 1| over the nonzero entries of x, t in {1e-4, 1e4}"""
    x = np.asarray(x, dtype=np.longdouble).ravel()
    x = x[x != 0]
    if x.size == 0:
        return np.inf
    return float(min(np.abs(x / np.longdouble(LO) - 1).min(), np.abs(x / np.longdouble(HI) - 1).min()))


def equilibrate(A, P_upper, b, c, cone, dtype=np.float64):
    """A: scipy CSC (m x n), P_upper: scipy CSC holding the upper triangle of P (or None), cone: dict.  Returns `Equilibrated`.

    clamp_margin is the smallest |x/t - 1| over every nonzero norm that enters the limit in any pass (sigma's included), t in
    {1e-4, 1e4}: the limit jumps at t, so a comparison of two implementations means something only when this is well above their
    rounding differences."""
    m, n = A.shape
    table = block_table(cone)
    prefix, blocks = table
    if table_rows(table) != m:
        raise ValueError("the cone has %d rows, A has %d" % (table_rows(table), m))
    one = dtype(1.0)
    ai = np.asarray(A.indices, dtype=np.int64)
    aj = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr))
    av = np.asarray(A.data, dtype=dtype).copy()
    rows_of_a = _Lines(ai, np.arange(ai.size), m)
    cols_of_a = _Lines(aj, np.arange(aj.size), n)
    pv = None
    if P_upper is not None:
        pi = np.asarray(P_upper.indices, dtype=np.int64)
        pj = np.repeat(np.arange(n, dtype=np.int64), np.diff(P_upper.indptr))
        if (pi > pj).any():
            raise ValueError("P_upper holds entries below the diagonal")
        pv = np.asarray(P_upper.data, dtype=dtype).copy()
        off = np.flatnonzero(pi != pj)  # (i, j) with i < j also stands in line i of the full matrix
        lines_of_p = _Lines(np.concatenate([pj, pi[off]]), np.concatenate([np.arange(pj.size), off]), n)
    D, E = np.ones(m, dtype=dtype), np.ones(n, dtype=dtype)
    margin, passes = np.inf, []
    for p in range(RUIZ_PASSES + L2_PASSES):
        l2 = p >= RUIZ_PASSES
        if l2:
            sq = av * av
            dn = np.sqrt(rows_of_a.reduce(np.add, sq))
            en = cols_of_a.reduce(np.add, sq)
            if pv is not None:
                en = en + lines_of_p.reduce(np.add, pv * pv)
            en = np.sqrt(en)
        else:
            mag = np.abs(av)
            dn = rows_of_a.reduce(np.maximum, mag)
            en = cols_of_a.reduce(np.maximum, mag)
            if pv is not None:
                en = np.maximum(en, lines_of_p.reduce(np.maximum, np.abs(pv)))
        for at, ln in blocks:
            seg = dn[at:at + ln]
            dn[at:at + ln] = seg.sum() / dtype(ln) if l2 else seg.max()
        margin = min(margin, _margin(dn), _margin(en))
        dt, et = one / np.sqrt(_limit(dn)), one / np.sqrt(_limit(en))
        av *= dt[ai] * et[aj]
        if pv is not None:
            pv *= et[pi] * et[pj]
        D *= dt
        E *= et
        passes.append((dn, en, dt, et))
    bh, ch = D * np.asarray(b, dtype=dtype), E * np.asarray(c, dtype=dtype)
    nrm = max(np.abs(bh).max() if m else dtype(0), np.abs(ch).max() if n else dtype(0))
    margin = min(margin, _margin([nrm]))
    sigma = one / _limit(np.asarray([nrm], dtype=dtype))[0]
    return Equilibrated(av, pv, sigma * bh, sigma * ch, D, E, sigma, table, margin, passes)
