"""The pack and sum kernels of the shared matrix gradient (csrc/grad_shared.hpp) through the one-shot entry `_scs_hip.grad_matrix_sum`,
on random stacks:
    dA[p] = sum_k ( Y[k,i] DC[k,j] - DB[k,i] X[k,j] )                                p = stored entry (i, j) of A
    dP[q] = sum_k ( DC[k,c] X[k,r] + DC[k,r] X[k,c] )  (c < r),   sum_k DC[k,r] X[k,r]  on the diagonal

Reference, per entry: math.fsum of the 2K float products (K on the diagonal of P) — exact but for the products' own rounding.
Bound, per entry: (2K + 2) 2^-52 sum|products| — the first-order bound of a sum of 2K terms in ANY order (2K - 1 additions of relative
error 2^-53 each) plus one rounding per product (the device may contract a product into an fma or not; the reference rounds it), doubled.
It is derived, not measured, and scales with sum|products|, so it also holds where the members cancel."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from scs import _scs_hip

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
KC = 256  # csrc/grad_shared.hpp kGradSumKc: members per chunk; a lane holds members l, l + 64, ... of a chunk (the wave: 64)
K_VALUES = [1, 2, 3, 63, 64, 65, KC - 1, KC, KC + 1, 2 * KC + 1]


def pattern_a(rng, m=37, n=23, density=0.3):
    """about 30 % dense, with an empty first column, an empty last column, an empty row, one full column and one single-entry column"""
    mask = rng.random((m, n)) < density
    mask[:, 0] = False
    mask[:, n - 1] = False
    mask[:, 5] = True
    mask[:, 9] = False
    mask[11, 9] = True
    mask[7, :] = False  # (after the full column: row 7 is empty everywhere)
    A = sp.csc_matrix(mask.astype(np.float64))
    A.sort_indices()
    assert A.indptr[1] == 0 and A.indptr[n] == A.indptr[n - 1] and A.indptr[6] - A.indptr[5] == m - 1 and A.indptr[10] - A.indptr[9] == 1
    return A


def pattern_p_diag(n):
    return sp.identity(n, format="csc")


def pattern_p_tri(rng, n):
    """an upper triangle with off-diagonal entries and one missing diagonal entry"""
    mask = np.triu(rng.random((n, n)) < 0.3, 1) | np.eye(n, dtype=bool)
    mask[n // 2, n // 2] = False
    if n > 1:
        mask[0, n - 1] = True
    P = sp.csc_matrix(mask.astype(np.float64))
    P.sort_indices()
    return P


def stacks(rng, K, m, n, kind):
    X, Y = rng.standard_normal((K, n)), rng.standard_normal((K, m))
    DB, DC = rng.standard_normal((K, m)), rng.standard_normal((K, n))
    if kind == "zeros":  # several members whose DB, DC rows are exactly zero
        for k in range(0, K, 3):
            DB[k] = 0.0
            DC[k] = 0.0
    if kind == "cancel":  # one pair of members that cancel exactly: the same solution, negated db and dc
        a, b = 0, K - 1
        X[b], Y[b], DB[b], DC[b] = X[a], Y[a], -DB[a], -DC[a]
    return X, Y, DB, DC


def fsum_rows(prods):
    """per entry: (the exact sum of its products, sum|products|); prods: (terms, entries)"""
    cols = np.ascontiguousarray(prods.T)
    return np.array([math.fsum(r) for r in cols]), np.abs(cols).sum(axis=1)


def reference(A, P, X, Y, DB, DC):
    """((dA, its bound), (dP, its bound) or None)"""
    K, n = X.shape
    rows, cols = A.indices, np.repeat(np.arange(n), np.diff(A.indptr))
    ref_a, mag_a = fsum_rows(np.concatenate([Y[:, rows] * DC[:, cols], -(DB[:, rows] * X[:, cols])], axis=0))
    out_a = (ref_a, (2 * K + 2) * EPS * mag_a)
    if P is None:
        return out_a, None
    c, r = P.indices, np.repeat(np.arange(n), np.diff(P.indptr))
    assert (c <= r).all()
    first, second = DC[:, c] * X[:, r], np.where(c < r, DC[:, r] * X[:, c], 0.0)  # (a diagonal entry: K products, the others are no terms)
    ref_p, mag_p = fsum_rows(np.concatenate([first, second], axis=0))
    return out_a, (ref_p, (2 * K + 2) * EPS * mag_p)


def check(A, P, X, Y, DB, DC):
    dA, dP = _scs_hip.grad_matrix_sum(A, P, X, Y, DB, DC)
    again = _scs_hip.grad_matrix_sum(A, P, X, Y, DB, DC)
    assert np.array_equal(dA, again[0])  # two calls: equal bits
    (ref_a, bound_a), p_side = reference(A, P, X, Y, DB, DC)
    assert dA.shape == ref_a.shape
    err = np.abs(dA - ref_a)
    assert (err <= bound_a).all(), (float((err / np.maximum(bound_a, 1e-300)).max()), int(np.argmax(err - bound_a)))
    if P is None:
        assert dP is None and again[1] is None
        return
    assert np.array_equal(dP, again[1])
    ref_p, bound_p = p_side
    assert dP.shape == ref_p.shape
    err = np.abs(dP - ref_p)
    assert (err <= bound_p).all(), (float((err / np.maximum(bound_p, 1e-300)).max()), int(np.argmax(err - bound_p)))


@pytest.mark.parametrize("K", K_VALUES)
def test_sums_match_the_exact_reference(K):
    rng = np.random.default_rng(4200 + K)
    A = pattern_a(rng)
    m, n = A.shape
    kinds = ["normal"] + (["zeros"] if K >= 3 else []) + (["cancel"] if K >= 2 else [])
    for kind in kinds:
        st = stacks(rng, K, m, n, kind)
        for P in (pattern_p_tri(rng, n), pattern_p_diag(n), None):
            check(A, P, *st)
    # one column
    A1 = sp.csc_matrix((np.ones(3), np.array([0, 2, 4]), np.array([0, 3])), shape=(5, 1))
    for kind in kinds:
        st = stacks(rng, K, 5, 1, kind)
        check(A1, pattern_p_diag(1), *st)
        check(A1, None, *st)


@pytest.mark.parametrize("K", [1, KC + 1])
def test_a_pattern_without_an_entry(K):
    rng = np.random.default_rng(7)
    m, n = 4, 3
    A = sp.csc_matrix((m, n))
    X, Y, DB, DC = stacks(rng, K, m, n, "normal")
    dA, dP = _scs_hip.grad_matrix_sum(A, None, X, Y, DB, DC)
    assert dA.shape == (0,) and dP is None
    dA, dP = _scs_hip.grad_matrix_sum(A, sp.csc_matrix((n, n)), X, Y, DB, DC)
    assert dA.shape == (0,) and dP.shape == (0,)
    check(A, pattern_p_diag(n), X, Y, DB, DC)  # an empty A beside a P with entries


def test_exact_cancellation_leaves_what_the_bound_allows():
    """two members only, which cancel: the exact sum is 0 and the bound, which scales with sum|products|, is not"""
    rng = np.random.default_rng(11)
    A = pattern_a(rng)
    m, n = A.shape
    X, Y, DB, DC = stacks(rng, 2, m, n, "cancel")
    (ref_a, bound_a), _ = reference(A, None, X, Y, DB, DC)
    assert not ref_a.any() and (bound_a > 0).all()
    check(A, pattern_p_tri(rng, n), X, Y, DB, DC)


def test_a_larger_pattern_over_several_blocks():
    rng = np.random.default_rng(12)
    m, n, K = 3000, 2000, 130
    A = sp.random(m, n, density=2e4 / (m * n), format="csc", random_state=np.random.RandomState(5))
    A.sort_indices()
    P = sp.triu(sp.random(n, n, density=4e3 / (n * n), format="csc", random_state=np.random.RandomState(6)) + sp.identity(n), format="csc")
    P.sort_indices()
    check(A, P, *stacks(rng, K, m, n, "normal"))


def test_a_chunk_lowered_to_the_panel_cap():
    """2 (n + m) doubles per member at 256 members exceed the 256 MiB of panels: the chunk drops to a whole wave, 64, and K = 70 takes
    two chunks of other sizes than KC"""
    rng = np.random.default_rng(13)
    m, n, K = 140000, 2, 70
    assert 2 * (n + m) * 8 * KC > 256 << 20 and 2 * (n + m) * 8 * 64 <= 256 << 20 < 2 * (n + m) * 8 * 128
    rows = np.sort(rng.choice(m, size=40, replace=False))
    A = sp.csc_matrix((np.ones(40), rows, np.array([0, 25, 40])), shape=(m, n))
    X, DC = rng.standard_normal((K, n)), rng.standard_normal((K, n))
    Y, DB = np.zeros((K, m)), np.zeros((K, m))
    Y[:, rows], DB[:, rows] = rng.standard_normal((K, 40)), rng.standard_normal((K, 40))
    check(A, pattern_p_tri(rng, n), X, Y, DB, DC)


def test_refused_arguments():
    A = sp.csc_matrix(np.ones((3, 2)))
    with pytest.raises(ValueError, match="X must be"):
        _scs_hip.grad_matrix_sum(A, None, np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 2)))
    bad = sp.csc_matrix(np.ones((3, 2)))
    bad.indices = bad.indices.copy()
    bad.indices[0] = 7
    with pytest.raises(RuntimeError, match="row index out of range"):
        _scs_hip.grad_matrix_sum(bad, None, np.zeros((1, 2)), np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 2)))
