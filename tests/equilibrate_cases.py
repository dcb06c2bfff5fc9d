"""The edge cases of the equilibration tests (test_equilibrate_ref_cpu.py, test_equilibrate_gpu.py): one generator, fixed seeds.

A case is a random sparse A (and P) in which listed rows and columns are scaled by 1e-7 (`tiny`: a norm below the lower clamp, so the
factor is 1), scaled by 1e7 (`huge`: clamped at 1e4 for several passes), emptied, or made dense.  `case(name)` returns a dict with A, P
(upper triangle), b, c, cone, rows (the row count written out by hand, for the check of the block table) and spectral."""
import functools

import numpy as np
from scipy import sparse

TINY, HUGE = 1e-7, 1e7

# three bounds: the box takes 4 rows (t and one per bound), so the separable prefix is 3 + 40 + 4 = 47 rows
_KITCHEN = {"z": 3, "l": 40, "bu": [1.0, 2.0, 0.5], "bl": [-1.0, 0.0, -0.5], "q": [1, 7, 64, 1, 65, 129], "s": [1, 12, 3],
            "cs": [1, 3], "ep": 2, "ed": 1, "p": [0.3, -0.6]}
_Q0 = 47                     # first row of the q cones
_Q7 = _Q0 + 1                # the 7-cone
_Q129 = _Q0 + 1 + 7 + 64 + 1 + 65  # the 129-cone
_Q2100 = _Q129 + 129         # the 2100-cone of `long` (appended to q, so it sits behind the 129-cone)
_KITCHEN_ROWS = 47 + 267 + (1 + 78 + 6) + (1 + 9) + 3 * 5  # 424
# the lines the kitchen-sink cone marks; `long` keeps them
_KITCHEN_MARKS = dict(tiny_rows=[5, _Q7 + 1, _Q129 + 5], huge_rows=[10, 45, _Q7 + 2, _Q129 + 15], empty_rows=[20, _Q7 + 3, _Q129 + 65],
                      tiny_cols=[12, 50], huge_cols=[25], empty_cols=[7, 33])

_SPECTRAL = {"l": 2, "q": [3], "d": [1, 5], "nuc_m": [3, 70], "nuc_n": [2, 1], "ell1": [1, 100], "sl_n": [4, 11], "sl_k": [2, 3]}
_SPECTRAL_ROWS = 2 + 3 + (3 + 17) + (7 + 71) + (2 + 101) + (11 + 67)  # 284
_ELL1_100 = 2 + 3 + 3 + 17 + 7 + 71 + 2  # first row of the 101-row ell1 block

NAMES = ("kitchen", "long", "thin", "no_prefix", "many_blocks", "tiny_dense", "tiny_zero", "spectral")


def _random_A(m, n, rng, density=None, per_col=None):
    if density is not None:
        A = sparse.rand(m, n, density, format="csc", random_state=rng)
        A.data = rng.randn(A.nnz)
        return A
    rows = rng.randint(0, m, size=(n, per_col))
    cols = np.repeat(np.arange(n), per_col)
    A = sparse.csc_matrix((rng.randn(n * per_col), (rows.ravel(), cols)), shape=(m, n))  # (duplicates are summed)
    return A


def _random_P(n, rng, density):
    B = sparse.rand(n, n, density, format="csc", random_state=rng)
    B.data = rng.randn(B.nnz)
    return (B.T @ B + sparse.eye(n)).tocsc()


def _scale_lines(M, rows, cols):
    return (sparse.diags(rows) @ M @ sparse.diags(cols)).tocsc()


def _finish(M):
    M = M.tocsc()
    M.eliminate_zeros()
    M.sum_duplicates()
    M.sort_indices()
    return M


def _build(cone, rows, n, seed, density=None, per_col=None, p_density=0.05, tiny_rows=(), huge_rows=(), empty_rows=(), dense_rows=(),
           tiny_cols=(), huge_cols=(), empty_cols=(), dense_cols=(), p_dense_line=None, spectral=False):
    rng = np.random.RandomState(seed)
    m = rows
    A = _random_A(m, n, rng, density, per_col).tolil()
    for r in dense_rows:
        A[r, :] = rng.randn(n)
    for j in dense_cols:
        A[:, j] = rng.randn(m, 1)
    rs, cs = np.ones(m), np.ones(n)
    rs[list(tiny_rows)], rs[list(huge_rows)], rs[list(empty_rows)] = TINY, HUGE, 0.0
    cs[list(tiny_cols)], cs[list(huge_cols)], cs[list(empty_cols)] = TINY, HUGE, 0.0
    A = _finish(_scale_lines(A.tocsc(), rs, cs))
    P = _random_P(n, rng, p_density).tolil()
    if p_dense_line is not None:
        v = rng.randn(n)
        P[p_dense_line, :] = v
        P[:, p_dense_line] = v.reshape(n, 1)
    # the tiny and the empty columns of A have no entry in P either: their norm is tiny / zero with P as well
    ps = np.ones(n)
    ps[list(tiny_cols) + list(empty_cols)] = 0.0
    P = _finish(sparse.triu(_scale_lines(P.tocsc(), ps, ps)))
    b, c = rng.randn(m), rng.randn(n)
    b[::7] = 0.0  # exact zeros stay zero
    c[::5] = 0.0
    return dict(A=A, P=P, b=b, c=c, cone=cone, rows=rows, spectral=spectral)


def _thin(seed):
    """l 3000, n = 40, one or two nonzeros per row: 1024 rows hold fewer than 2048 nonzeros, so the row cap ends the row blocks"""
    rng = np.random.RandomState(seed)
    m, n = 3000, 40
    cnt = rng.randint(1, 3, size=m)
    rows = np.repeat(np.arange(m), cnt)
    cols = np.concatenate([rng.choice(n, size=k, replace=False) for k in cnt])
    A = _finish(sparse.csc_matrix((rng.randn(rows.size), (rows, cols)), shape=(m, n)))
    P = _finish(sparse.triu(_random_P(n, rng, 0.05)))
    b, c = rng.randn(m), rng.randn(n)
    b[::7] = 0.0
    return dict(A=A, P=P, b=b, c=c, cone={"l": m}, rows=m, spectral=False)


def _tiny_zero():
    """l 4, n = 3, no nonzero anywhere: every norm is zero, D = E = 1 exactly and sigma = 1"""
    m, n = 4, 3
    return dict(A=sparse.csc_matrix((m, n)), P=sparse.csc_matrix((n, n)), b=np.zeros(m), c=np.zeros(n), cone={"l": m}, rows=m,
                spectral=False)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "kitchen":
        return _build(_KITCHEN, _KITCHEN_ROWS, 60, 101, density=0.15, **_KITCHEN_MARKS)
    if name == "long":
        cone = dict(_KITCHEN, q=_KITCHEN["q"] + [2100])
        marks = dict(_KITCHEN_MARKS, dense_rows=[8, _Q2100 + 1000], dense_cols=[100], p_dense_line=200)
        return _build(cone, _KITCHEN_ROWS + 2100, 2500, 102, per_col=4, p_density=0.001, **marks)
    if name == "thin":
        return _thin(103)
    if name == "no_prefix":
        return _build({"q": [2100]}, 2100, 40, 104, density=0.1, empty_rows=[0])
    if name == "many_blocks":
        return _build({"q": [3] * 300, "ep": 50}, 900 + 150, 30, 105, density=0.15)
    if name == "tiny_dense":
        return _build({"l": 5}, 5, 3, 106, density=1.0, p_density=1.0)
    if name == "tiny_zero":
        return _tiny_zero()
    if name == "spectral":
        return _build(_SPECTRAL, _SPECTRAL_ROWS, 40, 107, density=0.15, huge_rows=[_ELL1_100 + 40], spectral=True)
    raise KeyError(name)
