"""SCS.update_matrix: the pure-Python argument check (scs._scs_hip._matrix_values, scs._update_arg) — pattern, length, dtype, explicit
zeros, None — which runs before the library is called and needs no GPU; and the new symbols in the header and the export list."""
import os
import re
import warnings

import numpy as np
import pytest
from scipy import sparse

import scs
from scs import _scs_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pattern_of(M):
    return (M.indptr.astype(np.int32), M.indices.astype(np.int32))


def example():
    A = sparse.csc_matrix(np.array([[1.0, 0.0, 2.0], [0.0, 3.0, 0.0], [4.0, 0.0, 5.0], [0.0, 6.0, 7.0]]))
    return A, pattern_of(A)


def test_values_alone_are_checked_for_length_and_type():
    A, pat = example()
    out = _scs_hip._matrix_values("A", A.data * 2, pat)
    assert out.dtype == np.float64 and np.array_equal(out, A.data * 2) and out is not A.data
    with pytest.raises(ValueError, match="A has 6 values, the solver's pattern has 7"):
        _scs_hip._matrix_values("A", A.data[:-1], pat)
    with pytest.raises(TypeError, match="1-D"):
        _scs_hip._matrix_values("A", np.zeros((7, 1)), pat)
    with pytest.raises(TypeError, match="not list"):
        _scs_hip._matrix_values("A", [0.0] * 7, pat)
    with pytest.raises(TypeError, match="floats"):
        _scs_hip._matrix_values("A", np.array(["a"] * 7), pat)


def test_dtype_is_coerced_to_float64():
    A, pat = example()
    for dt in (np.float32, np.int64):
        out = _scs_hip._matrix_values("A", np.arange(7).astype(dt), pat)
        assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, np.arange(7.0))
    out = _scs_hip._matrix_values("A", np.arange(14.0)[::2], pat)  # a strided view
    assert out.flags["C_CONTIGUOUS"] and np.array_equal(out, np.arange(14.0)[::2])


def test_a_sparse_matrix_must_keep_the_pattern():
    A, pat = example()
    same = _scs_hip._matrix_values("A", scs._update_arg(A * 3.0, "A", False), pat)
    assert np.array_equal(same, A.data * 3.0)
    moved = A.tolil()
    moved[1, 0] = 9.0
    with pytest.raises(ValueError, match="A: sparsity pattern differs"):
        _scs_hip._matrix_values("A", scs._update_arg(moved.tocsc(), "A", False), pat)
    lost = A.copy()
    lost.data[2] = 0.0
    lost.eliminate_zeros()
    with pytest.raises(ValueError, match="sparsity pattern differs"):
        _scs_hip._matrix_values("A", scs._update_arg(lost, "A", False), pat)
    with pytest.raises(ValueError, match="sparsity pattern differs"):  # same count, another place
        swapped = sparse.csc_matrix((A.data, A.indices[::-1].copy(), A.indptr), shape=A.shape)
        _scs_hip._matrix_values("A", (swapped.data, swapped.indices, swapped.indptr), pat)


def test_explicit_zeros_are_values():
    A, pat = example()
    Z = A.copy()
    Z.data[3] = 0.0  # stays stored
    out = _scs_hip._matrix_values("A", scs._update_arg(Z, "A", False), pat)
    assert out[3] == 0.0 and out.shape[0] == A.nnz


def test_canonical_form_is_the_constructors():
    A, pat = example()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        data, indices, indptr = scs._update_arg(A.tocsr(), "A", False)  # another format: converted, as by the constructor
    assert np.array_equal(indptr, pat[0]) and np.array_equal(indices, pat[1]) and np.array_equal(data, A.data)
    rev = np.concatenate([np.arange(A.indptr[j], A.indptr[j + 1])[::-1] for j in range(A.shape[1])])  # every column back to front
    unsorted = sparse.csc_matrix((A.data[rev], A.indices[rev], A.indptr), shape=A.shape)
    unsorted.has_sorted_indices = False
    kept = unsorted.indices.copy()
    d2, i2, p2 = scs._update_arg(unsorted, "A", False)
    assert np.array_equal(i2, pat[1]) and np.array_equal(d2, A.data) and np.array_equal(p2, pat[0])
    assert np.array_equal(unsorted.indices, kept)  # sorted in a copy: the caller's object is not touched
    P = sparse.csc_matrix(np.array([[2.0, 0.5, 0.0], [0.5, 1.0, -0.25], [0.0, -0.25, 3.0]]))
    U = sparse.triu(P, format="csc")
    pd, pi, pp = scs._update_arg(P, "P", True)  # the full symmetric matrix: its upper triangle, as in the constructor
    assert np.array_equal(pi, U.indices) and np.array_equal(pp, U.indptr) and np.array_equal(pd, U.data)
    assert np.array_equal(_scs_hip._matrix_values("P", (pd, pi, pp), pattern_of(U)), U.data)


def test_none_and_missing_P():
    assert scs._update_arg(None, "A", False) is None
    arr = np.zeros(3)
    assert scs._update_arg(arr, "P", True) is arr  # values alone pass through
    with pytest.raises(ValueError, match="P given, but the solver was created without P"):
        _scs_hip._matrix_values("P", np.zeros(3), None)


def test_methods_exist_on_every_front_end():
    from scs import _scs_hip_dense
    for cls in (scs.SCS, _scs_hip.SCS, _scs_hip_dense.SCS):
        assert callable(getattr(cls, "update_matrix")) and callable(getattr(cls, "update_matrix_device"))


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "scs_hip.h")).read()
    for name in ("scs_hip_update_matrix", "scs_hip_update_matrix_device"):
        assert re.search(r"SCS_HIP_API\s+scs_int\s+%s\s*\(" % name, header), name
    # csrc/exports.map lists what the library exports by pattern: the new names must fall under it and be defined in the library
    exports = open(os.path.join(ROOT, "scs-python_amd", "csrc", "exports.map")).read()
    assert "scs_*" in exports
    lib = _scs_hip._lib
    assert lib.scs_hip_update_matrix and lib.scs_hip_update_matrix_device
    assert lib.scs_hip_update_matrix(None, None, None) == -1  # a NULL workspace is refused with a reason (no device needed)
    assert "null workspace" in _scs_hip.last_error()
