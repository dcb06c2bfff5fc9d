"""dA / dP of SCS.derivative, derivative_device, derivative_many[_device], derivative_batch[_device] and data_perturbation: the
pure-Python argument checks (scs._scs_hip._diff_mat, _diff_vec, _many_diff_args, _device_vec), which run before the library is called
and need no GPU; and the new symbols in the header and the library."""
import inspect
import os
import re

import numpy as np
import pytest

import scs
from scs import _scs_hip, _scs_hip_dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNZ_A, NNZ_P = 5, 4


def shell(m=4, n=3, with_P=True):
    """a raw solver object whose workspace handle is never handed to the library: every call below must fail in Python first"""
    sv = object.__new__(_scs_hip.SCS)
    sv._blank()
    sv._shape(m, n)
    sv._work = 1
    pa = (np.array([0, 2, 3, 5], dtype=np.int32), np.array([0, 2, 1, 0, 3], dtype=np.int32))
    pp = (np.array([0, 1, 2, 4], dtype=np.int32), np.array([0, 1, 0, 2], dtype=np.int32))
    sv._pattern = {"A": pa, "P": pp if with_P else None}
    return sv


def forget(*svs):
    for sv in svs:
        sv._work = None  # (the destructor must not finish a handle that is none)


def test_the_keywords_come_after_the_existing_arguments():
    for cls in (scs.SCS, _scs_hip.SCS, _scs_hip_dense.SCS):
        for name in ("derivative", "derivative_device", "derivative_many", "derivative_many_device"):
            assert list(inspect.signature(getattr(cls, name)).parameters)[1:] == ["db", "dc", "tol", "max_iters", "dA", "dP"], (cls, name)
    for mod in (scs, _scs_hip, _scs_hip_dense):
        for name in ("derivative_batch", "derivative_batch_device"):
            assert list(inspect.signature(getattr(mod, name)).parameters) == ["solvers", "db", "dc", "tol", "max_iters", "dA", "dP"], (mod, name)
    assert callable(_scs_hip.data_perturbation) and callable(_scs_hip.SCS.data_perturbation_device)


def test_wrong_length_dtype_and_kind():
    sv = shell()
    try:
        for call in (sv.derivative, sv.data_perturbation):
            with pytest.raises(ValueError, match="dA has incompatible dimension with A"):
                call(dA=np.zeros(NNZ_A + 1))
            with pytest.raises(ValueError, match="dP has incompatible dimension with A"):
                call(dP=np.zeros(NNZ_P - 1))
            with pytest.raises(TypeError, match="dA must be a 1-D numpy array of floats"):
                call(dA=np.zeros(NNZ_A, dtype=np.int64))
            with pytest.raises(TypeError, match="dP must be a 1-D numpy array of floats"):
                call(dP=[0.0] * NNZ_P)
            with pytest.raises(TypeError, match="dA must be a 1-D numpy array of floats"):
                call(dA=np.zeros((NNZ_A, 1)))
        # a (data, indices, indptr) triple must carry the constructor's pattern
        ip, ind = sv._pattern["A"]
        with pytest.raises(ValueError, match="dA: sparsity pattern differs"):
            sv.derivative(dA=(np.zeros(NNZ_A), ind[::-1].copy(), ip))
        with pytest.raises(ValueError, match="dA has 4 values, the solver's pattern has 5"):
            sv.derivative(dA=(np.zeros(4), ind, ip))
    finally:
        forget(sv)
    good = _scs_hip._diff_mat("dA", np.arange(2 * NNZ_A, dtype=np.float32)[::2], (ip, ind))
    assert good.dtype == np.float64 and good.flags["C_CONTIGUOUS"]
    assert _scs_hip._diff_mat("dP", None, None) is None


def test_dP_without_P():
    sv = shell(with_P=False)
    other = shell(with_P=True)
    try:
        for call in (sv.derivative, sv.derivative_device, sv.data_perturbation, sv.data_perturbation_device):
            with pytest.raises(ValueError, match="dP given, but the solver was created without P"):
                call(dP=np.zeros(NNZ_P))
        for call in (sv.derivative_many, sv.derivative_many_device):
            with pytest.raises(ValueError, match="dP given, but the solver was created without P"):
                call(dP=np.zeros((2, NNZ_P)))
        with pytest.raises(ValueError, match="dP given, but the solver was created without P"):
            _scs_hip.derivative_batch([other, sv], dP=[np.zeros(NNZ_P), np.zeros(NNZ_P)])
        with pytest.raises(ValueError, match="created without P"):
            _scs_hip._diff_mat("dP", np.zeros(NNZ_P), None)
    finally:
        forget(sv, other)


def test_rows_of_a_batch():
    sv, tw = shell(), shell()
    try:
        with pytest.raises(ValueError, match="dA holds 3 rows for 2 problems"):
            sv.derivative_many(db=np.zeros((2, 4)), dA=np.zeros((3, NNZ_A)))
        with pytest.raises(ValueError, match="dP holds 1 rows for 2 problems"):
            _scs_hip.derivative_batch([sv, tw], dP=np.zeros((1, NNZ_P)))
        with pytest.raises(ValueError, match=r"dA\[1\] has incompatible dimension with A"):
            _scs_hip.derivative_batch([sv, tw], dA=[np.zeros(NNZ_A), np.zeros(NNZ_A + 2)])
        with pytest.raises(ValueError, match="dA must be C-contiguous"):
            sv.derivative_many(dA=np.zeros((NNZ_A, 2)).T)
        with pytest.raises(ValueError, match=r"dP\[0\] must be contiguous"):
            _scs_hip.derivative_batch([sv, tw], dP=[np.zeros(2 * NNZ_P)[::2], None])
        with pytest.raises(TypeError, match="dA must be a 2-D numpy array of floats"):
            sv.derivative_many(dA=np.zeros((2, NNZ_A), dtype=np.int32))
        with pytest.raises(ValueError, match="dA must be 2-D, one row per problem"):
            sv.derivative_many(dA=np.zeros(NNZ_A))
        with pytest.raises(ValueError, match="rows, but solve_many has solved 1 member"):
            sv.derivative_many(dA=np.zeros((2, NNZ_A)))  # (the rows are fine: K members must exist)
    finally:
        forget(sv, tw)


def test_device_arguments():
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="dA must be a float64 tensor"):
        _scs_hip._device_vec("dA", torch.zeros(NNZ_A, dtype=torch.float32), NNZ_A, 0)
    with pytest.raises(ValueError, match="dP must be a 1-D tensor of length 4"):
        _scs_hip._device_vec("dP", torch.zeros(NNZ_P + 1, dtype=torch.float64), NNZ_P, 0)
    with pytest.raises(ValueError, match="dA must be contiguous"):
        _scs_hip._device_vec("dA", torch.zeros(2 * NNZ_A, dtype=torch.float64)[::2], NNZ_A, 0)
    with pytest.raises(ValueError, match="dA must live on the workspace's GPU"):
        _scs_hip._device_vec("dA", torch.zeros(NNZ_A, dtype=torch.float64), NNZ_A, 0)
    with pytest.raises(ValueError, match=r"dA\[0\] must be contiguous"):
        _scs_hip._many_diff_args((("dA", torch.zeros((2, 2 * NNZ_A), dtype=torch.float64)[:, ::2], NNZ_A),), None, device=0)
    with pytest.raises(TypeError, match="dA must be a 2-D torch.Tensor"):
        _scs_hip._many_diff_args((("dA", np.zeros(NNZ_A), NNZ_A),), None, device=0)


def test_the_front_end_takes_a_sparse_matrix_of_the_constructor_s_pattern():
    from scipy import sparse
    A = sparse.csc_matrix(np.array([[1.0, 0.0, 2.0], [0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.0, 0.0, 5.0]]))
    sv = shell()
    front = object.__new__(scs.SCS)
    front._settings = {}
    front._solver = sv
    try:
        sv._pattern["A"] = (A.indptr.astype(np.int32), A.indices.astype(np.int32))
        with pytest.raises(ValueError, match="dA: sparsity pattern differs"):
            front.derivative(dA=sparse.csc_matrix(np.eye(4, 3)))
        low = sparse.csc_matrix(np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [3.0, 0.0, 4.0]]))
        with pytest.raises(ValueError, match="dP: sparsity pattern differs"):
            front.derivative(dP=low)  # (its upper triangle has three entries, the pattern's has four)
        with pytest.raises(ValueError, match="dA has incompatible dimension with A"):
            front.derivative(dA=np.zeros(9))
    finally:
        forget(sv)


def test_symbols_are_declared_and_defined():
    header = open(os.path.join(ROOT, "include", "scs_hip.h")).read()
    names = ("scs_hip_derivative_full", "scs_hip_derivative_full_device", "scs_hip_derivative_full_batch", "scs_hip_derivative_full_batch_device",
             "scs_hip_data_perturbation", "scs_hip_data_perturbation_device")
    for name in names:
        assert re.search(r"SCS_HIP_API\s+scs_int\s+%s\s*\(" % name, header), name
    lib = _scs_hip._lib
    # a NULL workspace is refused with a reason (no device needed)
    assert lib.scs_hip_derivative_full(None, None, None, None, None, None, None, None, None, None) == -1
    assert "scs_hip_derivative_full: null workspace" in _scs_hip.last_error()
    assert lib.scs_hip_data_perturbation_device(None, None, None, None, None) == -1
    assert "scs_hip_data_perturbation_device: null workspace" in _scs_hip.last_error()
    assert lib.scs_hip_derivative_full_batch(None, None, None, None, None, None, None, None, None, None, 0) == -1
    assert "count must be positive" in _scs_hip.last_error()
