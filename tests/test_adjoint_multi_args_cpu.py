"""The Python surface of the multi derivatives (K directions at one solution) and its argument checks (scs/_scs_hip.py
`_multi_diff_args`): pure Python, no GPU."""
import numpy as np
import pytest

import scs
from scs import _scs_hip, _scs_hip_dense

METHOD_NAMES = ("adjoint_multi", "adjoint_multi_device", "derivative_multi", "derivative_multi_device", "jacobian", "jacobian_device")
M, N, K = 7, 4, 5


def test_the_new_names_exist():
    for cls in (scs.SCS, _scs_hip.SCS, _scs_hip_dense.SCS):
        for name in METHOD_NAMES:
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(_scs_hip._multi_diff_args)
    assert _scs_hip.MULTI_MAX == 32
    assert _scs_hip._ADJOINT_MULTI.entry == "scs_hip_adjoint_multi" and _scs_hip._DERIVATIVE_MULTI.entry == "scs_hip_derivative_multi"
    assert [name for name, _ in _scs_hip._DERIVATIVE_MULTI.ins] == ["db", "dc"]  # (no dA / dP perturbations in derivative_multi)


def test_the_library_exports_the_entries():
    for name in ("scs_hip_adjoint_multi", "scs_hip_adjoint_multi_device", "scs_hip_derivative_multi", "scs_hip_derivative_multi_device"):
        assert hasattr(_scs_hip._lib, name), name


def spec(dx=None, dy=None, ds=None, n=N, m=M):
    return (("dx", dx, n), ("dy", dy, m), ("ds", ds, m))


def test_good_arguments_pass_and_K_is_read_from_them():
    k, got = _scs_hip._multi_diff_args(spec(np.ones((K, N)), None, np.zeros((K, M), dtype=np.float32)))
    assert k == K and got[1] is None
    assert got[0].shape == (K, N) and got[2].shape == (K, M)
    assert all(g.dtype == np.float64 and g.flags["C_CONTIGUOUS"] for g in (got[0], got[2]))
    # a transposed view is taken as a fresh C-contiguous copy: row k is direction k
    src = np.arange(K * N, dtype=np.float64).reshape(N, K)
    k, got = _scs_hip._multi_diff_args(spec(src.T))
    assert k == K and got[0].flags["C_CONTIGUOUS"] and np.array_equal(got[0], src.T)
    k, got = _scs_hip._multi_diff_args(spec(None, np.ones((40, M))))
    assert k == 40  # (the C limit is not a Python limit)


def test_all_inputs_None_is_refused():
    with pytest.raises(ValueError, match="no direction given: dx, dy, ds are all None"):
        _scs_hip._multi_diff_args(spec())


def test_a_disagreeing_K_is_refused():
    with pytest.raises(ValueError, match="dy holds 4 directions where the arguments before it hold 5"):
        _scs_hip._multi_diff_args(spec(np.ones((K, N)), np.ones((K - 1, M))))
    with pytest.raises(ValueError, match="ds holds 6 directions"):
        _scs_hip._multi_diff_args(spec(None, np.ones((K, M)), np.ones((K + 1, M))))
    with pytest.raises(ValueError, match="holds no direction"):
        _scs_hip._multi_diff_args(spec(np.ones((0, N))))


def test_a_wrong_second_dimension_is_refused():
    with pytest.raises(ValueError, match="dx has incompatible dimension with A: rows of 4 elements, not 5"):
        _scs_hip._multi_diff_args(spec(np.ones((K, N + 1))))
    with pytest.raises(ValueError, match="incompatible dimension"):
        _scs_hip._multi_diff_args(spec(None, np.ones((K, N))))
    with pytest.raises(ValueError, match="2-D"):
        _scs_hip._multi_diff_args(spec(np.ones(N)))
    with pytest.raises(ValueError, match="2-D"):
        _scs_hip._multi_diff_args(spec(np.ones((K, N, 1))))


def test_a_wrong_type_is_refused():
    with pytest.raises(TypeError, match="floats"):
        _scs_hip._multi_diff_args(spec(np.ones((K, N), dtype=np.int64)))
    with pytest.raises(TypeError, match="2-D numpy array"):
        _scs_hip._multi_diff_args(spec([[1.0] * N] * K))
    with pytest.raises(TypeError):
        _scs_hip._multi_diff_args(spec("abc"))
