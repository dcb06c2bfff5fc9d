"""SCS.adjoint / adjoint_device / derivative / derivative_device: the pure-Python argument checks (scs._scs_hip._diff_vec, _diff_want,
_diff_opts, _device_vec), which run before the library is called and need no GPU; and the new symbols in the header and the library."""
import os
import re

import numpy as np
import pytest

from scs import _scs_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shell(m=4, n=3, with_P=True):
    """a raw solver object whose workspace handle is never handed to the library: every call below must fail in Python first"""
    sv = object.__new__(_scs_hip.SCS)
    sv._blank()
    sv._shape(m, n)
    sv._work = 1
    ip = np.zeros(n + 1, dtype=np.int32)
    sv._pattern = {"A": (ip, np.zeros(0, dtype=np.int32)), "P": (ip, np.zeros(0, dtype=np.int32)) if with_P else None}
    return sv


def forget(sv):
    sv._work = None  # (the destructor must not finish a handle that is none)


def test_vectors_are_checked_for_type_and_length():
    out = _scs_hip._diff_vec("dx", np.arange(3, dtype=np.float32), 3)
    assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, [0.0, 1.0, 2.0])
    assert _scs_hip._diff_vec("dx", None, 3) is None
    strided = np.arange(6.0)[::2]
    assert _scs_hip._diff_vec("dy", strided, 3).flags["C_CONTIGUOUS"]
    for bad in ([0.0] * 3, np.zeros((3, 1)), np.arange(3), "abc"):
        with pytest.raises(TypeError, match="dx must be a 1-D numpy array of floats"):
            _scs_hip._diff_vec("dx", bad, 3)
    with pytest.raises(ValueError, match="ds has incompatible dimension with A"):
        _scs_hip._diff_vec("ds", np.zeros(5), 4)


def test_every_host_argument_of_adjoint_and_derivative():
    sv = shell()
    try:
        for kw in ("dx", "dy", "ds"):
            with pytest.raises(TypeError, match="%s must be a 1-D numpy array of floats" % kw):
                sv.adjoint(**{kw: [1.0]})
            with pytest.raises(ValueError, match="%s has incompatible dimension with A" % kw):
                sv.adjoint(**{kw: np.zeros(7)})
        for kw in ("db", "dc"):
            with pytest.raises(TypeError, match="%s must be a 1-D numpy array of floats" % kw):
                sv.derivative(**{kw: (1.0,)})
            with pytest.raises(ValueError, match="%s has incompatible dimension with A" % kw):
                sv.derivative(**{kw: np.zeros(7)})
    finally:
        forget(sv)


def test_want():
    assert _scs_hip._diff_want(["c", "A"], False) == ("c", "A")
    assert _scs_hip._diff_want(("b", "c", "A", "P"), True) == ("b", "c", "A", "P")
    assert _scs_hip._diff_want((), False) == ()
    with pytest.raises(TypeError, match="want must be a tuple"):
        _scs_hip._diff_want("bc", True)
    with pytest.raises(TypeError, match="want must be a tuple"):
        _scs_hip._diff_want(None, True)
    with pytest.raises(ValueError, match="the names are 'b', 'c', 'A', 'P'"):
        _scs_hip._diff_want(("b", "x"), True)
    with pytest.raises(ValueError, match="the names are"):
        _scs_hip._diff_want(("b", 1), True)
    with pytest.raises(ValueError, match="twice"):
        _scs_hip._diff_want(("b", "b"), True)
    with pytest.raises(ValueError, match="dP wanted, but the solver was created without P"):
        _scs_hip._diff_want(("P",), False)
    sv = shell(with_P=False)
    try:
        for method in (sv.adjoint, sv.adjoint_device):
            with pytest.raises(ValueError, match="created without P"):
                method(want=("b", "P"))
            with pytest.raises(TypeError, match="want must be a tuple"):
                method(want="b")
    finally:
        forget(sv)


def test_tol_and_max_iters():
    o = _scs_hip._diff_opts(1e-10, None)
    assert o.tol == 1e-10 and o.max_iters == 0
    assert _scs_hip._diff_opts(np.float32(0.5), np.int64(7)).max_iters == 7
    for bad in (0.0, -1e-8, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="tol must be a positive finite number"):
            _scs_hip._diff_opts(bad, None)
    for bad in ("1e-8", None):
        with pytest.raises(TypeError, match="must be real number"):
            _scs_hip._diff_opts(bad, None)
    for bad in (0, -3, True):
        with pytest.raises(ValueError, match="max_iters must be positive"):
            _scs_hip._diff_opts(1e-8, bad)
    with pytest.raises(TypeError, match="cannot be interpreted as an integer"):
        _scs_hip._diff_opts(1e-8, 2.5)
    sv = shell()
    try:
        for method in (sv.adjoint, sv.adjoint_device, sv.derivative, sv.derivative_device):
            with pytest.raises(ValueError, match="tol must be a positive finite number"):
                method(tol=0.0)
            with pytest.raises(ValueError, match="max_iters must be positive"):
                method(max_iters=0)
            with pytest.raises(TypeError, match="cannot be interpreted as an integer"):
                method(max_iters=1.5)
    finally:
        forget(sv)


def test_device_vectors_must_be_float64_tensors_of_the_right_length():
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="dx must be a torch.Tensor on the workspace's GPU, not ndarray"):
        _scs_hip._device_vec("dx", np.zeros(3), 3, 0)
    with pytest.raises(TypeError, match="dy must be a float64 tensor"):
        _scs_hip._device_vec("dy", torch.zeros(4, dtype=torch.float32), 4, 0)
    with pytest.raises(ValueError, match="ds must be a 1-D tensor of length 4"):
        _scs_hip._device_vec("ds", torch.zeros(5, dtype=torch.float64), 4, 0)
    with pytest.raises(ValueError, match="db must be contiguous"):
        _scs_hip._device_vec("db", torch.zeros(8, dtype=torch.float64)[::2], 4, 0)
    with pytest.raises(ValueError, match="dc must live on the workspace's GPU"):
        _scs_hip._device_vec("dc", torch.zeros(3, dtype=torch.float64), 3, 0)


def test_a_finished_solver_is_refused():
    sv = shell()
    forget(sv)
    for method in (sv.adjoint, sv.adjoint_device, sv.derivative, sv.derivative_device):
        with pytest.raises(ValueError, match="Workspace not initialized!"):
            method()


def test_symbols_are_declared_and_defined():
    header = open(os.path.join(ROOT, "include", "scs_hip.h")).read()
    for name in ("scs_hip_adjoint", "scs_hip_adjoint_device", "scs_hip_derivative", "scs_hip_derivative_device"):
        assert re.search(r"SCS_HIP_API\s+scs_int\s+%s\s*\(" % name, header), name
    assert re.search(r"SCS_HIP_API\s+int\s+scs_hip_dproj_cone\s*\(", header)
    assert "ScsHipDiffOpts" in header and "ScsHipDiffInfo" in header
    lib = _scs_hip._lib
    # a NULL workspace is refused with a reason (no device needed)
    assert lib.scs_hip_adjoint(None, None, None, None, None, None, None, None, None, None) == -1
    assert "null workspace" in _scs_hip.last_error()
    assert lib.scs_hip_derivative_device(None, None, None, None, None, None, None, None) == -1
    assert "scs_hip_derivative_device: null workspace" in _scs_hip.last_error()
