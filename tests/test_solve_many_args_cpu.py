"""Argument checks of SCS.solve_many (scs/_scs_hip.py _many_args): they run before anything touches the device, and the faults that
`update` / `solve` know keep the messages pinned for those (tests/test_boundary_cpu.py)."""
import numpy as np
import pytest

from scs import _scs_hip

M, N = 6, 4


def _ok(k=3):
    return np.zeros((k, M)), np.zeros((k, N))


def test_shapes_and_copies():
    b, c = _ok()
    K, rows = _scs_hip._many_args(M, N, b, c, False, None, None, None)
    assert K == 3 and rows["b"].shape == (3, M) and rows["c"].shape == (3, N)
    assert rows["b"] is not b and rows["b"].dtype == np.float64
    K, rows = _scs_hip._many_args(M, N, None, c.astype(np.float32), False, None, None, None)
    assert K == 3 and rows["b"] is None and rows["c"].dtype == np.float64
    assert _scs_hip._many_args(M, N, None, None, False, None, None, None)[0] == 1
    # warm-start rows are ignored without warm_start, as solve() ignores x, y, s
    assert _scs_hip._many_args(M, N, b, c, False, "junk", None, None)[1]["x"] is None


@pytest.mark.parametrize("b, c, exc, match", [
    (np.zeros(M), None, TypeError, "b_new must be"),
    (None, [[0.0] * N], TypeError, "c_new must be"),
    (np.zeros((2, M), dtype=np.int64), None, TypeError, "b_new must be"),
    (np.zeros((2, M + 1)), None, ValueError, "b_new has incompatible dimension with A"),
    (None, np.zeros((2, N - 1)), ValueError, "c_new has incompatible dimension with A"),
    (np.zeros((2, M)), np.zeros((3, N)), ValueError, "same number of rows"),
    (np.zeros((0, M)), None, ValueError, "at least one problem"),
])
def test_bad_b_c(b, c, exc, match):
    with pytest.raises(exc, match=match):
        _scs_hip._many_args(M, N, b, c, False, None, None, None)


@pytest.mark.parametrize("name, arr", [("x", np.zeros((3, N + 1))), ("y", np.zeros(M)), ("s", np.zeros((2, M))),
                                       ("x", np.zeros((3, N), dtype=np.int32))])
def test_bad_warm_start_rows(name, arr):
    b, c = _ok()
    kw = {"x": None, "y": None, "s": None}
    kw[name] = arr
    with pytest.raises(ValueError, match="Unable to parse %s warm-start" % name):
        _scs_hip._many_args(M, N, b, c, True, kw["x"], kw["y"], kw["s"])


def test_warm_start_flag_type():
    with pytest.raises(TypeError, match="argument 1 must be bool"):
        _scs_hip._many_args(M, N, None, None, 1, None, None, None)


def test_checks_come_before_the_workspace():
    sv = object.__new__(_scs_hip.SCS)  # no device workspace behind it
    sv.m, sv.n, sv._work = M, N, None
    with pytest.raises(ValueError, match="b_new has incompatible dimension with A"):
        sv.solve_many(b=np.zeros((2, M + 2)))
    with pytest.raises(ValueError, match="Workspace not initialized!"):
        sv.solve_many(b=np.zeros((2, M)))
    assert hasattr(_scs_hip.SCS, "clone") and hasattr(_scs_hip.SCS, "shares_matrix")
