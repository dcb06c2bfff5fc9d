"""The Python surface of the grouped derivatives and its argument checks (scs/_scs_hip.py `_many_diff_args`): pure Python, no GPU."""
import subprocess
import sys

import numpy as np
import pytest

import scs
from scs import _scs_hip, _scs_hip_dense

MODULE_NAMES = ("adjoint_batch", "derivative_batch", "adjoint_batch_device", "derivative_batch_device", "diff_batch_plan",
                "diff_group_launches")
METHOD_NAMES = ("adjoint_many", "adjoint_many_device", "derivative_many", "derivative_many_device")
M, N, K = 7, 4, 3


def test_the_new_names_exist():
    for mod in (scs, _scs_hip, _scs_hip_dense):
        for name in MODULE_NAMES:
            assert callable(getattr(mod, name)), (mod.__name__, name)
    for cls in (scs.SCS, _scs_hip.SCS, _scs_hip_dense.SCS):
        for name in METHOD_NAMES:
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(_scs_hip._many_diff_args)


def spec(dx=None, dy=None, ds=None, n=N, m=M):
    return (("dx", dx, n), ("dy", dy, m), ("ds", ds, m))


def test_good_arguments_pass():
    k, rows = _scs_hip._many_diff_args(spec(np.ones((K, N)), None, np.zeros((K, M), dtype=np.float32)), None, ("b", "c", "A", "P"), True)
    assert k == K and rows["dy"] is None and len(rows["dx"]) == K
    assert all(r.dtype == np.float64 and r.flags["C_CONTIGUOUS"] and r.shape == (M,) for r in rows["ds"])
    k, rows = _scs_hip._many_diff_args(spec([np.ones(N), None, np.ones(N)]), K)
    assert k == K and rows["dx"][1] is None and rows["dx"][0].shape == (N,)
    assert _scs_hip._many_diff_args(spec(), None) == (None, {"dx": None, "dy": None, "ds": None})
    # one length per member (a mixed batch)
    k, rows = _scs_hip._many_diff_args((("dx", [np.ones(2), np.ones(5)], [2, 5]),), 2)
    assert [r.shape[0] for r in rows["dx"]] == [2, 5]


def test_a_wrong_K_is_refused():
    with pytest.raises(ValueError, match="dy holds 2 rows for 3 problems"):
        _scs_hip._many_diff_args(spec(np.ones((K, N)), np.ones((K - 1, M))), None)
    with pytest.raises(ValueError, match="dx holds 3 rows for 5 problems"):
        _scs_hip._many_diff_args(spec(np.ones((K, N))), 5)
    with pytest.raises(ValueError, match="at least one problem"):
        _scs_hip._many_diff_args(spec(np.ones((0, N))), None)


def test_lists_of_another_length_than_the_solvers_are_refused():
    with pytest.raises(ValueError, match="dx holds 2 rows for 3 problems"):
        _scs_hip._many_diff_args(spec([np.ones(N), np.ones(N)]), K)
    with pytest.raises(ValueError, match="ds holds 4 rows for 3 problems"):
        _scs_hip._many_diff_args(spec(None, None, [None] * 4), K)


def test_a_wrong_row_length_is_refused():
    with pytest.raises(ValueError, match="incompatible dimension"):
        _scs_hip._many_diff_args(spec(np.ones((K, N + 1))), None)
    with pytest.raises(ValueError, match="incompatible dimension"):
        _scs_hip._many_diff_args(spec(None, [np.ones(M), np.ones(M - 1), None]), K)
    with pytest.raises(ValueError, match="2-D"):
        _scs_hip._many_diff_args(spec(np.ones(N)), None)


def test_a_wrong_dtype_is_refused():
    with pytest.raises(TypeError, match="floats"):
        _scs_hip._many_diff_args(spec(np.ones((K, N), dtype=np.int64)), None)
    with pytest.raises(TypeError, match="floats"):
        _scs_hip._many_diff_args(spec([np.ones(N, dtype=np.int32)] * K), K)
    with pytest.raises(TypeError):
        _scs_hip._many_diff_args(spec("abc"), None)
    with pytest.raises(TypeError, match="floats"):
        _scs_hip._many_diff_args(spec([[1.0] * N] * K), K)


def test_a_non_contiguous_input_is_refused():
    with pytest.raises(ValueError, match="contiguous"):
        _scs_hip._many_diff_args(spec(np.ones((N, K)).T), None)
    with pytest.raises(ValueError, match="contiguous"):
        _scs_hip._many_diff_args(spec([np.ones(2 * N)[::2]] * K), K)


def test_want_outside_b_c_A_P_is_refused():
    with pytest.raises(ValueError, match="the names are"):
        _scs_hip._many_diff_args(spec(), K, ("b", "x"), True)
    with pytest.raises(TypeError, match="want must be a tuple"):
        _scs_hip._many_diff_args(spec(), K, "bc", True)
    with pytest.raises(ValueError, match="without P"):
        _scs_hip._many_diff_args(spec(), K, ("b", "P"), False)


def test_batch_entries_check_before_the_library_is_called():
    with pytest.raises(TypeError, match="scs.SCS objects"):
        scs.adjoint_batch([object()])
    with pytest.raises(TypeError, match="scs.SCS objects"):
        scs.diff_batch_plan([None])
    assert scs.adjoint_batch([]) == [] and scs.derivative_batch([]) == [] and scs.diff_batch_plan([]) == []


def test_import_scs_leaves_torch_out():
    code = ("import sys; import scs; assert 'torch' not in sys.modules, 'torch'; assert 'scs.autograd' not in sys.modules, 'autograd'; "
            "assert callable(scs.adjoint_batch)")
    env_path = [p for p in sys.path if p]
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r; %s" % (env_path, code)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
