"""SCS.update_device / solve_device / solve_many_device: the argument helper, on CPU tensors and non-tensors (no GPU): the faults
are reported before anything touches the device, and `import scs` does not import torch."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from scs import _scs_hip


def test_non_tensors_and_wrong_dtype_are_type_errors():
    with pytest.raises(TypeError, match="b_new must be a torch.Tensor on the workspace's GPU, not ndarray"):
        _scs_hip._device_vec("b_new", np.zeros(4), 4, 0)
    with pytest.raises(TypeError, match="x must be a torch.Tensor on the workspace's GPU, not list"):
        _scs_hip._device_vec("x", [0.0] * 4, 4, 0)
    with pytest.raises(TypeError, match="c_new must be a float64 tensor, not torch.float32"):
        _scs_hip._device_vec("c_new", torch.zeros(4, dtype=torch.float32), 4, 0)
    with pytest.raises(TypeError, match="float64"):
        _scs_hip._device_vec("c_new", torch.zeros(4, dtype=torch.int64), 4, 0)


def test_wrong_length_shape_layout_and_device_are_value_errors():
    with pytest.raises(ValueError, match=r"b_new must be a 1-D tensor of length 5, not of shape \(4,\)"):
        _scs_hip._device_vec("b_new", torch.zeros(4, dtype=torch.float64), 5, 0)
    with pytest.raises(ValueError, match=r"length 4, not of shape \(2, 2\)"):
        _scs_hip._device_vec("b_new", torch.zeros((2, 2), dtype=torch.float64), 4, 0)
    with pytest.raises(ValueError, match="b_new must be contiguous"):
        _scs_hip._device_vec("b_new", torch.zeros(8, dtype=torch.float64)[::2], 4, 0)
    with pytest.raises(ValueError, match=r"b_new must live on the workspace's GPU \(cuda:0\), not on cpu"):
        _scs_hip._device_vec("b_new", torch.zeros(4, dtype=torch.float64), 4, 0)


def test_solve_many_device_checks_rows_before_the_workspace():
    good = torch.zeros((2, 4), dtype=torch.float64)
    with pytest.raises(TypeError, match="b_new must be a torch.Tensor"):
        _scs_hip._many_device_args(4, 3, 0, np.zeros((2, 4)), None, False, None, None, None)
    with pytest.raises(ValueError, match="b_new must be a 2-D tensor, one row per problem"):
        _scs_hip._many_device_args(4, 3, 0, torch.zeros(4, dtype=torch.float64), None, False, None, None, None)
    with pytest.raises(ValueError, match="length 4"):
        _scs_hip._many_device_args(4, 3, 0, torch.zeros((2, 5), dtype=torch.float64), None, False, None, None, None)
    with pytest.raises(ValueError, match="workspace's GPU"):  # rows of the right shape, on the CPU
        _scs_hip._many_device_args(4, 3, 0, good, None, False, None, None, None)
    with pytest.raises(TypeError, match="argument 1 must be bool"):
        _scs_hip._many_device_args(4, 3, 0, None, None, 1, None, None, None)
    # warm-start rows are only looked at with warm_start=True
    assert _scs_hip._many_device_args(4, 3, 0, None, None, False, "ignored", None, None) == (1, dict.fromkeys("bcxys"))


def test_import_scs_does_not_import_torch():
    code = "import sys, scs; from scs import _scs_hip; sys.exit(1 if 'torch' in sys.modules else 0)"
    env_path = [p for p in sys.path if p]
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r\n%s" % (env_path, code)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
