"""The Python surface of SCS.refine / refine_device and the argument refusals that never reach the library (scs/_scs_hip.py
`_refine_opts`): pure Python, no GPU."""
import ctypes as C

import numpy as np
import pytest

import scs
from scs import _scs_hip, _scs_hip_dense


def test_the_new_names_exist():
    for cls in (scs.SCS, _scs_hip.SCS, _scs_hip_dense.SCS):
        for name in ("refine", "refine_device"):
            assert callable(getattr(cls, name)), (cls, name)
    assert _scs_hip.REFINE_STOP == {1: "converged", 2: "max_steps", 3: "no_decrease"}


def test_the_library_exports_the_entries():
    for name in ("scs_hip_refine", "scs_hip_refine_device"):
        assert hasattr(_scs_hip._lib, name), name


def test_the_structs_have_the_layout_of_the_header():
    """ScsHipRefineOpts: double, int, double, int; ScsHipRefineInfo: four ints, then eleven doubles"""
    assert [n for n, _ in _scs_hip._ScsHipRefineOpts._fields_] == ["tol", "max_steps", "lsqr_tol", "lsqr_max_iters"]
    assert C.sizeof(_scs_hip._ScsHipRefineOpts) == 32
    names = [n for n, _ in _scs_hip._ScsHipRefineInfo._fields_]
    assert names == ["steps", "halvings", "lsqr_iters", "stop", "merit_before", "merit_after", "res_pri_before", "res_dual_before", "gap_before",
                     "res_pri", "res_dual", "gap", "pobj", "dobj", "time_ms"]
    assert C.sizeof(_scs_hip._ScsHipRefineInfo) == 4 * 4 + 11 * 8


def test_defaults_and_good_arguments():
    o = _scs_hip._refine_opts(1e-9, 10, 1e-8, None)
    assert (o.tol, o.max_steps, o.lsqr_tol, o.lsqr_max_iters) == (1e-9, 10, 1e-8, 0)
    o = _scs_hip._refine_opts(np.float64(1e-6), np.int64(3), 1e-10, 500)
    assert (o.tol, o.max_steps, o.lsqr_tol, o.lsqr_max_iters) == (1e-6, 3, 1e-10, 500)


@pytest.mark.parametrize("bad", [0, 0.0, -1e-9, float("nan"), float("inf"), True])
def test_a_bad_tol_is_refused(bad):
    with pytest.raises(ValueError, match="^tol must be a positive finite number"):
        _scs_hip._refine_opts(bad, 10, 1e-8, None)
    with pytest.raises(ValueError, match="^lsqr_tol must be a positive finite number"):
        _scs_hip._refine_opts(1e-9, 10, bad, None)


def test_bad_counts_are_refused():
    for bad in (0, -1, False):
        with pytest.raises(ValueError, match="max_steps must be at least 1"):
            _scs_hip._refine_opts(1e-9, bad, 1e-8, None)
    for bad in (0, -5):
        with pytest.raises(ValueError, match="lsqr_max_iters must be positive"):
            _scs_hip._refine_opts(1e-9, 10, 1e-8, bad)


def test_wrong_types_are_refused():
    with pytest.raises(TypeError):
        _scs_hip._refine_opts("1e-9", 10, 1e-8, None)
    with pytest.raises(TypeError):
        _scs_hip._refine_opts(None, 10, 1e-8, None)
    with pytest.raises(TypeError):
        _scs_hip._refine_opts(1e-9, 2.5, 1e-8, None)
    with pytest.raises(TypeError):
        _scs_hip._refine_opts(1e-9, 10, 1e-8, 7.0)


def test_the_info_dict_names_the_stop():
    info = _scs_hip._ScsHipRefineInfo()
    for stop, text in ((1, "converged"), (2, "max_steps"), (3, "no_decrease"), (0, "unknown")):
        info.stop = stop
        d = _scs_hip._refine_info_dict(info)
        assert d["stop"] == stop and d["stop_reason"] == text
    assert set(d) == {n for n, _ in _scs_hip._ScsHipRefineInfo._fields_} | {"stop_reason"}


def test_the_layer_documents_its_switch():
    import scs.autograd
    assert "autograd_refine_tol" in scs.autograd.__doc__
