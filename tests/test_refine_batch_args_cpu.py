"""The Python surface of scs.refine_batch / SCS.refine_many and the refusals that never reach the library: pure Python, no GPU."""
import pytest

import scs
import scs.autograd
from scs import _scs_hip, _scs_hip_dense


def test_the_new_names_exist():
    for mod in (scs, _scs_hip, _scs_hip_dense):
        for name in ("refine_batch", "refine_batch_device"):
            assert callable(getattr(mod, name)), (mod, name)
    for cls in (scs.SCS, _scs_hip.SCS, _scs_hip_dense.SCS):
        for name in ("refine_many", "refine_many_device"):
            assert callable(getattr(cls, name)), (cls, name)


def test_the_library_exports_the_entries():
    for name in ("scs_hip_refine_batch", "scs_hip_refine_batch_device"):
        assert hasattr(_scs_hip._lib, name), name


@pytest.mark.parametrize("mod", [scs, _scs_hip, _scs_hip_dense], ids=["scs", "hip", "dense"])
def test_a_non_list_and_a_non_solver_are_refused(mod):
    for call in (mod.refine_batch, mod.refine_batch_device):
        for bad in (None, 3, "solvers", {}, object()):
            with pytest.raises(TypeError, match="expects a list of solvers"):
                call(bad)
        with pytest.raises(TypeError, match="member 0"):
            call([object()])
        with pytest.raises(TypeError, match="member 0"):
            call((None, 5))


def test_an_empty_list_is_refused_by_name():
    for mod in (scs, _scs_hip, _scs_hip_dense):
        for call in (mod.refine_batch, mod.refine_batch_device):
            with pytest.raises(ValueError, match="empty.*member 0"):
                call([])


@pytest.mark.parametrize("kw", [dict(tol=0), dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=True), dict(lsqr_tol=-1.0),
                                dict(max_steps=0), dict(max_steps=False), dict(lsqr_max_iters=0)])
def test_bad_options_are_refused_through_refine_opts(kw):
    """the options go through `_refine_opts` before the members are touched: a member list that would be refused later does not matter"""
    sv = object.__new__(_scs_hip.SCS)  # (never initialised: no library call may see it)
    sv._blank()
    for call in (_scs_hip.refine_batch, _scs_hip.refine_batch_device, _scs_hip_dense.refine_batch):
        with pytest.raises(ValueError, match="must be"):
            call([sv], **kw)
    for call in (sv.refine_many, sv.refine_many_device):
        with pytest.raises(ValueError, match="must be"):
            call(**kw)
    with pytest.raises(TypeError):
        _scs_hip.refine_batch([sv], tol="1e-9")


def test_the_layer_documents_refinement_for_solve_many():
    doc = scs.autograd.__doc__
    assert "autograd_refine_tol" in doc and "refine_many_device" in doc
    assert "does not refine" not in doc
