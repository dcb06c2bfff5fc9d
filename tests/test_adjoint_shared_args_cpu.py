"""`reduce="sum"` of the adjoint of a list of members (SCS.adjoint_many, adjoint_batch and their device twins), without a GPU: the
argument checks, and — with the host entries of the library replaced by recording stubs, as tests/test_diff_glue_cpu.py does — which
entry is called with which slots.  From include/scs_hip.h:

  scs_hip_adjoint_shared(w, gx, gy, gs, db, dc, dAx_sum, dPx_sum, opts, info, count)
      gx .. dc: arrays of `count` entries as in scs_hip_adjoint_batch; dAx_sum, dPx_sum: ONE vector each, NULL = not wanted."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import scs
from scs import _scs_hip, _scs_hip_dense
from test_derivative_matrix_args_cpu import NNZ_A, NNZ_P, forget, shell  # (m, n) = (4, 3), nnz(A) = 5, nnz(P) = 4
from test_diff_glue_cpu import GIVEN, HOST_ENTRIES, NULL, is_null

M, N = 4, 3
SHARED = "scs_hip_adjoint_shared"


class Recorder(object):
    """stubs for the host entries: (entry, works, NULL-ness of every slot before opts — a tuple per array slot, a bool per vector —, count)"""

    def __init__(self):
        self.calls = []

    def stub(self, name):
        def call(*args):
            works, slots, count = args[0], args[1:-3], args[-1]
            nulls = []
            for a in slots:
                if isinstance(a, int) or a is None:  # one vector for all members (or a NULL array: both read as NULL)
                    nulls.append(is_null(a))
                else:
                    nulls.append(tuple(is_null(a[i]) for i in range(count)))
            self.calls.append((name, [works[i] for i in range(count)], tuple(nulls), count))
            return 0
        return call


@pytest.fixture
def recorded():
    rec = Recorder()
    names = HOST_ENTRIES + (SHARED,)
    saved = {name: getattr(_scs_hip._lib, name) for name in names}
    try:
        for name in names:
            setattr(_scs_hip._lib, name, rec.stub(name))
        yield rec
    finally:
        for name, fn in saved.items():
            setattr(_scs_hip._lib, name, fn)


def one(rec):
    assert len(rec.calls) == 1, rec.calls
    return rec.calls.pop()


def pair():
    sv, clone = shell(), shell()
    sv._work, clone._work = 21, 22
    sv._many = [clone]  # (as if solve_many had solved two members)
    return sv, clone


def test_the_keyword_comes_last():
    for cls in (scs.SCS, _scs_hip.SCS, _scs_hip_dense.SCS):
        for name in ("adjoint_many", "adjoint_many_device"):
            assert list(inspect.signature(getattr(cls, name)).parameters)[1:] == ["dx", "dy", "ds", "want", "tol", "max_iters", "reduce"], (cls, name)
    for mod in (scs, _scs_hip, _scs_hip_dense):
        for name in ("adjoint_batch", "adjoint_batch_device"):
            sig = inspect.signature(getattr(mod, name))
            assert list(sig.parameters) == ["solvers", "dx", "dy", "ds", "want", "tol", "max_iters", "reduce"], (mod, name)
            assert sig.parameters["reduce"].default is None
    assert callable(_scs_hip.grad_matrix_sum)


def test_the_entries_are_declared_and_exported():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scs_hip.h")).read()
    for name in ("scs_hip_adjoint_shared", "scs_hip_adjoint_shared_device"):
        assert re.search(r"SCS_HIP_API\s+scs_int\s+%s\s*\(" % name, header)
        assert isinstance(getattr(_scs_hip._lib, name), ctypes._CFuncPtr)
    assert re.search(r"SCS_HIP_API\s+int\s+scs_hip_grad_matrix_sum\s*\(", header)


def test_reduce_values():
    sv, clone = pair()
    try:
        for call in (sv.adjoint_many, sv.adjoint_many_device, lambda **kw: _scs_hip.adjoint_batch([sv, clone], **kw),
                     lambda **kw: _scs_hip.adjoint_batch_device([sv, clone], **kw)):
            for bad in ("mean", "SUM", True, 1, ("sum",)):
                with pytest.raises(ValueError, match="reduce must be None or 'sum'"):
                    call(want=("A",), reduce=bad)
            with pytest.raises(ValueError, match="want must hold 'A' or 'P'"):
                call(reduce="sum")  # want = (b, c)
            with pytest.raises(ValueError, match="want must hold 'A' or 'P'"):
                call(want=(), reduce="sum")
        noP = shell(with_P=False)
        noP._many = []
        try:
            with pytest.raises(ValueError, match="dP wanted, but the solver was created without P"):
                noP.adjoint_many(want=("P",), reduce="sum")
            with pytest.raises(ValueError, match="dP wanted, but the solver was created without P"):
                _scs_hip.adjoint_batch([noP], want=("A", "P"), reduce="sum")
        finally:
            forget(noP)
    finally:
        sv._many = []
        forget(sv, clone)


def test_shared_slots(recorded):
    sv, clone = pair()
    every = (GIVEN, GIVEN)
    try:
        res, grads = sv.adjoint_many(dx=np.ones((2, N)), want=("b", "c", "A", "P"), reduce="sum")
        assert one(recorded) == (SHARED, [21, 22], (every, NULL, NULL, every, every, GIVEN, GIVEN), 2)
        assert [sorted(r) for r in res] == [["db", "dc", "info"]] * 2 and res[1]["db"].shape == (M,)
        assert sorted(grads) == ["dA", "dP"] and grads["dA"].shape == (NNZ_A,) and grads["dP"].shape == (NNZ_P,)
        res, grads = sv.adjoint_many(dy=np.ones((2, M)), want=("A",), reduce="sum")  # A alone: NULL db, dc arrays and a NULL dPx_sum
        assert one(recorded) == (SHARED, [21, 22], (NULL, every, NULL, NULL, NULL, GIVEN, NULL), 2)
        assert [sorted(r) for r in res] == [["info"]] * 2 and list(grads) == ["dA"]
        res, grads = sv.adjoint_many(ds=np.ones((1, M)), want=("P", "c"), reduce="sum")  # one row: the first member alone
        assert one(recorded) == (SHARED, [21], (NULL, NULL, (GIVEN,), NULL, (GIVEN,), NULL, GIVEN), 1)
        assert list(res[0]) == ["dc", "info"] and list(grads) == ["dP"]
        res, grads = _scs_hip.adjoint_batch([clone, sv], dx=[np.ones(N), None], want=("c", "A"), reduce="sum")
        assert one(recorded) == (SHARED, [22, 21], ((GIVEN, NULL), NULL, NULL, NULL, every, GIVEN, NULL), 2)
        assert len(res) == 2 and list(res[0]) == ["dc", "info"] and grads["dA"].shape == (NNZ_A,)
        assert _scs_hip.adjoint_batch([], want=("A",), reduce="sum") == ([], {})
    finally:
        sv._many = []
        forget(sv, clone)


def test_without_reduce_the_old_entries_are_reached_unchanged(recorded):
    sv, clone = pair()
    every = (GIVEN, GIVEN)
    try:
        for kw in ({}, {"reduce": None}):
            res = sv.adjoint_many(dx=np.ones((2, N)), want=("b", "c", "A"), **kw)
            assert one(recorded) == ("scs_hip_adjoint_batch", [21, 22], (every, NULL, NULL, every, every, every, NULL), 2)
            assert len(res) == 2 and res[0]["dA"].shape == (NNZ_A,)
            res = _scs_hip.adjoint_batch([sv, clone], want=("P",), **kw)
            assert one(recorded) == ("scs_hip_adjoint_batch", [21, 22], (NULL, NULL, NULL, NULL, NULL, NULL, every), 2)
            assert [list(r) for r in res] == [["dP", "info"]] * 2
    finally:
        sv._many = []
        forget(sv, clone)


def test_the_stubs_are_gone():
    assert isinstance(_scs_hip._lib.scs_hip_adjoint_shared, ctypes._CFuncPtr)
    assert _scs_hip._lib.scs_hip_adjoint_shared(None, None, None, None, None, None, None, None, None, None, 0) == -1  # (the library again)
    assert "count must be positive" in _scs_hip.last_error()
