"""What the Python glue hands to C for the six host derivative functions (SCS.adjoint, SCS.derivative, SCS.adjoint_many,
SCS.derivative_many, adjoint_batch, derivative_batch): which entry of libscs_hip.so is called, with how many pointer slots, which of
them are NULL, and `count`.  The six host entries are replaced by recording stubs, so nothing reaches the library and no device is
needed.  The expected table below is written from include/scs_hip.h and the docstrings:

  scs_hip_adjoint(w, gx, gy, gs, db, dc, dAx, dPx, opts, info)             a NULL input counts as 0, a NULL output is skipped
  scs_hip_derivative(w, db, dc, dx, dy, ds, opts, info)                    the entry of a call without dA and dP
  scs_hip_derivative_full(w, db, dc, dAx, dPx, dx, dy, ds, opts, info)
  the *_batch entries: the same slots as arrays of `count` entries (a NULL array: no such vector for any member; an entry may be
  NULL too), then opts, info, count."""
import ctypes

import numpy as np
import pytest

from scs import _scs_hip
from test_adjoint_args_cpu import shell as empty_shell  # (m, n) = (4, 3), A and P without a stored entry
from test_derivative_matrix_args_cpu import NNZ_A, NNZ_P, forget, shell  # (m, n) = (4, 3), nnz(A) = 5, nnz(P) = 4

M, N = 4, 3
HOST_ENTRIES = ("scs_hip_adjoint", "scs_hip_derivative", "scs_hip_derivative_full", "scs_hip_adjoint_batch", "scs_hip_derivative_batch",
                "scs_hip_derivative_full_batch")
GIVEN, NULL = False, True  # (how a slot reads in the tables below)


def is_null(p):
    if p is None:
        return True
    if isinstance(p, int):
        return p == 0
    return not bool(p)  # (a ctypes pointer or c_void_p)


class Recorder(object):
    """stubs for the host entries: each call is kept as (entry, work(s), NULL-ness of every pointer slot, count or None)"""

    def __init__(self):
        self.calls = []

    def stub(self, name):
        batch = name.endswith("_batch")

        def call(*args):
            if batch:
                works, slots, count = args[0], args[1:-3], args[-1]
                assert len(works) == count and len(args[-2]) == count  # (one workspace and one info per member)
                nulls = tuple(NULL if is_null(a) else tuple(is_null(a[i]) for i in range(count)) for a in slots)
                self.calls.append((name, [works[i] for i in range(count)], nulls, count))
            else:
                self.calls.append((name, args[0], tuple(is_null(a) for a in args[1:-2]), None))
            return 0
        return call


@pytest.fixture
def recorded():
    rec = Recorder()
    saved = {name: getattr(_scs_hip._lib, name) for name in HOST_ENTRIES}
    try:
        for name in HOST_ENTRIES:
            setattr(_scs_hip._lib, name, rec.stub(name))
        yield rec
    finally:
        for name, fn in saved.items():
            setattr(_scs_hip._lib, name, fn)
        assert _scs_hip._lib.scs_hip_adjoint is saved["scs_hip_adjoint"]


def one(rec):
    assert len(rec.calls) == 1, rec.calls
    return rec.calls.pop()


def test_adjoint_slots(recorded):
    sv = shell()
    try:
        res = sv.adjoint()  # no cotangent; want = (b, c): the dAx / dPx slots are NULL
        assert one(recorded) == ("scs_hip_adjoint", 1, (NULL, NULL, NULL, GIVEN, GIVEN, NULL, NULL), None)
        assert sorted(res) == ["db", "dc", "info"] and res["db"].shape == (M,) and res["dc"].shape == (N,)
        assert sorted(res["info"]) == ["iters", "normal_residual", "residual", "stop", "time_ms"]
        res = sv.adjoint(dy=np.ones(M), want=("A",))  # the db / dc slots are NULL
        assert one(recorded) == ("scs_hip_adjoint", 1, (NULL, GIVEN, NULL, NULL, NULL, GIVEN, NULL), None)
        assert sorted(res) == ["dA", "info"] and res["dA"].shape == (NNZ_A,)
        res = sv.adjoint(np.ones(N), np.ones(M), np.ones(M), want=("P", "c", "b", "A"))
        assert one(recorded) == ("scs_hip_adjoint", 1, (GIVEN,) * 7, None)
        assert list(res) == ["dP", "dc", "db", "dA", "info"] and res["dP"].shape == (NNZ_P,)
        sv.adjoint(ds=np.ones(M), want=())
        assert one(recorded) == ("scs_hip_adjoint", 1, (NULL, NULL, GIVEN, NULL, NULL, NULL, NULL), None)
    finally:
        forget(sv)


def test_a_wanted_output_without_an_entry_is_still_a_request(recorded):
    """the library takes a non-NULL dAx / dPx as `wanted` whatever its length (its refusals for dPx fire, the batch groups by it): the
    host glue passes the address of the empty result"""
    sv = empty_shell()
    try:
        res = sv.adjoint(want=("b", "A", "P"))
        assert one(recorded) == ("scs_hip_adjoint", 1, (NULL, NULL, NULL, GIVEN, NULL, GIVEN, GIVEN), None)
        assert res["dA"].shape == (0,) and res["dP"].shape == (0,)
    finally:
        forget(sv)


def test_derivative_slots(recorded):
    sv = shell()
    try:
        res = sv.derivative()  # the short entry: five pointer slots before opts
        assert one(recorded) == ("scs_hip_derivative", 1, (NULL, NULL, GIVEN, GIVEN, GIVEN), None)
        assert sorted(res) == ["ds", "dx", "dy", "info"] and res["dx"].shape == (N,) and res["dy"].shape == (M,) and res["ds"].shape == (M,)
        sv.derivative(db=np.ones(M))
        assert one(recorded) == ("scs_hip_derivative", 1, (GIVEN, NULL, GIVEN, GIVEN, GIVEN), None)
        sv.derivative(dA=np.ones(NNZ_A))  # the full entry: seven
        assert one(recorded) == ("scs_hip_derivative_full", 1, (NULL, NULL, GIVEN, NULL, GIVEN, GIVEN, GIVEN), None)
        sv.derivative(dc=np.ones(N), dP=np.ones(NNZ_P))
        assert one(recorded) == ("scs_hip_derivative_full", 1, (NULL, GIVEN, NULL, GIVEN, GIVEN, GIVEN, GIVEN), None)
    finally:
        forget(sv)


def test_adjoint_batch_slots(recorded):
    sv, tw = shell(), shell()
    sv._work, tw._work = 11, 12
    every = (GIVEN, GIVEN)
    try:
        res = _scs_hip.adjoint_batch([sv, tw], dx=[np.ones(N), None])  # one row is None: a NULL entry; dy, ds: NULL arrays
        assert one(recorded) == ("scs_hip_adjoint_batch", [11, 12], ((GIVEN, NULL), NULL, NULL, every, every, NULL, NULL), 2)
        assert [sorted(r) for r in res] == [["db", "dc", "info"]] * 2 and res[1]["dc"].shape == (N,)
        res = _scs_hip.adjoint_batch([tw, sv], dy=np.ones((2, M)), ds=[None, np.ones(M)], want=("A", "P"))
        assert one(recorded) == ("scs_hip_adjoint_batch", [12, 11], (NULL, every, (NULL, GIVEN), NULL, NULL, every, every), 2)
        assert [list(r) for r in res] == [["dA", "dP", "info"]] * 2 and res[0]["dA"].shape == (NNZ_A,)
    finally:
        forget(sv, tw)


def test_derivative_batch_slots(recorded):
    sv, tw = shell(), shell()
    sv._work, tw._work = 11, 12
    every = (GIVEN, GIVEN)
    try:
        res = _scs_hip.derivative_batch([sv, tw], db=np.ones((2, M)))  # without dA and dP: the short entry
        assert one(recorded) == ("scs_hip_derivative_batch", [11, 12], (every, NULL, every, every, every), 2)
        assert [sorted(r) for r in res] == [["ds", "dx", "dy", "info"]] * 2 and res[0]["ds"].shape == (M,)
        _scs_hip.derivative_batch([sv, tw], dc=[None, np.ones(N)], dP=[np.ones(NNZ_P), None])  # with dP: the full one
        assert one(recorded) == ("scs_hip_derivative_full_batch", [11, 12], (NULL, (NULL, GIVEN), NULL, (GIVEN, NULL), every, every, every), 2)
        _scs_hip.derivative_batch([sv], dA=np.ones((1, NNZ_A)))
        assert one(recorded) == ("scs_hip_derivative_full_batch", [11], (NULL, NULL, (GIVEN,), NULL, (GIVEN,), (GIVEN,), (GIVEN,)), 1)
    finally:
        forget(sv, tw)


def test_the_many_methods_end_in_the_batch_entries(recorded):
    sv, clone = shell(), shell()
    sv._work, clone._work = 21, 22
    sv._many = [clone]  # (as if solve_many had solved two members)
    every = (GIVEN, GIVEN)
    try:
        res = sv.adjoint_many(dx=np.ones((2, N)))
        assert one(recorded) == ("scs_hip_adjoint_batch", [21, 22], (every, NULL, NULL, every, every, NULL, NULL), 2)
        assert len(res) == 2 and sorted(res[1]) == ["db", "dc", "info"]
        res = sv.adjoint_many()  # no rows: every member solve_many has solved
        assert one(recorded) == ("scs_hip_adjoint_batch", [21, 22], (NULL, NULL, NULL, every, every, NULL, NULL), 2)
        res = sv.adjoint_many(ds=np.ones((1, M)), want=("c", "A"))  # one row: the first member alone
        assert one(recorded) == ("scs_hip_adjoint_batch", [21], (NULL, NULL, (GIVEN,), NULL, (GIVEN,), (GIVEN,), NULL), 1)
        assert list(res[0]) == ["dc", "dA", "info"]
        res = sv.derivative_many(dc=np.ones((2, N)))
        assert one(recorded) == ("scs_hip_derivative_batch", [21, 22], (NULL, every, every, every, every), 2)
        assert len(res) == 2 and res[1]["dx"].shape == (N,)
        sv.derivative_many(db=np.ones((2, M)), dA=np.ones((2, NNZ_A)))
        assert one(recorded) == ("scs_hip_derivative_full_batch", [21, 22], (every, NULL, every, NULL, every, every, every), 2)
    finally:
        sv._many = []
        forget(sv, clone)


def test_the_stubs_are_gone():
    assert isinstance(_scs_hip._lib.scs_hip_adjoint, ctypes._CFuncPtr)
    assert _scs_hip._lib.scs_hip_adjoint(None, None, None, None, None, None, None, None, None, None) == -1  # (the library again)
    assert "null workspace" in _scs_hip.last_error()
