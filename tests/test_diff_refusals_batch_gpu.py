"""A batch derivative entry refuses a member in the words of the member's own call: the message of `adjoint_batch` / `derivative_batch`
for an offending member is the message of `adjoint` / `derivative` on that solver with the entry's name replaced and "member i: "
inserted after it (csrc/scs_hip.hip: both entries run one refusal ladder, diff_check).  No device work precedes a refusal, so the
other member stays usable.

The refusals are the ones Python can reach: no solve yet, a stale solution, a solve that did not end solved, a cone without a
derivative.  A solve stopped by a small `max_iters` does not give the third: it ends "solved (inaccurate - reached max_iters)" (checked
for max_iters = 1, 2, 3, 5, 10, 20 on the problem below), which the library differentiates; the case uses an infeasible LP, as
tests/test_adjoint_gpu.py does."""
import gc

import numpy as np
import pytest
from scipy import sparse

import adjoint_ref as ar
import problem_gen as pg

import scs
from scs import _scs_hip

pytestmark = pytest.mark.gpu

IND = scs.LinearSolver.HIP_INDIRECT
STG = dict(eps_abs=1e-7, eps_rel=1e-7, verbose=False, max_iters=100000)
_good = []


def make_qp():
    return ar.gen_problem(13, n=12, z=2, l=5, tight_l=2, q=(3, 4, 6), q_case=("polar", "bd", "in"), with_P=True)


def qp_solver():
    p = make_qp()
    return scs.SCS(ar.data_of(p), p["cone"], linear_solver=IND, **STG), p


@pytest.fixture(scope="module", autouse=True)
def _finish_cached_solvers():
    """the solver this module solves once and shares is finished with it (the block pool's account is an invariant of
    tests/test_pool_lifecycle_gpu.py)"""
    def in_use():
        st = _scs_hip.pool_stats()
        return st["live_bytes"] - st["held_bytes"]
    before = in_use()
    yield
    _good.clear()
    gc.collect()
    assert in_use() <= before, (in_use(), before)


def good():
    if not _good:
        sv, _ = qp_solver()
        assert sv.solve(warm_start=False)["info"]["status"] == "solved"
        _good.append(sv)
    return _good[0]


def never_solved():
    return qp_solver()[0]


def stale():
    sv, p = qp_solver()
    assert sv.solve(warm_start=False)["info"]["status"] == "solved"
    sv.update(b=p["b"].copy())
    return sv


def not_solved():
    sv = scs.SCS({"A": sparse.csc_matrix(np.array([[-1.0], [1.0]])), "b": np.array([-1.0, 0.0]), "c": np.array([1.0])}, {"l": 2},
                 linear_solver=IND, **STG)
    assert sv.solve(warm_start=False)["info"]["status"] == "infeasible"
    return sv


def exp_cone():
    K = {"l": 2, "ep": 1}
    data, _, _ = pg.gen_feasible(K, 3, 2, 5, lambda z, cone: _scs_hip.proj_cone(z, cone, dual=True))
    sv = scs.SCS(data, K, linear_solver=IND, **STG)
    assert sv.solve(warm_start=False)["info"]["status"] == "solved"
    return sv


CASES = {"no_solve": (never_solved, "no solve yet"), "stale": (stale, "the resident solution is stale"),
         "not_solved": (not_solved, "the last solve did not end solved (status -2)"), "unsupported_cone": (exp_cone, "exponential (ep) cone")}
ENTRIES = {"adjoint": (lambda sv: sv.adjoint(), lambda svs: scs.adjoint_batch(svs)),
           "derivative": (lambda sv: sv.derivative(), lambda svs: scs.derivative_batch(svs))}


def refusal(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_batch_refuses_a_member_in_the_words_of_its_own_call(case):
    make, words = CASES[case]
    ok, bad = good(), make()
    gx = np.linspace(-1.0, 1.0, 12)  # (n = 12)
    before = ok.adjoint(dx=gx)
    for entry, (single, batch) in sorted(ENTRIES.items()):
        own = refusal(lambda: single(bad))
        head = "libscs_hip: scs_hip_%s: " % entry
        print(case, entry, "|", own)
        assert own.startswith(head) and words in own, own
        got = refusal(lambda: batch([ok, bad]))
        print(case, entry + "_batch", "|", got)
        assert got == "libscs_hip: scs_hip_%s_batch: member 1: " % entry + own[len(head):]
    # nothing ran: the other member is differentiated as before
    after = ok.adjoint(dx=gx)
    assert after["info"]["iters"] == before["info"]["iters"] >= 1
    assert np.array_equal(after["db"], before["db"]) and np.array_equal(after["dc"], before["dc"])
