"""The mirrored suites once more, under the policy a user gets: `LinearSolver.AUTO` as scs/__init__.py `_resolve_auto` resolves it
(the dense direct solver of the device for n <= 4096 when it fits, the indirect solver otherwise).

Everywhere else tests/conftest.py pins AUTO to the indirect module; this module carries the `auto_resolution` marker, so the pin
leaves it alone.  The test functions are the ones of the source modules, imported and collected here under a prefix (rc_, api_,
sp_, par_): their assertions are theirs, unchanged, and the source modules keep running pinned to the indirect path.

  rc_   tests/test_reference_cases_gpu.py   every test
  api_  tests/test_scs_api_gpu.py           every test but the two listed below
  sp_   tests/test_spectral_cones_gpu.py    the whole-solve tests: norm bounds, the solve that recovers the projection, the ell1 / LP
                                            and the standard-cone reformulations, bit identity of two solves, warm start and
                                            update, batch = separate solves, the refused limits, the largest accepted sizes (d = 64
                                            and sl = 64 go to the dense solver, n = 8193 of the two nuclear-norm cases does not),
                                            the row count; the reference's spectral cases are restated below without a solver name
  par_  tests/test_hip_parity.py            the whole-solve flows against the oracle's direct LDL' (feasible, infeasible, unbounded
                                            golden instances, generated LP+SOC / mixed-cone parity at rtol 1e-4 with eps 1e-9, the
                                            warm-start regression QP, bit determinism).  Those tests call the raw backend `hip.SCS`;
                                            here the `hip` fixture hands them `scs.SCS` with no solver named.
  and one concurrency scenario of AUTO-made workspaces on eight threads (after tests/test_concurrency_gpu.py).

Left out, and why:
  api_ test_sigint_stops_the_device_loop_with_status_interrupted[scs_solve, solve_batch]: its child process names
       LinearSolver.HIP_INDIRECT itself.
  sp_  test_reference_spectral_cases: parametrised over NAMED solvers (its `auto` id already carries auto_resolution); restated here.
  sp_  the kernel-level tests (test_kernel_projection_matches_reference, test_several_cones_of_every_kind_in_one_vector,
       test_cross_check_against_standard_hip_kernels): no solve, no linear solver.
  par_ test_iteration_counts_track_oracle_cg, test_determinism_bit_exact_with_P, test_kkt_solve_*, test_run_ahead_*,
       test_device_setup_*, test_full_solve_on_column_sorted_layouts, test_solve_with_dense_rows_*: they assert CG counters, CG
       layouts or the indirect KKT solve itself.
  par_ test_config1_lp_golden_*, test_psd_*, test_cs_*, test_random_mixed_cone_qp_sweep, test_psd_heavy_parity: sizes and cones
       tests/test_dense_gpu.py already runs through LinearSolver.HIP_DENSE by name, or n > 4096 (AUTO = indirect: nothing new).
  The parametrised ids that name a solver (rc_test_settings_keep_the_answer[linear_solver=hip_indirect],
  api_test_one_variable_lp_and_soc[hip_indirect]) run as they are; they do not count below.

Not vacuous: an autouse fixture records what `_resolve_auto` returned in every test and checks, on every `SCS.solve` of an
AUTO-made workspace with n <= 4096, that info["lin_sys_solver"] starts with "dense-direct".  The last test of the module asserts
that the dense direct module was chosen in at least MIN_DENSE_TESTS = 145 of its 153 tests (147 when this was written; four resolve to the indirect solver only: n = 8193 or more)."""
import collections
import gc
import threading

import numpy as np
import pytest

import test_hip_parity as _par
import test_reference_cases_gpu as _rc
import test_scs_api_gpu as _api
import test_spectral_cones_gpu as _sp

_OMIT = {
    "api": {"test_sigint_stops_the_device_loop_with_status_interrupted"},
}
_ONLY = {
    "sp": {"test_norm_bounds", "test_solve_recovers_the_projection", "test_ell1_agrees_with_its_lp_reformulation",
           "test_two_solves_are_bit_identical", "test_warm_start_and_update", "test_batch_equals_separate_solves",
           "test_limits_are_refused_with_a_reason", "test_largest_accepted_sizes_solve", "test_row_count_of_the_core",
           "test_spectral_cone_agrees_with_its_standard_reformulation"},
    "par": {"test_solve_feasible_golden", "test_solve_infeasible_golden", "test_solve_unbounded_golden", "test_lp_soc_generated_parity",
            "test_mixed_cones_generated_parity", "test_qp_with_P_parity", "test_determinism_bit_exact"},
}
for _prefix, _mod in (("rc", _rc), ("api", _api), ("sp", _sp), ("par", _par)):
    for _name, _obj in list(vars(_mod).items()):
        if not _name.startswith("test_") or not callable(_obj):
            continue
        if _name in _OMIT.get(_prefix, ()) or (_prefix in _ONLY and _name not in _ONLY[_prefix]):
            continue
        globals()["test_%s_%s" % (_prefix, _name[5:])] = _obj
for _prefix in _ONLY:
    assert all("test_%s_%s" % (_prefix, n[5:]) in globals() for n in _ONLY[_prefix]), _prefix

oracle = _par.oracle  # (module fixture of tests/test_hip_parity.py: the CPU checker)

# assigned AFTER the imports: this module's marks, not a source module's
pytestmark = [pytest.mark.gpu, pytest.mark.auto_resolution]

# tests in which AUTO must have chosen the dense direct module at least once (counted by the last test): the 61 + 24 + 50 + 17 ids
# of the four sources and the thread scenario (153) all go through calls that name no solver on problems with n <= 4096, except the
# two ids that name the indirect solver, the two largest nuclear-norm sizes (n = 8193) and the handful that only check rejected
# calls before a solver is chosen: 147 when this was written.  Of these, the tests that also SOLVE had lin_sys_solver checked.
MIN_DENSE_TESTS = 145
MIN_CHECKED_TESTS = 135

_CHOSEN = collections.defaultdict(list)     # test id -> [(n, module name)]
_CHECKED = collections.Counter()            # test id -> solves whose lin_sys_solver was checked


@pytest.fixture(scope="module")
def scs():
    import scs as _scs
    from scs import _scs_hip
    assert _scs_hip.device_count() > 0
    return _scs


class _Raw(object):
    """the raw backend call surface `SCS(shape, Ax, Ai, Ap, Px, Pi, Pp, b, c, cone, **settings)` over the public scs.SCS"""

    def __init__(self, shape, Ax, Ai, Ap, Px, Pi, Pp, b, c, cone, **settings):
        import scs as _scs
        from scipy import sparse
        data = {"A": sparse.csc_matrix((Ax, Ai, Ap), shape=shape), "b": b, "c": c}
        if Px is not None:
            data["P"] = sparse.csc_matrix((Px, Pi, Pp), shape=(shape[1], shape[1]))
        self._sv = _scs.SCS(data, cone, **settings)

    def solve(self, warm_start=True, x=None, y=None, s=None):
        return self._sv.solve(warm_start, x, y, s)

    def update(self, b=None, c=None):
        self._sv.update(b, c)


class _Hip(object):
    SCS = _Raw


@pytest.fixture(scope="module")
def hip():
    """what tests/test_hip_parity.py's whole-solve tests call as the backend: here the public front end, no solver named"""
    return _Hip


@pytest.fixture(autouse=True)
def _record_auto(request, monkeypatch):
    """records _resolve_auto's answers of this test; every solve of an AUTO-made workspace with n <= 4096 must report the dense
    direct linear solver"""
    import scs as _scs
    nodeid = request.node.nodeid
    tl = threading.local()
    orig_resolve, orig_init, orig_solve = _scs._resolve_auto, _scs.SCS.__init__, _scs.SCS.solve

    def resolve(m=None, n=None, A=None):
        mod = orig_resolve(m, n, A)
        _CHOSEN[nodeid].append((n, mod.__name__))
        tl.last = (n, mod.__name__)
        return mod

    def init(self, data, cone, **settings):
        tl.last = None
        orig_init(self, data, cone, **settings)
        self._auto_made = tl.last

    def solve(self, *args, **kwargs):
        sol = orig_solve(self, *args, **kwargs)
        made = getattr(self, "_auto_made", None)
        if made is not None and made[0] is not None and made[0] <= 4096:
            assert sol["info"]["lin_sys_solver"].startswith("dense-direct"), (made, sol["info"]["lin_sys_solver"])
            _CHECKED[nodeid] += 1
        return sol

    monkeypatch.setattr(_scs, "_resolve_auto", resolve)
    monkeypatch.setattr(_scs.SCS, "__init__", init)
    monkeypatch.setattr(_scs.SCS, "solve", solve)
    yield
    gc.collect()


# ---------------------------------------------------------------- the reference's spectral cases, no solver named
@pytest.mark.parametrize("seed,cone,max_iters", _sp.REF_CASES, ids=[str(c[0]) for c in _sp.REF_CASES])
def test_sp_reference_spectral_cases_default_solver(scs, seed, cone, max_iters):
    data = _sp._gen_feasible_qp(cone, np.random.RandomState(seed))
    kw = {"max_iters": max_iters} if max_iters else {}
    sol = scs.solve(data, cone, verbose=False, **kw)
    assert sol["info"]["status_val"] in (1, 2), sol["info"]["status"]
    assert sol["info"]["lin_sys_solver"].startswith("dense-direct"), sol["info"]["lin_sys_solver"]


# ---------------------------------------------------------------- AUTO-made workspaces on several threads
def test_auto_made_workspaces_on_eight_threads(scs, oracle):
    """eight threads, each with problems of its own (LP, SOCP, a larger LP, the config-5 shape), built and solved through
    scs.SCS with no solver named: every thread gets the bits of a solve made alone, and the answer of the oracle's direct LDL'
    within rtol 1e-4 at eps 1e-9 (the bound of tests/test_dense_gpu.py and of smoke())."""
    import problem_gen as pg
    import test_concurrency_gpu as cc
    stg = dict(eps_abs=1e-9, eps_rel=1e-9, verbose=False)
    probs = []
    for t in range(8):
        if t % 4 == 0:
            data, K = cc._make_larger_lp(n=20 + t, seed=42 + t)
        elif t % 4 == 1:
            K = {"l": 200 + 10 * t, "q": [10] * 12}
            data = pg.gen_feasible_qp(K, 150 + t, 10, 70 + t, lambda z, K: oracle.proj_cone(z, K, dual=True))[0]
        elif t % 4 == 2:
            K = {"z": 5, "l": 100, "q": [6, 9], "ep": 4, "ed": 3, "p": [0.3, -0.6]}
            data = pg.gen_feasible_qp(K, 90 + t, 8, 80 + t, lambda z, K: oracle.proj_cone(z, K, dual=True))[0]
        else:
            K = {"l": 150, "q": [8] * 5, "s": [6, 4]}
            data = pg.gen_feasible_qp(K, 120 + t, 8, 90 + t, lambda z, K: oracle.proj_cone(z, K, dual=True))[0]
        probs.append((data, K))
    solo = [scs.SCS(d, K, **stg).solve(warm_start=False) for d, K in probs]
    got = [None] * 8

    def worker(t):
        def run():
            d, K = probs[t]
            for _ in range(3):
                got[t] = scs.SCS(d, K, **stg).solve(warm_start=False)
        return run

    cc._run_threads([worker(t) for t in range(8)], timeout=100)
    import helpers
    refs = helpers.oracle_solve_many(oracle, [(d, K, dict(stg, indirect=False)) for d, K in probs])
    for t in range(8):
        assert got[t]["info"]["lin_sys_solver"].startswith("dense-direct")
        cc._same_bits(got[t], solo[t], "thread %d" % t)
        assert got[t]["info"]["status"] == "solved" and refs[t]["info"]["status"] == "solved", (t, got[t]["info"], refs[t]["info"])
        if "P" in probs[t][0]:      # (strictly convex: x, y, s unique; the LP of t % 4 == 0 is pinned by its optimal value)
            for key in ("x", "y", "s"):
                np.testing.assert_allclose(got[t][key], refs[t][key], rtol=1e-4, atol=1e-4 * np.abs(refs[t][key]).max(),
                                           err_msg="thread %d %s" % (t, key))
        else:
            assert abs(got[t]["info"]["pobj"] - refs[t]["info"]["pobj"]) <= 1e-6 * max(1.0, abs(refs[t]["info"]["pobj"]))


# ---------------------------------------------------------------- last: how many tests really ran the dense direct solver
def test_zz_dense_direct_was_chosen_as_often_as_claimed():
    dense = sorted(t for t, picks in _CHOSEN.items() if any(name.endswith("_scs_hip_dense") for _, name in picks))
    indirect_only = sorted(t for t, picks in _CHOSEN.items() if not any(name.endswith("_scs_hip_dense") for _, name in picks))
    checked = sum(1 for t in dense if _CHECKED[t] > 0)
    print("AUTO resolved to the dense direct solver in %d tests (%d of them had lin_sys_solver checked on a solve); "
          "to the indirect solver only in %d: %s" % (len(dense), checked, len(indirect_only), indirect_only))
    assert len(dense) >= MIN_DENSE_TESTS, (len(dense), MIN_DENSE_TESTS)
    assert checked >= MIN_CHECKED_TESTS, checked
