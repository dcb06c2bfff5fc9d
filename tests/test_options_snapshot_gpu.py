"""GPU tests of the per-workspace options snapshot (csrc/options.hpp; csrc/work.hpp MatrixSet::opt / ScsHipWork::opt).

A workspace keeps the SCS_HIP_* options it was created under for its whole life, its clones inherit them, and nothing that happens to
the environment or to the process-global options afterwards — a setenv, another scs_init, on this thread or another — reaches a
solve.  Every test compares bits only: workspaces created under "environment X"

    SCS_HIP_PSD_TOL=fixed   read at every iteration of a solve        (work.hpp psd_tol2_of)
    SCS_HIP_AA=gram         read when the Anderson workspace is made  (aa.hpp DeviceAa::init: scs_init AND scs_hip_clone)
    SCS_HIP_PSD_SPLIT=1     read when the cone metadata is uploaded   (setup.hpp upload_cone_meta: scs_init AND scs_hip_clone)
    SCS_HIP_PSD_REFINE=0    read by the PSD pipeline                  (work.hpp launch_psd)

must reproduce the solve of a workspace that was created AND solved under X, whatever the environment says when they solve or are
cloned.  The instance: LP rows + one PSD cone of order 40 (the block / split kernels) + one of order 12 (the small-matrix kernel),
30 variables, max_iters fixed so that no solve depends on convergence, default Anderson acceleration (lookback 10: extrapolations
from iteration 10 on).  On this instance the default environment gives other bits than X (asserted: without that the tests would
prove nothing)."""
import threading

import numpy as np
import pytest

import problem_gen as pg

pytestmark = pytest.mark.gpu

ENV_X = {"SCS_HIP_PSD_TOL": "fixed", "SCS_HIP_AA": "gram", "SCS_HIP_PSD_SPLIT": "1", "SCS_HIP_PSD_REFINE": "0"}
K = {"l": 20, "s": [40, 12]}
N_VARS = 30
STG = dict(verbose=False, max_iters=60, eps_abs=1e-12, eps_rel=1e-12)
STG_LONG = dict(STG, max_iters=300)


def _proj(z, cone):
    from scs import _scs_hip
    return _scs_hip.proj_cone(z, cone, dual=True)


def _set_x(monkeypatch):
    for k, v in ENV_X.items():
        monkeypatch.setenv(k, v)


def _unset_x(monkeypatch):
    for k in ENV_X:
        monkeypatch.delenv(k, raising=False)


def _new(data, **stg):
    import scs
    return scs.SCS(data, K, linear_solver=scs.LinearSolver.HIP_INDIRECT, **stg)


def _publish_other_options():
    """a throw-away workspace: scs_init re-reads the environment and publishes it as the process-global options"""
    import scs
    from scipy import sparse
    lp = {"A": sparse.identity(3, format="csc"), "b": np.ones(3), "c": -np.ones(3)}
    scs.SCS(lp, {"l": 3}, linear_solver=scs.LinearSolver.HIP_INDIRECT, verbose=False, max_iters=5)


def _same_bits(got, want, tag):
    for key in ("x", "y", "s"):
        assert np.array_equal(got[key], want[key], equal_nan=True), "%s: %s differs (max |d| = %g)" % (
            tag, key, np.nanmax(np.abs(got[key] - want[key])))
    assert got["info"]["iter"] == want["info"]["iter"], tag


_REF = {}


def _case(monkeypatch):
    """the instance, two more feasible (b, c) pairs over its matrix and the under-X answers — computed once, shared, never changed"""
    if not _REF:
        data, _, _ = pg.gen_feasible(K, N_VARS, 8, 4242, _proj)
        rng = np.random.default_rng(77)
        A = data["A"]
        pairs = []
        for _ in range(2):
            z = rng.standard_normal(A.shape[0])
            y = np.asarray(_proj(z, K), dtype=np.float64)
            x = rng.standard_normal(A.shape[1])
            pairs.append((A @ x + (y - z), -(A.T @ y)))
        _set_x(monkeypatch)
        want = _new(data, **STG).solve(warm_start=False)
        want_long = _new(data, **STG_LONG).solve(warm_start=False)
        # solve_many's member 0 is the workspace itself, which has solved once by then, member 1 a clone made for the call.  A cold
        # solve of a workspace that solved before still starts its eigen-solves from the eigenvectors the last one left (psd.hpp
        # psd_warm), so the reference of member 0 has the same history: created under X, solved once, updated, solved
        want_pairs = []
        for i, (b, c) in enumerate(pairs):
            sv = _new(data, **STG)
            if i == 0:
                sv.solve(warm_start=False)
            sv.update(b, c)
            want_pairs.append(sv.solve(warm_start=False))
        _unset_x(monkeypatch)
        dflt = _new(data, **STG).solve(warm_start=False)
        _REF.update(data=data, pairs=pairs, want=want, want_long=want_long, want_pairs=want_pairs, dflt=dflt)
    return _REF


def test_default_environment_gives_other_bits(monkeypatch):
    """the premise of every test below: on this instance X is visible in the bits of x"""
    ref = _case(monkeypatch)
    assert ref["want"]["info"]["iter"] == STG["max_iters"] == ref["dflt"]["info"]["iter"]  # (nothing stopped early)
    assert not np.array_equal(ref["want"]["x"], ref["dflt"]["x"])


def test_solve_clone_and_solve_many_keep_the_options_of_creation(monkeypatch):
    ref = _case(monkeypatch)
    _set_x(monkeypatch)
    a = _new(ref["data"], **STG)
    _unset_x(monkeypatch)
    _publish_other_options()
    # a solve re-reads nothing (the per-iteration PSD stopping level above all)
    _same_bits(a.solve(warm_start=False), ref["want"], "solve after the environment changed")
    # a clone is its parent's workspace again: Anderson factorisation, PSD pipeline and refinement as the parent was created with
    b = a.clone()
    _same_bits(b.solve(warm_start=False), ref["want"], "clone made after the environment changed")
    # solve_many makes its clones now, and its batch call refreshes the global options: the members still are X workspaces
    bs = np.stack([p[0] for p in ref["pairs"]])
    cs = np.stack([p[1] for p in ref["pairs"]])
    for i, (got, want) in enumerate(zip(a.solve_many(bs, cs), ref["want_pairs"])):
        _same_bits(got, want, "solve_many member %d" % i)


def test_solve_is_unmoved_by_another_thread_creating_workspaces(monkeypatch):
    """one thread solves an X workspace while this thread keeps changing SCS_HIP_PSD_TOL and creating workspaces (each scs_init publishes
    new global options) until that solve returns"""
    ref = _case(monkeypatch)
    _set_x(monkeypatch)
    a = _new(ref["data"], **STG_LONG)
    out = {}

    def run():
        try:
            out["sol"] = a.solve(warm_start=False)
        except BaseException as e:  # noqa: BLE001  (re-raised below, on the main thread)
            out["err"] = e

    t = threading.Thread(target=run)
    t.start()
    flip = 0
    while t.is_alive():
        flip ^= 1
        if flip:
            monkeypatch.delenv("SCS_HIP_PSD_TOL", raising=False)
        else:
            monkeypatch.setenv("SCS_HIP_PSD_TOL", "fixed")
        _publish_other_options()  # (one other workspace alive at a time: it is gone when the call returns)
    t.join()
    if "err" in out:
        raise out["err"]
    _same_bits(out["sol"], ref["want_long"], "solve under concurrent scs_init")
