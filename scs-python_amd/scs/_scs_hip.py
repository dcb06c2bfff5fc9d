"""scs._scs_hip — the MI355X (gfx950) backend module selected by
``LinearSolver.HIP_INDIRECT``.

It is the counterpart of one of the reference's per-backend CPython extension
modules (R:scs/scspy.c, R:scs/scsmodule.h, R:scs/scsobject.h — compiled once per
backend, R:meson.build:238-391).  Same module surface:

* ``version()``, ``sizeof_int()``, ``sizeof_float()``         (R:scs/scsmodule.h:16-23)
* type ``SCS(shape, Ax, Ai, Ap, Px, Pi, Pp, b, c, cone, **settings)`` with
  ``solve(warm_start, x, y, s)`` and ``update(b, c)``          (R:scs/scsobject.h:442-1225)

The reference glue is C against the CPython API; this one is Python over the
C-ABI of ``libscs_hip.so`` (include/scs_hip.h) via ctypes.  ctypes drops the GIL
for the duration of every foreign call, which reproduces the reference's
``Py_BEGIN_ALLOW_THREADS`` around scs_init/scs_solve/scs_update
(R:scs/scsobject.h:902-905,984-987,1216-1219); a per-instance lock protects
work/sol exactly as there (:892-899).

There is NO CPU fallback: if the shared library or a GPU is missing this module
raises (ImportError at import for a missing library; ValueError("ScsWork
allocation error!") from the constructor when no device is usable).
"""
import collections
import contextlib
import functools
import ctypes as C
import importlib.util
import operator
import os
import threading
import warnings

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libscs_hip.so"

c_int, c_dbl = C.c_int, C.c_double
_PI, _PD = C.POINTER(c_int), C.POINTER(c_dbl)


# ---------------------------------------------------------------- C structs (include/scs_types.h)
class _ScsMatrix(C.Structure):
    _fields_ = [("x", _PD), ("i", _PI), ("p", _PI), ("m", c_int), ("n", c_int)]


class _ScsData(C.Structure):
    _fields_ = [("m", c_int), ("n", c_int), ("A", C.POINTER(_ScsMatrix)),
                ("P", C.POINTER(_ScsMatrix)), ("b", _PD), ("c", _PD)]


class _ScsCone(C.Structure):
    _fields_ = [("z", c_int), ("l", c_int), ("bu", _PD), ("bl", _PD), ("bsize", c_int),
                ("q", _PI), ("qsize", c_int), ("s", _PI), ("ssize", c_int),
                ("cs", _PI), ("cssize", c_int), ("ep", c_int), ("ed", c_int),
                ("p", _PD), ("psize", c_int),
                # spectral cones (include/scs_types.h under USE_SPECTRAL_CONES; the *_spectral entry points read them)
                ("d", _PI), ("dsize", c_int), ("nuc_m", _PI), ("nuc_n", _PI), ("nucsize", c_int),
                ("ell1", _PI), ("ell1_size", c_int), ("sl_n", _PI), ("sl_k", _PI), ("sl_size", c_int)]


class _ScsSettings(C.Structure):
    _fields_ = [("normalize", c_int), ("scale", c_dbl), ("adaptive_scale", c_int),
                ("rho_x", c_dbl), ("max_iters", c_int), ("eps_abs", c_dbl),
                ("eps_rel", c_dbl), ("eps_infeas", c_dbl), ("alpha", c_dbl),
                ("time_limit_secs", c_dbl), ("verbose", c_int), ("warm_start", c_int),
                ("acceleration_lookback", c_int), ("acceleration_interval", c_int),
                ("acceleration_type_1", c_int), ("acceleration_regularization", c_dbl),
                ("acceleration_relaxation", c_dbl), ("write_data_filename", C.c_char_p),
                ("log_csv_filename", C.c_char_p)]


class _ScsSolution(C.Structure):
    _fields_ = [("x", _PD), ("y", _PD), ("s", _PD)]


class _ScsAaStats(C.Structure):
    _fields_ = [("iter", c_int), ("n_accept", c_int), ("n_reject_lapack", c_int),
                ("n_reject_rank0", c_int), ("n_reject_nonfinite", c_int),
                ("n_reject_weight_cap", c_int), ("n_safeguard_reject", c_int),
                ("last_rank", c_int), ("last_aa_norm", c_dbl), ("last_regularization", c_dbl)]


class _ScsInfo(C.Structure):
    _fields_ = [("iter", c_int), ("status", C.c_char * 128), ("lin_sys_solver", C.c_char * 128),
                ("status_val", c_int), ("scale_updates", c_int), ("pobj", c_dbl), ("dobj", c_dbl),
                ("res_pri", c_dbl), ("res_dual", c_dbl), ("gap", c_dbl), ("res_infeas", c_dbl),
                ("res_unbdd_a", c_dbl), ("res_unbdd_p", c_dbl), ("comp_slack", c_dbl),
                ("setup_time", c_dbl), ("solve_time", c_dbl), ("scale", c_dbl),
                ("lin_sys_time", c_dbl), ("cone_time", c_dbl), ("accel_time", c_dbl),
                ("rejected_accel_steps", c_int), ("accepted_accel_steps", c_int),
                ("aa_stats", _ScsAaStats), ("cg_iters", c_int)]


class _ScsHipDiffOpts(C.Structure):
    _fields_ = [("tol", c_dbl), ("max_iters", c_int)]


class _ScsHipDiffInfo(C.Structure):
    _fields_ = [("iters", c_int), ("residual", c_dbl), ("normal_residual", c_dbl), ("stop", c_int), ("time_ms", c_dbl)]


class _ScsHipRefineOpts(C.Structure):
    _fields_ = [("tol", c_dbl), ("max_steps", c_int), ("lsqr_tol", c_dbl), ("lsqr_max_iters", c_int)]


class _ScsHipRefineInfo(C.Structure):
    _fields_ = [("steps", c_int), ("halvings", c_int), ("lsqr_iters", c_int), ("stop", c_int),
                ("merit_before", c_dbl), ("merit_after", c_dbl), ("res_pri_before", c_dbl), ("res_dual_before", c_dbl),
                ("gap_before", c_dbl), ("res_pri", c_dbl), ("res_dual", c_dbl), ("gap", c_dbl), ("pobj", c_dbl), ("dobj", c_dbl),
                ("time_ms", c_dbl)]


class _ScsHipPoolStats(C.Structure):
    _fields_ = [("held_bytes", C.c_size_t), ("held_blocks", C.c_size_t), ("live_bytes", C.c_size_t),
                ("hits", C.c_size_t), ("misses", C.c_size_t)]


# ---------------------------------------------------------------- library loading
def _preload_hip_runtime():
    """Make sure exactly ONE HIP runtime ends up in the process.

    PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7,
    same as /opt/rocm's).  If libscs_hip.so pulled in the system copy first and
    torch were imported afterwards, torch would load its bundled copy too (it asks
    for the un-versioned file name) and the process would hold two runtimes.
    Preloading torch's copy (without importing torch) makes both resolve to it.
    SCS_HIP_RUNTIME=system skips this.
    """
    if os.environ.get("SCS_HIP_RUNTIME", "torch") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def _runtime_env():
    """Runtime configuration that must be in the environment BEFORE the HIP runtime reads its flags (csrc/runtime.hpp
    scs_hip_runtime_env has the measurements): keep the runtime from pinning the caller's pageable arrays for host <->
    device copies — the driver evicts the process's queues for 30-80 ms some time after such pages are released.
    An existing value wins; SCS_HIP_RUNTIME_ENV=0 leaves the environment alone."""
    if os.environ.get("SCS_HIP_RUNTIME_ENV", "1") != "0":
        os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "1000000")


def _load():
    _runtime_env()
    path = os.environ.get("SCS_HIP_LIB") or os.path.join(_HERE, _LIB_NAME)   # (SCS_HIP_LIB: an alternative build of the library, A/B labs)
    if not os.path.exists(path):
        raise ImportError(
            "scs._scs_hip: %s is not built (run `python __graft_entry__.py` / "
            "`make -C scs-python_amd`); this backend has no CPU fallback" % path)
    _preload_hip_runtime()
    try:
        lib = C.CDLL(path)
    except OSError as e:  # missing ROCm runtime etc.
        raise ImportError("scs._scs_hip: cannot load %s: %s" % (path, e))
    lib.scs_init.restype = C.c_void_p
    lib.scs_init.argtypes = [C.POINTER(_ScsData), C.POINTER(_ScsCone), C.POINTER(_ScsSettings)]
    lib.scs_hip_init_linsys.restype = C.c_void_p
    lib.scs_hip_init_linsys.argtypes = [C.POINTER(_ScsData), C.POINTER(_ScsCone), C.POINTER(_ScsSettings), c_int]
    lib.scs_init_spectral.restype = C.c_void_p
    lib.scs_init_spectral.argtypes = [C.POINTER(_ScsData), C.POINTER(_ScsCone), C.POINTER(_ScsSettings)]
    lib.scs_hip_init_linsys_spectral.restype = C.c_void_p
    lib.scs_hip_init_linsys_spectral.argtypes = [C.POINTER(_ScsData), C.POINTER(_ScsCone), C.POINTER(_ScsSettings), c_int]
    lib.scs_hip_proj_cone_spectral.restype = c_int
    lib.scs_hip_proj_cone_spectral.argtypes = [_PD, C.POINTER(_ScsCone), c_int, c_int]
    lib.scs_hip_linsys_kind.restype = c_int
    lib.scs_hip_linsys_kind.argtypes = [C.c_void_p]
    lib.scs_hip_kkt_solve_dense.restype = c_int
    lib.scs_hip_kkt_solve_dense.argtypes = [C.POINTER(_ScsMatrix), C.POINTER(_ScsMatrix), _PD, _PD]
    lib.scs_solve.restype = c_int
    lib.scs_solve.argtypes = [C.c_void_p, C.POINTER(_ScsSolution), C.POINTER(_ScsInfo), c_int]
    lib.scs_hip_solve_batch.restype = c_int
    lib.scs_hip_solve_batch.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.POINTER(_ScsSolution)),
                                        C.POINTER(C.POINTER(_ScsInfo)), c_int, c_int]
    lib.scs_hip_batch_plan.restype = c_int
    lib.scs_hip_batch_plan.argtypes = [C.POINTER(C.c_void_p), c_int, C.POINTER(c_int)]
    lib.scs_hip_clone.restype = C.c_void_p
    lib.scs_hip_clone.argtypes = [C.c_void_p]
    lib.scs_hip_shares_matrix.restype = c_int
    lib.scs_hip_shares_matrix.argtypes = [C.c_void_p, C.c_void_p]
    lib.scs_update.restype = c_int
    lib.scs_update.argtypes = [C.c_void_p, _PD, _PD]
    lib.scs_finish.restype = None
    lib.scs_finish.argtypes = [C.c_void_p]
    lib.scs_set_default_settings.restype = None
    lib.scs_set_default_settings.argtypes = [C.POINTER(_ScsSettings)]
    lib.scs_version.restype = C.c_char_p
    lib.scs_sizeof_int.restype = C.c_size_t
    lib.scs_sizeof_float.restype = C.c_size_t
    lib.scs_hip_device_count.restype = c_int
    lib.scs_hip_set_device.restype = c_int
    lib.scs_hip_set_device.argtypes = [c_int]
    lib.scs_hip_labs_build.restype = c_int
    lib.scs_hip_mem_info.restype = c_int
    lib.scs_hip_mem_info.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.scs_hip_set_thread_device.restype = c_int
    lib.scs_hip_set_thread_device.argtypes = [c_int]
    lib.scs_hip_last_error.restype = C.c_char_p
    lib.scs_hip_spmv.restype = c_int
    lib.scs_hip_spmv.argtypes = [C.POINTER(_ScsMatrix), _PD, _PD, c_int]
    lib.scs_hip_cs_layout_host_spmv.restype = c_int
    lib.scs_hip_cs_layout_host_spmv.argtypes = [C.POINTER(_ScsMatrix), _PD, _PD, c_int, c_int, c_int]
    lib.scs_hip_spmv_bench.restype = c_dbl
    lib.scs_hip_spmv_bench.argtypes = [C.POINTER(_ScsMatrix), c_int, c_int]
    lib.scs_hip_proj_cone.restype = c_int
    lib.scs_hip_proj_cone.argtypes = [_PD, C.POINTER(_ScsCone), c_int, c_int]
    lib.scs_hip_proj_cone_seq.restype = c_int
    lib.scs_hip_proj_cone_seq.argtypes = [_PD, C.POINTER(_ScsCone), c_int, c_int, c_int, _PD, c_int]
    lib.scs_hip_kkt_solve.restype = c_int
    lib.scs_hip_kkt_solve.argtypes = [C.POINTER(_ScsMatrix), C.POINTER(_ScsMatrix), _PD, _PD, c_dbl, _PI]
    lib.scs_hip_normalize.restype = c_int
    lib.scs_hip_normalize.argtypes = [C.POINTER(_ScsMatrix), C.POINTER(_ScsMatrix), _PD, _PD,
                                      C.POINTER(_ScsCone), _PD, _PD, _PD]
    lib.scs_hip_normalize_spectral.restype = c_int
    lib.scs_hip_normalize_spectral.argtypes = lib.scs_hip_normalize.argtypes
    lib.scs_hip_set_profiling.restype = None
    lib.scs_hip_set_profiling.argtypes = [C.c_void_p, c_int]
    lib.scs_hip_kernel_times.restype = None
    lib.scs_hip_kernel_times.argtypes = [C.c_void_p, _PD]
    lib.scs_hip_solution_to_device.restype = c_int
    lib.scs_hip_solution_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.scs_hip_update_device.restype = c_int
    lib.scs_hip_update_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.scs_hip_update_matrix.restype = c_int
    lib.scs_hip_update_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.scs_hip_update_matrix_device.restype = c_int
    lib.scs_hip_update_matrix_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.scs_hip_solve_device.restype = c_int
    lib.scs_hip_solve_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_ScsInfo), c_int]
    lib.scs_hip_solve_batch_device.restype = c_int
    lib.scs_hip_solve_batch_device.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                               C.POINTER(C.POINTER(_ScsInfo)), c_int, c_int]
    for name in ("scs_hip_adjoint", "scs_hip_adjoint_device"):
        fn = getattr(lib, name)
        fn.restype = c_int
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 7 + [C.POINTER(_ScsHipDiffOpts), C.POINTER(_ScsHipDiffInfo)]
    for name in ("scs_hip_derivative", "scs_hip_derivative_device"):
        fn = getattr(lib, name)
        fn.restype = c_int
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.POINTER(_ScsHipDiffOpts), C.POINTER(_ScsHipDiffInfo)]
    for name in ("scs_hip_derivative_full", "scs_hip_derivative_full_device"):
        fn = getattr(lib, name)
        fn.restype = c_int
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 7 + [C.POINTER(_ScsHipDiffOpts), C.POINTER(_ScsHipDiffInfo)]
    for name in ("scs_hip_data_perturbation", "scs_hip_data_perturbation_device"):
        fn = getattr(lib, name)
        fn.restype = c_int
        fn.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    _PV = C.POINTER(C.c_void_p)
    for fn in (lib.scs_hip_derivative_full_batch, lib.scs_hip_derivative_full_batch_device):
        fn.restype = c_int
        fn.argtypes = [_PV] + [_PV] * 7 + [C.POINTER(_ScsHipDiffOpts), C.POINTER(C.POINTER(_ScsHipDiffInfo)), c_int]
    for fn in (lib.scs_hip_adjoint_batch, lib.scs_hip_adjoint_batch_device):
        fn.restype = c_int
        fn.argtypes = [_PV] + [_PV] * 7 + [C.POINTER(_ScsHipDiffOpts), C.POINTER(C.POINTER(_ScsHipDiffInfo)), c_int]
    for fn in (lib.scs_hip_adjoint_shared, lib.scs_hip_adjoint_shared_device):  # (the two sums: one vector each, not an array of them)
        fn.restype = c_int
        fn.argtypes = [_PV] + [_PV] * 5 + [C.c_void_p] * 2 + [C.POINTER(_ScsHipDiffOpts), C.POINTER(C.POINTER(_ScsHipDiffInfo)), c_int]
    lib.scs_hip_grad_matrix_sum.restype = c_int
    lib.scs_hip_grad_matrix_sum.argtypes = [c_int, c_int, _PI, _PI, _PI, _PI, c_int, _PD, _PD, _PD, _PD, _PD, _PD]
    for fn in (lib.scs_hip_derivative_batch, lib.scs_hip_derivative_batch_device):
        fn.restype = c_int
        fn.argtypes = [_PV] + [_PV] * 5 + [C.POINTER(_ScsHipDiffOpts), C.POINTER(C.POINTER(_ScsHipDiffInfo)), c_int]
    lib.scs_hip_diff_batch_plan.restype = c_int
    lib.scs_hip_diff_batch_plan.argtypes = [_PV, c_int, c_int, c_int, C.POINTER(c_int)]
    lib.scs_hip_diff_group_launches.restype = C.c_long
    lib.scs_hip_diff_group_launches.argtypes = []
    for name, slots in (("scs_hip_adjoint_multi", 7), ("scs_hip_derivative_multi", 5)):  # (infos: an array of K, not one)
        for fn in (getattr(lib, name), getattr(lib, name + "_device")):
            fn.restype = c_int
            fn.argtypes = [C.c_void_p, c_int] + [C.c_void_p] * slots + [C.POINTER(_ScsHipDiffOpts), C.POINTER(_ScsHipDiffInfo)]
    for fn in (lib.scs_hip_refine, lib.scs_hip_refine_device):
        fn.restype = c_int
        fn.argtypes = [C.c_void_p, C.POINTER(_ScsSolution), C.POINTER(_ScsHipRefineOpts), C.POINTER(_ScsHipRefineInfo)]
    for fn in (lib.scs_hip_refine_batch, lib.scs_hip_refine_batch_device):
        fn.restype = c_int
        fn.argtypes = [_PV, C.POINTER(C.POINTER(_ScsSolution)), C.POINTER(_ScsHipRefineOpts), C.POINTER(C.POINTER(_ScsHipRefineInfo)), c_int]
    lib.scs_hip_diff_group_syncs.restype = C.c_long
    lib.scs_hip_diff_group_syncs.argtypes = []
    lib.scs_hip_diff_lane_tile.restype = C.c_int
    lib.scs_hip_diff_lane_tile.argtypes = [C.c_int]
    lib.scs_hip_dproj_cone.restype = c_int
    lib.scs_hip_dproj_cone.argtypes = [_PD, _PD, C.POINTER(_ScsCone), c_int, _PD, _PD]
    lib.scs_hip_work_device.restype = c_int
    lib.scs_hip_work_device.argtypes = [C.c_void_p]
    lib.scs_hip_set_mark.restype = None
    lib.scs_hip_set_mark.argtypes = [C.c_void_p, c_int]
    lib.scs_hip_get_mark.restype = None
    lib.scs_hip_get_mark.argtypes = [C.c_void_p, _PD]
    lib.scs_hip_time_psd.restype = c_int
    lib.scs_hip_time_psd.argtypes = [C.c_void_p, c_int, _PD]
    lib.scs_hip_time_dproj.restype = c_int
    lib.scs_hip_time_dproj.argtypes = [C.c_void_p, c_int, _PD]
    lib.scs_hip_trim_pool.restype = None
    lib.scs_hip_trim_pool.argtypes = []
    lib.scs_hip_pool_stats.restype = None
    lib.scs_hip_pool_stats.argtypes = [C.POINTER(_ScsHipPoolStats)]
    lib.scs_hip_tiled_launches.restype = C.c_long
    lib.scs_hip_tiled_launches.argtypes = []
    lib.scs_hip_spin_fallbacks.restype = C.c_long
    lib.scs_hip_spin_fallbacks.argtypes = []
    lib.scs_hip_psd_refine_stats.restype = c_int
    lib.scs_hip_psd_refine_stats.argtypes = [C.c_void_p, _PD, c_int]
    lib.scs_hip_time_matvec.restype = c_int
    lib.scs_hip_time_matvec.argtypes = [C.c_void_p, c_int, _PD]
    lib.scs_hip_copy_bandwidth.restype = c_dbl
    lib.scs_hip_copy_bandwidth.argtypes = [C.c_size_t, c_int]
    lib.scs_hip_aa_init.restype = C.c_void_p
    lib.scs_hip_aa_init.argtypes = [c_int, c_int, c_int, c_dbl, c_dbl, c_dbl, c_dbl]
    lib.scs_hip_aa_apply.restype = c_dbl
    lib.scs_hip_aa_apply.argtypes = [C.c_void_p, _PD, _PD]
    lib.scs_hip_aa_safeguard.restype = c_int
    lib.scs_hip_aa_safeguard.argtypes = [C.c_void_p, _PD, _PD]
    lib.scs_hip_aa_reset.restype = None
    lib.scs_hip_aa_reset.argtypes = [C.c_void_p]
    lib.scs_hip_aa_get_stats.restype = None
    lib.scs_hip_aa_get_stats.argtypes = [C.c_void_p, C.POINTER(_ScsAaStats)]
    lib.scs_hip_aa_last_gamma.restype = c_int
    lib.scs_hip_aa_last_gamma.argtypes = [C.c_void_p, _PD]
    lib.scs_hip_aa_finish.restype = None
    lib.scs_hip_aa_finish.argtypes = [C.c_void_p]
    return lib


_lib = _load()


def version():
    return _lib.scs_version().decode()


def sizeof_int():
    return int(_lib.scs_sizeof_int())


def sizeof_float():
    return int(_lib.scs_sizeof_float())


def device_count():
    return int(_lib.scs_hip_device_count())


def labs_build():
    """True when the loaded library is the -DSCS_HIP_LABS build (csrc/options.hpp: the experiments that lost and the lab switches of
    the kernels read the environment there; the product does not contain them)"""
    return bool(_lib.scs_hip_labs_build())


def mem_info():
    """(free, total) HBM bytes of the device the next SCS(...) would use (blocks this library caches count as free); None without a device"""
    f, t = C.c_size_t(0), C.c_size_t(0)
    if _lib.scs_hip_mem_info(C.byref(f), C.byref(t)) != 0:
        return None
    return int(f.value), int(t.value)


def set_device(dev):
    if _lib.scs_hip_set_device(int(dev)) != 0:
        raise ValueError("invalid HIP device %r" % (dev,))


def set_thread_device(dev):
    """device of the calling THREAD's subsequent SCS(...) constructions (None / negative: back to the process default)"""
    if _lib.scs_hip_set_thread_device(-1 if dev is None else int(dev)) != 0:
        raise ValueError("invalid HIP device index %r" % (dev,))


def last_error():
    return _lib.scs_hip_last_error().decode()


# ---------------------------------------------------------------- argument parsing
def _pd(a):
    return a.ctypes.data_as(_PD)


def _pi(a):
    return a.ctypes.data_as(_PI)


def _float_array(name, a, length=None, exc_len=ValueError, len_msg=None):
    """1-D numpy float array of any float dtype -> contiguous float64 copy
    (R:scs/scsobject.h:60-68,574-592; integer arrays are rejected, test
    R:test/test_scs_coverage.py:1698-1720)."""
    if not isinstance(a, np.ndarray):
        raise TypeError("%s must be a 1-D numpy array of floats" % name)
    if not np.issubdtype(a.dtype, np.floating) or a.ndim != 1:
        raise TypeError("%s must be a 1-D numpy array of floats" % name)
    if length is not None and a.shape[0] != length:
        raise exc_len(len_msg or ("%s has incompatible dimension" % name))
    return np.array(a, dtype=np.float64, order="C", copy=True)


def _int_array(name, a):
    if not isinstance(a, np.ndarray):
        raise TypeError("%s must be a 1-D numpy array of ints" % name)
    if not np.issubdtype(a.dtype, np.integer) or a.ndim != 1:
        raise TypeError("%s must be a 1-D numpy array of ints" % name)
    if a.size and (a.max() > np.iinfo(np.int32).max or a.min() < np.iinfo(np.int32).min):
        raise ValueError("%s does not fit the 32-bit index type of the GPU backend" % name)
    return np.array(a, dtype=np.int32, order="C", copy=True)


def _as_c_int(name, v):
    """mirrors the 'i' format unit of PyArg_ParseTupleAndKeywords"""
    if isinstance(v, bool):
        return int(v)
    if isinstance(v, (float, np.floating)):
        raise TypeError("'float' object cannot be interpreted as an integer")
    try:
        iv = v.__index__()
    except AttributeError:
        raise TypeError("'%s' object cannot be interpreted as an integer" % type(v).__name__)
    if not -2 ** 31 <= iv < 2 ** 31:
        raise OverflowError("signed integer is greater than maximum")
    return int(iv)


def _as_c_double(name, v):
    """mirrors the 'd' format unit"""
    if isinstance(v, (str, bytes)) or v is None:
        raise TypeError("must be real number, not %s" % type(v).__name__)
    try:
        return float(v)
    except (TypeError, ValueError):
        raise TypeError("must be real number, not %s" % type(v).__name__)


def _as_bool(name, v):
    """mirrors 'O!' with PyBool_Type (R:scs/scsobject.h:534-536)"""
    if not isinstance(v, (bool, np.bool_)):
        raise TypeError("argument '%s' must be bool, not %s" % (name, type(v).__name__))
    return 1 if v else 0


def _as_filename(name, v):
    if v is None:
        return None
    if isinstance(v, str):
        return v.encode()
    raise TypeError("argument '%s' must be str or None, not %s" % (name, type(v).__name__))


_INT_SETTINGS = ("max_iters", "acceleration_lookback", "acceleration_interval", "acceleration_type_1")
_FLOAT_SETTINGS = ("scale", "eps_abs", "eps_rel", "eps_infeas", "alpha", "rho_x", "time_limit_secs",
                   "acceleration_regularization", "acceleration_relaxation")
_BOOL_SETTINGS = ("verbose", "normalize", "adaptive_scale")
_FILE_SETTINGS = ("write_data_filename", "log_csv_filename")


def _cone_err(key):
    return ValueError("Invalid value for cone field '%s'" % key)


def _cone_pos_int(cone, key):
    """R:scs/scsobject.h:86-127 — python ints only, non-negative, must fit scs_int"""
    if key not in cone:
        return 0
    v = cone[key]
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise _cone_err(key)
    v = int(v)
    if v < 0 or v >= 2 ** 31:
        raise _cone_err(key)
    return v


def _cone_int_list(cone, key):
    """list, bare int or numpy int array of non-negative ints (R:scs/scsobject.h:148-238)"""
    if key not in cone or cone[key] is None:
        return np.zeros(0, dtype=np.int32)
    v = cone[key]
    if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
        v = [int(v)]
    if isinstance(v, np.ndarray):
        if v.ndim != 1 or not np.issubdtype(v.dtype, np.integer):
            raise _cone_err(key)
        vals = [int(t) for t in v]
    elif isinstance(v, (list, tuple)):
        vals = []
        for t in v:
            if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)):
                raise _cone_err(key)
            vals.append(int(t))
    else:
        raise _cone_err(key)
    for t in vals:
        if t < 0 or t >= 2 ** 31:
            raise _cone_err(key)
    return np.asarray(vals, dtype=np.int32)


def _spectral_lists(cone):
    """the spectral cone keys, parsed as R:scs/scsobject.h:751-794 does (before the core is entered)"""
    out = {}
    for key in ("d", "nuc_m", "nuc_n", "ell1", "sl_n", "sl_k"):
        try:
            out[key] = _cone_int_list(cone, key)
        except ValueError:
            raise ValueError("Failed to parse cone field %s" % key)
        if key == "nuc_n" and out["nuc_n"].size != out["nuc_m"].size:
            raise ValueError("nuc_m and nuc_n must have the same length")
        if key == "sl_k" and out["sl_k"].size != out["sl_n"].size:
            raise ValueError("sl_n and sl_k must have the same length")
    return out


def _set_spectral(k, sp):
    """fill the spectral fields of a _ScsCone from _spectral_lists (the arrays must outlive the call)"""
    k.d, k.dsize = _pi(sp["d"]), sp["d"].size
    k.nuc_m, k.nuc_n, k.nucsize = _pi(sp["nuc_m"]), _pi(sp["nuc_n"]), sp["nuc_m"].size
    k.ell1, k.ell1_size = _pi(sp["ell1"]), sp["ell1"].size
    k.sl_n, k.sl_k, k.sl_size = _pi(sp["sl_n"]), _pi(sp["sl_k"]), sp["sl_n"].size


def _cone_float_list(cone, key):
    if key not in cone or cone[key] is None:
        return np.zeros(0, dtype=np.float64)
    v = cone[key]
    if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)):
        v = [float(v)]
    try:
        arr = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise _cone_err(key)
    if arr.ndim != 1:
        raise _cone_err(key)
    return np.ascontiguousarray(arr)


def _info_dict(info):
    """ScsInfo -> the reference's info dict (R:scs/scsobject.h:1073-1111) + this backend's extras"""
    aa = info.aa_stats
    return {
        "status_val": int(info.status_val),
        "iter": int(info.iter),
        "scale_updates": int(info.scale_updates),
        "scale": float(info.scale),
        "pobj": float(info.pobj),
        "dobj": float(info.dobj),
        "res_pri": float(info.res_pri),
        "res_dual": float(info.res_dual),
        "gap": float(info.gap),
        "res_infeas": float(info.res_infeas),
        "res_unbdd_a": float(info.res_unbdd_a),
        "res_unbdd_p": float(info.res_unbdd_p),
        "comp_slack": float(info.comp_slack),
        "solve_time": float(info.solve_time),
        "setup_time": float(info.setup_time),
        "lin_sys_time": float(info.lin_sys_time),
        "cone_time": float(info.cone_time),
        "accel_time": float(info.accel_time),
        "rejected_accel_steps": int(info.rejected_accel_steps),
        "accepted_accel_steps": int(info.accepted_accel_steps),
        "status": info.status.decode(),
        "aa_stats": {
            "iter": int(aa.iter), "n_accept": int(aa.n_accept),
            "n_reject_lapack": int(aa.n_reject_lapack), "n_reject_rank0": int(aa.n_reject_rank0),
            "n_reject_nonfinite": int(aa.n_reject_nonfinite),
            "n_reject_weight_cap": int(aa.n_reject_weight_cap),
            "n_safeguard_reject": int(aa.n_safeguard_reject), "last_rank": int(aa.last_rank),
            "last_aa_norm": float(aa.last_aa_norm),
            "last_regularization": float(aa.last_regularization),
        },
        # extras of this backend (the reference's dict is a subset)
        "cg_iters": int(info.cg_iters),
        "lin_sys_solver": info.lin_sys_solver.decode(),
    }


class SCS(object):
    """Raw backend type; `scs.SCS` (scs/__init__.py) is the user-facing wrapper."""

    # linear-system solver this backend type builds (include/scs_hip.h scs_hip_init_linsys): the MODULE decides, as in the reference
    # (R:scs/py/__init__.py:40-66) — 1 = sparse indirect (PCG) here, scs._scs_hip_dense.SCS sets 2 (dense direct).  Only the bare
    # C entry scs_init consults SCS_HIP_LINSYS (LinearSolver.HIP_INDIRECT must not turn dense behind the caller's back).
    _LINSYS = 1

    def __init__(self, shape, Ax, Ai, Ap, Px, Pi, Pp, b, c, cone, **settings):
        if getattr(self, "_work", None):
            raise ValueError("Workspace already setup!")
        self._blank()
        # ---- shape "(ii)"
        if not isinstance(shape, tuple) or len(shape) != 2:
            raise TypeError("argument 1 must be 2-item sequence (m, n)")
        m, n = _as_c_int("m", shape[0]), _as_c_int("n", shape[1])
        if not isinstance(cone, dict):
            raise TypeError("argument 10 must be dict, not %s" % type(cone).__name__)
        # ---- settings (keyword table R:scs/scsobject.h:467-495)
        st = _ScsSettings()
        _lib.scs_set_default_settings(C.byref(st))
        for key, val in settings.items():
            if key in _INT_SETTINGS:
                setattr(st, key, _as_c_int(key, val))
            elif key in _FLOAT_SETTINGS:
                setattr(st, key, _as_c_double(key, val))
            elif key in _BOOL_SETTINGS:
                setattr(st, key, _as_bool(key, val))
            elif key in _FILE_SETTINGS:
                fn = _as_filename(key, val)
                self._fn_keep.append(fn)
                setattr(st, key, fn)
            else:
                raise TypeError("'%s' is an invalid keyword argument for SCS()" % key)
        if m <= 0:
            raise ValueError("m must be a positive integer")
        if n <= 0:
            raise ValueError("n must be a positive integer")
        self._shape(m, n)
        # ---- data
        Axc = _float_array("Ax", Ax)
        Aic = _int_array("Ai", Ai)
        Apc = _int_array("Ap", Ap)
        if Apc.shape[0] != n + 1 or Axc.shape[0] != Aic.shape[0] or (Apc.size and Apc[-1] != Axc.shape[0]):
            raise ValueError("A has inconsistent CSC arrays")
        have_P = Px is not None and Pi is not None and Pp is not None
        if have_P:
            Pxc = _float_array("Px", Px)
            Pic = _int_array("Pi", Pi)
            Ppc = _int_array("Pp", Pp)
            if Ppc.shape[0] != n + 1 or Pxc.shape[0] != Pic.shape[0] or (Ppc.size and Ppc[-1] != Pxc.shape[0]):
                raise ValueError("P has inconsistent CSC arrays")
        cc = _float_array("c", c, n, ValueError, "c has incompatible dimension with A")
        bc = _float_array("b", b, m, ValueError, "b has incompatible dimension with A")
        # ---- cone (R:scs/scsobject.h:684-749)
        f_tmp = _cone_pos_int(cone, "f")
        z = _cone_pos_int(cone, "z")
        if f_tmp > 0:
            warnings.warn("The 'f' cone field is deprecated; use 'z' (Zero cone) instead. "
                          "If both 'f' and 'z' are set they are summed.", DeprecationWarning, stacklevel=2)
            z += f_tmp
        lcone = _cone_pos_int(cone, "l")
        bu = _cone_float_list(cone, "bu")
        bl = _cone_float_list(cone, "bl")
        if bu.size != bl.size:
            raise ValueError("bu different dimension to bl")
        q = _cone_int_list(cone, "q")
        s = _cone_int_list(cone, "s")
        cs = _cone_int_list(cone, "cs")
        p = _cone_float_list(cone, "p")
        ep = _cone_pos_int(cone, "ep")
        ed = _cone_pos_int(cone, "ed")
        spec = _spectral_lists(cone)
        # ---- settings validation (R:scs/scsobject.h:810-868)
        if st.max_iters <= 0:
            raise ValueError("max_iters must be positive")
        if st.acceleration_lookback < 0:
            raise ValueError("acceleration_lookback must be nonnegative (use acceleration_type_1=0 for type-II AA)")
        if st.acceleration_interval <= 0:
            raise ValueError("acceleration_interval must be positive")
        if not np.isfinite(st.acceleration_regularization) or st.acceleration_regularization < 0:
            raise ValueError("acceleration_regularization must be a nonnegative finite number")
        if (not np.isfinite(st.acceleration_relaxation) or st.acceleration_relaxation < 0
                or st.acceleration_relaxation > 2):
            raise ValueError("acceleration_relaxation must be in [0, 2]")
        if not np.isfinite(st.scale) or st.scale <= 0:
            raise ValueError("scale must be a positive finite number")
        if np.isnan(st.time_limit_secs) or st.time_limit_secs < 0:
            raise ValueError("time_limit_secs must be nonnegative")
        if np.isnan(st.eps_abs) or st.eps_abs < 0:
            raise ValueError("eps_abs must be nonnegative")
        if np.isnan(st.eps_rel) or st.eps_rel < 0:
            raise ValueError("eps_rel must be nonnegative")
        if np.isnan(st.eps_infeas) or st.eps_infeas < 0:
            raise ValueError("eps_infeas must be nonnegative")
        if not np.isfinite(st.alpha) or st.alpha <= 0 or st.alpha >= 2:
            raise ValueError("alpha must be in (0, 2)")
        if not np.isfinite(st.rho_x) or st.rho_x <= 0:
            raise ValueError("rho_x must be a positive finite number")
        st.warm_start = 0
        # ---- hand over to the C core (it copies everything, R:scs/scsobject.h:908)
        A = _ScsMatrix(_pd(Axc), _pi(Aic), _pi(Apc), m, n)
        P = _ScsMatrix(_pd(Pxc), _pi(Pic), _pi(Ppc), n, n) if have_P else None
        d = _ScsData(m, n, C.pointer(A), C.pointer(P) if have_P else None, _pd(bc), _pd(cc))
        k = _ScsCone(z, lcone, _pd(bu), _pd(bl), (bu.size + 1) if bu.size > 0 else 0,
                     _pi(q), q.size, _pi(s), s.size, _pi(cs), cs.size, ep, ed, _pd(p), p.size)
        _set_spectral(k, spec)
        if self._LINSYS:
            work = _lib.scs_hip_init_linsys_spectral(C.byref(d), C.byref(k), C.byref(st), self._LINSYS)
        else:
            work = _lib.scs_init_spectral(C.byref(d), C.byref(k), C.byref(st))  # GIL released by ctypes
        if not work:
            # the reference's message (R:scs/scsobject.h:903-912) + the backend's own reason: invalid data, no GPU,
            # out of HBM, or a limit this backend has and the reference has not (INTEGRATION.md "Limits")
            self._init_error = last_error()
            raise ValueError("ScsWork allocation error!" + (" (%s)" % self._init_error if self._init_error else ""))
        self._work = work
        # the sparsity pattern as given (update_matrix checks new matrices against it; the arrays are the ones built above: no copy)
        self._pattern = {"A": (Apc, Aic), "P": (Ppc, Pic) if have_P else None}

    # every attribute of an instance is set by these two: the constructor and clone() build their objects through them
    def _blank(self):
        self._work = None
        self._lock = threading.Lock()
        self._fn_keep = []
        self._many = []  # solve_many's clones (members 1 .. K-1), kept for the next call
        self._many_K = None  # members of the last solve_many (refine_many's default)
        self._pattern = None  # {"A": (indptr, indices), "P": ... or None}: what update_matrix checks against

    def _shape(self, m, n):
        self.m, self.n = m, n
        self._x, self._y, self._s = np.zeros(n), np.zeros(m), np.zeros(m)

    # ------------------------------------------------------------------ solve
    def _warm(self, name, dst, src):
        """R:scs/scsobject.h:129-146"""
        if not isinstance(src, np.ndarray) or not np.issubdtype(src.dtype, np.floating) or src.ndim != 1:
            raise ValueError("Unable to parse %s warm-start" % name)
        if src.shape[0] != dst.shape[0]:
            raise ValueError("Unable to parse %s warm-start" % name)
        dst[:] = src

    def solve(self, warm_start=True, x=None, y=None, s=None):
        if not isinstance(warm_start, (bool, np.bool_)):
            raise TypeError("argument 1 must be bool, not %s" % type(warm_start).__name__)
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            if warm_start:
                if x is not None:
                    self._warm("x", self._x, x)
                if y is not None:
                    self._warm("y", self._y, y)
                if s is not None:
                    self._warm("s", self._s, s)
            sol = _ScsSolution(_pd(self._x), _pd(self._y), _pd(self._s))
            info = _ScsInfo()
            _lib.scs_solve(self._work, C.byref(sol), C.byref(info), 1 if warm_start else 0)
            # fresh copies owning their data (R:scs/scsobject.h:993-1043), taken under the lock
            xo, yo, so = self._x.copy(), self._y.copy(), self._s.copy()
        info_dict = _info_dict(info)
        return {"x": xo, "y": yo, "s": so, "info": info_dict}

    # ----------------------------------------------------------------- update
    def update(self, b=None, c=None):
        cc = bc = None
        if c is not None:
            if not isinstance(c, np.ndarray) or not np.issubdtype(c.dtype, np.floating) or c.ndim != 1:
                raise TypeError("c_new must be a 1-D numpy array of floats")
            if c.shape[0] != self.n:
                raise ValueError("c_new has incompatible dimension with A")
            cc = np.array(c, dtype=np.float64, order="C", copy=True)
        if b is not None:
            if not isinstance(b, np.ndarray) or not np.issubdtype(b.dtype, np.floating) or b.ndim != 1:
                raise TypeError("b_new must be a 1-D numpy array of floats")
            if b.shape[0] != self.m:
                raise ValueError("b_new has incompatible dimension with A")
            bc = np.array(b, dtype=np.float64, order="C", copy=True)
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            _lib.scs_update(self._work, _pd(bc) if bc is not None else None, _pd(cc) if cc is not None else None)
        return None

    # ---------------------------------------------------------- matrix values
    def _finish_many(self):
        """solve_many's cached clones share the matrix set, which a matrix update may not write under a reader: they are finished
        here (internal objects; the next solve_many makes new ones)"""
        pool, self._many = self._many, []
        for sv in pool:
            sv.__del__()

    def _update_matrix_call(self, fn, ap, pp):
        self._finish_many()
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            rc = fn(self._work, ap, pp)
            err = last_error() if rc != 0 else ""
        if rc != 0:
            raise ValueError("libscs_hip: " + err)
        return None

    def update_matrix(self, A=None, P=None):
        """New VALUES of A and / or P on the sparsity pattern of the constructor (include/scs_hip.h: scs_hip_update_matrix); None =
        keep.  Each argument is a 1-D float array of nnz values in the constructor's CSC order (P: its upper triangle), or a
        (data, indices, indptr) triple of a canonical CSC matrix whose pattern must equal the constructor's (`scs.SCS.update_matrix`
        builds it from a scipy matrix).  Afterwards the solver is in the state a new one built from the new matrices and the current
        b, c would be in: a following solve returns that solver's bits."""
        if not self._work:
            raise ValueError("Workspace not initialized!")
        av = _matrix_values("A", A, self._pattern["A"]) if A is not None else None
        pv = _matrix_values("P", P, self._pattern["P"]) if P is not None else None
        if av is None and pv is None:
            return None
        return self._update_matrix_call(_lib.scs_hip_update_matrix, _pd(av) if av is not None else None, _pd(pv) if pv is not None else None)

    def update_matrix_device(self, A=None, P=None):
        """`update_matrix` for values that live on the workspace's GPU: float64, 1-D, contiguous torch tensors of nnz(A) / nnz(P)
        elements in the constructor's CSC order, None = keep.  Same bits as `update_matrix` with the same values."""
        dev = self._device_index()
        if P is not None and self._pattern["P"] is None:
            raise ValueError("P given, but the solver was created without P")
        ap = _device_vec("A", A, int(self._pattern["A"][1].shape[0]), dev) if A is not None else None
        pp = _device_vec("P", P, int(self._pattern["P"][1].shape[0]), dev) if P is not None else None
        if ap is None and pp is None:
            return None
        _sync_torch_stream(dev)  # the stream contract: inputs complete before the library's own stream reads them
        return self._update_matrix_call(_lib.scs_hip_update_matrix_device, ap, pp)

    # ------------------------------------------------- one matrix, many (b, c)
    def clone(self):
        """A new solver in the state the constructor left this one in (its original b, c and settings, cold start) that SHARES this
        one's matrix data on the device (include/scs_hip.h: scs_hip_clone) and allocates per-solve state only."""
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            work = _lib.scs_hip_clone(self._work)
        if not work:
            raise ValueError("ScsWork allocation error!" + (" (%s)" % last_error() if last_error() else ""))
        new = object.__new__(type(self))
        new._blank()
        new._shape(self.m, self.n)
        new._work = work
        new._pattern = self._pattern
        return new

    def shares_matrix(self, other):
        """True when `other` holds the same device matrix set (this solver's clone, its parent, a clone of a clone)."""
        if not isinstance(other, SCS) or not self._work or not other._work:
            return False
        return bool(_lib.scs_hip_shares_matrix(self._work, other._work))

    def solve_many(self, b=None, c=None, warm_start=False, x=None, y=None, s=None):
        """K problems over this solver's matrix in one batch: b (K, m) and c (K, n) float64, either None = keep.  Member 0 is this
        solver, members 1..K-1 are clones kept on it (made on demand, reused by the next call — with warm_start=True each member
        starts from its own previous solution, or from row i of x / y / s).  Each member is `update`d, then ONE solve_batch runs over
        all of them.  Returns the K result dicts `solve()` would return."""
        K, rows = _many_args(self.m, self.n, b, c, warm_start, x, y, s)
        if not self._work:
            raise ValueError("Workspace not initialized!")
        pool = self._many
        while len(pool) < K - 1:
            pool.append(self.clone())
        members = [self] + pool[:K - 1]
        self._many_K = K
        for i, sv in enumerate(members):
            bi, ci = rows["b"][i] if b is not None else None, rows["c"][i] if c is not None else None
            if bi is not None or ci is not None:
                sv.update(bi, ci)
            if warm_start:
                with sv._lock:
                    for name, dst in (("x", sv._x), ("y", sv._y), ("s", sv._s)):
                        if rows[name] is not None:
                            sv._warm(name, dst, rows[name][i])
        return solve_batch(members, bool(warm_start))

    # ------------------------------------------ device-resident endpoints (torch tensors; include/scs_hip.h)
    def _device_index(self):
        if not self._work:
            raise ValueError("Workspace not initialized!")
        return int(_lib.scs_hip_work_device(self._work))

    def update_device(self, b=None, c=None):
        """`update` for b (m) / c (n) that live on the workspace's GPU: float64, 1-D, contiguous torch tensors, None = keep.  Nothing of
        length n or m crosses the host; a following solve gives the bits `update` with the same values would give."""
        dev = self._device_index()
        bp = _device_vec("b_new", b, self.m, dev) if b is not None else None
        cp = _device_vec("c_new", c, self.n, dev) if c is not None else None
        _sync_torch_stream(dev)  # the stream contract: inputs complete before the library's own stream reads them
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            rc = _lib.scs_hip_update_device(self._work, bp, cp)
            err = last_error() if rc != 0 else ""
        if rc != 0:
            raise RuntimeError("libscs_hip: " + err)
        return None

    def _previous_to_device(self, ptrs):
        """the workspace's last solution into the device vectors {name: address} (zeros before the first solve); lock held"""
        got = _lib.scs_hip_solution_to_device(self._work, ptrs.get("x"), ptrs.get("y"), ptrs.get("s")) == 0
        return got

    def solve_device(self, warm_start=False, x=None, y=None, s=None):
        """`solve` with the endpoints on the device: returns {"x", "y", "s", "info"} with three fresh float64 torch tensors on the
        workspace's GPU.  warm_start=True starts from the device tensors x / y / s; an omitted one starts from this solver's previous
        solution as it lies on the device (zeros before the first solve)."""
        if not isinstance(warm_start, (bool, np.bool_)):
            raise TypeError("argument 1 must be bool, not %s" % type(warm_start).__name__)
        dev = self._device_index()
        given = {}
        if warm_start:
            for name, t, length in (("x", x, self.n), ("y", y, self.m), ("s", s, self.m)):
                if t is not None:
                    _device_vec(name, t, length, dev)
                    given[name] = t
        import torch
        tdev = torch.device("cuda", dev)
        out = {"x": torch.empty(self.n, dtype=torch.float64, device=tdev), "y": torch.empty(self.m, dtype=torch.float64, device=tdev),
               "s": torch.empty(self.m, dtype=torch.float64, device=tdev)}
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            if warm_start:
                for name, t in given.items():
                    out[name].copy_(t)
                missing = {name: out[name].data_ptr() for name in out if name not in given}
                if missing:
                    for name in missing:
                        out[name].zero_()
                    _sync_torch_stream(dev)
                    self._previous_to_device(missing)
            _sync_torch_stream(dev)
            info = _ScsInfo()
            rc = _lib.scs_hip_solve_device(self._work, out["x"].data_ptr(), out["y"].data_ptr(), out["s"].data_ptr(), C.byref(info),
                                           1 if warm_start else 0)
            err = last_error() if rc == -1 else ""
        if rc == -1 and info.status_val == 0:  # refused arguments (an unbounded problem also returns -1, with its info filled)
            raise RuntimeError("libscs_hip: " + err)
        out["info"] = _info_dict(info)
        return out

    def solve_many_device(self, b=None, c=None, warm_start=False, x=None, y=None, s=None):
        """`solve_many` with the endpoints on the device: b (K, m), c (K, n) and the warm starts (K, .) are float64 torch tensors on the
        workspace's GPU.  Members are this solver and its cached clones; each is `update_device`d from its row, then ONE grouped solve
        writes straight into the rows of the result: {"x": (K, n), "y": (K, m), "s": (K, m), "info": [K dicts]}."""
        dev = self._device_index()
        K, rows = _many_device_args(self.m, self.n, dev, b, c, warm_start, x, y, s)
        pool = self._many
        while len(pool) < K - 1:
            pool.append(self.clone())
        members = [self] + pool[:K - 1]
        self._many_K = K
        for i, sv in enumerate(members):
            bi, ci = rows["b"][i] if b is not None else None, rows["c"][i] if c is not None else None
            if bi is not None or ci is not None:
                sv.update_device(bi, ci)
        import torch
        tdev = torch.device("cuda", dev)
        out = {"x": torch.empty((K, self.n), dtype=torch.float64, device=tdev), "y": torch.empty((K, self.m), dtype=torch.float64, device=tdev),
               "s": torch.empty((K, self.m), dtype=torch.float64, device=tdev)}
        with _locked(members) as works:
            if warm_start:
                missing = [name for name in ("x", "y", "s") if rows[name] is None]
                for name in ("x", "y", "s"):
                    if rows[name] is not None:
                        out[name].copy_(rows[name])
                    else:
                        out[name].zero_()
                _sync_torch_stream(dev)
                if missing:
                    for i, sv in enumerate(members):
                        sv._previous_to_device({name: out[name][i].data_ptr() for name in missing})
            _sync_torch_stream(dev)
            infos = [_ScsInfo() for _ in members]
            ptrs = {name: (C.c_void_p * K)(*[out[name][i].data_ptr() for i in range(K)]) for name in ("x", "y", "s")}
            infp = (C.POINTER(_ScsInfo) * K)(*[C.pointer(io) for io in infos])
            rc = _lib.scs_hip_solve_batch_device(works, ptrs["x"], ptrs["y"], ptrs["s"], infp, K, 1 if warm_start else 0)
            err = last_error() if rc != 0 else ""
        out["info"] = [_info_dict(io) for io in infos]
        if rc != 0 and any(o["status_val"] == 0 for o in out["info"]):  # (as solve_batch: only a call that failed as a whole raises)
            raise RuntimeError("libscs_hip: " + err)
        return out

    # ------------------------------------------------------ derivatives of the last solve (include/scs_hip.h)
    # The twelve public functions (here and adjoint_batch ... below) name a kind (_ADJOINT / _DERIVATIVE), a memory (host arrays or
    # device tensors) and their arguments; `_diff` serves one solver, `_diff_list` a list of members.  The multi functions
    # (adjoint_multi ... jacobian) are the same kinds and memories in a third call shape: `_diff_multi`, K directions of one solver.
    def _diff_call(self, fn, ptrs, opts):
        info = _ScsHipDiffInfo()
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            rc = fn(self._work, *(list(ptrs) + [C.byref(opts), C.byref(info)]))
            err = last_error() if rc != 0 else ""
        if rc != 0:
            raise ValueError("libscs_hip: " + err)
        return _diff_info_dict(info)

    def _lens(self):
        """the lengths of the vectors of a derivative call, by the key the kinds use: n, m and the stored values of A and of P"""
        pa, pp = self._pattern["A"], self._pattern["P"]
        return {"n": self.n, "m": self.m, "A": int(pa[1].shape[0]), "P": int(pp[1].shape[0]) if pp is not None else 0}

    def _refuse_dP(self, kind, vals):
        """an input of nnz(P) values (dP) for a solver without P is refused here, before the library is called"""
        if self._pattern["P"] is None:
            for (name, key), v in zip(kind.ins, vals):
                if key == "P" and v is not None:
                    raise ValueError("%s given, but the solver was created without P" % name)

    def _diff(self, kind, device, vals, want, tol, max_iters):
        """One solver's call of `kind`: vals = the inputs in the order of kind.ins, on the host or (device) on the solver's GPU; want =
        the outputs' names, None = all of them."""
        if not self._work:
            raise ValueError("Workspace not initialized!")
        if want is not None:
            want = _diff_want(want, self._pattern["P"] is not None)
        lens, nv = self._lens(), kind.vectors
        if device:  # (tol, max_iters and dP need no call of the library to be refused: they come before the first one, _device_index)
            opts = _diff_opts(tol, max_iters)
            self._refuse_dP(kind, vals)
            mem = _device_memory(self._device_index())
            ins = [mem.check(self, name, v, key, lens) for (name, key), v in zip(kind.ins, vals)]
        else:  # (as the arguments come: the vectors, then the matrix values, then tol and max_iters)
            mem = _HOST
            ins = [mem.check(self, name, v, key, lens) for (name, key), v in zip(kind.ins[:nv], vals)]
            self._refuse_dP(kind, vals)
            ins += [mem.check(self, name, v, key, lens) for (name, key), v in zip(kind.ins[nv:], vals[nv:])]
            opts = _diff_opts(tol, max_iters)
        out = {k: mem.zeros(lens[kind.outs[k]]) for k in _diff_chosen(kind, want)}
        fn, ins = _diff_entry(kind, mem, False, ins)
        ptrs = [mem.address(v) if v is not None else None for v in ins] + [mem.address(out[k]) if k in out else None for k in kind.outs]
        mem.ready()
        out["info"] = self._diff_call(fn, ptrs, opts)
        return out

    def adjoint(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None):
        """The adjoint of the last solve: given dL/dx (n), dL/dy (m), dL/ds (m) — None = 0 — returns {"db", "dc", ["dA"], ["dP"],
        "info"}, the gradients of L with respect to b, c and (`want` adds "A" / "P") the stored values of A and of the upper triangle
        of P in the constructor's order.  One LSQR solve on the device with tolerance `tol` and at most `max_iters` iterations (None:
        4 (n + m)); info = {"iters", "residual", "normal_residual", "stop", "time_ms"}.  A degenerate solution is not an error: the
        minimum-norm least-squares answer comes back with stop == 2."""
        return self._diff(_ADJOINT, False, (dx, dy, ds), want, tol, max_iters)

    def adjoint_device(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None):
        """`adjoint` over float64 torch tensors on the solver's GPU: takes and returns device tensors; nothing of length n or m
        crosses the host.  Same bits as `adjoint` on the same values."""
        return self._diff(_ADJOINT, True, (dx, dy, ds), want, tol, max_iters)

    def derivative(self, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
        """The forward derivative of the last solve: the change {"dx", "dy", "ds", "info"} of the solution for a change db (m), dc (n)
        of the data and dA, dP of the stored VALUES of A and of the upper triangle of P (None = 0); LSQR as in `adjoint`.  dA / dP: a 1-D
        float array of nnz values in the constructor's CSC order (an off-diagonal value of dP stands for both mirror images, as in
        `adjoint`'s dP), or a (data, indices, indptr) triple of a canonical CSC matrix of the constructor's pattern (`update_matrix`)."""
        return self._diff(_DERIVATIVE, False, (db, dc, dA, dP), None, tol, max_iters)

    def derivative_device(self, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
        """`derivative` over float64 torch tensors on the solver's GPU (dA, dP: 1-D value tensors of nnz(A) / nnz(P) elements)."""
        return self._diff(_DERIVATIVE, True, (db, dc, dA, dP), None, tol, max_iters)

    def _data_perturbation(self, device, dA, dP):
        if not self._work:
            raise ValueError("Workspace not initialized!")
        self._refuse_dP(_DERIVATIVE, (None, None, dA, dP))
        mem = _device_memory(self._device_index()) if device else _HOST
        lens = self._lens()
        ins = [mem.check(self, name, v, key, lens) for (name, key), v in zip(_DERIVATIVE.ins[2:], (dA, dP))]
        out_c, out_b = mem.zeros(self.n), mem.zeros(self.m)
        ptrs = [mem.address(v) if v is not None else None for v in ins] + [mem.address(out_c), mem.address(out_b)]
        mem.ready()
        with self._lock:
            rc = getattr(_lib, "scs_hip_data_perturbation" + mem.suffix)(self._work, *ptrs)
            err = last_error() if rc != 0 else ""
        if rc != 0:
            raise ValueError("libscs_hip: " + err)
        return out_c, out_b

    def data_perturbation(self, dA=None, dP=None):
        """(dP x + dA' y, dA x) at the resident solution of the last solve: the perturbation products of `derivative(dA=, dP=)` on
        their own (include/scs_hip.h: scs_hip_data_perturbation; tests)."""
        return self._data_perturbation(False, dA, dP)

    def data_perturbation_device(self, dA=None, dP=None):
        """`data_perturbation` over float64 torch tensors on the solver's GPU (taken and returned); same bits."""
        return self._data_perturbation(True, dA, dP)

    # ------------------------------------- derivatives of solve_many's members in lock step (adjoint_batch below)
    def _many_members(self, K):
        """this solver and the clones solve_many cached on it: the first K of them (None: all)"""
        if not self._work:
            raise ValueError("Workspace not initialized!")
        have = 1 + len(self._many)
        if K is None:
            K = have
        if K > have:
            raise ValueError("%d rows, but solve_many has solved %d member%s of this solver" % (K, have, "" if have == 1 else "s"))
        return [self] + self._many[:K - 1]

    def _diff_many(self, kind, device, vals, want, tol, max_iters, reduce=None):
        """`kind` of the members the last solve_many solved: vals = (K, .) stacks in the order of kind.ins.  On the device the results
        are stacks too, and the one grouped call writes straight into their rows."""
        kind = _diff_reduce(kind, reduce, want)
        self._refuse_dP(kind, vals)
        mem = _device_memory(self._device_index()) if device else _HOST
        lens = self._lens()
        K, rows = _many_diff_args(_diff_spec(kind, vals, lens), None, want, self._pattern["P"] is not None, device=mem.device)
        members = self._many_members(K)
        return _diff_list(kind, mem, members, rows, [lens] * len(members), want, tol, max_iters, stacked=device)

    def adjoint_many(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None, reduce=None):
        """`adjoint` of the K members the last `solve_many` solved, in lock step (`adjoint_batch`): dx (K, n), dy (K, m), ds (K, m),
        None = 0.  Returns the K dicts `adjoint` would return, with the same bits.  reduce="sum" (with "A" or "P" in `want`): the
        members share this solver's matrix, and the gradients of its values come summed over them — the pair (results, grads) of the K
        dicts without dA / dP and {"dA": (nnz,), "dP": (nnz(P),)} (include/scs_hip.h: scs_hip_adjoint_shared)."""
        return self._diff_many(_ADJOINT, False, (dx, dy, ds), want, tol, max_iters, reduce)

    def derivative_many(self, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
        """`derivative` of the K members the last `solve_many` solved, in lock step: db (K, m), dc (K, n), dA (K, nnz(A)),
        dP (K, nnz(P)), None = 0."""
        return self._diff_many(_DERIVATIVE, False, (db, dc, dA, dP), None, tol, max_iters)

    def adjoint_many_device(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None, reduce=None):
        """`adjoint_many` over float64 torch tensors (K, .) on the solver's GPU: one grouped call that writes straight into the rows of
        {"db": (K, m), "dc": (K, n), ["dA": (K, nnz)], ["dP"], "info": [K dicts]}.  reduce="sum": the same dict with dA (nnz,) and
        dP (nnz(P),) summed over the members; no (K, nnz) stack is formed."""
        return self._diff_many(_ADJOINT, True, (dx, dy, ds), want, tol, max_iters, reduce)

    def derivative_many_device(self, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
        """`derivative_many` over float64 torch tensors (K, .) on the solver's GPU: {"dx": (K, n), "dy": (K, m), "ds": (K, m), "info"}."""
        return self._diff_many(_DERIVATIVE, True, (db, dc, dA, dP), None, tol, max_iters)

    # ------------------------------------- several directions at ONE solution (include/scs_hip.h: scs_hip_adjoint_multi)
    def _diff_multi(self, kind, device, vals, want, tol, max_iters):
        """`kind` of this solver's last solve along K directions at once: vals = (K, .) stacks in the order of kind.ins, on the host
        or (device) on the solver's GPU; the results are (K, .) stacks whose rows the library writes, in chunks of the C limit."""
        if not self._work:
            raise ValueError("Workspace not initialized!")
        if want is not None:
            want = _diff_want(want, self._pattern["P"] is not None)
        lens = self._lens()
        opts = _diff_opts(tol, max_iters)
        mem = _device_memory(self._device_index()) if device else _HOST
        K, ins = _multi_diff_args(_diff_spec(kind, vals, lens), device=mem.device)
        out = {k: mem.zeros((K, lens[kind.outs[k]])) for k in _diff_chosen(kind, want)}
        fn = getattr(_lib, kind.entry + mem.suffix)
        mem.ready()
        infos = []
        for lo in range(0, K, MULTI_MAX):
            hi = min(K, lo + MULTI_MAX)
            ptrs = [mem.address(v[lo:hi]) if v is not None else None for v in ins]
            ptrs += [mem.address(out[k][lo:hi]) if k in out else None for k in kind.outs]
            chunk = (_ScsHipDiffInfo * (hi - lo))()
            with self._lock:
                if not self._work:
                    raise ValueError("Workspace not initialized!")
                rc = fn(self._work, hi - lo, *(ptrs + [C.byref(opts), chunk]))
                err = last_error() if rc != 0 else ""
            if rc != 0:
                raise ValueError("libscs_hip: " + err)
            infos += [_diff_info_dict(io) for io in chunk]
        out["info"] = infos
        return out

    def adjoint_multi(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None):
        """`adjoint` of the last solve for K cotangents at once: dx (K, n), dy (K, m), ds (K, m), None = 0, K read from them.  Returns
        {"db": (K, m), "dc": (K, n), ["dA": (K, nnz)], ["dP"], "info": [K dicts]}; row k has the bits of `adjoint` on direction k.  The
        preparation runs once and the K LSQR solves advance in lock step, reading the matrices once per tile of directions."""
        return self._diff_multi(_ADJOINT_MULTI, False, (dx, dy, ds), want, tol, max_iters)

    def adjoint_multi_device(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None):
        """`adjoint_multi` over (K, .) float64 torch tensors on the solver's GPU (taken and returned); same bits."""
        return self._diff_multi(_ADJOINT_MULTI, True, (dx, dy, ds), want, tol, max_iters)

    def derivative_multi(self, db=None, dc=None, tol=1e-8, max_iters=None):
        """`derivative` of the last solve for K perturbations at once: db (K, m), dc (K, n), None = 0.  Returns {"dx": (K, n),
        "dy": (K, m), "ds": (K, m), "info": [K dicts]}; row k has the bits of `derivative` on direction k."""
        return self._diff_multi(_DERIVATIVE_MULTI, False, (db, dc), None, tol, max_iters)

    def derivative_multi_device(self, db=None, dc=None, tol=1e-8, max_iters=None):
        """`derivative_multi` over (K, .) float64 torch tensors on the solver's GPU (taken and returned); same bits."""
        return self._diff_multi(_DERIVATIVE_MULTI, True, (db, dc), None, tol, max_iters)

    def _jacobian(self, device, of, wrt, rows, tol, max_iters):
        if of not in ("x", "y", "s"):
            raise ValueError("of must be 'x', 'y' or 's', not %r" % (of,))
        if wrt not in ("b", "c"):
            raise ValueError("wrt must be 'b' or 'c', not %r" % (wrt,))
        size = self.n if of == "x" else self.m
        rows = list(range(size)) if rows is None else [operator.index(r) for r in rows]
        for r in rows:
            if not 0 <= r < size:
                raise ValueError("rows holds %d: %s has %d entries" % (r, of, size))
        if not rows:
            raise ValueError("rows is empty")
        if device:
            import torch
            G = torch.zeros((len(rows), size), dtype=torch.float64, device=torch.device("cuda", self._device_index()))
            G[torch.arange(len(rows)), torch.tensor(rows, dtype=torch.long)] = 1.0
        else:
            G = np.zeros((len(rows), size))
            G[np.arange(len(rows)), rows] = 1.0
        res = self._diff_multi(_ADJOINT_MULTI, device, tuple(G if k == of else None for k in ("x", "y", "s")), (wrt,), tol, max_iters)
        return res["d" + wrt], res["info"]

    def jacobian(self, of="x", wrt="b", rows=None, tol=1e-8, max_iters=None):
        """The dense block d of[rows] / d wrt of the last solve, (len(rows), len(wrt)): of in "x", "y", "s", wrt in "b", "c", rows =
        indices into `of` (None: all).  `adjoint_multi` with the unit cotangents of the rows.  Returns (J, infos)."""
        return self._jacobian(False, of, wrt, rows, tol, max_iters)

    def jacobian_device(self, of="x", wrt="b", rows=None, tol=1e-8, max_iters=None):
        """`jacobian` as a float64 torch tensor on the solver's GPU."""
        return self._jacobian(True, of, wrt, rows, tol, max_iters)

    # -------------------------------------------------- bench hooks (not part of the reference surface)
    # ------------------------------------------------------ Newton polish of the last solve (include/scs_hip.h: scs_hip_refine)
    def _refine_call(self, fn, sol, opts):
        """lock held"""
        info = _ScsHipRefineInfo()
        rc = fn(self._work, C.byref(sol), C.byref(opts), C.byref(info))
        if rc != 0:
            raise ValueError("libscs_hip: " + last_error())
        return _refine_info_dict(info)

    def refine(self, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None):
        """Polish the solution of the last solve by Newton steps on its optimality conditions, on the device: each step is one LSQR
        solve of the system `derivative` solves (lsqr_tol, lsqr_max_iters: None = 4 (n + m)) and a backtracking line search; it stops
        when the solver's three criteria hold with eps_abs = eps_rel = tol, after max_steps accepted steps, or when no step length
        gives a decrease.  Returns {"x", "y", "s", "info"}; info = the figures of ScsHipRefineInfo and "stop_reason" ("converged",
        "max_steps", "no_decrease").  The polished point replaces the resident solution: `adjoint`, `derivative`, `jacobian` and
        `solve(warm_start=True)` start from it."""
        opts = _refine_opts(tol, max_steps, lsqr_tol, lsqr_max_iters)
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            sol = _ScsSolution(_pd(self._x), _pd(self._y), _pd(self._s))
            info = self._refine_call(_lib.scs_hip_refine, sol, opts)
            xo, yo, so = self._x.copy(), self._y.copy(), self._s.copy()
        return {"x": xo, "y": yo, "s": so, "info": info}

    def refine_device(self, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None):
        """`refine` with the result as three fresh float64 torch tensors on the solver's GPU; same bits."""
        opts = _refine_opts(tol, max_steps, lsqr_tol, lsqr_max_iters)
        dev = self._device_index()
        import torch
        tdev = torch.device("cuda", dev)
        out = {"x": torch.empty(self.n, dtype=torch.float64, device=tdev), "y": torch.empty(self.m, dtype=torch.float64, device=tdev),
               "s": torch.empty(self.m, dtype=torch.float64, device=tdev)}
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            _sync_torch_stream(dev)
            sol = _ScsSolution(C.cast(out["x"].data_ptr(), _PD), C.cast(out["y"].data_ptr(), _PD), C.cast(out["s"].data_ptr(), _PD))
            out["info"] = self._refine_call(_lib.scs_hip_refine_device, sol, opts)
        return out

    def refine_many(self, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None, K=None):
        """`refine` of the first K members the last `solve_many` solved (None: all of them; before any `solve_many`: this solver
        alone), in lock step (`refine_batch`).  Returns
        {"x": (K, n), "y": (K, m), "s": (K, m), "info": [K dicts]}, row k with the bits of `refine` on member k.  Every member's
        polished point becomes its resident solution: `adjoint_many` and a warm-started `solve_many` read it."""
        opts = _refine_opts(tol, max_steps, lsqr_tol, lsqr_max_iters)
        res = _refine_list(self._many_members(self._many_K if K is None else K), opts, False)
        return {"x": np.stack([r["x"] for r in res]), "y": np.stack([r["y"] for r in res]), "s": np.stack([r["s"] for r in res]),
                "info": [r["info"] for r in res]}

    def refine_many_device(self, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None, K=None):
        """`refine_many` with "x", "y", "s" as fresh (K, .) float64 torch tensors on the solver's GPU, whose rows the one grouped
        call writes; same bits."""
        opts = _refine_opts(tol, max_steps, lsqr_tol, lsqr_max_iters)
        return _refine_list(self._many_members(self._many_K if K is None else K), opts, True, stacked=True)

    def _set_profiling(self, on):
        with self._lock:
            _lib.scs_hip_set_profiling(self._work, 1 if on else 0)

    def _kernel_times(self):
        out = np.zeros(12)
        with self._lock:
            _lib.scs_hip_kernel_times(self._work, _pd(out))
        return {"k1_ms": out[0], "k1_n": int(out[1]), "k2_ms": out[2], "k2_n": int(out[3]),
                "nnz": int(out[4]), "k1_wgs": int(out[5]), "k2_wgs": int(out[6]), "nnz_p": int(out[7]),
                "cone_ms": out[8], "cone_n": int(out[9]), "k3_ms": out[10], "k3_n": int(out[11])}

    def solution_to_device(self, x_ptr=None, y_ptr=None, s_ptr=None):
        """copy the last solve's (x, y, s) from the workspace's HBM buffers to DEVICE addresses (ints, e.g.
        torch.Tensor.data_ptr() of float64 tensors on the same GPU); None skips a vector"""
        with self._lock:
            if not self._work:
                raise ValueError("Workspace not initialized!")
            rc = _lib.scs_hip_solution_to_device(self._work, x_ptr or None, y_ptr or None, s_ptr or None)
        if rc != 0:
            raise RuntimeError("libscs_hip: " + last_error())

    def _set_mark(self, it):
        _lib.scs_hip_set_mark(self._work, int(it))

    def _get_mark(self):
        out = np.zeros(4)
        _lib.scs_hip_get_mark(self._work, _pd(out))
        return {"ms": float(out[0]), "cg_iters": int(out[1]), "aa_calls": int(out[2]), "aa_accept": int(out[3])}

    def _time_psd(self, reps=20):
        out = np.zeros(4)
        with self._lock:
            rc = _lib.scs_hip_time_psd(self._work, int(reps), _pd(out))
        if rc == 1:
            return None
        _check(rc)
        return {"ms": float(out[0]), "matrices": int(out[1]), "max_order": int(out[2]), "ref_flops": float(out[3])}

    def _time_dproj(self, reps=50):
        """after a solve: ms per launch of the box and power derivative kernels and of the projections of the same cones
        (include/scs_hip.h scs_hip_time_dproj; tools/adjoint_bench.py --cones)"""
        out = np.zeros(8)
        with self._lock:
            rc = _lib.scs_hip_time_dproj(self._work, int(reps), _pd(out))
        if rc != 0:
            raise ValueError("libscs_hip: " + last_error())
        return {"box_apply_one_wg_ms": float(out[0]), "box_apply_two_launch_ms": float(out[1]), "box_proj_ms": float(out[2]), "bsize": int(out[3]),
                "pow_apply_ms": float(out[4]), "pow_prep_ms": float(out[5]), "pow_proj_ms": float(out[6]), "pow_cones": int(out[7])}

    def _psd_refine_stats(self, cap=4096):
        """per PSD matrix of order > 32: [calls refined, refinements sent back to the sweeps, |K1|_F^2 at the last gate,
        mixed-sign off-norm^2 / |A|^2 after the last refinement, stage flag of the last call, then what the last call's matrix looked like
        as it arrived: |K1|_F^2, |off|^2 / |A|^2, omega] (include/scs_hip.h)"""
        out = np.zeros(8 * cap)
        with self._lock:
            cnt = _lib.scs_hip_psd_refine_stats(self._work, _pd(out), int(cap))
        if cnt < 0:
            raise RuntimeError("libscs_hip: " + last_error())
        return out[:8 * cnt].reshape(cnt, 8)

    def _time_matvec(self, reps=20):
        out = np.zeros(4)
        with self._lock:
            rc = _lib.scs_hip_time_matvec(self._work, int(reps), _pd(out))
        if rc != 0:
            raise RuntimeError("libscs_hip: " + last_error())
        return {"k1_ms": float(out[0]), "k2_ms": float(out[1]), "k3_ms": float(out[2]), "k3_back_to_back_ms": float(out[3])}

    def __del__(self):
        lock = getattr(self, "_lock", None)
        work = getattr(self, "_work", None)
        if work and lock is not None and _lib is not None:  # (_lib is None while the interpreter shuts down)
            with lock:
                _lib.scs_finish(self._work)
                self._work = None


def _matrix_values(name, M, pattern):
    """The one argument check of SCS.update_matrix, before the library is called (no GPU needed): `M` is a 1-D float array of nnz values,
    or a (data, indices, indptr) triple of a canonical CSC matrix; `pattern` = the (indptr, indices) the constructor was given, None for
    a solver without that matrix.  Returns the float64 values (a fresh contiguous array).  Explicit zeros are values: nothing is
    eliminated, so a matrix that lost or gained a stored entry differs in its pattern."""
    if pattern is None:
        raise ValueError("%s given, but the solver was created without %s" % (name, name))
    indptr, indices = pattern
    nnz = int(indices.shape[0])
    if isinstance(M, tuple):
        if len(M) != 3:
            raise TypeError("%s must be a 1-D float array of values or a (data, indices, indptr) triple" % name)
        data, ind, ptr = M
        ind, ptr = np.asarray(ind), np.asarray(ptr)
        if ptr.shape != indptr.shape or ind.shape != indices.shape or not np.array_equal(ptr, indptr) or not np.array_equal(ind, indices):
            raise ValueError("%s: sparsity pattern differs from the one the solver was created with" % name)
        M = data
    if not isinstance(M, np.ndarray):
        raise TypeError("%s must be a 1-D float array of values or a sparse matrix, not %s" % (name, type(M).__name__))
    if M.ndim != 1 or not (np.issubdtype(M.dtype, np.floating) or np.issubdtype(M.dtype, np.integer)):
        raise TypeError("%s values must be a 1-D numpy array of floats" % name)
    if M.shape[0] != nnz:
        raise ValueError("%s has %d values, the solver's pattern has %d" % (name, M.shape[0], nnz))
    return np.array(M, dtype=np.float64, order="C", copy=True)


def _diff_vec(name, a, length):
    """A host vector of `adjoint` / `derivative`, checked before the library is called (no GPU needed): None, or a 1-D numpy float array
    of `length` elements; returns a fresh contiguous float64 copy."""
    if a is None:
        return None
    if not isinstance(a, np.ndarray) or not np.issubdtype(a.dtype, np.floating) or a.ndim != 1:
        raise TypeError("%s must be a 1-D numpy array of floats" % name)
    if a.shape[0] != length:
        raise ValueError("%s has incompatible dimension with A" % name)
    return np.array(a, dtype=np.float64, order="C", copy=True)


def _diff_mat(name, M, pattern):
    """dA / dP of `derivative`, checked before the library is called (no GPU needed): None, a 1-D numpy float array of nnz values
    (`_diff_vec`), or a (data, indices, indptr) triple of the constructor's pattern (`_matrix_values`); `pattern` = the (indptr, indices)
    the constructor was given, None for a solver without that matrix.  Returns a fresh contiguous float64 array."""
    if M is None:
        return None
    if pattern is None:
        raise ValueError("%s given, but the solver was created without %s" % (name, name[1:]))
    if isinstance(M, tuple):
        return _matrix_values(name, M, pattern)
    return _diff_vec(name, M, int(pattern[1].shape[0]))


def _diff_want(want, have_P):
    """`want` of `adjoint`: a tuple or list of distinct names out of "b", "c", "A", "P"; returns it as a tuple."""
    if isinstance(want, (str, bytes)) or not isinstance(want, (tuple, list)):
        raise TypeError("want must be a tuple of names out of 'b', 'c', 'A', 'P', not %s" % type(want).__name__)
    for k in want:
        if not isinstance(k, str) or k not in ("b", "c", "A", "P"):
            raise ValueError("want holds %r: the names are 'b', 'c', 'A', 'P'" % (k,))
    if len(set(want)) != len(want):
        raise ValueError("want names an output twice")
    if "P" in want and not have_P:
        raise ValueError("dP wanted, but the solver was created without P")
    return tuple(want)


def _diff_opts(tol, max_iters):
    """tol: a positive finite real; max_iters: None (the default, 4 (n + m)) or a positive int"""
    t = _as_c_double("tol", tol)
    if isinstance(tol, (bool, np.bool_)) or not np.isfinite(t) or t <= 0:
        raise ValueError("tol must be a positive finite number")
    it = 0
    if max_iters is not None:
        it = _as_c_int("max_iters", max_iters)
        if isinstance(max_iters, (bool, np.bool_)) or it <= 0:
            raise ValueError("max_iters must be positive")
    return _ScsHipDiffOpts(t, it)


REFINE_STOP = {1: "converged", 2: "max_steps", 3: "no_decrease"}


def _refine_opts(tol, max_steps, lsqr_tol, lsqr_max_iters):
    """tol, lsqr_tol: positive finite reals; max_steps: an int >= 1; lsqr_max_iters: None (4 (n + m)) or a positive int"""
    vals = []
    for name, v in (("tol", tol), ("lsqr_tol", lsqr_tol)):
        t = _as_c_double(name, v)
        if isinstance(v, (bool, np.bool_)) or not np.isfinite(t) or t <= 0:
            raise ValueError("%s must be a positive finite number" % name)
        vals.append(t)
    steps = _as_c_int("max_steps", max_steps)
    if isinstance(max_steps, (bool, np.bool_)) or steps < 1:
        raise ValueError("max_steps must be at least 1")
    it = 0
    if lsqr_max_iters is not None:
        it = _as_c_int("lsqr_max_iters", lsqr_max_iters)
        if isinstance(lsqr_max_iters, (bool, np.bool_)) or it <= 0:
            raise ValueError("lsqr_max_iters must be positive")
    return _ScsHipRefineOpts(vals[0], steps, vals[1], it)


def _refine_info_dict(info):
    d = {name: getattr(info, name) for name, _ in _ScsHipRefineInfo._fields_}
    d["stop_reason"] = REFINE_STOP.get(d["stop"], "unknown")
    return d


def _device_vec(name, t, length, device):
    """The one argument check of the device-resident endpoints, before anything touches the device: `t` must be a float64, 1-D,
    contiguous torch tensor of `length` elements on GPU `device` (an index); returns its device address.  torch is imported here,
    not by `import scs`.  (Other device-array objects — DLPack, __cuda_array_interface__ — would be added here.)"""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor on the workspace's GPU, not %s" % (name, type(t).__name__))
    if t.dtype != torch.float64:
        raise TypeError("%s must be a float64 tensor, not %s" % (name, t.dtype))
    if t.dim() != 1 or t.shape[0] != length:
        raise ValueError("%s must be a 1-D tensor of length %d, not of shape %s" % (name, length, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if t.device.type != "cuda" or t.device.index != device:
        raise ValueError("%s must live on the workspace's GPU (cuda:%d), not on %s" % (name, device, t.device))
    return t.data_ptr()


def _sync_torch_stream(device):
    """Stream contract of the device-resident endpoints (include/scs_hip.h): what torch has queued on its current stream of `device`
    is complete before the library's own stream reads it."""
    import torch
    torch.cuda.current_stream(device).synchronize()


def _many_device_args(m, n, device, b, c, warm_start, x, y, s):
    """Argument checks of SCS.solve_many_device, before anything touches the device: (K, {name: (K, .) tensor or None}); every row goes
    through `_device_vec`."""
    if not isinstance(warm_start, (bool, np.bool_)):
        raise TypeError("argument 1 must be bool, not %s" % type(warm_start).__name__)
    rows = {"b": None, "c": None, "x": None, "y": None, "s": None}
    K = None
    for name, t, width, used in (("c", c, n, True), ("b", b, m, True), ("x", x, n, warm_start), ("y", y, m, warm_start),
                                 ("s", s, m, warm_start)):
        if t is None or not used:
            continue
        label = name + "_new" if name in ("b", "c") else name
        if not hasattr(t, "dim"):
            _device_vec(label, t, width, device)  # (not a tensor: its TypeError)
        if t.dim() != 2:
            raise ValueError("%s must be a 2-D tensor, one row per problem" % label)
        if K is not None and t.shape[0] != K:
            raise ValueError("%s must have one row per problem (%d), not %d" % (label, K, t.shape[0]))
        K = t.shape[0]
        if K < 1:
            raise ValueError("solve_many_device needs at least one problem")
        for i in range(K):
            _device_vec(label, t[i], width, device)
        rows[name] = t
    if K is None:
        K = 1
    return K, rows


def _many_args(m, n, b, c, warm_start, x, y, s):
    """Argument checks of SCS.solve_many, before anything touches the device: (K, {name: 2-D float64 array or None}).  The faults
    `update` / `solve` know keep their messages."""
    if not isinstance(warm_start, (bool, np.bool_)):
        raise TypeError("argument 1 must be bool, not %s" % type(warm_start).__name__)
    rows = {"b": None, "c": None, "x": None, "y": None, "s": None}
    K = None
    for name, arr, width in (("c", c, n), ("b", b, m)):
        if arr is None:
            continue
        if not isinstance(arr, np.ndarray) or not np.issubdtype(arr.dtype, np.floating) or arr.ndim != 2:
            raise TypeError("%s_new must be a 2-D numpy array of floats, one row per problem" % name)
        if arr.shape[1] != width:
            raise ValueError("%s_new has incompatible dimension with A" % name)
        if K is not None and arr.shape[0] != K:
            raise ValueError("b_new and c_new must have the same number of rows (one per problem)")
        K = arr.shape[0]
        rows[name] = np.array(arr, dtype=np.float64, order="C", copy=True)
    for name, arr, width in (("x", x, n), ("y", y, m), ("s", s, m)):
        if arr is None or not warm_start:
            continue
        if not isinstance(arr, np.ndarray) or not np.issubdtype(arr.dtype, np.floating) or arr.ndim != 2 or arr.shape[1] != width:
            raise ValueError("Unable to parse %s warm-start" % name)
        if K is not None and arr.shape[0] != K:
            raise ValueError("Unable to parse %s warm-start" % name)
        if K is None:
            K = arr.shape[0]
        rows[name] = np.ascontiguousarray(arr, dtype=np.float64)
    if K is None:
        K = 1
    if K < 1:
        raise ValueError("solve_many needs at least one problem")
    return K, rows


@contextlib.contextmanager
def _locked(solvers):
    """Every member's lock for the length of a grouped call, taken in `id` order — one global lock order: two overlapping batches
    cannot deadlock.  A finished member is refused; yields the C array of the members' workspaces, in the order given."""
    ordered = sorted(solvers, key=id)
    for sv in ordered:
        sv._lock.acquire()
    try:
        for sv in solvers:
            if not sv._work:
                raise ValueError("Workspace not initialized!")
        yield (C.c_void_p * len(solvers))(*[sv._work for sv in solvers])
    finally:
        for sv in ordered:
            sv._lock.release()


def _batch_solvers(solvers, who):
    solvers = list(solvers)
    for sv in solvers:
        if not isinstance(sv, SCS):
            raise TypeError("%s expects scs._scs_hip.SCS objects" % who)
    if len(set(id(sv) for sv in solvers)) != len(solvers):
        raise ValueError("%s: a solver appears twice" % who)
    return solvers


def solve_batch(solvers, warm_start=False):
    """Grouped solve of several backend `SCS` objects (include/scs_hip.h: scs_hip_solve_batch): equally shaped
    problems share every kernel launch of the ADMM loop.  Returns the list of result dicts `solve()` would have
    returned for each (iterates bit-identical to separate solves).  warm_start uses each object's stored solution.
    A member that fails comes back with status "failure" like a failed .solve(); RuntimeError only for argument /
    whole-call errors."""
    if not isinstance(warm_start, (bool, np.bool_)):
        raise TypeError("argument 2 must be bool, not %s" % type(warm_start).__name__)
    solvers = list(solvers)
    if not solvers:
        return []
    if len(set(id(sv) for sv in solvers)) != len(solvers):
        raise ValueError("solve_batch: a solver appears twice")
    for sv in solvers:
        if not isinstance(sv, SCS):
            raise TypeError("solve_batch expects scs._scs_hip.SCS objects")
    with _locked(solvers) as works:
        cnt = len(solvers)
        sols = [_ScsSolution(_pd(sv._x), _pd(sv._y), _pd(sv._s)) for sv in solvers]
        infos = [_ScsInfo() for _ in solvers]
        solp = (C.POINTER(_ScsSolution) * cnt)(*[C.pointer(so) for so in sols])
        infp = (C.POINTER(_ScsInfo) * cnt)(*[C.pointer(io) for io in infos])
        rc = _lib.scs_hip_solve_batch(works, solp, infp, cnt, 1 if warm_start else 0)  # GIL released by ctypes
        err = last_error() if rc != 0 else ""
        out = [{"x": sv._x.copy(), "y": sv._y.copy(), "s": sv._s.copy(), "info": _info_dict(io)}
               for sv, io in zip(solvers, infos)]
    # rc != 0 also when a single member ended SCS_FAILED: its dict says so (status_val -4, NaN vectors) exactly as .solve() would
    # report it, and the other members keep their results.  Only a call that failed as a whole raises.
    if rc != 0 and any(o["info"]["status_val"] == 0 for o in out):
        raise RuntimeError("libscs_hip: " + err)
    return out


def _plan_call(solvers, plan):
    """a grouping entry under every member's lock: plan(works, K, out) fills out[i] with member i's group"""
    with _locked(solvers) as works:
        out = (c_int * len(solvers))()
        rc = plan(works, len(solvers), out)
        err = last_error() if rc < 0 else ""
    if rc < 0:
        raise RuntimeError("libscs_hip: " + err)
    return [int(v) for v in out]


def batch_plan(solvers):
    """The grouping solve_batch(solvers) would use (include/scs_hip.h: scs_hip_batch_plan), without solving: a list with,
    for each solver, the index of the group it would join, or -1 where it would be solved alone."""
    solvers = list(solvers)
    if not solvers:
        return []
    if len(set(id(sv) for sv in solvers)) != len(solvers):
        raise ValueError("batch_plan: a solver appears twice")
    for sv in solvers:
        if not isinstance(sv, SCS):
            raise TypeError("batch_plan expects scs._scs_hip.SCS objects")
    return _plan_call(solvers, _lib.scs_hip_batch_plan)


# ---------------------------------------------------------------- derivatives: the two kinds, the two memories, the two call shapes
# A kind of derivative call is its vectors in the slot order of its C entries (include/scs_hip.h), each with the key of its length in
# `SCS._lens()`: `ins` are the public arguments in their order, the first `vectors` of them data vectors and the rest values of the
# matrices; `outs` are the results under the names they are returned by (a dict in slot order).  `entry` is the stem of its four C entries: + "_batch" for a
# list of members, + "_device" for device pointers.  `short`: the stem for a call whose matrix values are all None, which takes the
# slots without them (scs_hip_derivative[_batch][_device] are the full entries with NULL dAx and dPx, under their own names).
# `summed`: the results that are ONE vector for all members of a list — the sum over them — where the others are one per member; a kind
# with such results has list entries only, under its stem as it stands (scs_hip_adjoint_shared[_device]).
_DiffKind = collections.namedtuple("_DiffKind", "ins vectors outs entry short summed")
_ADJOINT = _DiffKind(ins=(("dx", "n"), ("dy", "m"), ("ds", "m")), vectors=3, outs={"db": "m", "dc": "n", "dA": "A", "dP": "P"},
                     entry="scs_hip_adjoint", short=None, summed=())  # (`want` selects among the outputs: "b" is db ...)
_DERIVATIVE = _DiffKind(ins=(("db", "m"), ("dc", "n"), ("dA", "A"), ("dP", "P")), vectors=2, outs={"dx": "n", "dy": "m", "ds": "m"},
                        entry="scs_hip_derivative_full", short="scs_hip_derivative", summed=())
_ADJOINT_SUM = _ADJOINT._replace(entry="scs_hip_adjoint_shared", summed=("dA", "dP"))  # members of ONE matrix: `reduce="sum"`


# K directions at ONE solution: the slots of the single entries, each a (K, .) stack, behind a count (`SCS._diff_multi`)
_ADJOINT_MULTI = _ADJOINT._replace(entry="scs_hip_adjoint_multi")
_DERIVATIVE_MULTI = _DERIVATIVE._replace(ins=_DERIVATIVE.ins[:2], entry="scs_hip_derivative_multi", short=None)
MULTI_MAX = 32  # directions per C call (include/scs_hip.h); more are served in chunks


def _multi_diff_args(spec, device=None):
    """Argument checks of the multi entries, before the library is called (pure Python; torch is touched only for device arguments).
    spec: (name, value, length) triples; a value is None (0 for every direction) or a (K, length) stack — on the host a numpy array of
    floats, on the device (device = the GPU index) a contiguous float64 torch tensor there.  K is read from the values: they must
    agree, and one at least must be given.  Returns (K, [None or the stack, as a fresh C-contiguous float64 array on the host])."""
    K, got = None, []
    for name, val, length in spec:
        if val is None:
            got.append(None)
            continue
        if device is None:
            if not isinstance(val, np.ndarray) or not np.issubdtype(val.dtype, np.floating):
                raise TypeError("%s must be a 2-D numpy array of floats, one row per direction" % name)
        else:
            import torch
            if not isinstance(val, torch.Tensor):
                raise TypeError("%s must be a 2-D torch.Tensor on the solver's GPU, one row per direction, not %s" % (name, type(val).__name__))
            if val.dtype != torch.float64:
                raise TypeError("%s must be a float64 tensor, not %s" % (name, val.dtype))
        if val.ndim != 2:
            raise ValueError("%s must be 2-D, one row per direction" % name)
        if int(val.shape[0]) < 1:
            raise ValueError("%s holds no direction" % name)
        if int(val.shape[1]) != length:
            raise ValueError("%s has incompatible dimension with A: rows of %d elements, not %d" % (name, length, int(val.shape[1])))
        if K is None:
            K = int(val.shape[0])
        if int(val.shape[0]) != K:
            raise ValueError("%s holds %d directions where the arguments before it hold %d" % (name, int(val.shape[0]), K))
        if device is None:
            got.append(np.array(val, dtype=np.float64, order="C", copy=True))
        else:
            if not val.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
            if val.device.type != "cuda" or val.device.index != device:
                raise ValueError("%s must live on the workspace's GPU (cuda:%d), not on %s" % (name, device, val.device))
            got.append(val)
    if K is None:
        raise ValueError("no direction given: %s are all None" % ", ".join(name for name, _, _ in spec))
    return K, got


def _diff_reduce(kind, reduce, want):
    """`reduce` of the adjoint of a list of members: None = every member's own dA / dP; "sum" = their sums over the members, which
    needs "A" or "P" in `want`.  Returns the kind that serves the call."""
    if reduce is None:
        return kind
    if not isinstance(reduce, str) or reduce != "sum":
        raise ValueError("reduce must be None or 'sum', not %r" % (reduce,))
    if isinstance(want, (tuple, list)) and not ("A" in want or "P" in want):
        raise ValueError("reduce='sum' sums the gradients of the matrices: want must hold 'A' or 'P'")
    return _ADJOINT_SUM

# Where the vectors live.  check(solver, name, value, key, lens): one input, checked before the library is called, as it goes on;
# zeros(shape): a result; address(vector): what C gets; ready(): right before the call; device: the GPU index, None on the host.
_Memory = collections.namedtuple("_Memory", "suffix device check zeros address ready")


def _host_check(sv, name, v, key, lens):
    return _diff_mat(name, v, sv._pattern[key]) if key in ("A", "P") else _diff_vec(name, v, lens[key])


_HOST = _Memory("", None, _host_check, np.zeros, lambda a: a.ctypes.data, lambda: None)


@functools.lru_cache(maxsize=None)
def _device_memory(dev):
    """float64 torch tensors on GPU `dev` (torch is imported here, not by `import scs`)"""
    import torch
    tdev = torch.device("cuda", dev)

    def check(sv, name, t, key, lens):
        if t is not None:
            _device_vec(name, t, lens[key], dev)
        return t

    # A result without an element: C takes a non-NULL output as wanted, whatever its length — the refusals for dPx fire, a batch groups
    # its members by it (csrc/scs_hip.hip diff_check, diff_batch_entry) — so NULL and the address of an empty array are two requests.
    # The host passes the address numpy gives an empty array; an empty tensor has none (its data_ptr() is 0), so here it is NULL.
    return _Memory("_device", dev, check, functools.partial(torch.zeros, dtype=torch.float64, device=tdev), torch.Tensor.data_ptr,
                   lambda: _sync_torch_stream(dev))  # the stream contract: inputs complete before the library's own stream reads them


def _diff_chosen(kind, want):
    """the names of the results: those `want` selects, in its order, or (None) all of the kind"""
    return ["d" + k for k in want] if want is not None else list(kind.outs)


def _diff_entry(kind, mem, batch, ins):
    """the C entry of a call and the inputs that fill its slots"""
    stem = kind.entry
    # dA is None and dP is None: the short entry (the same path in the library; a refusal then names the entry it always named)
    if kind.short and all(v is None for v in ins[kind.vectors:]):
        stem, ins = kind.short, ins[:kind.vectors]
    return getattr(_lib, stem + ("_batch" if batch and not kind.summed else "") + mem.suffix), ins


def _diff_info_dict(info):
    return {"iters": int(info.iters), "residual": float(info.residual), "normal_residual": float(info.normal_residual),
            "stop": int(info.stop), "time_ms": float(info.time_ms)}


def _diff_spec(kind, vals, lens):
    """the (name, value, length) triples `_many_diff_args` takes; lens: the `_lens()` of all members, or a list of each member's"""
    if isinstance(lens, dict):
        return tuple((name, v, lens[key]) for (name, key), v in zip(kind.ins, vals))
    return tuple((name, v, [ln[key] for ln in lens]) for (name, key), v in zip(kind.ins, vals))


def _many_diff_args(spec, K, want=None, have_P=True, device=None):
    """Argument checks of the batch derivative entries, before the library is called (pure Python; torch is touched only for device
    arguments).  spec: (name, value, length) triples; `length` is an int or a list of one int per member.  A value is None (0 for every
    member), a (K, length) array, or a sequence of K entries, each None or a vector of its member's length.  K: the number of members,
    or None to take it from the values (None where every value is None).  Host values: numpy arrays of floats, C-contiguous; device
    values (device = the GPU index): float64 contiguous torch tensors there.  Returns (K, {name: None or a list / 2-D array of K rows})."""
    if want is not None:
        _diff_want(want, have_P)
    rows = {}
    for name, val, length in spec:
        rows[name] = None
        if val is None:
            continue
        if name == "dP" and not have_P:
            raise ValueError("dP given, but the solver was created without P")
        two_d = not isinstance(val, (list, tuple)) and getattr(val, "ndim", None) == 2
        if not two_d and not isinstance(val, (list, tuple)):
            if device is None and not isinstance(val, np.ndarray):
                raise TypeError("%s must be a 2-D numpy array of floats, one row per problem, or a sequence of vectors" % name)
            if device is not None and not hasattr(val, "data_ptr"):
                raise TypeError("%s must be a 2-D torch.Tensor on the solver's GPU, one row per problem, or a sequence of tensors" % name)
            raise ValueError("%s must be 2-D, one row per problem" % name)
        cnt = int(val.shape[0]) if two_d else len(val)
        if K is None:
            K = cnt
        if cnt != K:
            raise ValueError("%s holds %d rows for %d problems" % (name, cnt, K))
        if K < 1:
            raise ValueError("a batch needs at least one problem")
        lens = length if isinstance(length, (list, tuple)) else [length] * K
        if two_d and device is None:
            if not isinstance(val, np.ndarray) or not np.issubdtype(val.dtype, np.floating):
                raise TypeError("%s must be a 2-D numpy array of floats" % name)
            if not val.flags["C_CONTIGUOUS"]:
                raise ValueError("%s must be C-contiguous" % name)
        got = []
        for i in range(K):
            v = val[i]
            if v is None:
                got.append(None)
            elif device is not None:
                _device_vec("%s[%d]" % (name, i), v, lens[i], device)
                got.append(v)
            else:
                if isinstance(v, np.ndarray) and v.ndim == 1 and not v.flags["C_CONTIGUOUS"]:
                    raise ValueError("%s[%d] must be contiguous" % (name, i))
                got.append(_diff_vec("%s[%d]" % (name, i), v, lens[i]))
        rows[name] = got
    return K, rows


def _ptr_array(K, ptrs):
    """a C array of K addresses (None entries = NULL), or None for `no such argument`"""
    if ptrs is None or all(p is None for p in ptrs):
        return None
    return (C.c_void_p * K)(*ptrs)


def _diff_batch_call(fn, solvers, ptr_lists, opts):
    """one call of a batch derivative entry under every member's lock; returns the K info dicts.  ptr_lists: per slot the K addresses
    of an array argument (or None), or ONE address (an int) where the slot is one vector for all members"""
    K = len(solvers)
    with _locked(solvers) as works:
        infos = [_ScsHipDiffInfo() for _ in solvers]
        infp = (C.POINTER(_ScsHipDiffInfo) * K)(*[C.pointer(io) for io in infos])
        rc = fn(works, *([pl if isinstance(pl, int) else _ptr_array(K, pl) for pl in ptr_lists] + [C.byref(opts), infp, K]))
        err = last_error() if rc != 0 else ""
    if rc != 0:
        raise ValueError("libscs_hip: " + err)
    return [_diff_info_dict(io) for io in infos]


def _diff_list(kind, mem, solvers, rows, lens, want, tol, max_iters, stacked=False):
    """`kind` of a list of distinct members in ONE call of its batch entry.  rows: what `_many_diff_args` made of the inputs; lens: each
    member's `_lens()`.  Returns one result dict per member — or (stacked: members of one shape) one dict of (K, .) stacks, whose rows
    the call writes straight into, with the list of the K infos.  The results a kind sums over the members (kind.summed) are one vector
    each: an entry of the stacked dict, or — member by member — a second dict beside the list, (results, grads)."""
    K = len(solvers)
    opts = _diff_opts(tol, max_iters)
    chosen, sizes = _diff_chosen(kind, want), kind.outs
    one = [k for k in chosen if k in kind.summed]
    if stacked:
        out = cols = {k: mem.zeros(lens[0][sizes[k]] if k in one else (K, lens[0][sizes[k]])) for k in chosen}
    else:
        grads = {k: mem.zeros(lens[0][sizes[k]]) for k in one}
        out = [{k: mem.zeros(ln[sizes[k]]) for k in chosen if k not in one} for ln in lens]
        cols = {k: grads[k] if k in one else [o[k] for o in out] for k in chosen}
    fn, ins = _diff_entry(kind, mem, True, [rows[name] for name, _ in kind.ins])
    ptrs = [[mem.address(v) if v is not None else None for v in r] if r is not None else None for r in ins]
    ptrs += [(int(mem.address(cols[k])) if k in one else [mem.address(a) for a in cols[k]]) if k in cols else None for k in kind.outs]
    mem.ready()
    infos = _diff_batch_call(fn, solvers, ptrs, opts)
    if stacked:
        out["info"] = infos
    else:
        for o, info in zip(out, infos):
            o["info"] = info
    return (out, grads) if kind.summed and not stacked else out


def _diff_batch(kind, device, who, solvers, vals, want, tol, max_iters, reduce=None):
    """`kind` of a list of solvers the caller names: vals = one sequence (or (K, .) array) per input, in the order of kind.ins"""
    kind = _diff_reduce(kind, reduce, want)
    solvers = _batch_solvers(solvers, who)
    dev = None
    if device:
        devs = set(sv._device_index() for sv in solvers)
        if len(devs) > 1:
            raise ValueError("%s: the solvers live on different GPUs" % who)
        dev = devs.pop() if devs else 0
    if not solvers:
        return ([], {}) if kind.summed else []
    lens = [sv._lens() for sv in solvers]
    have_P = all(sv._pattern["P"] is not None for sv in solvers)
    _, rows = _many_diff_args(_diff_spec(kind, vals, lens), len(solvers), want, have_P, device=dev)
    return _diff_list(kind, _device_memory(dev) if device else _HOST, solvers, rows, lens, want, tol, max_iters)


def adjoint_batch(solvers, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None, reduce=None):
    """`adjoint` of several solved backend `SCS` objects in one call (include/scs_hip.h: scs_hip_adjoint_batch): equally shaped members
    share every kernel launch of the LSQR iteration.  dx, dy, ds: sequences (or (K, .) arrays) with one vector per solver; None, or a
    None entry, counts as 0.  Returns the list of dicts `adjoint` would return for each, with the same bits.  reduce="sum" (with "A" or
    "P" in `want`; the solvers must share one matrix: a solver and its `clone()`s): the pair (results, grads) — the dicts without
    dA / dP, and {"dA", "dP"} summed over the solvers (scs_hip_adjoint_shared)."""
    return _diff_batch(_ADJOINT, False, "adjoint_batch", solvers, (dx, dy, ds), want, tol, max_iters, reduce)


def derivative_batch(solvers, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
    """`derivative` of several solved backend `SCS` objects in one call: db, dc, dA, dP as the vectors of `adjoint_batch` (dA / dP: one
    value array of nnz(A) / nnz(P) elements per solver).  Returns the list of dicts `derivative` would return for each, with the same
    bits."""
    return _diff_batch(_DERIVATIVE, False, "derivative_batch", solvers, (db, dc, dA, dP), None, tol, max_iters)


def adjoint_batch_device(solvers, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None, reduce=None):
    """`adjoint_batch` over float64 torch tensors on the solvers' GPU (taken and returned); same bits."""
    return _diff_batch(_ADJOINT, True, "adjoint_batch_device", solvers, (dx, dy, ds), want, tol, max_iters, reduce)


def derivative_batch_device(solvers, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
    """`derivative_batch` over float64 torch tensors on the solvers' GPU."""
    return _diff_batch(_DERIVATIVE, True, "derivative_batch_device", solvers, (db, dc, dA, dP), None, tol, max_iters)


def diff_batch_plan(solvers, want=("b", "c")):
    """The grouping `adjoint_batch(solvers, want=want)` / `derivative_batch(solvers)` would use (include/scs_hip.h:
    scs_hip_diff_batch_plan): for each solver the index of the group it would share launches with, -1 where it is served alone."""
    solvers = _batch_solvers(solvers, "diff_batch_plan")
    if not solvers:
        return []
    want = _diff_want(want, True)
    return _plan_call(solvers, lambda works, K, out: _lib.scs_hip_diff_batch_plan(works, K, 1 if "A" in want else 0, 1 if "P" in want else 0, out))


def data_perturbation(solver, dA=None, dP=None):
    """(dP x + dA' y, dA x) at the resident solution of a solved backend `SCS` (include/scs_hip.h: scs_hip_data_perturbation): the
    perturbation products of `derivative(dA=, dP=)` on their own, on host arrays (tests)."""
    if not isinstance(solver, SCS):
        raise TypeError("data_perturbation expects a scs._scs_hip.SCS object")
    return solver.data_perturbation(dA, dP)


def diff_group_launches():
    """Grouped launches the batch derivative entries have issued in this process (tests, tools/adjoint_batch_bench.py)."""
    return int(_lib.scs_hip_diff_group_launches())


def diff_group_syncs():
    """Host synchronisations the groups of the batch derivative and refine entries have made in this process (tools)."""
    return int(_lib.scs_hip_diff_group_syncs())


# ---------------------------------------------------------------- Newton polish of a batch (include/scs_hip.h: scs_hip_refine_batch)
def _refine_solvers(solvers, who):
    """the list a refine_batch call names: a list or tuple of distinct backend SCS objects, each refusal with its member's index"""
    if not isinstance(solvers, (list, tuple)):
        raise TypeError("%s expects a list of solvers, not %s" % (who, type(solvers).__name__))
    if not solvers:
        raise ValueError("%s: the list of solvers is empty: there is no member 0" % who)
    seen = set()
    for i, sv in enumerate(solvers):
        if not isinstance(sv, SCS):
            raise TypeError("%s: member %d: expects scs._scs_hip.SCS objects, not %s" % (who, i, type(sv).__name__))
        if id(sv) in seen:
            raise ValueError("%s: member %d: a solver appears twice" % (who, i))
        seen.add(id(sv))
    return list(solvers)


def _refine_list(solvers, opts, device, stacked=False):
    """ONE call of scs_hip_refine_batch[_device] over distinct members, under every member's lock.  Host: every member's x, y, s land
    in its own result arrays (as `refine`) and come back as copies.  Device: fresh float64 torch tensors on the members' GPU — per
    member, or (stacked: members of one shape) three (K, .) stacks whose rows the call writes.  Returns the list of result dicts, or
    the stacked dict with the list of infos."""
    K = len(solvers)
    if device:
        import torch
        devs = set(sv._device_index() for sv in solvers)
        if len(devs) > 1:
            raise ValueError("refine_batch_device: the solvers live on different GPUs")
        dev = devs.pop()
        tdev = torch.device("cuda", dev)
        if stacked:
            out = {"x": torch.empty((K, solvers[0].n), dtype=torch.float64, device=tdev),
                   "y": torch.empty((K, solvers[0].m), dtype=torch.float64, device=tdev),
                   "s": torch.empty((K, solvers[0].m), dtype=torch.float64, device=tdev)}
            rows = [{k: out[k][i] for k in "xys"} for i in range(K)]
        else:
            rows = [{"x": torch.empty(sv.n, dtype=torch.float64, device=tdev), "y": torch.empty(sv.m, dtype=torch.float64, device=tdev),
                     "s": torch.empty(sv.m, dtype=torch.float64, device=tdev)} for sv in solvers]
    with _locked(solvers) as works:
        if device:
            _sync_torch_stream(dev)
            sols = [_ScsSolution(C.cast(r["x"].data_ptr(), _PD), C.cast(r["y"].data_ptr(), _PD), C.cast(r["s"].data_ptr(), _PD)) for r in rows]
        else:
            sols = [_ScsSolution(_pd(sv._x), _pd(sv._y), _pd(sv._s)) for sv in solvers]
        solp = (C.POINTER(_ScsSolution) * K)(*[C.pointer(so) for so in sols])
        infos = [_ScsHipRefineInfo() for _ in solvers]
        infp = (C.POINTER(_ScsHipRefineInfo) * K)(*[C.pointer(io) for io in infos])
        fn = _lib.scs_hip_refine_batch_device if device else _lib.scs_hip_refine_batch
        rc = fn(works, solp, C.byref(opts), infp, K)
        err = last_error() if rc != 0 else ""
        if rc == 0 and not device:
            rows = [{"x": sv._x.copy(), "y": sv._y.copy(), "s": sv._s.copy()} for sv in solvers]
    if rc != 0:
        raise ValueError("libscs_hip: " + err)
    dicts = [_refine_info_dict(io) for io in infos]
    if stacked:
        out["info"] = dicts
        return out
    for r, d in zip(rows, dicts):
        r["info"] = d
    return rows


def refine_batch(solvers, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None):
    """`refine` of several solved backend `SCS` objects in one call (include/scs_hip.h: scs_hip_refine_batch): equally shaped members
    are polished in lock step — one launch per kernel and one host synchronisation per evaluation for the group — each with its own
    number of steps, halvings and stop reason.  Returns the list of dicts `refine` would return for each, with the same bits
    (info["time_ms"] is the group's).  The options hold for every member."""
    solvers = _refine_solvers(solvers, "refine_batch")
    return _refine_list(solvers, _refine_opts(tol, max_steps, lsqr_tol, lsqr_max_iters), False)


def refine_batch_device(solvers, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None):
    """`refine_batch` with every member's "x", "y", "s" as fresh float64 torch tensors on the solvers' GPU; same bits."""
    solvers = _refine_solvers(solvers, "refine_batch_device")
    return _refine_list(solvers, _refine_opts(tol, max_steps, lsqr_tol, lsqr_max_iters), True)


# ---------------------------------------------------------------- kernel-level entry points (tests, bench)
def _matrix(A):
    """scipy CSC -> (_ScsMatrix, keepalive)"""
    x = np.ascontiguousarray(A.data, dtype=np.float64)
    i = np.ascontiguousarray(A.indices, dtype=np.int32)
    p = np.ascontiguousarray(A.indptr, dtype=np.int32)
    return _ScsMatrix(_pd(x), _pi(i), _pi(p), A.shape[0], A.shape[1]), (x, i, p)


def _cone_struct(cone):
    z = _cone_pos_int(cone, "z") + _cone_pos_int(cone, "f")
    bu, bl = _cone_float_list(cone, "bu"), _cone_float_list(cone, "bl")
    q, s, cs = _cone_int_list(cone, "q"), _cone_int_list(cone, "s"), _cone_int_list(cone, "cs")
    p = _cone_float_list(cone, "p")
    k = _ScsCone(z, _cone_pos_int(cone, "l"), _pd(bu), _pd(bl), (bu.size + 1) if bu.size else 0,
                 _pi(q), q.size, _pi(s), s.size, _pi(cs), cs.size,
                 _cone_pos_int(cone, "ep"), _cone_pos_int(cone, "ed"), _pd(p), p.size)
    spec = _spectral_lists(cone)
    _set_spectral(k, spec)
    return k, (bu, bl, q, s, cs, p, spec)


def _check(rc):
    if rc != 0:
        raise RuntimeError("libscs_hip: " + last_error())


def spmv(A, x, transpose=False):
    """y = A x (or A' x) through the hot-path SpMV kernel; A scipy CSC."""
    M, keep = _matrix(A)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    y = np.zeros(A.shape[1] if transpose else A.shape[0])
    _check(_lib.scs_hip_spmv(C.byref(M), _pd(xx), _pd(y), 1 if transpose else 0))
    return y


def cs_layout_host_spmv(A, x, transpose=False, rpt=0, split=1):
    """HOST-ONLY: A x (or A' x) evaluated by walking the column-sorted pass layout of the large-matrix SpMV kernels
    as built by the host builder; None when the pattern does not fit the format.  (tests, no GPU needed)"""
    M, keep = _matrix(A)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    y = np.zeros(A.shape[1] if transpose else A.shape[0])
    rc = _lib.scs_hip_cs_layout_host_spmv(C.byref(M), _pd(xx), _pd(y), 1 if transpose else 0, int(rpt), int(split))
    if rc == 1:
        return None
    _check(rc)
    return y


def cs_layout_host_spmv_pieces(A, x, transpose=False, piece_len=24):
    """HOST-ONLY: the same walk for the virtual-row variant of the layout — rows too long for the count fields cut into pieces of
    at most piece_len nonzeros that ride in the passes, a row's pieces added as the device adds them; None when no row is that
    long or the pattern does not fit.  (tests, no GPU needed)"""
    M, keep = _matrix(A)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    y = np.zeros(A.shape[1] if transpose else A.shape[0])
    rc = _lib.scs_hip_cs_layout_host_spmv_pieces(C.byref(M), _pd(xx), _pd(y), 1 if transpose else 0, int(piece_len))
    if rc == 1:
        return None
    _check(rc)
    return y


def spmv_bench(A, transpose=False, reps=20):
    M, keep = _matrix(A)
    ms = _lib.scs_hip_spmv_bench(C.byref(M), 1 if transpose else 0, int(reps))
    if ms < 0:
        raise RuntimeError("libscs_hip: " + last_error())
    return ms


def proj_cone(z, cone, dual=False):
    x = np.array(z, dtype=np.float64, copy=True)
    k, keep = _cone_struct(cone)
    _check(_lib.scs_hip_proj_cone_spectral(_pd(x), C.byref(k), x.size, 1 if dual else 0))
    return x


def dproj_cone(v, u, cone):
    """(W u, (W - I) u) with W the derivative of the projection onto the cone at v: the kernels of `SCS.adjoint` (z, l, box, q, s and p cones)"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    if v.ndim != 1 or v.shape != u.shape:
        raise ValueError("v and u must be 1-D arrays of one length")
    k, _keep = _cone_struct(cone)
    wu, wmiu = np.zeros_like(v), np.zeros_like(v)
    _check(_lib.scs_hip_dproj_cone(_pd(v), _pd(u), C.byref(k), v.shape[0], _pd(wu), _pd(wmiu)))
    return wu, wmiu


def grad_matrix_sum(A, P, X, Y, DB, DC):
    """(dA, dP): the summed matrix gradients of K members from their stacks X, DC (K, n) and Y, DB (K, m) over the patterns of the scipy
    CSC matrices A (m x n) and P (an upper triangle of order n, or None: dP is None) — the pack and sum kernels of
    `adjoint_many(reduce="sum")` on their own (include/scs_hip.h: scs_hip_grad_matrix_sum; tests)."""
    m, n = A.shape
    X, Y, DB, DC = (np.ascontiguousarray(v, dtype=np.float64) for v in (X, Y, DB, DC))
    K = X.shape[0] if X.ndim == 2 else 0
    for name, v, ln in (("X", X, n), ("Y", Y, m), ("DB", DB, m), ("DC", DC, n)):
        if v.ndim != 2 or v.shape != (K, ln):
            raise ValueError("%s must be a (K, %d) array" % (name, ln))
    ap, ai = np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32)
    dA, dP, pp, pi = np.zeros(ai.shape[0]), None, None, None
    if P is not None:
        if P.shape != (n, n):
            raise ValueError("P must be %d x %d" % (n, n))
        pp, pi = np.ascontiguousarray(P.indptr, dtype=np.int32), np.ascontiguousarray(P.indices, dtype=np.int32)
        dP = np.zeros(pi.shape[0])
    _check(_lib.scs_hip_grad_matrix_sum(m, n, _pi(ap), _pi(ai), _pi(pp) if pp is not None else None, _pi(pi) if pi is not None else None,
                                        K, _pd(X), _pd(Y), _pd(DB), _pd(DC), _pd(dA), _pd(dP) if dP is not None else None))
    return dA, dP


def trim_pool():
    """return the library's cached device blocks to the driver (include/scs_hip.h scs_hip_trim_pool)"""
    _lib.scs_hip_trim_pool()


def pool_stats():
    """the block pool's account (include/scs_hip.h scs_hip_pool_stats): dict of held_bytes, held_blocks, live_bytes, hits, misses"""
    st = _ScsHipPoolStats()
    _lib.scs_hip_pool_stats(C.byref(st))
    return {name: int(getattr(st, name)) for name, _ in _ScsHipPoolStats._fields_}


def tiled_launches():
    """tiled CSR-stream launches (one read of a shared matrix per tile of members) issued by grouped solves of this process so far"""
    return int(_lib.scs_hip_tiled_launches())


def spin_fallbacks():
    """solves of this process restarted without spinning multi-workgroup kernels after a barrier timed out (include/scs_hip.h)"""
    return int(_lib.scs_hip_spin_fallbacks())


def _no_spectral(cone, what):
    """entry points whose C functions read ScsCone only up to psize (include/scs_hip.h): refuse spectral keys with a reason"""
    k, keep = _cone_struct(cone)
    if k.dsize or k.nucsize or k.ell1_size or k.sl_size:
        raise ValueError("%s: spectral cones (d, nuc, ell1, sl) are not supported by this entry point" % what)
    return k, keep


def proj_cone_seq(zs, cone, dual=False, stats_cap=0):
    """rows of zs projected one after the other through one set of warm-started cone workspaces (include/scs_hip.h);
    returns (projections, refinement records of the large PSD matrices)"""
    xs = np.array(zs, dtype=np.float64, copy=True, order="C")
    assert xs.ndim == 2
    k, keep = _no_spectral(cone, "proj_cone_seq")
    st = np.zeros(8 * max(stats_cap, 1))
    cnt = _lib.scs_hip_proj_cone_seq(_pd(xs), C.byref(k), xs.shape[1], 1 if dual else 0, xs.shape[0], _pd(st), int(stats_cap))
    if cnt < 0:
        raise RuntimeError("libscs_hip: " + last_error())
    return xs, st[:8 * cnt].reshape(cnt, 8)


def kkt_solve(A, P, diag_r, rhs, tol=1e-12):
    M, keep = _matrix(A)
    Pm = None
    if P is not None:
        Pm, keep2 = _matrix(P)
    r = np.array(rhs, dtype=np.float64, copy=True)
    dr = np.ascontiguousarray(diag_r, dtype=np.float64)
    its = c_int(0)
    _check(_lib.scs_hip_kkt_solve(C.byref(M), C.byref(Pm) if Pm is not None else None, _pd(dr), _pd(r),
                                  float(tol), C.byref(its)))
    return r, its.value


def kkt_solve_dense(A, P, diag_r, rhs):
    """The same KKT system through the dense direct linsys (csrc/dense.hpp): explicit inverse of the reduced matrix."""
    M, keep = _matrix(A)
    Pm = None
    if P is not None:
        Pm, keep2 = _matrix(P)
    r = np.array(rhs, dtype=np.float64, copy=True)
    dr = np.ascontiguousarray(diag_r, dtype=np.float64)
    _check(_lib.scs_hip_kkt_solve_dense(C.byref(M), C.byref(Pm) if Pm is not None else None, _pd(dr), _pd(r)))
    return r


def _normalize(entry, k, A, P, b, c):
    M, keepA = _matrix(A.copy())
    Pm, keepP = (None, None)
    if P is not None:
        Pm, keepP = _matrix(P.copy())
    bb = np.array(b, dtype=np.float64, copy=True)
    cc = np.array(c, dtype=np.float64, copy=True)
    D, E, sig = np.zeros(A.shape[0]), np.zeros(A.shape[1]), np.zeros(1)
    _check(entry(C.byref(M), C.byref(Pm) if Pm is not None else None, _pd(bb), _pd(cc), C.byref(k), _pd(D), _pd(E), _pd(sig)))
    return keepA[0], (keepP[0] if keepP else None), bb, cc, D, E, float(sig[0])


def normalize(A, P, b, c, cone):
    """Returns (A_data_hat, P_data_hat, b_hat, c_hat, D, E, sigma) as scs_init computes them."""
    k, keep = _no_spectral(cone, "normalize")
    return _normalize(_lib.scs_hip_normalize, k, A, P, b, c)


def normalize_spectral(A, P, b, c, cone):
    """`normalize` for a cone that may carry spectral keys (d, nuc_m/nuc_n, ell1, sl_n/sl_k): each such cone is one block of rows
    with one scale (include/scs_hip.h scs_hip_normalize_spectral)."""
    k, keep = _cone_struct(cone)
    return _normalize(_lib.scs_hip_normalize_spectral, k, A, P, b, c)


def copy_bandwidth(nbytes=1 << 30, reps=10):
    return float(_lib.scs_hip_copy_bandwidth(int(nbytes), int(reps)))


_AA_STAT_FIELDS = ("iter", "n_accept", "n_reject_lapack", "n_reject_rank0", "n_reject_nonfinite",
                   "n_reject_weight_cap", "n_safeguard_reject", "last_rank", "last_aa_norm", "last_regularization")


class AndersonAccelerator(object):
    """The device Anderson accelerator of the ADMM loop as a standalone object on host vectors — the
    aa_init / aa_apply / aa_safeguard / aa_reset interface of the SCS core's aa.c (tests drive it next to the oracle)."""

    def __init__(self, dim, mem, type1=True, regularization=1e-8, relaxation=1.0, safeguard_factor=1.0,
                 max_weight_norm=1e10):
        self._h = _lib.scs_hip_aa_init(int(dim), int(mem), 1 if type1 else 0, float(regularization),
                                       float(relaxation), float(safeguard_factor), float(max_weight_norm))
        if not self._h:
            raise RuntimeError("libscs_hip: " + last_error())
        self.dim = int(dim)

    def apply(self, f, x):
        """f = F(x).  Returns (aa_norm, f_out): f_out is the extrapolated iterate when the step was accepted."""
        ff = np.array(f, dtype=np.float64, copy=True)
        xx = np.ascontiguousarray(x, dtype=np.float64)
        assert ff.size == self.dim and xx.size == self.dim
        nrm = _lib.scs_hip_aa_apply(self._h, _pd(ff), _pd(xx))
        if nrm != nrm and last_error():
            raise RuntimeError("libscs_hip: " + last_error())
        return nrm, ff

    def safeguard(self, f_new, x_new):
        """Returns (rc, f_new, x_new); rc = -1: rejected, the pair was rolled back to the pre-extrapolation one."""
        ff = np.array(f_new, dtype=np.float64, copy=True)
        xx = np.array(x_new, dtype=np.float64, copy=True)
        rc = _lib.scs_hip_aa_safeguard(self._h, _pd(ff), _pd(xx))
        if rc == -2:
            raise RuntimeError("libscs_hip: " + last_error())
        return rc, ff, xx

    def reset(self):
        _lib.scs_hip_aa_reset(self._h)

    def stats(self):
        st = _ScsAaStats()
        _lib.scs_hip_aa_get_stats(self._h, C.byref(st))
        return {k: getattr(st, k) for k in _AA_STAT_FIELDS}

    def last_gamma(self):
        n = _lib.scs_hip_aa_last_gamma(self._h, None)
        g = np.zeros(max(n, 1))
        _lib.scs_hip_aa_last_gamma(self._h, _pd(g))
        return g[:n]

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.scs_hip_aa_finish(h)
