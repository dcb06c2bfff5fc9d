"""`scs` — drop-in Python front end for the MI355X-native SCS hot path.

Mirrors the reference's pure-Python layer R:scs/py/__init__.py (L0/L1 of
SURVEY.md §1): `SCS(data, cone, **settings)` (:87-184), `.solve(warm_start, x,
y, s)` (:186-203), `.update(b, c)` (:205-214), legacy `solve(data, cone,
**settings)` (:218-230), the `LinearSolver` enum and its enum->module dispatch
(:28-74) and the status integers (:16-25).  Behaviour kept identical: argument
checks and their messages, CSC coercion with a warning, never mutating the
caller's matrices, upper-triangular extraction of P, `linear_solver` popped
before the backend sees the settings.

What differs: the backend modules shipped here are `scs._scs_hip`
(`LinearSolver.HIP_INDIRECT`) and `scs._scs_hip_dense` (`LinearSolver.HIP_DENSE`);
`AUTO` resolves — as the reference's does (R:scs/py/__init__.py:45-54: "the best
available direct solver") — to the direct one when it can take the problem and to
the indirect one otherwise (`_resolve_auto`); the CPU/CUDA members raise ImportError
exactly like an un-built optional backend of the reference does
(R:test/test_solve_random_cone_prob.py:24-30).
"""
import enum
import warnings
from importlib import import_module

import numpy as np
from scipy import sparse

from scs import _scs_hip

__version__ = _scs_hip.version()
__sizeof_int__ = _scs_hip.sizeof_int()
__sizeof_float__ = _scs_hip.sizeof_float()

# exit flags of scs_solve (R:scs/py/__init__.py:16-25)
INFEASIBLE_INACCURATE = -7
UNBOUNDED_INACCURATE = -6
SIGINT = -5
FAILED = -4
INDETERMINATE = -3
INFEASIBLE = -2
UNBOUNDED = -1
UNFINISHED = 0
SOLVED = 1
SOLVED_INACCURATE = 2


class LinearSolver(enum.Enum):
  """Which linear-system backend module `SCS` instantiates."""
  AUTO = "auto"
  QDLDL = "qdldl"
  CPU_INDIRECT = "cpu_indirect"
  MKL = "mkl"
  ACCELERATE = "accelerate"
  CPU_DENSE = "cpu_dense"
  GPU_INDIRECT = "gpu_indirect"
  CUDSS = "cudss"
  HIP_INDIRECT = "hip_indirect"  # MI355X (gfx950): device-resident indirect solver
  HIP_DENSE = "hip_dense"  # MI355X (gfx950): device dense direct solver for small problems (n <= 8192)


# enum member -> extension-module name under the `scs` package
_BACKEND_MODULES = {
    LinearSolver.QDLDL: "_scs_direct",
    LinearSolver.CPU_INDIRECT: "_scs_indirect",
    LinearSolver.MKL: "_scs_mkl",
    LinearSolver.ACCELERATE: "_scs_accelerate",
    LinearSolver.CPU_DENSE: "_scs_dense",
    LinearSolver.GPU_INDIRECT: "_scs_gpu",
    LinearSolver.CUDSS: "_scs_cudss",
    LinearSolver.HIP_INDIRECT: "_scs_hip",
    LinearSolver.HIP_DENSE: "_scs_hip_dense",
}


def _load_module(name):
  return import_module("scs." + name)


# AUTO's view of the dense direct solver (csrc/dense.hpp): the order up to which it wins a whole solve against the indirect path
# (measured: profiles/r06_auto_crossover.txt — 2.4 x at n = 1350, 1.3 x at 4096, 0.6-0.7 x at 6144 / 8192, where the 2 n^3-flop
# re-inversions at every adaptive-scale update and the 8 n^2-byte product per iteration cost more than ~10 launch-bound PCG steps;
# `LinearSolver.HIP_DENSE` by name accepts n <= 8192), the share of the free HBM its inverse may take and the work of forming
# G = R_x + P + A' R_y^-1 A (one product per pair of nonzeros of a row of A) it is worth paying at every scale update.
_AUTO_DENSE_MAX_N = 4096
_AUTO_DENSE_HBM_SHARE = 0.25
_AUTO_DENSE_MAX_BUILD_PRODUCTS = 2e9


def _dense_direct_fits(m, n, A):
  """True when the device's direct solver can take an m x n problem with the CSC matrix A."""
  if n > _AUTO_DENSE_MAX_N:
    return False
  info = _scs_hip.mem_info()
  if info is None:  # no device: let the indirect module report it ("ScsWork allocation error! (no HIP device ...)")
    return False
  npad = -(-n // 64) * 64
  if 8.0 * npad * npad > _AUTO_DENSE_HBM_SHARE * info[0]:
    return False
  if A is not None and A.nnz:
    try:
      row_len = np.bincount(A.indices, minlength=m).astype(np.float64)
    except ValueError:  # negative row indices: the backend's own validation reports them
      return False
    if float(row_len @ row_len) > _AUTO_DENSE_MAX_BUILD_PRODUCTS:
      return False
  return True


def _resolve_auto(m=None, n=None, A=None):
  """AUTO = the best DIRECT solver that is usable, as in the reference (R:scs/py/__init__.py:45-54: MKL Pardiso, else the
  bundled QDLDL).  Here: the dense direct solver of the device when the problem fits it (n <= 4096, the n x n inverse within a
  quarter of the free HBM, G cheap to form), else the indirect solver — a sparse factorisation of the BASELINE patterns fills to
  0.06 N^2 and does not exist on the device."""
  if n is not None and _dense_direct_fits(m, n, A):
    return _load_module("_scs_hip_dense")
  return _scs_hip


def _select_scs_module(stgs, m=None, n=None, A=None):
  """Pop `linear_solver` (enum member or its string value) and load that backend."""
  choice = stgs.pop("linear_solver", LinearSolver.AUTO)
  if isinstance(choice, str):
    choice = LinearSolver(choice)
  if choice is LinearSolver.AUTO:
    return _resolve_auto(m, n, A)
  if choice is LinearSolver.HIP_INDIRECT:
    return _scs_hip
  return _load_module(_BACKEND_MODULES[choice])


def _has_lower_tri(P):
  """True when a sorted CSC matrix stores anything strictly below the diagonal."""
  counts = np.diff(P.indptr)
  cols = np.flatnonzero(counts)
  if cols.size == 0:
    return False
  bottom = P.indices[P.indptr[cols + 1] - 1]  # largest row index of each non-empty column
  return bool((bottom > cols).any())


def _csc_sorted(M, what):
  """CSC with sorted indices, never touching the caller's object."""
  if M.format != "csc":
    warnings.warn("Converting %s to a CSC (compressed sparse column) matrix; may take a while." % what)
    M = M.tocsc()
  if not M.has_sorted_indices:
    M = M.sorted_indices()  # a copy; sort_indices() would mutate the caller's matrix
  return M


def _dense_1d(v):
  if sparse.issparse(v):
    return np.asarray(v.todense()).ravel()
  return v


def _update_arg(M, what, upper):
  """A matrix argument of `SCS.update_matrix` as the backend takes it: a sparse matrix becomes the (data, indices, indptr) of the form
  the constructor hands over (`_csc_sorted`, upper triangle for P), anything else passes through."""
  if M is None or not sparse.issparse(M):
    return M
  M = _csc_sorted(M, what)
  if upper and _has_lower_tri(M):
    M = sparse.triu(M, format="csc")
  return (M.data, M.indices, M.indptr)


class SCS(object):

  def __init__(self, data, cone, **settings):
    """Set up a solver workspace.

    @param data     dict with `A`, `b`, `c` and optionally `P`.
    @param cone     dict describing the cone K.
    @param settings solver settings as keyword arguments, plus `linear_solver`.
    """
    self._settings = settings
    if not data or not cone:
      raise ValueError("Missing data or cone information")
    if "b" not in data or "c" not in data:
      raise ValueError("Missing one of b, c from data dictionary")
    if "A" not in data:
      raise ValueError("Missing A from data dictionary")
    A, b, c = data["A"], data["b"], data["c"]
    if A is None or b is None or c is None:
      raise ValueError("Incomplete data specification")
    if not sparse.issparse(A):
      raise TypeError("A is required to be a sparse matrix")
    A = _csc_sorted(A, "A")
    b, c = _dense_1d(b), _dense_1d(c)
    m, n = len(b), len(c)
    if A.shape != (m, n):
      raise ValueError("A shape not compatible with b,c")

    Px = Pi = Pp = None
    P = data.get("P", None)
    if P is not None:
      if not sparse.issparse(P):
        raise TypeError("P is required to be a sparse matrix")
      if P.shape != (n, n):
        raise ValueError("P shape not compatible with A,b,c")
      P = _csc_sorted(P, "P")
      if _has_lower_tri(P):  # the core wants the upper triangle only
        P = sparse.triu(P, format="csc")
      Px, Pi, Pp = P.data, P.indices, P.indptr

    backend = _select_scs_module(self._settings, m, n, A)
    self._solver = backend.SCS((m, n), A.data, A.indices, A.indptr, Px, Pi, Pp, b, c, cone,
                               **self._settings)

  def solve(self, warm_start=True, x=None, y=None, s=None):
    """Run the solver.

    @param warm_start  start from the previous solution (or from x, y, s when given).
    @return dict with keys 'x', 'y', 's', 'info'.
    """
    return self._solver.solve(warm_start, x, y, s)

  def update(self, b=None, c=None):
    """Replace `b` and/or `c`, re-using the workspace for the next solve."""
    self._solver.update(b, c)


  def update_matrix(self, A=None, P=None):
    """Replace the VALUES of `A` and / or `P`, keeping the sparsity pattern the solver was created with (None = keep).  Each argument
    is a scipy sparse matrix — brought to the form the constructor uses (sorted CSC, upper triangle of P; explicit zeros stay), its
    pattern must equal the constructor's, else ValueError — or a 1-D float array of the stored values in that order.  The solver is
    then in the state a new `SCS` on the new matrices and the current b, c would be in (cold start: pass x, y, s to `solve` for a warm
    one); clones held by the caller must be gone (ValueError otherwise)."""
    self._solver.update_matrix(_update_arg(A, "A", False), _update_arg(P, "P", True))

  def update_matrix_device(self, A=None, P=None):
    """`update_matrix` for values on the solver's GPU: float64, 1-D, contiguous torch tensors of the stored values in the constructor's
    CSC order (P: its upper triangle).  The tensors must be complete on torch's current stream (the call synchronises it)."""
    self._solver.update_matrix_device(A, P)

  def clone(self):
    """A second solver over the SAME device matrix: the state this one had when it was constructed (its original b, c and
    settings, cold start); only per-solve state is allocated.  Solve it on its own, from another thread, or in `solve_batch`."""
    new = object.__new__(SCS)
    new._settings = dict(self._settings)
    new._solver = self._solver.clone()
    return new

  def shares_matrix(self, other):
    """True when `other` reads the same device matrix data (a clone, the parent, a clone of a clone)."""
    return isinstance(other, SCS) and self._solver.shares_matrix(other._solver)

  def solve_many(self, b=None, c=None, warm_start=False, x=None, y=None, s=None):
    """Solve K problems that differ in b (K, m) and / or c (K, n) only, as one batch over one device copy of the matrix.
    Returns a list of K dicts like `solve()`; with warm_start=True a repeated call starts every member from its last solution
    (or from the rows of x, y, s)."""
    return self._solver.solve_many(b, c, warm_start, x, y, s)

  def update_device(self, b=None, c=None):
    """`update` for b / c that already live on the solver's GPU: float64, 1-D, contiguous torch tensors (None = keep).  No vector
    crosses the host.  The tensors must be complete on torch's current stream (the call synchronises it)."""
    self._solver.update_device(b, c)

  def solve_device(self, warm_start=False, x=None, y=None, s=None):
    """`solve` whose warm start and solution stay on the GPU: x, y, s are torch tensors (an omitted one = the previous solution),
    the result's "x", "y", "s" are fresh float64 device tensors; "info" as `solve()`."""
    return self._solver.solve_device(warm_start, x, y, s)

  def solve_many_device(self, b=None, c=None, warm_start=False, x=None, y=None, s=None):
    """`solve_many` over device tensors b (K, m), c (K, n) and warm starts (K, .): one grouped solve that writes into the rows of
    {"x": (K, n), "y": (K, m), "s": (K, m)} on the GPU; "info" is the list of K info dicts."""
    return self._solver.solve_many_device(b, c, warm_start, x, y, s)


  def adjoint(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None):
    """Gradients of a scalar L of the last solution: given dL/dx, dL/dy, dL/ds (numpy vectors, None = 0) returns {"db", "dc", "info"}
    and, when `want` names "A" / "P", "dA" / "dP": value arrays in the order of the (sorted CSC, upper-triangle) matrices the
    constructor used.  Solved on the GPU by LSQR to `tol`; a degenerate solution gives the minimum-norm least-squares answer
    (info["stop"] == 2).  Zero, nonnegative, second-order and real PSD (s) cones; ValueError after an update without a new solve."""
    return self._solver.adjoint(dx, dy, ds, want, tol, max_iters)

  def adjoint_device(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None):
    """`adjoint` over float64 torch tensors on the solver's GPU (taken and returned); same bits."""
    return self._solver.adjoint_device(dx, dy, ds, want, tol, max_iters)

  def derivative(self, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
    """The change {"dx", "dy", "ds", "info"} of the last solution for a change db, dc of the data (numpy vectors, None = 0) and dA, dP of
    the matrices: each a scipy sparse matrix of the constructor's pattern (brought to its form as `update_matrix` does) or a 1-D float
    array of the stored values in that order; an off-diagonal value of dP stands for both of its mirror images."""
    return self._solver.derivative(db, dc, tol, max_iters, dA=_update_arg(dA, "dA", False), dP=_update_arg(dP, "dP", True))

  def derivative_device(self, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
    """`derivative` over float64 torch tensors on the solver's GPU (dA, dP: 1-D tensors of the stored values)."""
    return self._solver.derivative_device(db, dc, tol, max_iters, dA=dA, dP=dP)


  def refine(self, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None):
    """Polish the last solution on the GPU by Newton steps on its optimality conditions (each one LSQR solve of `derivative`'s system
    to `lsqr_tol` plus a backtracking line search) until the solver's three stopping criteria hold with eps_abs = eps_rel = `tol`, at
    most `max_steps` steps.  Returns {"x", "y", "s", "info"}; info["stop_reason"] is "converged", "max_steps" or "no_decrease".  The
    polished point becomes the solver's solution: `adjoint`, `derivative`, `jacobian` and the next warm start read it.  Cones as
    `adjoint`; ValueError before a solve, after one that did not end solved, and after an update without a new solve."""
    return self._solver.refine(tol, max_steps, lsqr_tol, lsqr_max_iters)

  def refine_device(self, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None):
    """`refine` with "x", "y", "s" as fresh float64 torch tensors on the solver's GPU; same bits."""
    return self._solver.refine_device(tol, max_steps, lsqr_tol, lsqr_max_iters)

  def refine_many(self, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None, K=None):
    """`refine` of the K problems the last `solve_many` solved (K=None: all of them), polished in lock step (`refine_batch`).  Returns
    {"x": (K, n), "y": (K, m), "s": (K, m), "info": [K dicts]}, row k with the bits `refine` gives on problem k alone.  Every problem's
    polished point becomes its solution: a following `adjoint_many` and a warm-started `solve_many` read it.  ValueError for a K above
    what `solve_many` has solved, and for a problem `refine` would refuse (with its index, "member k")."""
    return self._solver.refine_many(tol, max_steps, lsqr_tol, lsqr_max_iters, K=K)

  def refine_many_device(self, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None, K=None):
    """`refine_many` with "x", "y", "s" as fresh (K, .) float64 torch tensors on the solver's GPU; same bits."""
    return self._solver.refine_many_device(tol, max_steps, lsqr_tol, lsqr_max_iters, K=K)


  def adjoint_many(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None, reduce=None):
    """`adjoint` of the K problems the last `solve_many` solved, differentiated in lock step: dx (K, n), dy (K, m), ds (K, m), None = 0.
    Returns K dicts like `adjoint()`, with the bits K separate calls would give.  reduce="sum" (needs "A" or "P" in `want`): the gradients
    of the shared matrix summed over the K problems, without a (K, nnz) stack — the pair (results, grads) of the K dicts without dA / dP
    and {"dA": (nnz,), "dP": (nnz(P),)}."""
    return self._solver.adjoint_many(dx, dy, ds, want, tol, max_iters, reduce=reduce)

  def adjoint_many_device(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None, reduce=None):
    """`adjoint_many` over (K, .) float64 torch tensors on the solver's GPU: {"db": (K, m), "dc": (K, n), ["dA"], ["dP"], "info": [K]}.
    reduce="sum": dA (nnz,) and dP (nnz(P),) are the sums over the K problems."""
    return self._solver.adjoint_many_device(dx, dy, ds, want, tol, max_iters, reduce=reduce)

  def derivative_many(self, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
    """`derivative` of the K problems the last `solve_many` solved, in lock step: db (K, m), dc (K, n), dA (K, nnz(A)), dP (K, nnz(P)),
    None = 0."""
    return self._solver.derivative_many(db, dc, tol, max_iters, dA=dA, dP=dP)

  def derivative_many_device(self, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
    """`derivative_many` over (K, .) float64 torch tensors on the solver's GPU."""
    return self._solver.derivative_many_device(db, dc, tol, max_iters, dA=dA, dP=dP)

  def adjoint_multi(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None):
    """`adjoint` of the last solve for K cotangents at once: dx (K, n), dy (K, m), ds (K, m), None = 0; K is read from them.  Returns
    {"db": (K, m), "dc": (K, n), ["dA"], ["dP"], "info": [K dicts]}, row k with the bits of `adjoint` on direction k: one preparation,
    K LSQR solves in lock step that read the matrices once per tile of directions.  Any K (served in chunks of 32)."""
    return self._solver.adjoint_multi(dx, dy, ds, want, tol, max_iters)

  def adjoint_multi_device(self, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None):
    """`adjoint_multi` over (K, .) float64 torch tensors on the solver's GPU (taken and returned); same bits."""
    return self._solver.adjoint_multi_device(dx, dy, ds, want, tol, max_iters)

  def derivative_multi(self, db=None, dc=None, tol=1e-8, max_iters=None):
    """`derivative` of the last solve for K perturbations at once: db (K, m), dc (K, n), None = 0.  Returns {"dx": (K, n), "dy": (K, m),
    "ds": (K, m), "info": [K dicts]}, row k with the bits of `derivative` on direction k."""
    return self._solver.derivative_multi(db, dc, tol, max_iters)

  def derivative_multi_device(self, db=None, dc=None, tol=1e-8, max_iters=None):
    """`derivative_multi` over (K, .) float64 torch tensors on the solver's GPU (taken and returned); same bits."""
    return self._solver.derivative_multi_device(db, dc, tol, max_iters)

  def jacobian(self, of="x", wrt="b", rows=None, tol=1e-8, max_iters=None):
    """The dense block d of[rows] / d wrt of the last solve, shape (len(rows), len(wrt)): of in "x", "y", "s"; wrt in "b", "c"; rows =
    indices into `of` (None: all of them).  One `adjoint_multi` with the rows' unit cotangents.  Returns (J, infos)."""
    return self._solver.jacobian(of, wrt, rows, tol, max_iters)

  def jacobian_device(self, of="x", wrt="b", rows=None, tol=1e-8, max_iters=None):
    """`jacobian` as a float64 torch tensor on the solver's GPU."""
    return self._solver.jacobian_device(of, wrt, rows, tol, max_iters)


def solve(data, cone, **settings):
  """Legacy one-shot API; warm-start vectors may ride along in `data`."""
  solver = SCS(data, cone, **settings)
  return solver.solve(warm_start=True, x=data.get("x"), y=data.get("y"), s=data.get("s"))


def solve_batch(solvers, warm_start=False):
  """Solve several `SCS` objects of the HIP backend as one batch: equally shaped problems advance in lock step and
  share every kernel launch (the MI355X answer to the reference's "independent instances run concurrently",
  R:test/test_thread_safety.py:78-93).  Returns one result dict per solver, identical to what `.solve()` returns."""
  raw = []
  for sv in solvers:
    if not isinstance(sv, SCS) or not isinstance(sv._solver, _scs_hip.SCS):
      raise TypeError("solve_batch needs scs.SCS objects created with LinearSolver.HIP_INDIRECT")
    raw.append(sv._solver)
  return _scs_hip.solve_batch(raw, warm_start)


def batch_plan(solvers):
  """How `solve_batch(solvers)` would split the batch, without solving: one int per solver, the index of the group it would
  share launches with, or -1 where it would be solved alone (a shape of its own, or a cone the grouped kernels do not cover)."""
  raw = []
  for sv in solvers:
    if not isinstance(sv, SCS) or not isinstance(sv._solver, _scs_hip.SCS):
      raise TypeError("batch_plan needs scs.SCS objects of the HIP backend")
    raw.append(sv._solver)
  return _scs_hip.batch_plan(raw)


def _raw_solvers(solvers, who, as_list=False):
  """the backend objects of a batch; as_list: the batch must be a list or tuple, and a refusal names the member's index"""
  if as_list and not isinstance(solvers, (list, tuple)):
    raise TypeError("%s expects a list of solvers, not %s" % (who, type(solvers).__name__))
  raw = []
  for i, sv in enumerate(solvers):
    if not isinstance(sv, SCS) or not isinstance(sv._solver, _scs_hip.SCS):
      raise TypeError("%s%s needs scs.SCS objects of the HIP backend" % (who, ": member %d:" % i if as_list else ""))
    raw.append(sv._solver)
  return raw


def adjoint_batch(solvers, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None, reduce=None):
  """`SCS.adjoint` of several solved `SCS` objects as one batch: equally shaped problems are differentiated in lock step and share
  every kernel launch.  dx, dy, ds: one vector per solver (a sequence, or a (K, .) array); None, or a None entry, is 0.  Returns one
  dict per solver, with the bits `.adjoint()` gives.  reduce="sum" (needs "A" or "P" in `want`; the solvers are one solver and its
  `clone()`s): (results, grads) — the dicts without dA / dP, and {"dA", "dP"} summed over the solvers."""
  return _scs_hip.adjoint_batch(_raw_solvers(solvers, "adjoint_batch"), dx, dy, ds, want, tol, max_iters, reduce=reduce)


def derivative_batch(solvers, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
  """`SCS.derivative` of several solved `SCS` objects as one batch (see `adjoint_batch`); dA, dP: one value array per solver."""
  return _scs_hip.derivative_batch(_raw_solvers(solvers, "derivative_batch"), db, dc, tol, max_iters, dA=dA, dP=dP)


def adjoint_batch_device(solvers, dx=None, dy=None, ds=None, want=("b", "c"), tol=1e-8, max_iters=None, reduce=None):
  """`adjoint_batch` over float64 torch tensors on the solvers' GPU (taken and returned)."""
  return _scs_hip.adjoint_batch_device(_raw_solvers(solvers, "adjoint_batch_device"), dx, dy, ds, want, tol, max_iters, reduce=reduce)


def derivative_batch_device(solvers, db=None, dc=None, tol=1e-8, max_iters=None, dA=None, dP=None):
  """`derivative_batch` over float64 torch tensors on the solvers' GPU."""
  return _scs_hip.derivative_batch_device(_raw_solvers(solvers, "derivative_batch_device"), db, dc, tol, max_iters, dA=dA, dP=dP)


def refine_batch(solvers, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None):
  """`SCS.refine` of several solved `SCS` objects as one batch: equally shaped problems are polished in lock step — one launch per kernel
  and one host synchronisation per evaluation for the group — each with its own number of steps, halvings and stop reason.  The options
  hold for every solver.  Returns one dict per solver, with the bits `.refine()` gives (info["time_ms"] is the group's); every solver's
  polished point becomes its solution.  A refusal names the solver's index ("member i") and leaves every solver as it was."""
  return _scs_hip.refine_batch(_raw_solvers(solvers, "refine_batch", as_list=True), tol, max_steps, lsqr_tol, lsqr_max_iters)


def refine_batch_device(solvers, tol=1e-9, max_steps=10, lsqr_tol=1e-8, lsqr_max_iters=None):
  """`refine_batch` with every solver's "x", "y", "s" as fresh float64 torch tensors on the solvers' GPU; same bits."""
  return _scs_hip.refine_batch_device(_raw_solvers(solvers, "refine_batch_device", as_list=True), tol, max_steps, lsqr_tol, lsqr_max_iters)


def diff_batch_plan(solvers, want=("b", "c")):
  """How `adjoint_batch(solvers, want=want)` would split the batch: one int per solver, the index of the group it would share launches
  with, or -1 where it is differentiated alone (a shape of its own, a pass or slab matrix layout, a PSD block above order 32, a box cone above 16384 rows)."""
  return _scs_hip.diff_batch_plan(_raw_solvers(solvers, "diff_batch_plan"), want)


def diff_group_launches():
  """Grouped launches the batch derivative entries have issued in this process."""
  return _scs_hip.diff_group_launches()


def diff_group_syncs():
  """Host synchronisations the groups of the batch derivative and refine entries have made in this process."""
  return _scs_hip.diff_group_syncs()
