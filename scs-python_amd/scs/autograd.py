"""`scs.autograd` — the solve as a layer of a torch program.  Imported on request only (`import scs.autograd`): `import scs` does not
import torch.

    x, y, s = scs.autograd.solve(solver, b, c)
    x, y, s = scs.autograd.solve(solver, b, c, A=Ax, P=Px)

`solver` is an `scs.SCS` of the HIP backend; b (m) and c (n) are float64 tensors on its GPU.  Forward is `update_device` +
`solve_device` (the first call starts cold, later calls warm-start from the solver's previous solution); backward is ONE
`adjoint_device` call for the gradients of b and c, with the LSQR tolerance `solver.autograd_tol` (default 1e-8).  The info dicts of
the last forward and backward are left in `solver.autograd_info` / `solver.autograd_adjoint_info`.

`solver.autograd_refine_tol` (default None: nothing changes) makes the forward of `solve` polish the solution after the solve:
`refine_device(tol=solver.autograd_refine_tol)`, Newton steps on the optimality conditions (`SCS.refine`).  The layer returns the
polished tensors and backward differentiates the polished, resident solution — a loose `eps` for the solve and a tight gradient.  A
refusal of `refine_device` (a solve that did not end solved) comes through as its ValueError; the info dict of the polish is left in
`solver.autograd_refine_info`.  `solve_many` honours the same switch: its forward calls `refine_many_device(tol=...)` after the solve
— the K members are polished in lock step (`SCS.refine_many`) — returns the polished (K, .) tensors, backward differentiates the K
polished solutions, and `solver.autograd_refine_info` holds the list of the K info dicts.  With the attribute unset (None) the layer
makes exactly the calls it makes without it.

A and P, when given, are float64 1-D tensors on the solver's GPU holding the stored VALUES of the matrices in the constructor's
canonical order (sorted CSC; P: its upper triangle, an off-diagonal value standing for both mirror images) — the learnable parameters
of a layer usually sit there.  Forward then is `update_matrix_device` with what is given, `update_device(b, c)` and the solve;
`update_matrix` leaves a cold iterate, so from the second call on the layer passes the previous solution explicitly
(`solve_device(warm_start=True, x=, y=, s=)`, from the tensors it returned last).  Backward is still ONE `adjoint_device` call whose
`want` holds exactly the inputs that need a gradient; the gradients of A and P are value tensors in the same order.  A solver whose
matrix has live clones cannot update it: the ValueError of `update_matrix` comes through.  With A = P = None the layer does what it
always did, call for call.

The adjoint differentiates the solution that is resident on the device, so backward must run before the same solver is solved or
updated again (RuntimeError otherwise).  Double backward and torch forward mode (`jvp`) are not covered; for directional derivatives
call `SCS.derivative_device(db, dc, dA=, dP=)`.

    X, Y, S = scs.autograd.solve_many(solver, B, C)
    X, Y, S = scs.autograd.solve_many(solver, B, C, A=Ax, P=Px)

is the same layer for K problems over the solver's matrix: B (K, m), C (K, n); forward is `solve_many_device` (warm-started from the
second call on), backward is ONE `adjoint_many_device` call — the K members are differentiated in lock step.  A and P, when given,
are the values of the ONE matrix the K problems share (as in `solve`): forward is `update_matrix_device` — which finishes the cached
members; the solve makes new ones on the new values — then `solve_many_device`, from the second call on warm-started explicitly from
the X, Y, S the layer returned last.  Backward stays one `adjoint_many_device` call whose `want` holds the inputs that need a
gradient, with `reduce="sum"` when A or P is among them: their gradients are (nnz,) tensors, the sums over the K members, and no
(K, nnz) stack is formed.  With A = P = None the layer makes the calls it always made."""
import torch


def _solved(ctx, solver, out):
  """a forward's book-keeping: the solver's generation counts its solves, and the backward of this one holds its number"""
  solver._autograd_generation = getattr(solver, "_autograd_generation", 0) + 1
  solver.autograd_info = out["info"]
  ctx.solver = solver
  ctx.generation = solver._autograd_generation
  return out["x"], out["y"], out["s"]


def _still_resident(ctx, who, what):
  if getattr(ctx.solver, "_autograd_generation", 0) != ctx.generation:
    raise RuntimeError("scs.autograd.%s: the solver was solved again before this backward; its resident %s" % (who, what))


class _Solve(torch.autograd.Function):
  """A, P: the values of the matrices as inputs, None = the solver's own"""

  @staticmethod
  def forward(ctx, solver, b, c, A, P):
    ctx.matrix = A is not None or P is not None
    if ctx.matrix:
      solver.update_matrix_device(A.detach().contiguous() if A is not None else None, P.detach().contiguous() if P is not None else None)
    solver.update_device(b.detach().contiguous(), c.detach().contiguous())
    last = getattr(solver, "_autograd_last", None)
    if not ctx.matrix:
      out = solver.solve_device(warm_start=bool(getattr(solver, "_autograd_generation", 0)))
    elif last is not None:  # (the new matrix left a cold iterate: the previous solution goes in explicitly)
      out = solver.solve_device(warm_start=True, x=last[0], y=last[1], s=last[2])
    else:
      out = solver.solve_device(warm_start=False)
    refine_tol = getattr(solver, "autograd_refine_tol", None)
    if refine_tol is not None:  # polish the resident solution: backward then differentiates an accurate fixed point
      info = out["info"]
      out = solver.refine_device(tol=refine_tol)
      solver.autograd_refine_info, out["info"] = out["info"], info
    # (detached views: the returned tensors get a grad_fn that holds ctx and with it the solver — the solver must not hold them back)
    solver._autograd_last = (out["x"].detach(), out["y"].detach(), out["s"].detach())
    return _solved(ctx, solver, out)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gx, gy, gs):
    _still_resident(ctx, "solve", "solution is another one")
    need = ctx.needs_input_grad[1:5]
    if not any(need):
      return None, None, None, None, None
    # (with matrices, `want` holds exactly the inputs that need a gradient; without, the call is the one it always was)
    want = tuple(k for k, nd in zip(("b", "c", "A", "P"), need) if nd) if ctx.matrix else ("b", "c")
    res = ctx.solver.adjoint_device(dx=gx.contiguous(), dy=gy.contiguous(), ds=gs.contiguous(), want=want,
                                    tol=getattr(ctx.solver, "autograd_tol", 1e-8))
    ctx.solver.autograd_adjoint_info = res["info"]
    return (None,) + tuple(res["d" + k] if nd else None for k, nd in zip(("b", "c", "A", "P"), need))


def solve(solver, b, c, A=None, P=None):
  """(x, y, s) of the solver's problem with the data b, c and — when given — the matrix values A, P (1-D tensors in the constructor's
  canonical order), differentiable with respect to each tensor passed."""
  return _Solve.apply(solver, b, c, A, P)


class _SolveMany(torch.autograd.Function):
  """`_Solve` for K problems over the solver's matrix.  A, P: the values of the SHARED matrices as inputs, None = the solver's own"""

  @staticmethod
  def forward(ctx, solver, B, C, A, P):
    ctx.matrix = A is not None or P is not None
    if ctx.matrix:  # (finishes the cached clones, which read the matrix set: solve_many_device makes new ones on the new values)
      solver.update_matrix_device(A.detach().contiguous() if A is not None else None, P.detach().contiguous() if P is not None else None)
    B, C = B.detach().contiguous(), C.detach().contiguous()
    last = getattr(solver, "_autograd_last_many", None)
    if not ctx.matrix:
      out = solver.solve_many_device(b=B, c=C, warm_start=bool(getattr(solver, "_autograd_generation", 0)))
    elif last is not None and last[0].shape[0] == B.shape[0]:  # (the members start cold: the previous solutions go in explicitly)
      out = solver.solve_many_device(b=B, c=C, warm_start=True, x=last[0], y=last[1], s=last[2])
    else:
      out = solver.solve_many_device(b=B, c=C, warm_start=False)
    refine_tol = getattr(solver, "autograd_refine_tol", None)
    if refine_tol is not None:  # polish the K resident solutions in lock step: backward then differentiates accurate fixed points
      info = out["info"]
      out = solver.refine_many_device(tol=refine_tol, K=int(B.shape[0]))
      solver.autograd_refine_info, out["info"] = out["info"], info
    if ctx.matrix:
      solver._autograd_last_many = (out["x"].detach(), out["y"].detach(), out["s"].detach())
    return _solved(ctx, solver, out)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gx, gy, gs):
    _still_resident(ctx, "solve_many", "solutions are others")
    need = ctx.needs_input_grad[1:5]
    if not any(need):
      return None, None, None, None, None
    # (as _Solve.backward; the gradients of the shared A and P are the sums over the K members: reduce="sum")
    want = tuple(k for k, nd in zip(("b", "c", "A", "P"), need) if nd) if ctx.matrix else ("b", "c")
    reduce = dict(reduce="sum") if need[2] or need[3] else {}
    res = ctx.solver.adjoint_many_device(dx=gx.contiguous(), dy=gy.contiguous(), ds=gs.contiguous(), want=want,
                                         tol=getattr(ctx.solver, "autograd_tol", 1e-8), **reduce)
    ctx.solver.autograd_adjoint_info = res["info"]
    return (None,) + tuple(res["d" + k] if nd else None for k, nd in zip(("b", "c", "A", "P"), need))


def solve_many(solver, B, C, A=None, P=None):
  """(X, Y, S), (K, .) tensors: the solutions of the solver's problem with the rows of B (K, m) and C (K, n) as data and — when given —
  the matrix values A, P (1-D tensors in the constructor's canonical order) shared by the K problems; differentiable with respect to
  each tensor passed (the gradients of A and P are summed over the K problems)."""
  return _SolveMany.apply(solver, B, C, A, P)
