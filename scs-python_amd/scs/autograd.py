"""`scs.autograd` — the solve as a layer of a torch program.  Imported on request only (`import scs.autograd`): `import scs` does not
import torch.

    x, y, s = scs.autograd.solve(solver, b, c)

`solver` is an `scs.SCS` of the HIP backend; b (m) and c (n) are float64 tensors on its GPU.  Forward is `update_device` +
`solve_device` (the first call starts cold, later calls warm-start from the solver's previous solution); backward is ONE
`adjoint_device` call for the gradients of b and c, with the LSQR tolerance `solver.autograd_tol` (default 1e-8).  The info dicts of
the last forward and backward are left in `solver.autograd_info` / `solver.autograd_adjoint_info`.

The adjoint differentiates the solution that is resident on the device, so backward must run before the same solver is solved or
updated again (RuntimeError otherwise).  A and P as differentiable inputs and double backward are not covered: call
`SCS.adjoint_device(want=("b", "c", "A", "P"))` for the matrix gradients.

    X, Y, S = scs.autograd.solve_many(solver, B, C)

is the same layer for K problems over the solver's matrix: B (K, m), C (K, n); forward is `solve_many_device` (warm-started from the
second call on), backward is ONE `adjoint_many_device` call — the K members are differentiated in lock step."""
import torch


class _Solve(torch.autograd.Function):

  @staticmethod
  def forward(ctx, solver, b, c):
    solver.update_device(b.detach().contiguous(), c.detach().contiguous())
    warm = bool(getattr(solver, "_autograd_generation", 0))
    out = solver.solve_device(warm_start=warm)
    solver._autograd_generation = getattr(solver, "_autograd_generation", 0) + 1
    solver.autograd_info = out["info"]
    ctx.solver = solver
    ctx.generation = solver._autograd_generation
    return out["x"], out["y"], out["s"]

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gx, gy, gs):
    solver = ctx.solver
    if getattr(solver, "_autograd_generation", 0) != ctx.generation:
      raise RuntimeError("scs.autograd.solve: the solver was solved again before this backward; its resident solution is another one")
    if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
      return None, None, None
    res = solver.adjoint_device(dx=gx.contiguous(), dy=gy.contiguous(), ds=gs.contiguous(), want=("b", "c"),
                                tol=getattr(solver, "autograd_tol", 1e-8))
    solver.autograd_adjoint_info = res["info"]
    return None, res["db"] if ctx.needs_input_grad[1] else None, res["dc"] if ctx.needs_input_grad[2] else None


def solve(solver, b, c):
  """(x, y, s) of the solver's problem with the data b, c, differentiable with respect to both."""
  return _Solve.apply(solver, b, c)


class _SolveMany(torch.autograd.Function):

  @staticmethod
  def forward(ctx, solver, B, C):
    warm = bool(getattr(solver, "_autograd_generation", 0))
    out = solver.solve_many_device(b=B.detach().contiguous(), c=C.detach().contiguous(), warm_start=warm)
    solver._autograd_generation = getattr(solver, "_autograd_generation", 0) + 1
    solver.autograd_info = out["info"]
    ctx.solver = solver
    ctx.generation = solver._autograd_generation
    return out["x"], out["y"], out["s"]

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gx, gy, gs):
    solver = ctx.solver
    if getattr(solver, "_autograd_generation", 0) != ctx.generation:
      raise RuntimeError("scs.autograd.solve_many: the solver was solved again before this backward; its resident solutions are others")
    if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
      return None, None, None
    res = solver.adjoint_many_device(dx=gx.contiguous(), dy=gy.contiguous(), ds=gs.contiguous(), want=("b", "c"),
                                     tol=getattr(solver, "autograd_tol", 1e-8))
    solver.autograd_adjoint_info = res["info"]
    return None, res["db"] if ctx.needs_input_grad[1] else None, res["dc"] if ctx.needs_input_grad[2] else None


def solve_many(solver, B, C):
  """(X, Y, S), (K, .) tensors: the solutions of the solver's problem with the rows of B (K, m) and C (K, n) as data, differentiable
  with respect to both."""
  return _SolveMany.apply(solver, B, C)
