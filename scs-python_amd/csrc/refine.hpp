// refine.hpp — Newton polish of the resident solution on the device (include/scs_hip.h: scs_hip_refine[_device]).
//
// The ADMM loop reaches 1e-4 quickly and 1e-9 slowly; everything diff.hpp differentiates is only meaningful at an accurate fixed
// point.  A Newton step on the optimality conditions of diff.hpp,
//     F1 = P x + A'(Pi(v) - v) + c,   F2 = A x + Pi(v) - b,   J = [[P, A'(W - I)], [A, W]],  W = D Pi_K(v),
// is one forward-mode solve J d = -F — the system scs_hip_derivative solves, through the same wiring (diff_wiring, diff_lsqr).  What
// this file adds is the evaluation of F at a trial point, the step control and the hand-over of the polished point.
//
// No projection kernel is needed: Pi_K is positively homogeneous, so Pi_K(v) = W(v) v.  One apply of the prepared plan with u = v
// leaves s^ = Pi(v^) in Wu and y^ = Pi(v^) - v^ in WmIu (launch_dproj), at the accuracy of the derivative's preparation, and never
// touches the state of the solve's own projections.  W depends on v, so every trial point of the line search prepares the plan anew
// (launch_dproj_prep at the trial v^); the base point keeps buffers of its own, and after an accepted step the plan IS the one of the
// new base point (k_refine_accept copies the trial into the base: the same numbers), so the next LSQR solve needs no preparation.
//
// All of it in the hatted coordinates of diff.hpp: x^ = sigma x / E, v^ = sigma (D s - y / D); b^ and c^ are the resident h = [c^ ; b^]
// the ADMM loop reads.  F^1 = sigma E F1 and F^2 = sigma D F2 row by row, so the residual pass un-scales its rows to evaluate the
// solver's own stop rule in the caller's units:
//     |Ax + s - b|_inf <= tol (1 + max(|Ax|_inf, |s|_inf, |b|_inf)),   |Px + A'y + c|_inf <= tol (1 + max(|Px|_inf, |A'y|_inf, |c|_inf)),
//     |x'Px + c'x + b'y| <= tol (1 + max(|x'Px|, |c'x|, |b'y|)).
// The merit of the line search is phi = |F^|_2, the residual of the system LSQR solves: a Newton direction descends on it.
//
// One evaluation: prep, apply, the three SpMVs into the product slots of lane 0, k_refine_residual (one pass over n + m: -F^ into the
// LSQR right-hand side uh, per-workgroup partials) and k_refine_finish (one workgroup: the partials in slot order, the figures and
// the decision into the state block).  Sums and maxima have a fixed order and there are no atomics: two calls on the same state
// give the same bits.  The host reads the state block once per evaluation; every loop is bounded on the host.
#pragma once

namespace scship {

// the state block k_refine_finish writes (doubles)
enum : int {
  RS_PHI = 0,                                    // |F^|_2
  RS_PRI, RS_AX, RS_S, RS_B,                     // max-norms of the primal rule (caller's units)
  RS_DUAL, RS_PX, RS_ATY, RS_C,                  // ... of the dual rule
  RS_XPX, RS_CTX, RS_BTY, RS_GAP,                // the three inner products and |their sum|
  RS_CONV,                                       // 1: the three criteria hold
  RS_COUNT = 16
};
enum : int { RP_SUMS = 4, RP_MAXS = 8, RP_COUNT = RP_SUMS + RP_MAXS };  // partial groups: phi^2, x^'P^x^, c^'x^, b^'y^ | the eight max-norms

// the starting point from the resident solution: x^ = sigma x / E, v^ = sigma (D s - y / D) (the arithmetic of k_dproj_vhat)
__device__ __forceinline__ void d_refine_start(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ s,
                                               const double *__restrict__ D, const double *__restrict__ E, double sigma, int n, int m,
                                               double *xh, double *vh) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    if (i < n) {
      xh[i] = E ? sigma * x[i] / E[i] : x[i];
    } else {
      const long k = i - n;
      vh[k] = D ? sigma * (D[k] * s[k] - y[k] / D[k]) : s[k] - y[k];
    }
  }
}
__global__ __launch_bounds__(kVecThreads) void k_refine_start(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ s,
                                                              const double *__restrict__ D, const double *__restrict__ E, double sigma, int n, int m,
                                                              double *xh, double *vh) {
  d_refine_start(x, y, s, D, E, sigma, n, m, xh, vh);
}

// what one evaluation of F^ reads: the point's x^, the apply's s^ and y^, the three products, h = [c^ ; b^] and the scaling
struct RefineEval {
  const double *xh;            // n
  const double *sh, *yh;       // m: W v^, (W - I) v^
  const double *Px, *Aty, *Ax; // P^ x^ (nullptr: no P), A^' y^, A^ x^
  const double *h;             // [c^ ; b^]
  const double *D, *E;         // nullptr: not normalised
  double sigma;
};

// uh = -F^ (rows < n: -(P^x^ + A^'y^ + c^); rows >= n: -(A^x^ + s^ - b^)); part[g * gridDim.x + blockIdx.x], g over the RP_COUNT groups
__device__ __forceinline__ void d_refine_residual(RefineEval e, int n, int m, double *uh, double *part) {
  __shared__ double sm[kVecThreads / 64];
  double sum[RP_SUMS] = {0., 0., 0., 0.};
  double mx[RP_MAXS] = {0., 0., 0., 0., 0., 0., 0., 0.};
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    if (i < n) {
      const double px = e.Px ? e.Px[i] : 0., aty = e.Aty[i], c = e.h[i], xi = e.xh[i];
      const double f = px + aty + c;
      uh[i] = -f;
      sum[0] += f * f;
      sum[1] += xi * px;
      sum[2] += c * xi;
      const double sc = e.E ? e.sigma * e.E[i] : 1.0;
      mx[4] = fmax(mx[4], abs_nan_inf(f / sc));
      mx[5] = fmax(mx[5], abs_nan_inf(px / sc));
      mx[6] = fmax(mx[6], abs_nan_inf(aty / sc));
      mx[7] = fmax(mx[7], abs_nan_inf(c / sc));
    } else {
      const long k = i - n;
      const double ax = e.Ax[k], s = e.sh[k], b = e.h[i];
      const double f = ax + s - b;
      uh[i] = -f;
      sum[0] += f * f;
      sum[3] += b * e.yh[k];
      const double sc = e.D ? e.sigma * e.D[k] : 1.0;
      mx[0] = fmax(mx[0], abs_nan_inf(f / sc));
      mx[1] = fmax(mx[1], abs_nan_inf(ax / sc));
      mx[2] = fmax(mx[2], abs_nan_inf(s / sc));
      mx[3] = fmax(mx[3], abs_nan_inf(b / sc));
    }
  }
#pragma unroll
  for (int g = 0; g < RP_SUMS; ++g) {
    const double v = block_sum<kVecThreads>(sum[g], sm);
    if (threadIdx.x == 0) part[(size_t)g * gridDim.x + blockIdx.x] = v;
  }
#pragma unroll
  for (int g = 0; g < RP_MAXS; ++g) {
    const double v = block_max<kVecThreads>(mx[g], sm);
    if (threadIdx.x == 0) part[(size_t)(RP_SUMS + g) * gridDim.x + blockIdx.x] = v;
  }
}
__global__ __launch_bounds__(kVecThreads) void k_refine_residual(RefineEval e, int n, int m, double *uh, double *part) {
  d_refine_residual(e, n, m, uh, part);
}

// one workgroup: the np partials of every group in slot order, the figures in the caller's units and the stop decision
__device__ __forceinline__ void d_refine_finish(const double *__restrict__ part, int np, double sigma, double tol, double *st) {
  __shared__ double sm[kVecThreads / 64];
  __shared__ double r[RP_COUNT];
  for (int g = 0; g < RP_COUNT; ++g) {
    const double v = g < RP_SUMS ? part_sum(part + (size_t)g * np, np, sm) : part_max(part + (size_t)g * np, np, sm);
    if (threadIdx.x == 0) r[g] = v;
  }
  if (threadIdx.x != 0) return;
  const double s2 = sigma * sigma;
  const double xpx = r[1] / s2, ctx = r[2] / s2, bty = r[3] / s2;
  const double gap = fabs(xpx + ctx + bty);
  const double *mx = r + RP_SUMS;
  st[RS_PHI] = sqrt(r[0]);
  st[RS_PRI] = mx[0]; st[RS_AX] = mx[1]; st[RS_S] = mx[2]; st[RS_B] = mx[3];
  st[RS_DUAL] = mx[4]; st[RS_PX] = mx[5]; st[RS_ATY] = mx[6]; st[RS_C] = mx[7];
  st[RS_XPX] = xpx; st[RS_CTX] = ctx; st[RS_BTY] = bty; st[RS_GAP] = gap;
  const bool pri = mx[0] <= tol * (1. + fmax(mx[1], fmax(mx[2], mx[3])));
  const bool dual = mx[4] <= tol * (1. + fmax(mx[5], fmax(mx[6], mx[7])));
  const bool gp = gap <= tol * (1. + fmax(fabs(xpx), fmax(fabs(ctx), fabs(bty))));
  st[RS_CONV] = (pri && dual && gp) ? 1. : 0.;  // (a NaN anywhere compares false)
}
__global__ __launch_bounds__(kVecThreads) void k_refine_finish(const double *__restrict__ part, int np, double sigma, double tol, double *st) {
  d_refine_finish(part, np, sigma, tol, st);
}

// trial point: x^_t = x^ + t dx, v^_t = v^ + t dv, d = (dx ; dv) as LSQR left it
__device__ __forceinline__ void d_refine_trial(const double *__restrict__ bx, const double *__restrict__ bv, const double *__restrict__ d,
                                               double t, int n, int m, double *tx, double *tv) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    if (i < n) tx[i] = bx[i] + t * d[i];
    else tv[i - n] = bv[i - n] + t * d[i];
  }
}
__global__ __launch_bounds__(kVecThreads) void k_refine_trial(const double *__restrict__ bx, const double *__restrict__ bv, const double *__restrict__ d,
                                                              double t, int n, int m, double *tx, double *tv) {
  d_refine_trial(bx, bv, d, t, n, m, tx, tv);
}

// the accepted trial becomes the base point and the resident solution: x = E x^ / sigma, y = D y^ / sigma, s = s^ / (D sigma)
// (the arithmetic of k_fwd_out), with s^, y^ of the trial's evaluation
__device__ __forceinline__ void d_refine_accept(const double *__restrict__ tx, const double *__restrict__ tv, const double *__restrict__ sh,
                                                const double *__restrict__ yh, const double *__restrict__ D, const double *__restrict__ E,
                                                double sigma, int n, int m, double *bx, double *bv, double *x, double *y, double *s) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    if (i < n) {
      const double xi = tx[i];
      bx[i] = xi;
      x[i] = E ? E[i] * xi / sigma : xi;
    } else {
      const long k = i - n;
      bv[k] = tv[k];
      y[k] = D ? D[k] * yh[k] / sigma : yh[k];
      s[k] = D ? sh[k] / (D[k] * sigma) : sh[k];
    }
  }
}
__global__ __launch_bounds__(kVecThreads) void k_refine_accept(const double *__restrict__ tx, const double *__restrict__ tv, const double *__restrict__ sh,
                                                               const double *__restrict__ yh, const double *__restrict__ D, const double *__restrict__ E,
                                                               double sigma, int n, int m, double *bx, double *bv, double *x, double *y, double *s) {
  d_refine_accept(tx, tv, sh, yh, D, E, sigma, n, m, bx, bv, x, y, s);
}

}  // namespace scship

// the options of a call (NULL or a non-positive member: the default)
struct RefineLimits {
  double tol;
  int max_steps;
  ScsHipDiffOpts lsqr;
  explicit RefineLimits(const ScsHipRefineOpts *o)
      : tol(o && o->tol > 0. ? o->tol : 1e-9), max_steps(o && o->max_steps > 0 ? (int)o->max_steps : 10),
        lsqr{o && o->lsqr_tol > 0. ? o->lsqr_tol : 1e-8, o && o->lsqr_max_iters > 0 ? o->lsqr_max_iters : 0} {}
};
constexpr int kRefineHalvings = 10;     // t = 1, 1/2, ..., 2^-10
constexpr double kRefineArmijo = 1e-4;  // accept phi(t) < (1 - 1e-4 t) phi

static void refine_alloc(ScsHipWork *w) {
  diff_alloc(w);
  DiffScratch::Refine &r = w->diff.refine;
  if (r.ready) return;
  ArenaScope no_arena(nullptr);  // exact-size blocks from the block pool, returned to it by scs_finish
  r.bx.alloc((size_t)w->n); r.tx.alloc((size_t)w->n);
  r.bv.alloc((size_t)w->m); r.tv.alloc((size_t)w->m);
  r.part.alloc((size_t)RP_COUNT * vec_blocks((long)w->n + w->m));
  r.st.alloc(RS_COUNT);
  r.ready = true;
}

// One workspace.  The caller holds w->mtx and the scratch turn, has selected the device and refused what diff_refusal refuses.
// Leaves the best accepted point in solx / soly / sols (untouched when no step was accepted).
static void refine_impl(ScsHipWork *w, const ScsHipRefineOpts *o, ScsHipRefineInfo *info) {
  const double t0 = now_ms();
  hipStream_t s = w->stream;
  const int n = w->n, m = w->m;
  const long N = (long)n + m;
  const RefineLimits lim(o);
  const DiffLimits llim(&lim.lsqr, N);
  refine_alloc(w);
  DiffScratch &d = w->diff;
  DiffScratch::Refine &r = d.refine;
  const double *D = w->normalized ? w->D.p : nullptr, *E = w->normalized ? w->E.p : nullptr;
  const double sigma = w->normalized ? w->scal.sigma : 1.0;
  const int nbN = vec_blocks(N);
  const dim3 gN(nbN), bV(kVecThreads);
  DiffCall fwd;
  fwd.adjoint = false;
  const DiffWiring wr = diff_wiring(w, fwd);
  // the plan over the base point and over the trial point: the same records, frames and tables, read against the v^ they were prepared at
  DprojPlan plan_b = diff_plan(w), plan_t = plan_b;
  plan_b.vh = r.bv.p;
  plan_t.vh = r.tv.p;

  // F^ at (xh, plan.vh): -F^ into uh, the figures into hst
  auto evaluate = [&](const DprojPlan &plan, const double *xh, double *hst) {
    launch_dproj_prep(plan, s);
    launch_dproj(plan, DprojIo{plan.vh, nullptr, d.dW.p, d.dWmI.p}, nullptr, s);
    launch_spmv(w->Ar.view(), xh, EpiStore{d.tA.p, 0}, nullptr, s);
    launch_spmv(w->At.view(), (const double *)d.dWmI.p, EpiStore{d.tAt.p, 0}, nullptr, s);
    if (w->has_P) launch_spmv(w->Pf.view(), xh, EpiStore{d.tP.p, 0}, nullptr, s);
    const RefineEval e{xh, d.dW.p, d.dWmI.p, w->has_P ? d.tP.p : nullptr, d.tAt.p, d.tA.p, w->h.p, D, E, sigma};
    hipLaunchKernelGGL(k_refine_residual, gN, bV, 0, s, e, n, m, d.uh.p, r.part.p);
    hipLaunchKernelGGL(k_refine_finish, dim3(1), bV, 0, s, (const double *)r.part.p, nbN, sigma, lim.tol, r.st.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(hst, r.st.p, sizeof(double) * RS_COUNT, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  };

  hipLaunchKernelGGL(k_refine_start, gN, bV, 0, s, (const double *)w->solx.p, (const double *)w->soly.p, (const double *)w->sols.p, D, E, sigma, n, m,
                     r.bx.p, r.bv.p);
  double cur[RS_COUNT], first[RS_COUNT], tri[RS_COUNT];
  evaluate(plan_b, r.bx.p, cur);
  std::copy(cur, cur + RS_COUNT, first);

  int steps = 0, halvings = 0, stop = cur[RS_CONV] != 0. ? 1 : 0;
  long lsqr_iters = 0;
  while (!stop) {
    int hfl[LF_COUNT];
    diff_lsqr(w, wr, plan_b, llim, hfl);  // uh = -F^ of the base point in, the step (dx ; dv) in d.x out
    lsqr_iters += std::min((long)hfl[LF_ITERS], llim.cap);
    bool accepted = false;
    double t = 1.0;
    for (int h = 0; h <= kRefineHalvings; ++h, t *= 0.5) {
      hipLaunchKernelGGL(k_refine_trial, gN, bV, 0, s, (const double *)r.bx.p, (const double *)r.bv.p, (const double *)d.x.p, t, n, m, r.tx.p, r.tv.p);
      evaluate(plan_t, r.tx.p, tri);
      if (tri[RS_PHI] < (1. - kRefineArmijo * t) * cur[RS_PHI]) {  // (a NaN merit compares false)
        accepted = true;
        break;
      }
      if (h < kRefineHalvings) ++halvings;
    }
    if (!accepted) {
      stop = 3;
      break;
    }
    hipLaunchKernelGGL(k_refine_accept, gN, bV, 0, s, (const double *)r.tx.p, (const double *)r.tv.p, (const double *)d.dW.p, (const double *)d.dWmI.p,
                       D, E, sigma, n, m, r.bx.p, r.bv.p, w->solx.p, w->soly.p, w->sols.p);
    std::copy(tri, tri + RS_COUNT, cur);
    ++steps;
    if (cur[RS_CONV] != 0.) stop = 1;
    else if (steps >= lim.max_steps) stop = 2;
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
  if (!info) return;
  info->steps = steps; info->halvings = halvings; info->lsqr_iters = (scs_int)lsqr_iters; info->stop = stop;
  info->merit_before = first[RS_PHI]; info->merit_after = cur[RS_PHI];
  info->res_pri_before = first[RS_PRI]; info->res_dual_before = first[RS_DUAL]; info->gap_before = first[RS_GAP];
  info->res_pri = cur[RS_PRI]; info->res_dual = cur[RS_DUAL]; info->gap = cur[RS_GAP];
  info->pobj = cur[RS_XPX] / 2. + cur[RS_CTX];
  info->dobj = -cur[RS_XPX] / 2. - cur[RS_BTY];
  info->time_ms = now_ms() - t0;
}
