// lsqr.hpp — LSQR (Paige & Saunders 1982) on the device, for a square, non-symmetric, possibly singular operator M of order N = n + m:
// min |M x - g|, the minimum-norm solution when M is singular (x starts at 0).  One implementation; the caller supplies the two
// products M v and M' u as launches (diff.hpp: M = J' for the adjoint of a solve, M = J for its forward derivative).
//
// Nothing of an iteration crosses the host.  The bidiagonalisation vectors are kept UN-normalised (uh = beta u, vh = alpha v); their
// norms come from fixed-order partials, summed in the prologue of the kernel that consumes them (as k_cg_update takes alpha, vec.hpp),
// and the rotation scalars live in a block of device doubles that workgroup 0 of each kernel moves on.  A slot is written by one of
// the two kernels and read by the other only, so no workgroup reads what a workgroup of its own launch writes (phibar: two slots,
// by iteration parity).  Iteration k >= 1 is
//     tu = M vh                        (products)
//     k_lsqr_u(k):  alpha_k = |vh|;  w = vh / alpha_k - (theta_k / rho_{k-1}) w;  uh = tu / alpha_k - (alpha_k / beta_k) uh;  partials |uh|^2
//                   workgroup 0: the stopping tests for x_{k-1} (they need alpha_k)
//     tv = M' uh                       (products)
//     k_lsqr_v(k):  beta_{k+1} = |uh|;  rotation;  x += (phi_k / rho_k) w;  vh = tv / beta_{k+1} - (beta_{k+1} / alpha_k) vh;  partials |vh|^2, |x|^2
// The host enqueues a chunk of iterations and reads the flag block, as run_cg does; every kernel returns at once when the done flag
// is up.  Stopping: the standard rules with atol = btol = tol (1: |r| <= tol |g| + tol |M| |x|; 2: |M' r| <= tol |M| |r|) and an
// iteration cap (3).  All sums have a fixed order: two calls on the same state give the same bits.
#pragma once
#include <memory>

#include "common.hpp"
#include "vec.hpp"

namespace scship {

enum : int {
  L_ALPHA = 0, L_BETA, L_RHOBAR, L_PHIBAR0, L_PHIBAR1, L_C, L_S, L_RHO, L_ANORM2, L_BNORM, L_RNORM, L_ARNORM, L_XNORM, L_ANORM, L_COUNT = 16
};
enum : int { LF_DONE = 0, LF_ITERS, LF_STOP, LF_COUNT = 4 };

// a product of the operator as the launches of diff.hpp leave it: rows < n: top1 (+ top2);  rows >= n: botA + botW, or botW - botA
struct LsqrProd {
  const double *top1, *top2;  // top2 nullable (no P)
  const double *botA, *botW;
  int bot_sub;
  __device__ __forceinline__ double at(long i, int n) const {
    if (i < n) return top2 ? top1[i] + top2[i] : top1[i];
    const long k = i - n;
    return bot_sub ? botW[k] - botA[k] : botA[k] + botW[k];
  }
};

__device__ __forceinline__ double lsqr_bcast(double v, double *slot) {  // tid 0's value to the workgroup
  __syncthreads();
  if (threadIdx.x == 0) *slot = v;
  __syncthreads();
  return *slot;
}
__device__ __forceinline__ double lsqr_inv(double a) { return a > 0. ? 1. / a : 0.; }

// start: uh = g (rows >= n: add1 + add2 when given, else what uh holds), x = w = 0, partials of |uh|^2, the state cleared
__device__ __forceinline__ void d_lsqr_start(double *uh, const double *__restrict__ add1, const double *__restrict__ add2, int n,
                                             long N, double *x, double *w, double *partU, double *st, int *fl) {
  __shared__ double sm[kVecThreads / 64];
  double s = 0.;
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < N; i += (long)gridDim.x * kVecThreads) {
    double g = uh[i];
    if (add1 && i >= n) {
      g = add1[i - n] + add2[i - n];
      uh[i] = g;
    }
    x[i] = 0.;
    w[i] = 0.;
    s += g * g;
  }
  s = block_sum<kVecThreads>(s, sm);
  if (threadIdx.x == 0) partU[blockIdx.x] = s;
  if (blockIdx.x == 0 && threadIdx.x < L_COUNT) st[threadIdx.x] = 0.;
  if (blockIdx.x == 0 && threadIdx.x < LF_COUNT) fl[threadIdx.x] = 0;
}
__global__ __launch_bounds__(kVecThreads) void k_lsqr_start(double *uh, const double *__restrict__ add1, const double *__restrict__ add2, int n,
                                                            long N, double *x, double *w, double *partU, double *st, int *fl) {
  d_lsqr_start(uh, add1, add2, n, N, x, w, partU, st, fl);
}

// k = 0: beta_1 = |uh|, vh = tv / beta_1.   k >= 1: see the header.
__device__ __forceinline__ void d_lsqr_v(int k, LsqrProd tv, double *vh, const double *__restrict__ w, double *x, int n, long N,
                                         const double *__restrict__ partU, int np, double *partV, double *partX, double *st,
                                         int *fl) {
  if (fl[LF_DONE]) return;
  __shared__ double sm[kVecThreads / 64];
  __shared__ double bc;
  const double beta = lsqr_bcast(sqrt(part_sum(partU, np, sm)), &bc);
  const double ib = lsqr_inv(beta);
  double rho = 0., c = 0., sn = 0., phibar = 0., step = 0., back = 0., alpha = 0.;
  if (k > 0) {
    alpha = st[L_ALPHA];
    const double rhobar = st[L_RHOBAR];
    phibar = st[(k & 1) ? L_PHIBAR1 : L_PHIBAR0];
    rho = hypot(rhobar, beta);
    const double ir = lsqr_inv(rho);
    c = rhobar * ir;
    sn = beta * ir;
    step = c * phibar * ir;  // phi_k / rho_k
    back = beta * lsqr_inv(alpha);
  }
  double sv = 0., sx = 0.;
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < N; i += (long)gridDim.x * kVecThreads) {
    double vi = tv.at(i, n) * ib;
    if (k > 0) {
      vi -= back * vh[i];
      const double xi = x[i] + step * w[i];
      x[i] = xi;
      sx += xi * xi;
    }
    vh[i] = vi;
    sv += vi * vi;
  }
  sv = block_sum<kVecThreads>(sv, sm);
  if (threadIdx.x == 0) partV[blockIdx.x] = sv;
  sx = block_sum<kVecThreads>(sx, sm);
  if (threadIdx.x == 0) partX[blockIdx.x] = sx;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st[L_BETA] = beta;
    if (k == 0) {
      st[L_BNORM] = beta;
      st[L_PHIBAR1] = beta;  // phibar_1
    } else {
      st[L_C] = c;
      st[L_S] = sn;
      st[L_RHO] = rho;
      st[((k + 1) & 1) ? L_PHIBAR1 : L_PHIBAR0] = sn * phibar;
      st[L_ANORM2] += alpha * alpha + beta * beta;
      fl[LF_ITERS] = k;
    }
  }
}
__global__ __launch_bounds__(kVecThreads) void k_lsqr_v(int k, LsqrProd tv, double *vh, const double *__restrict__ w, double *x, int n, long N,
                                                        const double *__restrict__ partU, int np, double *partV, double *partX, double *st,
                                                        int *fl) {
  d_lsqr_v(k, tv, vh, w, x, n, N, partU, np, partV, partX, st, fl);
}

// k >= 1.  tol: atol = btol.
__device__ __forceinline__ void d_lsqr_u(int k, LsqrProd tu, double *uh, const double *__restrict__ vh, double *w, int n, long N,
                                         const double *__restrict__ partV, const double *__restrict__ partX, int np,
                                         double *partU, double *st, int *fl, double tol) {
  // (workgroup 0 of THIS launch may raise the flag: one lane reads it for its workgroup, so a workgroup leaves or stays as a whole)
  __shared__ int leave;
  if (threadIdx.x == 0) leave = fl[LF_DONE];
  __syncthreads();
  if (leave) return;
  __shared__ double sm[kVecThreads / 64];
  __shared__ double bc;
  const double alpha = lsqr_bcast(sqrt(part_sum(partV, np, sm)), &bc);
  const double ia = lsqr_inv(alpha);
  const double beta = st[L_BETA];
  double cprev = 0., wback = 0., rhobar = alpha;
  if (k > 1) {
    cprev = st[L_C];
    wback = st[L_S] * alpha * lsqr_inv(st[L_RHO]);  // theta_k / rho_{k-1}
    rhobar = -cprev * alpha;
  }
  if (blockIdx.x == 0) {  // the tests for x_{k-1}
    const double xn2 = k > 1 ? part_sum(partX, np, sm) : 0.;
    if (threadIdx.x == 0) {
      const double phibar = st[(k & 1) ? L_PHIBAR1 : L_PHIBAR0], bnorm = st[L_BNORM];
      const double anorm = sqrt(st[L_ANORM2]), xnorm = sqrt(xn2);
      const double rnorm = phibar, arnorm = k > 1 ? phibar * alpha * fabs(cprev) : alpha * beta;
      st[L_ALPHA] = alpha;
      st[L_RHOBAR] = rhobar;
      st[L_RNORM] = rnorm;
      st[L_ARNORM] = arnorm;
      st[L_XNORM] = xnorm;
      st[L_ANORM] = anorm;
      int stop = 0;
      if (rnorm <= tol * bnorm + tol * anorm * xnorm) stop = 1;
      else if (arnorm <= tol * anorm * rnorm || alpha == 0.) stop = 2;
      if (stop) {
        fl[LF_STOP] = stop;
        fl[LF_DONE] = 1;
      }
    }
  }
  const double uback = alpha * lsqr_inv(beta);
  double su = 0.;
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < N; i += (long)gridDim.x * kVecThreads) {
    w[i] = vh[i] * ia - wback * w[i];
    const double ui = tu.at(i, n) * ia - uback * uh[i];
    uh[i] = ui;
    su += ui * ui;
  }
  su = block_sum<kVecThreads>(su, sm);
  if (threadIdx.x == 0) partU[blockIdx.x] = su;
}
__global__ __launch_bounds__(kVecThreads) void k_lsqr_u(int k, LsqrProd tu, double *uh, const double *__restrict__ vh, double *w, int n, long N,
                                                        const double *__restrict__ partV, const double *__restrict__ partX, int np,
                                                        double *partU, double *st, int *fl, double tol) {
  d_lsqr_u(k, tu, uh, vh, w, n, N, partV, partX, np, partU, st, fl, tol);
}

// Scratch of the derivative entry points (diff.hpp): taken from the block pool at a workspace's first call, kept until scs_finish.
// It has two parts.
//   What belongs to the SOLUTION (DiffScratch): the fixed point vhat, the SOC records cinfo, the PSD tables' V / V' / lam, the box state
//   and ticket, the power cones' W (sym3) and the triangle's column pointers tri_up.  One per workspace, written by the preparation.
//   What belongs to ONE RIGHT-HAND SIDE, a lane (DiffLane): the LSQR vectors uh, vh, w, x (n + m each), the product slots tA, dW, dWmI
//   (m) and tAt, tP (n), the norm partials, the state and flag blocks: 8 m + 6 n doubles plus partials.
// Lane 0 is the scratch itself (DiffScratch derives from DiffLane): every one-direction entry point uses it and nothing else.  Lanes
// 1 .. K-1 are taken from the block pool at the first call that differentiates K directions at once (diff.hpp diff_alloc_lanes), kept
// until scs_finish and returned to the pool with the rest.  The two apply frames of a PSD block (dproj_psd.hpp: 2 NP^2 doubles of the
// 4 NP^2 + NP per block) are per right-hand side too, but only the five-launch tile path touches them, and that path never runs in
// lock step (GroupDiff::member_ok): they stay where they are, inside lane 0's frames.
constexpr int kDiffLanesMax = 32;  // directions of one multi call (include/scs_hip.h)
struct DiffLane {
  DevBuf<double> uh, vh, w, x, tA, dW, dWmI, tAt, tP, partU, partV, partX, st;
  DevBuf<int> fl;
  void alloc_lane(size_t n, size_t m, size_t nb) {
    for (DevBuf<double> *b : {&uh, &vh, &w, &x}) b->alloc(n + m);
    for (DevBuf<double> *b : {&tA, &dW, &dWmI}) b->alloc(m);
    for (DevBuf<double> *b : {&tAt, &tP}) b->alloc(n);
    for (DevBuf<double> *b : {&partU, &partV, &partX}) b->alloc(nb);
    st.alloc(L_COUNT);
    fl.alloc(LF_COUNT);
  }
};
struct DiffScratch : DiffLane {
  bool ready = false, tri_ready = false;
  DevBuf<double> vhat, cinfo;
  DprojPsdTables psd;
  DevBuf<double> box, sym3;     // the box cone's state (dbox_scratch_doubles) and the power cones' W (6 per cone); none of either: not allocated
  DevBuf<unsigned> box_ticket;  // (k_proj_box_round, box cones above kDboxMultiMin only)
  DevBuf<int> tri_up;      // column pointers of the caller's triangle of P (the gather of dL/dP), built at the first request
  DevBuf<double> eff;      // (dc_eff ; db_eff) of a forward call that perturbs A or P (perturb.hpp): n + m, taken at the first such call
  std::vector<std::unique_ptr<DiffLane>> more;  // lanes 1 ..
  // scs_hip_refine (refine.hpp): the base and the trial point of the Newton iteration (x^ n and v^ m each: 2 (n + m) doubles), the
  // partials of the residual pass and its state block.  Taken at the first refine call; a workspace that never refines has none.
  struct Refine {
    bool ready = false;
    DevBuf<double> bx, bv, tx, tv, part, st;
  } refine;
  DiffLane &lane(int k) { return k == 0 ? static_cast<DiffLane &>(*this) : *more[(size_t)k - 1]; }
};

}  // namespace scship
