// dproj_psd.hpp — W = D Pi_{S+}(v), the derivative of the projection onto the real PSD cone, applied to a vector.
//
// One block of order p in svec layout (lower triangle by column, off-diagonals times sqrt(2), as psd.hpp).  With mat(v) = Q diag(lam) Q'
//     W u = svec(Q (B o (Q' smat(u) Q)) Q'),   B_ij = (lam_i^+ - lam_j^+) / (lam_i - lam_j):
// 1 where both eigenvalues are positive, 0 where neither is, hi / (hi - lo) across the sign change, and on the diagonal 1 if
// lam_i > 0, else 0 (psd.hpp psd_dmap: the divided difference `gdd` of psd_fmap, whose own limit on the diagonal is this rule).
// W is symmetric.  An order-1 block is a nonnegative row, an order-0 block is skipped.
//
// Preparation, once per adjoint / derivative call (launch_dproj_psd_prep): the blocks of v are copied into a temporary vector and
// decomposed by K9 in one launch — k_proj_psd<0>, one workgroup per matrix, cold start, refinement off, no cooperative launch and no
// spinning barrier — over K9-layout scratch of ITS OWN, taken from the block pool for the call and given back (the rotation log makes
// it ~30 times larger than V).  The solve's warm-start state (the workspace's psd_scratch) is neither read nor written.  The sweeps stop at
// ||offdiag||_F <= max(kDprojPsdTau, 8 NP 2^-52) ||A||_F — below the projection's kPsdOffTol2, because here the eigenvectors themselves are
// used and nothing corrects them to second order.  V, V' and lam = diag(V' A V) of every matrix are then gathered into compact frames.
// The padding rows n .. NP-1 of the NP x NP frame decouple: they are zero, wave_jacobi16 does not rotate an entry below 1e-300, so no
// rotation ever mixes a padding index with a real one: V is exactly [[Q, 0], [0, I]], lam is 0 there, and with u zero-padded the
// padding rows and columns of every product below are exactly zero.
//
// Apply (launch_dproj_psd), the DprojIo contract of dproj.hpp: u = a (+ b), Wu and/or WmIu = Wu - u written, outputs never alias
// inputs, every kernel starts with `if (done && *done) return;`.
//   tile path (orders > kDprojPsdFusedMax): five launches, every cone of the stage in the grid, per-cone task ranges from a table
//   (mixed orders share a launch); one wavefront = one task of 16x16 tiles on v_mfma_f64_16x16x4_f64, the task functions of psd.hpp:
//     (a) U = smat(a + b) into the frame, zero padding      (b) Tt = V' U (G1)      (c) A0 = V' U V, symmetric (G2)
//     (d) T = V (B o A0), B formed in the operand load (R1, kPsdMapDiff)      (e) V T' packed, Wu and Wu - u (R2's tiles)
//   8 NP^3 flops per cone per apply.
//   fused path (orders 1 .. kDprojPsdFusedMax = kPsdSmallMax): one launch, one wavefront per matrix, four matrices per 256-lane
//   workgroup; Q, U and the intermediate in LDS at leading dimension 33, the four products as FMA loops (latency-bound: the point is one
//   launch per LSQR iteration for problems with many small cones).  The order-1 blocks — nonnegative rows — ride in this launch.
// Every sum has a fixed order: two calls on the same state give the same bits.
#pragma once
#include "common.hpp"
#include "psd.hpp"  // (included from dproj.hpp, behind DprojIo)

namespace scship {

constexpr double kDprojPsdTau = 1e-13;  // stopping level of the decomposition (relative off-diagonal norm); spectral.hpp stops at the same 1e-26 squared
constexpr int kDprojPsdFusedMax = kPsdSmallMax;
constexpr int kDprojPsdThreads = 256;
inline double dproj_psd_tol2(int max_np) {
  const double lvl = std::max(kDprojPsdTau, 8. * max_np * 2.220446049250313e-16);
  return lvl * lvl;
}
__host__ __device__ inline long dproj_psd_frame_doubles(long n) {  // V, V', two apply frames, lam
  const long np = psd_np(n);
  return 4 * np * np + np;
}

// the PSD part of a DprojPlan: the workspace's tables (psd_off / psd_order / psd_woff: orders > kPsdSmallMax first) and DiffScratch's
struct DprojPsdPlan {
  int count = 0, n_tile = 0, n_small = 0, ntask = 0, max_np = 0;
  const int *off = nullptr, *order = nullptr;
  const long *woff = nullptr;   // K9-layout scratch offsets (preparation only)
  const long *foff = nullptr;   // offset of each block's frames in `frames`
  const int *tstart = nullptr;  // n_tile + 1: first task of tile-path entry k
  const int *tcone = nullptr;   // n_tile: its block
  const int *small = nullptr;   // n_small: the blocks of the fused path (orders 1 .. kDprojPsdFusedMax)
  double *frames = nullptr;
  const double *tol2 = nullptr;  // device: the stopping level, squared
  long scratch_doubles = 0;      // K9-layout scratch the preparation borrows
  double *tmp_m = nullptr;       // m doubles the preparation may overwrite
};

// V, V' and lam from the K9 scratch of block c into its frames; an order-1 block keeps its entry of v as lam[0]
__device__ __forceinline__ void d_dproj_psd_gather(DprojPsdPlan P, const double *__restrict__ scratch,
                                                   const double *__restrict__ vh) {
  const int c = blockIdx.x;
  const int n = P.order[c];
  if (n < 1) return;
  double *F = P.frames + P.foff[c];
  const int NP = (int)psd_np(n);
  double *V = F, *Vt = F + (size_t)NP * NP, *lam = F + (size_t)4 * NP * NP;
  if (n == 1) {
    if (threadIdx.x == 0) lam[0] = vh[P.off[c]];
    return;
  }
  const double *A = scratch + P.woff[c], *Vs = A + (size_t)NP * NP;
  for (int e = threadIdx.x; e < NP * NP; e += kDprojPsdThreads) {
    const int i = e % NP, j = e / NP;
    const double v = Vs[e];
    V[e] = v;
    Vt[j + (size_t)NP * i] = v;
  }
  for (int j = threadIdx.x; j < NP; j += kDprojPsdThreads) lam[j] = j < n ? A[j + (size_t)NP * j] : 0.;
}
__global__ __launch_bounds__(kDprojPsdThreads) void k_dproj_psd_gather(DprojPsdPlan P, const double *__restrict__ scratch,
                                                                       const double *__restrict__ vh) {
  d_dproj_psd_gather(P, scratch, vh);
}

// ---- tile path ----
enum : int { DPSD_UNPACK = 0, DPSD_G1, DPSD_G2, DPSD_R1, DPSD_R2 };
__host__ __device__ inline int dproj_psd_tasks(int n) {  // tasks of one stage: (tile, group of kPsdNJ tiles)
  const int ntile = (int)psd_np(n) / 16;
  return ntile * ((ntile + kPsdNJ - 1) / kPsdNJ);
}
__device__ __forceinline__ long dproj_psd_packed(int i, int j, int n) { return (long)j * n - (long)j * (j - 1) / 2 + (i - j); }  // i >= j

template <int STAGE>
__global__ __launch_bounds__(64) void k_dproj_psd_tile(DprojIo io, DprojPsdPlan P, const int *done) {
  if (done && *done) return;
  __shared__ double Sw[16 * 17];
  const int gtask = (int)blockIdx.x;
  int lo = 0, hi = P.n_tile;  // entry k with tstart[k] <= gtask < tstart[k + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (P.tstart[mid] <= gtask) lo = mid;
    else hi = mid;
  }
  const int c = P.tcone[lo], task = gtask - P.tstart[lo];
  const int n = P.order[c], NP = (int)psd_np(n), ntile = NP / 16, ld = NP;
  if (task >= dproj_psd_tasks(n)) return;
  double *V = P.frames + P.foff[c], *Vt = V + (size_t)NP * NP, *F0 = Vt + (size_t)NP * NP, *F1 = F0 + (size_t)NP * NP;
  const double *lam = F1 + (size_t)NP * NP;
  const long o0 = P.off[c];
  const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
  const double isq2 = 0.70710678118654752440, sq2 = 1.41421356237309504880;
  if (STAGE == DPSD_UNPACK) {
    const int tj = task % ntile, ti0 = (task / ntile) * kPsdNJ;
    for (int jj = 0; jj < kPsdNJ && ti0 + jj < ntile; ++jj)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = (ti0 + jj) * 16 + li, j = tj * 16 + lk + 4 * t;
        double v = 0.;
        if (i < n && j < n) v = i == j ? io.u(o0 + dproj_psd_packed(i, i, n)) : isq2 * io.u(o0 + dproj_psd_packed(max(i, j), min(i, j), n));
        F0[i + (size_t)ld * j] = v;
      }
  } else if (STAGE == DPSD_G1) {
    psd_task_g1(task, NP, F0, Vt, F1, Sw, li, lk);
  } else if (STAGE == DPSD_G2) {
    psd_task_g2(task, NP, F0, Vt, F1, Sw, li, lk);
  } else if (STAGE == DPSD_R1) {
    psd_task_r1<kPsdMapDiff>(task, NP, F0, V, F1, lam, Sw, li, lk);
  } else {  // V T' = (T V')' over the lower tiles of psd_task_r2, straight into the packed outputs
    const int ti = task % ntile, tj0 = (task / ntile) * kPsdNJ;
    if (tj0 > ti) return;
    f64x4 acc[kPsdNJ];
    mma_row(F1, V, ld, NP, ti, tj0, ti, li, lk, acc);
#pragma unroll
    for (int jj = 0; jj < kPsdNJ; ++jj) {
      const int tj = tj0 + jj;
      if (tj > ti) break;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = ti * 16 + lk + 4 * t, j = tj * 16 + li;
        if (i < n && j <= i) {
          const long at = o0 + dproj_psd_packed(i, j, n);
          io.put(at, i == j ? acc[jj][t] : acc[jj][t] * sq2, io.u(at));
        }
      }
    }
  }
}

// ---- fused path: one wavefront per matrix of order 1 .. kDprojPsdFusedMax ----
constexpr int kDprojPsdSz = 32 * kPsdSLd;                                                      // one 32 x 33 matrix
constexpr size_t kDprojPsdFusedLds = (size_t)(kDprojPsdThreads / 64) * 3 * kDprojPsdSz * sizeof(double);  // Q, U, T per wavefront
__device__ __forceinline__ void d_dproj_psd_fused(DprojIo io, DprojPsdPlan P, const int *done) {
  if (done && *done) return;
  extern __shared__ __attribute__((aligned(16))) double dpsd_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = (int)blockIdx.x * (kDprojPsdThreads / 64) + wave;
  if (k >= P.n_small) return;  // (no workgroup barrier below)
  const int c = P.small[k];
  const int n = P.order[c];
  const long o0 = P.off[c];
  const double *Vg = P.frames + P.foff[c];
  const int NP = (int)psd_np(n);
  const double *lamg = Vg + (size_t)4 * NP * NP;
  if (n == 1) {
    if (lane == 0) {
      const double ui = io.u(o0);
      io.put(o0, lamg[0] > 0. ? ui : 0., ui);
    }
    return;
  }
  constexpr int ld = kPsdSLd;
  double *Q = dpsd_lds + (size_t)wave * 3 * kDprojPsdSz, *U = Q + kDprojPsdSz, *T = U + kDprojPsdSz;
  const double isq2 = 0.70710678118654752440, sq2 = 1.41421356237309504880;
  for (int e = lane; e < n * n; e += 64) {
    const int i = e % n, j = e / n;
    Q[i + ld * j] = Vg[i + (size_t)NP * j];
    U[i + ld * j] = i == j ? io.u(o0 + dproj_psd_packed(i, i, n)) : isq2 * io.u(o0 + dproj_psd_packed(max(i, j), min(i, j), n));
  }
  wave_sync();
  // lane (j = lane & 31, h = lane >> 5) owns column j, rows h, h + 2, ...: one operand of every term is a broadcast read
  const int j = lane & 31, h = lane >> 5;
  const bool live = j < n;
  const int jc = live ? j : 0;
  const double lamj = lamg[jc];
  double acc[16];
  // T = U Q
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.;
  for (int q = 0; q < n; ++q) {
    const double y = Q[q + ld * jc];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fma(U[min(h + 2 * r, n - 1) + ld * q], y, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (live && h + 2 * r < n) T[(h + 2 * r) + ld * j] = acc[r];
  wave_sync();
  // U <- B o (Q' T)
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.;
  for (int q = 0; q < n; ++q) {
    const double y = T[q + ld * jc];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fma(Q[q + ld * min(h + 2 * r, n - 1)], y, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (live && h + 2 * r < n) U[(h + 2 * r) + ld * j] = psd_dmap(acc[r], lamg[h + 2 * r], lamj);
  wave_sync();
  // T <- Q U
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.;
  for (int q = 0; q < n; ++q) {
    const double y = U[q + ld * jc];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fma(Q[min(h + 2 * r, n - 1) + ld * q], y, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (live && h + 2 * r < n) T[(h + 2 * r) + ld * j] = acc[r];
  wave_sync();
  // out = T Q', lower triangle, packed
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.;
  for (int q = 0; q < n; ++q) {
    const double y = Q[jc + ld * q];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fma(T[min(h + 2 * r, n - 1) + ld * q], y, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = h + 2 * r;
    if (live && i < n && j <= i) {
      const long at = o0 + dproj_psd_packed(i, j, n);
      io.put(at, i == j ? acc[r] : acc[r] * sq2, io.u(at));
    }
  }
}
__global__ __launch_bounds__(kDprojPsdThreads) void k_dproj_psd_fused(DprojIo io, DprojPsdPlan P, const int *done) {
  d_dproj_psd_fused(io, P, done);
}

// ---- launches ----
// The decomposition.  `vh`: the fixed point (m doubles).  Synchronises the stream once (the borrowed scratch goes back to the pool).
inline void launch_dproj_psd_prep(const DprojPsdPlan &P, const double *vh, long m, hipStream_t s) {
  if (P.count <= 0) return;
  {
    ArenaScope no_arena(nullptr);
    DevBuf<double> scratch;
    scratch.alloc((size_t)std::max(P.scratch_doubles, 1L));
    HIP_CHECK(hipMemcpyAsync(P.tmp_m, vh, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, s));
    PsdBatch B{P.off, P.order, P.woff, P.count};
    hipLaunchKernelGGL(k_proj_psd<0>, dim3(P.count), dim3(kPsdThreads), kPsdLdsBytes, s, P.tmp_m, B, scratch.p, /*allow_warm=*/0, 0, (const int *)nullptr,
                       P.tol2, psd_refine_default(false), 0);
    hipLaunchKernelGGL(k_dproj_psd_gather, dim3(P.count), dim3(kDprojPsdThreads), 0, s, P, (const double *)scratch.p, vh);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    ++t_pool_release;  // the stream is idle: the block is the pool's again (a hit from the next call on)
    scratch.release();
    --t_pool_release;
  }
}
inline void launch_dproj_psd(const DprojPsdPlan &P, const DprojIo &io, const int *done, hipStream_t s) {
  if (P.n_small > 0)
    hipLaunchKernelGGL(k_dproj_psd_fused, dim3(ceil_div(P.n_small, kDprojPsdThreads / 64)), dim3(kDprojPsdThreads), kDprojPsdFusedLds, s, io, P, done);
  if (P.n_tile <= 0) return;
  const dim3 g((unsigned)P.ntask), b(64);
  hipLaunchKernelGGL(k_dproj_psd_tile<DPSD_UNPACK>, g, b, 0, s, io, P, done);
  hipLaunchKernelGGL(k_dproj_psd_tile<DPSD_G1>, g, b, 0, s, io, P, done);
  hipLaunchKernelGGL(k_dproj_psd_tile<DPSD_G2>, g, b, 0, s, io, P, done);
  hipLaunchKernelGGL(k_dproj_psd_tile<DPSD_R1>, g, b, 0, s, io, P, done);
  hipLaunchKernelGGL(k_dproj_psd_tile<DPSD_R2>, g, b, 0, s, io, P, done);
}

// What a workspace keeps for its PSD blocks from its first derivative call until scs_finish: per block V, V', lam and two apply frames
// (4 NP^2 + NP doubles) and the task tables, exact-size blocks of the block pool.
struct DprojPsdTables {
  DevBuf<long> foff;
  DevBuf<int> tstart, tcone, small;
  DevBuf<double> frames, tol2;
  DprojPsdPlan plan;
  // order_h: the orders behind `order` (the workspace's psd_order_h: orders > kPsdSmallMax first)
  void build(const std::vector<int> &order_h, const int *off, const int *order, const long *woff, hipStream_t s) {
    plan = DprojPsdPlan();
    const int count = (int)order_h.size();
    if (count == 0) return;
    std::vector<long> fo((size_t)count);
    std::vector<int> ts(1, 0), tc, sm;
    long ftot = 0, stot = 0;
    int max_np = 16;
    for (int c = 0; c < count; ++c) {
      const int n = order_h[(size_t)c];
      fo[(size_t)c] = ftot;
      ftot += dproj_psd_frame_doubles(n);
      stot += psd_scratch_doubles(n);
      max_np = std::max(max_np, (int)psd_np(n));
      if (n > kDprojPsdFusedMax) {
        tc.push_back(c);
        ts.push_back(ts.back() + dproj_psd_tasks(n));
      } else if (n >= 1) {
        sm.push_back(c);
      }
    }
    foff.upload(fo.data(), fo.size(), s);
    if (!tc.empty()) {
      tstart.upload(ts.data(), ts.size(), s);
      tcone.upload(tc.data(), tc.size(), s);
    }
    if (!sm.empty()) small.upload(sm.data(), sm.size(), s);
    frames.alloc((size_t)ftot);
    const double t2 = dproj_psd_tol2(max_np);
    tol2.upload(&t2, 1, s);
    HIP_CHECK(hipStreamSynchronize(s));  // (the host vectors are locals)
    plan.count = count; plan.n_tile = (int)tc.size(); plan.n_small = (int)sm.size(); plan.ntask = ts.back(); plan.max_np = max_np;
    plan.off = off; plan.order = order; plan.woff = woff;
    plan.foff = foff.p; plan.tstart = tstart.p; plan.tcone = tcone.p; plan.small = small.p;
    plan.frames = frames.p; plan.tol2 = tol2.p; plan.scratch_doubles = stot;
  }
};

}  // namespace scship
