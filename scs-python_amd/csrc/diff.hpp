// diff.hpp — derivatives of a solve on the device (include/scs_hip.h: scs_hip_adjoint[_device], scs_hip_derivative[_device]).
//
// At a solution let v = s - y: s = Pi_K(v), y = Pi_K(v) - v.  The optimality conditions in (x, v) are
//     F1 = P x + A'(Pi(v) - v) + c = 0,   F2 = A x + Pi(v) - b = 0,   J = [[P, A'(W - I)], [A, W]],  W = D Pi_K(v)  (dproj.hpp)
// adjoint:   g = (gx ; W gs + (W - I) gy),  J' lambda = g,  dL/dc = -lambda1,  dL/db = lambda2,
//            dL/dA_ij = -(y_i lambda1_j + lambda2_i x_j),  dL/dP_ij = -(lambda1_i x_j + lambda1_j x_i) (i < j),  dL/dP_ii = -lambda1_i x_i
// forward:   J (dx ; dv) = (-dc ; db),  ds = W dv,  dy = (W - I) dv
//            (with perturbations dA, dP of the matrix values: dc + dP x + dA' y and db - dA x in place of dc and db — perturb.hpp)
// The systems are solved by LSQR (lsqr.hpp) on the RESIDENT, equilibrated matrices A^ = D A E, P^ = E P E at v^ = sigma (D s - y / D):
// the hatted problem has the same F, and D is constant on every SOC block and on every PSD block (normalize_dev.hpp k_enforce_blocks), so
// Pi commutes with the scaling there and the derivation carries over to the s cones unchanged (dproj_psd.hpp).  The same holds for the
// power cones: each is a 3-row boundary of HostCone::boundaries, so D is constant on it.  The box cone in hatted coordinates is again
// a box cone, with the bounds bl_j D_{j+1} / D_0 — the workspace's working copies box_bl / box_bu (setup.hpp), not the _orig ones —
// so its W is that of the hatted cone at v^ (dproj_box_pow.hpp) and nothing else changes.
// In: gx^ = E gx / sigma, gy^ = D gy / sigma,
// gs^ = gs / (D sigma), dc^ = sigma E dc, db^ = sigma D db.  Out: dL/dc = sigma E dL/dc^, dL/db = sigma D dL/db^,
// dL/dA_ij = D_i E_j dL/dA^_ij, dL/dP_ij = E_i E_j dL/dP^_ij; dx = E dx^ / sigma, dy = D dy^ / sigma, ds = ds^ / (D sigma).  With
// mu = sigma E lambda1 = -dL/dc and nu = sigma D lambda2 = dL/db the matrix gradients need the caller's x, y only:
//     dL/dA_ij = -(y_i mu_j + nu_i x_j),   dL/dP_ij = -(mu_i x_j + mu_j x_i).
// D, E and sigma are constants here, which is exact: the solution of the caller's problem does not depend on them.
//
//     J' l = [P l1 + A' l2 ; (W - I)(A l1) + W l2] = [.. ; W (A l1 + l2) - A l1]        J q = [P q1 + A'((W - I) q2) ; A q1 + W q2]
// The products go through launch_spmv with EpiStore (every layout finishes it: the split pass layout through k_epi_finish).
//
// Every kernel here, in lsqr.hpp, dproj.hpp and dproj_psd.hpp is a __device__ body d_X with its one-problem entry k_X; a batch of
// workspaces is differentiated in lock step through the grouped entries of the same bodies (diff_batch.hpp).  Everything the two
// paths must agree on to give the same bits is defined once, below the kernels: DiffLimits and diff_fill_info (options in, figures
// out), diff_plan (the cone plan), DiffWiring (which scratch slot holds what, the operands and order of each product, which product
// each LSQR half step consumes) and lsqr_drive (the chunk schedule and the extra half step at the cap).  diff_impl launches from
// them; GroupDiff::run fills its tables from them.
//
// A call reads solx / soly / sols and the matrices, and writes the workspace's DiffScratch only (the eigen-decomposition of the PSD
// blocks borrows a block of the pool for the call; the solve's psd_scratch is not touched).
//
// Lanes (lsqr.hpp DiffScratch / DiffLane).  The scratch has a part that belongs to the SOLUTION — vhat, the cone records, the PSD
// tables, the box state, the power cones' W, tri_up: what the preparation writes and every apply of W reads — and a part that belongs
// to ONE right-hand side, a lane: the LSQR vectors, the product slots, the partials, the state and flag blocks.  Lane 0 is the scratch
// itself and all a one-direction call touches.  K directions at one solution (scs_hip_adjoint_multi / scs_hip_derivative_multi,
// csrc/scs_hip.hip diff_multi_entry) prepare once and then run K lanes: diff_wiring(w, call, lane) wires lane `lane` exactly as it
// wires lane 0, GroupDiff takes the (workspace, lane) pairs as its members, and the three SpMVs of a DiffProduct read the matrix once
// per tile of lanes (spmv_lanes.hpp).  Where GroupDiff::member_ok does not hold the K directions go through diff_impl in turn on lane 0.
#pragma once

namespace scship {

// uh[0..n) = E gx / sigma;  gyh = D gy / sigma;  gsh = gs / (D sigma)   (a missing input counts as 0; D == nullptr: as they are)
__device__ __forceinline__ void d_adj_in(const double *gx, const double *gy, const double *gs, const double *__restrict__ D,
                                         const double *__restrict__ E, double sigma, int n, int m, double *uh, double *gyh,
                                         double *gsh) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    if (i < n) {
      uh[i] = gx ? (E ? E[i] * gx[i] / sigma : gx[i]) : 0.;
    } else {
      const long k = i - n;
      gyh[k] = gy ? (D ? D[k] * gy[k] / sigma : gy[k]) : 0.;
      gsh[k] = gs ? (D ? gs[k] / (D[k] * sigma) : gs[k]) : 0.;
    }
  }
}
__global__ __launch_bounds__(kVecThreads) void k_adj_in(const double *gx, const double *gy, const double *gs, const double *__restrict__ D,
                                                        const double *__restrict__ E, double sigma, int n, int m, double *uh, double *gyh,
                                                        double *gsh) {
  d_adj_in(gx, gy, gs, D, E, sigma, n, m, uh, gyh, gsh);
}
// uh = (-sigma E dc ; sigma D db)
__device__ __forceinline__ void d_fwd_in(const double *db, const double *dc, const double *__restrict__ D,
                                         const double *__restrict__ E, double sigma, int n, int m, double *uh) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    if (i < n) uh[i] = dc ? -(E ? sigma * E[i] * dc[i] : dc[i]) : 0.;
    else uh[i] = db ? (D ? sigma * D[i - n] * db[i - n] : db[i - n]) : 0.;
  }
}
__global__ __launch_bounds__(kVecThreads) void k_fwd_in(const double *db, const double *dc, const double *__restrict__ D,
                                                        const double *__restrict__ E, double sigma, int n, int m, double *uh) {
  d_fwd_in(db, dc, D, E, sigma, n, m, uh);
}
// dc = -sigma E lambda1;  db = sigma D lambda2
__device__ __forceinline__ void d_adj_out(const double *__restrict__ lam, const double *__restrict__ D, const double *__restrict__ E,
                                          double sigma, int n, int m, double *dc, double *db) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    if (i < n) dc[i] = -(E ? sigma * E[i] * lam[i] : lam[i]);
    else db[i - n] = D ? sigma * D[i - n] * lam[i] : lam[i];
  }
}
__global__ __launch_bounds__(kVecThreads) void k_adj_out(const double *__restrict__ lam, const double *__restrict__ D, const double *__restrict__ E,
                                                         double sigma, int n, int m, double *dc, double *db) {
  d_adj_out(lam, D, E, sigma, n, m, dc, db);
}
// dx = E dx^ / sigma;  dy = D (W - I) dv^ / sigma;  ds = W dv^ / (D sigma)   (a nullptr output is skipped)
__device__ __forceinline__ void d_fwd_out(const double *__restrict__ q, const double *__restrict__ Wq, const double *__restrict__ WmIq,
                                          const double *__restrict__ D, const double *__restrict__ E, double sigma, int n, int m,
                                          double *dx, double *dy, double *ds) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    if (i < n) {
      if (dx) dx[i] = E ? E[i] * q[i] / sigma : q[i];
    } else {
      const long k = i - n;
      if (dy) dy[k] = D ? D[k] * WmIq[k] / sigma : WmIq[k];
      if (ds) ds[k] = D ? Wq[k] / (D[k] * sigma) : Wq[k];
    }
  }
}
__global__ __launch_bounds__(kVecThreads) void k_fwd_out(const double *__restrict__ q, const double *__restrict__ Wq, const double *__restrict__ WmIq,
                                                         const double *__restrict__ D, const double *__restrict__ E, double sigma, int n, int m,
                                                         double *dx, double *dy, double *ds) {
  d_fwd_out(q, Wq, WmIq, D, E, sigma, n, m, dx, dy, ds);
}
// dL/dA over the caller's CSC order = the CSR of A': slot p = (row j of A' = column of A, column i = row of A)
__device__ __forceinline__ void d_grad_a(const int *__restrict__ rp, const int *__restrict__ ci, int rows, long nnz,
                                         const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ dc,
                                         const double *__restrict__ db, double *dA) {
  for (long p = (long)blockIdx.x * kVecThreads + threadIdx.x; p < nnz; p += (long)gridDim.x * kVecThreads) {
    const int j = vm_row_of(rp, rows, p), i = ci[p];
    dA[p] = y[i] * dc[j] - db[i] * x[j];  // -(y_i mu_j + nu_i x_j), mu = -dc, nu = db
  }
}
__global__ __launch_bounds__(kVecThreads) void k_grad_a(const int *__restrict__ rp, const int *__restrict__ ci, int rows, long nnz,
                                                        const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ dc,
                                                        const double *__restrict__ db, double *dA) {
  d_grad_a(rp, ci, rows, nnz, x, y, dc, db, dA);
}
// dL/dP over the caller's triangle: the entries of row r of the full matrix on or below the diagonal are column r of the triangle, in
// order (matrix_update.hpp k_map_pf); up = the triangle's column pointers
__device__ __forceinline__ void d_grad_p(const int *__restrict__ rp, const int *__restrict__ ci, int n, long nnz,
                                         const int *__restrict__ up, const double *__restrict__ x, const double *__restrict__ dc,
                                         double *dP) {
  for (long q = (long)blockIdx.x * kVecThreads + threadIdx.x; q < nnz; q += (long)gridDim.x * kVecThreads) {
    const int r = vm_row_of(rp, n, q), c = ci[q];
    if (c > r) continue;
    const int k = (int)(q - rp[r]);
    if (k >= up[r + 1] - up[r]) continue;
    dP[up[r] + k] = c < r ? dc[c] * x[r] + dc[r] * x[c] : dc[r] * x[r];  // -(mu_c x_r + mu_r x_c), mu = -dc
  }
}
__global__ __launch_bounds__(kVecThreads) void k_grad_p(const int *__restrict__ rp, const int *__restrict__ ci, int n, long nnz,
                                                        const int *__restrict__ up, const double *__restrict__ x, const double *__restrict__ dc,
                                                        double *dP) {
  d_grad_p(rp, ci, n, nnz, up, x, dc, dP);
}

}  // namespace scship

// why this workspace cannot be differentiated ("" = it can): argument-free refusals, before any device work
static std::string diff_refusal(const ScsHipWork *w) {
  if (w->diff_state == 0) return "no solve yet: differentiate after scs_solve";
  if (w->diff_state == 2) return "the last solve did not end solved (status " + std::to_string(w->last_status_val) + "): there is no solution to differentiate";
  if (w->diff_state == 3) return "the resident solution is stale: b, c or the matrix changed since the last solve; solve again first";
  const HostCone &c = w->cone;
  const char *other = !c.cs.empty() ? "complex PSD (cs)" : c.ep > 0 ? "exponential (ep)" : c.ed > 0 ? "dual exponential (ed)" :
                      !c.d.empty() ? "log-det (d)" : !c.nuc_m.empty() ? "nuclear norm (nuc)" : !c.ell1.empty() ? "ell1" :
                      !c.sl_n.empty() ? "sum-of-largest (sl)" : nullptr;
  if (other)
    return std::string("the derivative of the ") + other + " cone projection is not implemented (z, l, q and s cones only, plus box and p)";
  return "";
}

// the box and power tables of a cone plan: the workspace's WORKING bounds (they follow the row scaling) and exponents, the caller's
// scratch (dbox_scratch_doubles(bsize) doubles, one ticket for a box above kDboxMultiMin, 6 doubles per power cone) and m doubles
// nobody reads during the preparation
static void dproj_plan_box_pow(DprojPlan &plan, const ScsHipWork *w, double *box_st, unsigned *ticket, double *sym3, double *tmp_m) {
  const HostCone &c = w->cone;
  if (c.bsize > 0) {
    plan.box.bsize = c.bsize; plan.box.off = c.off_box;
    plan.box.bl = w->box_bl.p; plan.box.bu = w->box_bu.p;
    plan.box.st = box_st; plan.box.ticket = ticket; plan.box.tmp = tmp_m + c.off_box;
  }
  if (!c.p.empty()) {
    plan.sym3.count = (int)c.p.size(); plan.sym3.off = c.off_p;
    plan.sym3.a = w->pow_a.p; plan.sym3.W = sym3;
  }
}

struct DiffCall {
  bool adjoint = true;
  const double *in[3] = {nullptr, nullptr, nullptr};          // adjoint: gx, gy, gs;  forward: db, dc
  double *out[4] = {nullptr, nullptr, nullptr, nullptr};      // adjoint: db, dc, dAx, dPx;  forward: dx, dy, ds
  const double *pert[2] = {nullptr, nullptr};                 // forward: dAx, dPx — perturbations of the matrix values (perturb.hpp)
  bool perturbs() const { return !adjoint && (pert[0] || pert[1]); }
  // the arguments' names in a refusal and their lengths in doubles (what a host twin stages)
  const char *in_name(int k) const {
    static const char *const adj[3] = {"gx", "gy", "gs"}, *const fwd[3] = {"db", "dc", ""};
    return (adjoint ? adj : fwd)[k];
  }
  const char *out_name(int k) const {
    static const char *const adj[4] = {"db", "dc", "dAx", "dPx"}, *const fwd[4] = {"dx", "dy", "ds", ""};
    return (adjoint ? adj : fwd)[k];
  }
  static const char *pert_name(int k) { return k == 0 ? "dAx" : "dPx"; }
  long in_len(const ScsHipWork *w, int k) const { return adjoint ? (k == 0 ? w->n : w->m) : (k == 0 ? w->m : k == 1 ? w->n : 0); }
  long out_len(const ScsHipWork *w, int k) const {
    if (adjoint) return k == 0 ? w->m : k == 1 ? w->n : pert_len(w, k - 2);
    return k == 0 ? w->n : k < 3 ? w->m : 0;
  }
  static long pert_len(const ScsHipWork *w, int k) { return k == 0 ? w->mats->a_nnz_in : w->mats->p_nnz_in; }
};

// the LSQR tolerance and iteration cap of a call over N = n + m unknowns
struct DiffLimits {
  double tol;
  long cap;
  DiffLimits(const ScsHipDiffOpts *o, long N) : tol(o && o->tol > 0. ? o->tol : 1e-8), cap(o && o->max_iters > 0 ? (long)o->max_iters : 4 * N) {}
};
// what a call reports, from the flag and state blocks LSQR left (info == nullptr: nothing)
static void diff_fill_info(ScsHipDiffInfo *info, const int *hfl, const double *hst, long cap, double ms) {
  if (!info) return;
  info->iters = (scs_int)std::min((long)hfl[LF_ITERS], cap);
  info->stop = hfl[LF_STOP] ? hfl[LF_STOP] : 3;
  info->residual = hst[L_BNORM] > 0. ? hst[L_RNORM] / hst[L_BNORM] : 0.;
  const double den = hst[L_ANORM] * hst[L_RNORM];
  info->normal_residual = den > 0. ? hst[L_ARNORM] / den : 0.;
  info->time_ms = ms;
}

static void diff_alloc(ScsHipWork *w) {
  DiffScratch &d = w->diff;
  if (d.ready) return;
  ArenaScope no_arena(nullptr);  // exact-size blocks from the block pool, returned to it by scs_finish
  const size_t n = (size_t)w->n, m = (size_t)w->m, N = n + m;
  for (DevBuf<double> *b : {&d.uh, &d.vh, &d.w, &d.x}) b->alloc(N);
  for (DevBuf<double> *b : {&d.tA, &d.dW, &d.dWmI, &d.vhat}) b->alloc(m);
  for (DevBuf<double> *b : {&d.tAt, &d.tP}) b->alloc(n);
  d.cinfo.alloc((size_t)3 * std::max(w->n_soc, 1));
  d.psd.build(w->psd_order_h, w->psd_off.p, w->psd_order.p, w->psd_woff.p, w->stream);
  if (w->cone.bsize > 0) d.box.alloc(dbox_scratch_doubles(w->cone.bsize));
  if (w->cone.bsize > kDboxMultiMin) d.box_ticket.alloc_zero(1, w->stream);
  if (!w->cone.p.empty()) d.sym3.alloc((size_t)6 * w->cone.p.size());
  const size_t nb = (size_t)vec_blocks((long)N);
  for (DevBuf<double> *b : {&d.partU, &d.partV, &d.partX}) b->alloc(nb);
  d.st.alloc(L_COUNT);
  d.fl.alloc(LF_COUNT);
  d.ready = true;
}
// lanes 1 .. K-1 of a call that differentiates K directions at once (lsqr.hpp DiffLane): taken at the first call that needs them
static void diff_alloc_lanes(ScsHipWork *w, int K) {
  diff_alloc(w);
  DiffScratch &d = w->diff;
  ArenaScope no_arena(nullptr);
  while ((int)d.more.size() + 1 < K) {
    std::unique_ptr<DiffLane> L(new DiffLane());
    L->alloc_lane((size_t)w->n, (size_t)w->m, (size_t)vec_blocks((long)w->n + w->m));
    d.more.push_back(std::move(L));
  }
}

// column pointers of the caller's triangle of P from the resident full matrix (once per workspace)
static void diff_build_tri(ScsHipWork *w) {
  DiffScratch &d = w->diff;
  if (d.tri_ready) return;
  ArenaScope no_arena(nullptr);
  hipStream_t s = w->stream;
  const int n = w->n;
  DevBuf<int> cnt, tmp;
  cnt.alloc((size_t)n);
  d.tri_up.alloc((size_t)n + 1);
  tmp.alloc_zero((size_t)(n / kScanTile + 4), s);
  hipLaunchKernelGGL(k_pf_lowcount, dim3(vec_blocks(n)), dim3(kVecThreads), 0, s, (const int *)w->Pf.rowptr.p, (const int *)w->Pf.col.p, n, cnt.p);
  device_exclusive_scan(cnt.p, d.tri_up.p, n, tmp.p, s);
  int total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, d.tri_up.p + n, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));  // (cnt / tmp are locals)
  if ((long)total != w->mats->p_nnz_in) {
    d.tri_up.release();
    throw std::runtime_error("P was given with " + std::to_string(w->mats->p_nnz_in) + " entries of which " + std::to_string(total) +
                             " lie in the upper triangle: its gradient cannot be gathered");
  }
  d.tri_ready = true;
}

// the cone plan of a call: the workspace's cone tables over its scratch.  psd.tmp_m and the box tmp inside it lie in dW, which is free
// until the right-hand side is formed.
static DprojPlan diff_plan(ScsHipWork *w) {
  DiffScratch &d = w->diff;
  DprojPlan plan;
  plan.z = w->cone.z; plan.l = w->cone.l; plan.n_soc = w->n_soc; plan.n_soc_big = w->n_soc_big; plan.G = w->soc_G;
  plan.off = w->soc_off.p; plan.dim = w->soc_dim.p; plan.big = w->soc_big.p;
  plan.vh = d.vhat.p; plan.cinfo = d.cinfo.p; plan.m = w->m;
  plan.psd = d.psd.plan;
  plan.psd.tmp_m = d.dW.p;
  dproj_plan_box_pow(plan, w, d.box.p, d.box_ticket.p, d.sym3.p, d.dW.p);
  return plan;
}

// One product of the operator on one workspace, J q or J' l: the apply of W, the three SpMVs (each with its input and where it stores)
// and the combination the LSQR kernel that consumes the product reads.  The pieces go in the order
//     J q:   apply, A (Ar), A' (At), P (Pf)             J' l:  A (Ar), apply (it reads A l1), A' (At), P (Pf)
// (transposed says which); a workspace without P skips pf.
struct DiffProduct {
  struct Spmv {
    const double *in;
    EpiStore out;
  };
  bool transposed;
  DprojIo io;
  Spmv ar, at, pf;
  LsqrProd read;
};

// Which buffer of one lane of a workspace's DiffScratch holds what during one call: the one place where slots are aliased and products are wired.
// Both call paths read it: diff_impl launches from it, GroupDiff::run (diff_batch.hpp) fills its tables from it.
struct DiffWiring {
  // adjoint right-hand side: k_adj_in leaves gx^ in uh[0..n), gy^ in gyh = x[n..) and gs^ in gsh = tA (both free until LSQR starts);
  // the two applies leave W gs^ in dW and (W - I) gy^ in dWmI, which k_lsqr_start adds into uh[n..) (start_add)
  double *gyh = nullptr, *gsh = nullptr;
  DprojIo rhs_gs{}, rhs_gy{};
  const double *start_add[2] = {nullptr, nullptr};
  // forward right-hand side: the caller's (dc ; db), or the effective pair in eff when the call perturbs A or P (eff_c != nullptr:
  // (dc + dP x + dA' y ; db - dA x), perturb.hpp, whose products pass through tAt, tP, tA — free until the LSQR products)
  const double *dc_in = nullptr, *db_in = nullptr;
  double *eff_c = nullptr, *eff_b = nullptr;
  // M = J' (adjoint) or J (forward).  pv = M' uh, which step_v consumes;  pu = M vh, which step_u consumes
  DiffProduct pv{}, pu{};
  // after the loop.  adjoint: dL/dc and dL/db in tP and tA (free now);  forward: the apply that turns dv^ = x[n..) into dW, dWmI
  double *dc = nullptr, *db = nullptr;
  DprojIo fin{};
};
static DiffWiring diff_wiring(ScsHipWork *w, const DiffCall &a, int lane = 0) {
  DiffLane &d = w->diff.lane(lane);
  const int n = w->n;
  const double *tP = w->has_P ? d.tP.p : nullptr;
  auto J = [&](const double *q) {
    return DiffProduct{false, DprojIo{q + n, nullptr, d.dW.p, d.dWmI.p}, {q, EpiStore{d.tA.p, 0}}, {d.dWmI.p, EpiStore{d.tAt.p, 0}},
                       {q, EpiStore{d.tP.p, 0}}, LsqrProd{d.tAt.p, tP, d.tA.p, d.dW.p, 0}};
  };
  auto Jt = [&](const double *l) {
    return DiffProduct{true, DprojIo{d.tA.p, l + n, d.dW.p, nullptr}, {l, EpiStore{d.tA.p, 0}}, {l + n, EpiStore{d.tAt.p, 0}},
                       {l, EpiStore{d.tP.p, 0}}, LsqrProd{d.tAt.p, tP, d.tA.p, d.dW.p, 1}};
  };
  DiffWiring wr;
  if (a.adjoint) {
    wr.gyh = d.x.p + n; wr.gsh = d.tA.p;
    wr.rhs_gs = DprojIo{wr.gsh, nullptr, d.dW.p, nullptr};
    wr.rhs_gy = DprojIo{wr.gyh, nullptr, nullptr, d.dWmI.p};
    wr.start_add[0] = d.dW.p; wr.start_add[1] = d.dWmI.p;
    wr.pv = J(d.uh.p); wr.pu = Jt(d.vh.p);
    wr.dc = d.tP.p; wr.db = d.tA.p;
  } else {
    wr.db_in = a.in[0]; wr.dc_in = a.in[1];
    if (a.perturbs()) {
      wr.dc_in = wr.eff_c = w->diff.eff.p;
      wr.db_in = wr.eff_b = w->diff.eff.p + n;
    }
    wr.pv = Jt(d.uh.p); wr.pu = J(d.vh.p);
    wr.fin = DprojIo{d.x.p + n, nullptr, d.dW.p, d.dWmI.p};
  }
  return wr;
}

// The host control of LSQR (lsqr.hpp): queue chunks of iterations between looks at the flags.  step_u(k) / step_v(k) queue the product
// and the kernel of that half step; finished() reads the flags back and says whether nothing is left to iterate.
template <class StepU, class StepV, class Finished> static void lsqr_drive(long cap, StepU &&step_u, StepV &&step_v, Finished &&finished) {
  step_v(0);
  long k = 0;  // iterations enqueued
  long chunk = 8;
  bool done;
  while (true) {
    const long upto = std::min(cap, k + chunk);
    while (k < upto) {
      ++k;
      step_u((int)k);
      step_v((int)k);
    }
    done = finished();
    if (done || k >= cap) break;
    chunk = std::max(4L, std::min(k / 2, 64L));
  }
  if (!done) {  // the cap: the tests (and the figures of info) for x_cap need alpha_{cap+1}
    step_u((int)(k + 1));
    finished();
  }
}

// LSQR on lane 0 of one workspace, from the right-hand side in uh (wr.start_add: what k_lsqr_start adds into its rows >= n) to the
// answer in x: the start, the products as `wr` wires them over `plan`, the chunks of lsqr_drive.  hfl: the flag block as LSQR left it.
// diff_impl and refine_impl (refine.hpp) both solve through here.
static void diff_lsqr(ScsHipWork *w, const DiffWiring &wr, const DprojPlan &plan, const DiffLimits &lim, int *hfl) {
  hipStream_t s = w->stream;
  const int n = w->n;
  const long N = (long)n + w->m;
  DiffScratch &d = w->diff;
  const int nbN = vec_blocks(N);
  const dim3 gN(nbN), bV(kVecThreads);
  const int *done = d.fl.p + LF_DONE;
  hipLaunchKernelGGL(k_lsqr_start, gN, bV, 0, s, d.uh.p, wr.start_add[0], wr.start_add[1], n, N, d.x.p, d.w.p, d.partU.p, d.st.p, d.fl.p);

  // ---- LSQR: the products leave their results in tAt, tP, tA, dW ----
  auto product = [&](const DiffProduct &p) {
    if (!p.transposed) launch_dproj(plan, p.io, done, s);
    launch_spmv(w->Ar.view(), p.ar.in, p.ar.out, done, s);
    if (p.transposed) launch_dproj(plan, p.io, done, s);
    launch_spmv(w->At.view(), p.at.in, p.at.out, done, s);
    if (w->has_P) launch_spmv(w->Pf.view(), p.pf.in, p.pf.out, done, s);
  };
  auto step_v = [&](int k) {
    product(wr.pv);
    hipLaunchKernelGGL(k_lsqr_v, gN, bV, 0, s, k, wr.pv.read, d.vh.p, (const double *)d.w.p, d.x.p, n, N, (const double *)d.partU.p, nbN, d.partV.p,
                       d.partX.p, d.st.p, d.fl.p);
  };
  auto step_u = [&](int k) {
    product(wr.pu);
    hipLaunchKernelGGL(k_lsqr_u, gN, bV, 0, s, k, wr.pu.read, d.uh.p, (const double *)d.vh.p, d.w.p, n, N, (const double *)d.partV.p,
                       (const double *)d.partX.p, nbN, d.partU.p, d.st.p, d.fl.p, lim.tol);
  };
  for (int k = 0; k < LF_COUNT; ++k) hfl[k] = 0;
  lsqr_drive(lim.cap, step_u, step_v, [&] {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(hfl, d.fl.p, sizeof(int) * LF_COUNT, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return hfl[LF_DONE] != 0;
  });
}

// One workspace.  The caller holds w->mtx and the scratch turn, has selected the device and refused bad arguments (diff_check).  All
// pointers are device pointers.
static void diff_impl(ScsHipWork *w, const DiffCall &a, const ScsHipDiffOpts *o, ScsHipDiffInfo *info) {
  const double t0 = now_ms();
  hipStream_t s = w->stream;
  const int n = w->n, m = w->m;
  const long N = (long)n + m;
  const DiffLimits lim(o, N);
  diff_alloc(w);
  if (a.adjoint && a.out[3]) diff_build_tri(w);
  if (a.perturbs()) pert_alloc(w, a.pert[0] != nullptr, a.pert[1] != nullptr, "scs_hip_derivative_full");
  DiffScratch &d = w->diff;
  const double *D = w->normalized ? w->D.p : nullptr, *E = w->normalized ? w->E.p : nullptr;
  const double sigma = w->normalized ? w->scal.sigma : 1.0;
  const int nbN = vec_blocks(N);
  const dim3 gN(nbN), bV(kVecThreads);
  const DiffWiring wr = diff_wiring(w, a);

  // ---- the fixed point and the cone records ----
  hipLaunchKernelGGL(k_dproj_vhat, dim3(vec_blocks(m)), bV, 0, s, (const double *)w->sols.p, (const double *)w->soly.p, D, sigma, m, d.vhat.p);
  const DprojPlan plan = diff_plan(w);
  launch_dproj_prep(plan, s);

  // ---- right-hand side into uh, x = w = 0 ----
  if (a.adjoint) {
    hipLaunchKernelGGL(k_adj_in, gN, bV, 0, s, a.in[0], a.in[1], a.in[2], D, E, sigma, n, m, d.uh.p, wr.gyh, wr.gsh);
    launch_dproj(plan, wr.rhs_gs, nullptr, s);
    launch_dproj(plan, wr.rhs_gy, nullptr, s);
  } else {
    if (wr.eff_c) pert_launch(w, a.pert[0], a.pert[1], a.in[1], a.in[0], -1.0, wr.eff_c, wr.eff_b, s);
    hipLaunchKernelGGL(k_fwd_in, gN, bV, 0, s, wr.db_in, wr.dc_in, D, E, sigma, n, m, d.uh.p);
  }
  // ---- LSQR ----
  int hfl[LF_COUNT] = {0, 0, 0, 0};
  diff_lsqr(w, wr, plan, lim, hfl);
  double hst[L_COUNT];
  HIP_CHECK(hipMemcpyAsync(hst, d.st.p, sizeof(hst), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));

  // ---- results ----
  if (a.adjoint) {
    hipLaunchKernelGGL(k_adj_out, gN, bV, 0, s, (const double *)d.x.p, D, E, sigma, n, m, wr.dc, wr.db);
    if (a.out[0]) HIP_CHECK(hipMemcpyAsync(a.out[0], wr.db, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
    if (a.out[1]) HIP_CHECK(hipMemcpyAsync(a.out[1], wr.dc, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    if (a.out[2] && w->At.nnz > 0)
      hipLaunchKernelGGL(k_grad_a, dim3(vec_blocks((long)w->At.nnz)), bV, 0, s, (const int *)w->At.rowptr.p, (const int *)w->At.col.p, w->At.rows,
                         (long)w->At.nnz, (const double *)w->solx.p, (const double *)w->soly.p, (const double *)wr.dc, (const double *)wr.db, a.out[2]);
    if (a.out[3] && w->Pf.nnz > 0)
      hipLaunchKernelGGL(k_grad_p, dim3(vec_blocks((long)w->Pf.nnz)), bV, 0, s, (const int *)w->Pf.rowptr.p, (const int *)w->Pf.col.p, n, (long)w->Pf.nnz,
                         (const int *)d.tri_up.p, (const double *)w->solx.p, (const double *)wr.dc, a.out[3]);
  } else {
    launch_dproj(plan, wr.fin, nullptr, s);
    hipLaunchKernelGGL(k_fwd_out, gN, bV, 0, s, (const double *)d.x.p, (const double *)d.dW.p, (const double *)d.dWmI.p, D, E, sigma, n, m, a.out[0],
                       a.out[1], a.out[2]);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));
  diff_fill_info(info, hfl, hst, lim.cap, now_ms() - t0);
}
