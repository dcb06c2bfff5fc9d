// perturb.hpp — perturbations of the matrix VALUES in the forward derivative (include/scs_hip.h: scs_hip_derivative_full[_device],
// scs_hip_data_perturbation[_device]).
//
// With F1 = P x + A' y + c and F2 = A x + s - b (diff.hpp) a perturbation (dA, dP, db, dc) of the data gives
//     J (dx ; dv) = (-(dc + dP x + dA' y) ; db - dA x),
// so the forward path of diff.hpp stays as it is and only its inputs change:
//     dc_eff = dc + dP x + dA' y   (n),      db_eff = db - dA x   (m),
// x, y = the resident solution in the caller's coordinates (solx, soly) — the scaling of k_fwd_in follows.  dA is nnz(A) values in the
// order of the CSC arrays scs_init got, dP nnz(P) values of the stored triangle (an off-diagonal value stands for both mirror images).
//
// The three products are CSR row products on the caller's PATTERN whose values are read through an index map,
//     r_i = sum_q val[map[q]] * vec[col[q]]      (q over row i; map == nullptr: the identity)
//   dA' y   rows of CSR(A') = the caller's CSC order: no map
//   dA x    rows of the resident CSR(A), map = MatrixSet::ValueMaps::ar (matrix_update.hpp k_map_transpose)
//   dP x    rows of the full CSR(P),     map = MatrixSet::ValueMaps::pf (k_pf_lowcount, scan, k_map_pf)
// The index arrays are those of the resident CSR forms (every layout keeps them); the maps are the ones scs_hip_update_matrix uses and
// are built here when it has not run (matrix_update.hpp build_csr_value_maps: the two CSR maps only, no layout map).
//
// d_pert_rows: a group of 2^lg consecutive lanes per row (lg follows from the mean row length of the matrix: 4 .. 64 lanes), the lanes
// stride over the row, then a fixed xor tree inside the group.  A row of more than kPertLongIters strides is handed to the whole
// workgroup (as the peeled rows of spmv.hpp): the groups list such rows in LDS and the workgroup sums them one after the other,
// lanes striding by kPertThreads, block_sum.  Which lane adds which product is a function of the pattern alone and every sum has a
// fixed order: no floating-point atomics, two calls give the same bits.  (The order in which the long rows of a workgroup are listed
// is not fixed; each is summed on its own, so it does not matter.)
#pragma once

namespace scship {

constexpr int kPertThreads = 256;
constexpr int kPertLongIters = 16;  // a row of more than kPertLongIters * 2^lg entries goes to the whole workgroup
constexpr int kPertLgMin = 2, kPertLgMax = 6;

// lanes per row = 2^lg: the smallest power of two in [4, 64] that covers the mean row length
inline int pert_lg(long nnz, int rows) {
  const long mean = rows > 0 ? (nnz + rows - 1) / rows : 0;
  int lg = kPertLgMin;
  while (lg < kPertLgMax && (1L << lg) < mean) ++lg;
  return lg;
}
inline int pert_blocks(int rows, int lg) { return rows > 0 ? (rows + (kPertThreads >> lg) - 1) / (kPertThreads >> lg) : 0; }

__device__ __forceinline__ void d_pert_rows(const int *__restrict__ rp, const int *__restrict__ ci, const int *__restrict__ map,
                                            const double *__restrict__ val, const double *__restrict__ vec, int rows, int lg, double *out) {
  const int per_wg = kPertThreads >> lg;
  if ((long)blockIdx.x * per_wg >= rows) return;  // (grouped launches: the grid is sized for the member with the most rows)
  __shared__ int nlong;
  __shared__ int long_row[kPertThreads >> kPertLgMin];
  __shared__ double red[kPertThreads / 64];
  const int tid = threadIdx.x, W = 1 << lg, sub = tid & (W - 1);
  const int r = (int)blockIdx.x * per_wg + (tid >> lg);
  if (tid == 0) nlong = 0;
  __syncthreads();
  int p0 = 0, p1 = 0;
  if (r < rows) {
    p0 = rp[r];
    p1 = rp[r + 1];
  }
  const bool is_long = p1 - p0 > (kPertLongIters << lg);
  double acc = 0.;
  if (!is_long) {
#pragma unroll 4
    for (int q = p0 + sub; q < p1; q += W) acc += val[map ? map[q] : q] * vec[ci[q]];
  }
  for (int o = W >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, W);
  if (r < rows && sub == 0) {
    if (is_long) long_row[atomicAdd(&nlong, 1)] = r;
    else out[r] = acc;
  }
  __syncthreads();
  const int nl = nlong;
  for (int i = 0; i < nl; ++i) {
    const int rr = long_row[i], e = rp[rr + 1];
    double s = 0.;
#pragma unroll 4
    for (int q = rp[rr] + tid; q < e; q += kPertThreads) s += val[map ? map[q] : q] * vec[ci[q]];
    s = block_sum<kPertThreads>(s, red);
    if (tid == 0) out[rr] = s;
    __syncthreads();
  }
}
__global__ __launch_bounds__(kPertThreads) void k_pert_rows(const int *__restrict__ rp, const int *__restrict__ ci, const int *__restrict__ map,
                                                            const double *__restrict__ val, const double *__restrict__ vec, int rows, int lg,
                                                            double *out) {
  d_pert_rows(rp, ci, map, val, vec, rows, lg, out);
}

// out_c = (dc + tP) + tAt;  out_b = db + sgn tA   (a nullptr input counts as 0, a nullptr output is skipped)
__device__ __forceinline__ void d_pert_eff(const double *dc, const double *db, const double *__restrict__ tP, const double *__restrict__ tAt,
                                           const double *__restrict__ tA, double sgn, int n, int m, double *out_c, double *out_b) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    if (i < n) {
      if (out_c) out_c[i] = ((dc ? dc[i] : 0.) + (tP ? tP[i] : 0.)) + (tAt ? tAt[i] : 0.);
    } else {
      const long k = i - n;
      if (out_b) out_b[k] = (db ? db[k] : 0.) + (tA ? sgn * tA[k] : 0.);
    }
  }
}
__global__ __launch_bounds__(kVecThreads) void k_pert_eff(const double *dc, const double *db, const double *__restrict__ tP,
                                                          const double *__restrict__ tAt, const double *__restrict__ tA, double sgn, int n,
                                                          int m, double *out_c, double *out_b) {
  d_pert_eff(dc, db, tP, tAt, tA, sgn, n, m, out_c, out_b);
}

}  // namespace scship

// What a call with dA / dP needs beyond diff_alloc: n + m doubles for (dc_eff ; db_eff) and the CSR value maps of the set, each taken
// at the first call that needs it and kept (the scratch until scs_finish, the maps with the matrix set).  A failed allocation throws.
static void pert_alloc(ScsHipWork *w, bool need_a, bool need_p, const char *who) {
  DiffScratch &d = w->diff;
  ArenaScope no_arena(nullptr);  // exact-size blocks from the block pool
  if (!d.eff.p) d.eff.alloc((size_t)w->n + (size_t)w->m);
  build_csr_value_maps(w, need_a, need_p && w->has_P, who);
}

// The rows of one product: tAt = dA' y, tA = dA x, tP = dP x at the resident solution (dA / dP == nullptr: that product is not run).
// The caller has run diff_alloc and pert_alloc; all pointers are device pointers.
struct PertProduct {
  const int *rp, *ci, *map;
  const double *val, *vec;
  int rows, lg;
  double *out;
  int blocks() const { return pert_blocks(rows, lg); }
};
static int pert_products(ScsHipWork *w, const double *dA, const double *dP, PertProduct (&out)[3]) {
  DiffScratch &d = w->diff;
  const MatrixSet::ValueMaps &vm = w->mats->vmaps;
  int cnt = 0;
  if (dA) {
    out[cnt++] = PertProduct{w->At.rowptr.p, w->At.col.p, nullptr, dA, w->soly.p, w->At.rows, pert_lg((long)w->At.nnz, w->At.rows), d.tAt.p};
    out[cnt++] = PertProduct{w->Ar.rowptr.p, w->Ar.col.p, vm.ar.p, dA, w->solx.p, w->Ar.rows, pert_lg((long)w->Ar.nnz, w->Ar.rows), d.tA.p};
  }
  if (dP) out[cnt++] = PertProduct{w->Pf.rowptr.p, w->Pf.col.p, vm.pf.p, dP, w->solx.p, w->Pf.rows, pert_lg((long)w->Pf.nnz, w->Pf.rows), d.tP.p};
  return cnt;
}
// out_c = dc + dP x + dA' y, out_b = db + sgn dA x
static void pert_launch(ScsHipWork *w, const double *dA, const double *dP, const double *dc, const double *db, double sgn, double *out_c,
                        double *out_b, hipStream_t s) {
  DiffScratch &d = w->diff;
  PertProduct pr[3];
  const int cnt = pert_products(w, dA, dP, pr);
  for (int k = 0; k < cnt; ++k)
    if (pr[k].blocks() > 0)
      hipLaunchKernelGGL(k_pert_rows, dim3(pr[k].blocks()), dim3(kPertThreads), 0, s, pr[k].rp, pr[k].ci, pr[k].map, pr[k].val, pr[k].vec, pr[k].rows,
                         pr[k].lg, pr[k].out);
  hipLaunchKernelGGL(k_pert_eff, dim3(vec_blocks((long)w->n + w->m)), dim3(kVecThreads), 0, s, dc, db, dP ? (const double *)d.tP.p : nullptr,
                     dA ? (const double *)d.tAt.p : nullptr, dA ? (const double *)d.tA.p : nullptr, sgn, w->n, w->m, out_c, out_b);
}
