// grad_shared.hpp — the matrix gradients of K members that share one matrix, SUMMED over the members (include/scs_hip.h:
// scs_hip_adjoint_shared[_device], scs_hip_grad_matrix_sum).
//
// With X, Y the members' solutions and DB, DC the db, dc of their adjoints (diff.hpp d_grad_a / d_grad_p per member):
//     dA_sum[p] = sum_k ( Y[k,i] DC[k,j] - DB[k,i] X[k,j] )                      p = stored entry (i, j), the caller's CSC order
//     dP_sum[q] = sum_k ( DC[k,c] X[k,r] + DC[k,r] X[k,c] )  (c < r),   sum_k DC[k,r] X[k,r]  (c == r)      the caller's triangle
// a sampled dense-dense product over the stored pattern: nnz outputs instead of the K x nnz stack of K calls, one walk of the pattern.
//
// The members' vectors lie wherever each workspace keeps them, so they are first packed into PANELS with the member index fastest,
// Xt[j * ks + k] (Xt, DCt: n rows; Yt, DBt: m rows), a chunk of at most kGradSumKc members at a time: 2 (n + m) ks doubles whatever K
// is, from the block pool for the call.  Should that exceed kGradSumPanelMax the chunk is lowered to fit (grad_sum_chunk).  d_pack_panels
// is a transpose through a 64 x 64 LDS tile (padded to 65: the column reads fall on distinct banks in each half wave): rows are read
// along the members' vectors and written along k, both as whole 512-byte runs.
//
// Mapping of the sums: LANES ACROSS k.  One wave owns a column j of A (a row r of the full P): lane l holds members l, l + 64, ... of the
// chunk, reads the column's two K-vectors once into registers and then walks the column's stored entries; per entry the two K-vectors
// of row i are two contiguous runs of the panel — a K-vector of 64 doubles is four 128-byte lines, read whole by one load of the wave —
// so the gathers the pattern makes random move full lines, which a lane per entry with a k loop would not (64 lanes on 64 different
// rows: 64 lines per load for 8 useful bytes each).  No LDS is needed for it, so occupancy is the register file's.  The lanes' partial
// sums are folded by wave_sum, a fixed butterfly; a lane adds its own members in ascending order first, and a later chunk adds its sum
// to what the earlier chunks left in the output.  The order of every sum therefore depends on K and the chunk size only — not on the
// grid, not on timing; there is no floating-point atomic, and two calls give the same bits.  A column is one wave's work however long
// it is: the longest column bounds the kernel, which the patterns here (tens of entries per column) do not feel.
#pragma once

namespace scship {

constexpr int kGradSumKc = 256;                            // members per chunk (a multiple of the wave: kGradSumKc / 64 slices per lane)
constexpr size_t kGradSumPanelMax = (size_t)256 << 20;     // bytes of panels at once (as kDiffPsdBorrowMax)
constexpr int kGradSumSlices = kGradSumKc / kWave;
constexpr int kPackTile = 64;

// one vector kind to pack: tab[k] = member k's vector of `rows` doubles; nullptr tab = not needed by this call
struct PackSrc {
  const double *const *tab;
  double *panel;
  int rows;
};
struct PackSrc4 {
  PackSrc v[4];  // X, DC (n rows); Y, DB (m rows)
};

// panel[r * ks + k] = tab[k0 + k][r] for k < kc, 0 for kc <= k < min(ks, kc rounded up to the wave): what the sums read.
// blockIdx.y = the vector kind, blockIdx.x strides over tiles of 64 rows.
__device__ __forceinline__ void d_pack_panels(PackSrc4 src, int k0, int kc, int ks) {
  __shared__ double tile[kPackTile][kPackTile + 1];
  const PackSrc v = src.v[blockIdx.y];
  if (!v.tab) return;
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  constexpr int kWaves = kVecThreads / 64;
  const int kfill = min(ks, (kc + 63) & ~63);
  for (long r0 = (long)blockIdx.x * kPackTile; r0 < v.rows; r0 += (long)gridDim.x * kPackTile) {
    for (int kb = 0; kb < kfill; kb += kPackTile) {
      for (int kk = wv; kk < kPackTile; kk += kWaves) {  // member kb + kk: one run of 64 rows (the table entry is wave-uniform)
        const int k = kb + kk;
        const long r = r0 + lane;
        tile[kk][lane] = (k < kc && r < v.rows) ? v.tab[k0 + k][r] : 0.;
      }
      __syncthreads();
      for (int rr = wv; rr < kPackTile; rr += kWaves) {  // row r0 + rr: one run of 64 members
        const long r = r0 + rr;
        const int k = kb + lane;
        if (r < v.rows && k < kfill) v.panel[(size_t)r * ks + k] = tile[lane][rr];
      }
      __syncthreads();
    }
  }
}
__global__ __launch_bounds__(kVecThreads) void k_pack_panels(PackSrc4 src, int k0, int kc, int ks) { d_pack_panels(src, k0, kc, ks); }

// lane l's members of a chunk's K-vector at `row`: l, l + 64, ... below kc (the panel is zero from kc to the end of kc's slice)
__device__ __forceinline__ void grad_sum_load(const double *__restrict__ panel, long row, int kc, int ks, int lane, double (&v)[kGradSumSlices]) {
#pragma unroll
  for (int u = 0; u < kGradSumSlices; ++u) {
    const int k = u * kWave + lane;
    v[u] = (u * kWave < kc && k < ks) ? panel[(size_t)row * ks + k] : 0.;
  }
}

// dA (+)= the chunk's sum, over the caller's CSC order = the CSR of A' (rp, ci: cols rows).  add: a later chunk.
__device__ __forceinline__ void d_grad_a_sum(const int *__restrict__ rp, const int *__restrict__ ci, int cols, int kc, int ks,
                                             const double *__restrict__ Xt, const double *__restrict__ Yt,
                                             const double *__restrict__ DCt, const double *__restrict__ DBt, int add, double *dA) {
  const int lane = (int)threadIdx.x & 63;
  constexpr int kWaves = kVecThreads / 64;
  for (long j = (long)blockIdx.x * kWaves + ((int)threadIdx.x >> 6); j < cols; j += (long)gridDim.x * kWaves) {
    const int lo = rp[j], hi = rp[j + 1];
    if (lo >= hi) continue;
    double xj[kGradSumSlices], cj[kGradSumSlices];
    grad_sum_load(Xt, j, kc, ks, lane, xj);
    grad_sum_load(DCt, j, kc, ks, lane, cj);
    for (int p = lo; p < hi; ++p) {
      const long i = ci[p];
      double y[kGradSumSlices], b[kGradSumSlices];
      grad_sum_load(Yt, i, kc, ks, lane, y);
      grad_sum_load(DBt, i, kc, ks, lane, b);
      double t = 0.;
#pragma unroll
      for (int u = 0; u < kGradSumSlices; ++u) t += y[u] * cj[u] - b[u] * xj[u];  // (as d_grad_a)
      t = wave_sum(t);
      if (lane == 0) dA[p] = add ? dA[p] + t : t;
    }
  }
}
__global__ __launch_bounds__(kVecThreads) void k_grad_a_sum(const int *__restrict__ rp, const int *__restrict__ ci, int cols, int kc, int ks,
                                                            const double *__restrict__ Xt, const double *__restrict__ Yt,
                                                            const double *__restrict__ DCt, const double *__restrict__ DBt, int add,
                                                            double *dA) {
  d_grad_a_sum(rp, ci, cols, kc, ks, Xt, Yt, DCt, DBt, add, dA);
}

// dP (+)= the chunk's sum, over the caller's triangle: the entries of row r of the full matrix (rp, ci) on or below the diagonal are
// column r of the triangle, in order (as d_grad_p); up = the triangle's column pointers (diff_build_tri)
__device__ __forceinline__ void d_grad_p_sum(const int *__restrict__ rp, const int *__restrict__ ci, int n, const int *__restrict__ up,
                                             int kc, int ks, const double *__restrict__ Xt, const double *__restrict__ DCt, int add,
                                             double *dP) {
  const int lane = (int)threadIdx.x & 63;
  constexpr int kWaves = kVecThreads / 64;
  for (long r = (long)blockIdx.x * kWaves + ((int)threadIdx.x >> 6); r < n; r += (long)gridDim.x * kWaves) {
    const int lo = rp[r], hi = rp[r + 1], cnt = up[r + 1] - up[r];
    if (lo >= hi || cnt <= 0) continue;
    double xr[kGradSumSlices], cr[kGradSumSlices];
    grad_sum_load(Xt, r, kc, ks, lane, xr);
    grad_sum_load(DCt, r, kc, ks, lane, cr);
    for (int q = lo; q < hi; ++q) {
      const int c = ci[q], k = q - lo;
      if (c > r || k >= cnt) continue;
      double t = 0.;
      if (c < r) {
        double xc[kGradSumSlices], cc[kGradSumSlices];
        grad_sum_load(Xt, c, kc, ks, lane, xc);
        grad_sum_load(DCt, c, kc, ks, lane, cc);
#pragma unroll
        for (int u = 0; u < kGradSumSlices; ++u) t += cc[u] * xr[u] + cr[u] * xc[u];
      } else {
#pragma unroll
        for (int u = 0; u < kGradSumSlices; ++u) t += cr[u] * xr[u];
      }
      t = wave_sum(t);
      if (lane == 0) dP[up[r] + k] = add ? dP[up[r] + k] + t : t;
    }
  }
}
__global__ __launch_bounds__(kVecThreads) void k_grad_p_sum(const int *__restrict__ rp, const int *__restrict__ ci, int n,
                                                            const int *__restrict__ up, int kc, int ks, const double *__restrict__ Xt,
                                                            const double *__restrict__ DCt, int add, double *dP) {
  d_grad_p_sum(rp, ci, n, up, kc, ks, Xt, DCt, add, dP);
}

// members per chunk: kGradSumKc, lowered (to whole waves while one fits) until the panels of `doubles_per_member` rows fit the cap
inline int grad_sum_chunk(size_t doubles_per_member, int K) {
  const size_t fit = kGradSumPanelMax / (sizeof(double) * std::max<size_t>(doubles_per_member, 1));
  int chunk = fit >= (size_t)kGradSumKc ? kGradSumKc : fit >= (size_t)kWave ? (int)(fit & ~(size_t)(kWave - 1)) : (int)std::max<size_t>(fit, 1);
  return std::max(1, std::min(chunk, K));
}

// The pattern the sums walk (device arrays) and what to write: dA of a_nnz entries and / or dP (nullptr: not wanted).  p_rp, p_ci: n rows
// whose entries on or below the diagonal are the triangle's columns (the resident full P, or the triangle's own CSC with p_up = p_rp).
struct GradSumJob {
  int n = 0, m = 0;
  const int *a_rp = nullptr, *a_ci = nullptr;
  long a_nnz = 0;
  const int *p_rp = nullptr, *p_ci = nullptr, *p_up = nullptr;
  long p_nnz = 0;  // entries of dP
  double *dA = nullptr, *dP = nullptr;
};

// X, DC (n doubles each), Y, DB (m): one DEVICE pointer per member, in member order.  Packs and sums chunk after chunk on `s`, waits
// for the stream and gives the panels back to the block pool.  An output without an entry launches nothing.
static void grad_sum_run(const GradSumJob &job, const std::vector<const double *> &X, const std::vector<const double *> &Y,
                         const std::vector<const double *> &DB, const std::vector<const double *> &DC, hipStream_t s) {
  const int K = (int)X.size(), n = job.n, m = job.m;
  const bool do_a = job.dA && job.a_nnz > 0 && n > 0, do_p = job.dP && job.p_nnz > 0 && n > 0;
  if (K <= 0 || (!do_a && !do_p)) return;
  ArenaScope no_arena(nullptr);
  const size_t per_member = 2 * ((size_t)n + (do_a ? (size_t)m : 0));
  const int ks = grad_sum_chunk(per_member, K);
  std::vector<const double *> tabs_h;
  tabs_h.reserve((size_t)4 * K);
  for (const std::vector<const double *> *v : {&X, &DC, &Y, &DB}) tabs_h.insert(tabs_h.end(), v->begin(), v->end());
  DevBuf<const double *> tabs;
  DevBuf<double> panels;
  tabs.upload(tabs_h.data(), tabs_h.size(), s);
  panels.alloc(per_member * (size_t)ks);
  double *Xt = panels.p, *DCt = Xt + (size_t)n * ks, *Yt = DCt + (size_t)n * ks, *DBt = Yt + (size_t)m * ks;
  PackSrc4 src;
  src.v[0] = PackSrc{tabs.p, Xt, n};
  src.v[1] = PackSrc{tabs.p + K, DCt, n};
  src.v[2] = PackSrc{do_a ? tabs.p + 2 * (size_t)K : nullptr, do_a ? Yt : nullptr, m};
  src.v[3] = PackSrc{do_a ? tabs.p + 3 * (size_t)K : nullptr, do_a ? DBt : nullptr, m};
  constexpr int kWaves = kVecThreads / 64;
  const unsigned max_grid = 1u << 16;
  const unsigned g_pack = std::min<unsigned>(max_grid, (unsigned)ceil_div(std::max(n, do_a ? m : 0), kPackTile));
  const unsigned g_sum = std::min<unsigned>(max_grid, (unsigned)ceil_div(n, kWaves));
  for (int k0 = 0; k0 < K; k0 += ks) {
    const int kc = std::min(ks, K - k0), add = k0 > 0 ? 1 : 0;
    hipLaunchKernelGGL(k_pack_panels, dim3(g_pack, do_a ? 4 : 2), dim3(kVecThreads), 0, s, src, k0, kc, ks);
    if (do_a)
      hipLaunchKernelGGL(k_grad_a_sum, dim3(g_sum), dim3(kVecThreads), 0, s, job.a_rp, job.a_ci, n, kc, ks, (const double *)Xt, (const double *)Yt,
                         (const double *)DCt, (const double *)DBt, add, job.dA);
    if (do_p)
      hipLaunchKernelGGL(k_grad_p_sum, dim3(g_sum), dim3(kVecThreads), 0, s, job.p_rp, job.p_ci, n, job.p_up, kc, ks, (const double *)Xt,
                         (const double *)DCt, add, job.dP);
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(s));  // the stream is drained: the panels are the pool's again
  ++t_pool_release;
  panels.release();
  tabs.release();
  --t_pool_release;
}

}  // namespace scship
