// dproj.hpp — W = D Pi_K(v), the derivative of the cone projection, applied to a vector: zero, nonnegative, box, second-order, real PSD
// and power cones.
//
// The adjoint and the forward derivative of a solve (lsqr.hpp, diff.hpp) need W u and (W - I) u at the fixed point v = s - y of the
// last solve.  W is symmetric and block diagonal by cone:
//   zero rows          W = 0
//   nonnegative rows   W_ii = 1 if v_i > 0 else 0
//   SOC, v = (t, z), r = |z|:   W = I if r <= t;   W = 0 if r <= -t;   else
//                      W = 1/(2r) [[r, z'], [z, (t + r) I - t z z'/r^2]]
//   PSD blocks         dproj_psd.hpp
//   box cone, power cones (a symmetric 3 x 3 block each)   dproj_box_pow.hpp
//
// Mapping to the machine follows the projections (cones.hpp): the off / dim tables, one lane group of soc_group() = 8/16/32/64 lanes per
// cone up to kSocBig entries, one workgroup per longer cone, q == 1 treated as a nonnegative row.  A preparation pass runs once per
// call: per cone its case, t and r (cinfo, three doubles per cone).  An apply then needs ONE dot product z'w per boundary cone; it is
// added by the butterfly of d_proj_soc_wave, so its bits do not depend on the group width.  One apply yields W u and (W - I) u.
#pragma once
#include "common.hpp"
#include "cones.hpp"
#include "vec.hpp"

namespace scship {

// ---- apply: u = a (+ b);  Wu = W u, WmIu = (W - I) u  (either output may be nullptr; outputs never alias inputs) ----
struct DprojIo {
  const double *a, *b;  // b nullable
  double *Wu, *WmIu;
  __device__ __forceinline__ double u(long i) const { return b ? a[i] + b[i] : a[i]; }
  __device__ __forceinline__ void put(long i, double wu, double ui) const {
    if (Wu) Wu[i] = wu;
    if (WmIu) WmIu[i] = wu - ui;
  }
};

}  // namespace scship

#include "dproj_psd.hpp"      // the PSD blocks (needs DprojIo)
#include "dproj_box_pow.hpp"  // the box cone and the three-row cones (needs DprojIo)

namespace scship {

enum : int { DP_INSIDE = 0, DP_POLAR = 1, DP_BOUNDARY = 2 };  // cinfo[3 c]: W = I, W = 0, the rank-structured block

// v_hat = sigma (D s - y / D) from the un-normalised solution (D == nullptr: s - y): the fixed point in the solver's coordinates
__device__ __forceinline__ void d_dproj_vhat(const double *__restrict__ s, const double *__restrict__ y,
                                             const double *__restrict__ D, double sigma, int m, double *vh) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < m; i += (long)gridDim.x * kVecThreads)
    vh[i] = D ? sigma * (D[i] * s[i] - y[i] / D[i]) : s[i] - y[i];
}
__global__ __launch_bounds__(kVecThreads) void k_dproj_vhat(const double *__restrict__ s, const double *__restrict__ y,
                                                            const double *__restrict__ D, double sigma, int m, double *vh) {
  d_dproj_vhat(s, y, D, sigma, m, vh);
}

// ---- preparation: case, t, r of every cone ----
__device__ __forceinline__ void d_dproj_prep_wave(const double *__restrict__ vh, const int *__restrict__ off,
                                                  const int *__restrict__ dim, int ncones, int G, double *cinfo) {
  const int lane = threadIdx.x & 63, gl = lane & (G - 1);
  const int wave = (int)blockIdx.x * (kConeThreads / 64) + (threadIdx.x >> 6);
  const int c = wave * (64 / G) + lane / G;
  const bool live = c < ncones;
  const int q = live ? dim[c] : 0;
  const double *v = vh + (live ? off[c] : 0);
  const bool small = q > 1 && q <= kSocBig;
  double ss = 0.;
  if (small)
    for (int i = 1 + gl; i < q; i += G) ss += v[i] * v[i];
  for (int o = G >> 1; o > 0; o >>= 1) ss += __shfl_xor(ss, o, kWave);  // every lane of the wave takes part
  if (!live || gl != 0) return;
  if (q == 1) {  // a nonnegative row
    cinfo[3 * c] = v[0] > 0. ? DP_INSIDE : DP_POLAR;
    cinfo[3 * c + 1] = v[0];
    cinfo[3 * c + 2] = 0.;
    return;
  }
  if (!small) return;
  const double r = sqrt(ss), t = v[0];
  cinfo[3 * c] = r <= t ? DP_INSIDE : r <= -t ? DP_POLAR : DP_BOUNDARY;
  cinfo[3 * c + 1] = t;
  cinfo[3 * c + 2] = r;
}
__global__ __launch_bounds__(kConeThreads) void k_dproj_prep_wave(const double *__restrict__ vh, const int *__restrict__ off,
                                                                  const int *__restrict__ dim, int ncones, int G, double *cinfo) {
  d_dproj_prep_wave(vh, off, dim, ncones, G, cinfo);
}
__device__ __forceinline__ void d_dproj_prep_block(const double *__restrict__ vh, const int *__restrict__ off,
                                                   const int *__restrict__ dim, const int *__restrict__ big, double *cinfo) {
  __shared__ double sm[kConeThreads / 64];
  const int c = big[blockIdx.x];
  const int q = dim[c];
  const double *v = vh + off[c];
  double ss = 0.;
  for (int i = 1 + threadIdx.x; i < q; i += kConeThreads) ss += v[i] * v[i];
  ss = block_sum<kConeThreads>(ss, sm);
  if (threadIdx.x != 0) return;
  const double r = sqrt(ss), t = v[0];
  cinfo[3 * c] = r <= t ? DP_INSIDE : r <= -t ? DP_POLAR : DP_BOUNDARY;
  cinfo[3 * c + 1] = t;
  cinfo[3 * c + 2] = r;
}
__global__ __launch_bounds__(kConeThreads) void k_dproj_prep_block(const double *__restrict__ vh, const int *__restrict__ off,
                                                                   const int *__restrict__ dim, const int *__restrict__ big, double *cinfo) {
  d_dproj_prep_block(vh, off, dim, big, cinfo);
}

// ---- apply (DprojIo above) ----
// the z zero rows and the l nonnegative rows
__device__ __forceinline__ void d_dproj_zl(DprojIo io, const double *__restrict__ vh, int z, int l, const int *done) {
  if (done && *done) return;
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)z + l; i += (long)gridDim.x * kVecThreads) {
    const double ui = io.u(i);
    io.put(i, (i >= z && vh[i] > 0.) ? ui : 0., ui);
  }
}
__global__ __launch_bounds__(kVecThreads) void k_dproj_zl(DprojIo io, const double *__restrict__ vh, int z, int l, const int *done) {
  d_dproj_zl(io, vh, z, l, done);
}
// the coefficients of a boundary block: W u = (top ; cz z + cw w) with u = (u0 ; w), d = z'w
__device__ __forceinline__ void dproj_coef(double t, double r, double u0, double d, double &top, double &cz, double &cw) {
  const double dr = d / r;
  top = 0.5 * (u0 + dr);
  cz = 0.5 * (u0 - t * dr / r) / r;
  cw = 0.5 * (1. + t / r);
}
__device__ __forceinline__ void d_dproj_soc_wave(DprojIo io, const double *__restrict__ vh, const double *__restrict__ cinfo,
                                                 const int *__restrict__ off, const int *__restrict__ dim, int ncones, int G,
                                                 const int *done) {
  if (done && *done) return;
  const int lane = threadIdx.x & 63, gl = lane & (G - 1);
  const int wave = (int)blockIdx.x * (kConeThreads / 64) + (threadIdx.x >> 6);
  const int c = wave * (64 / G) + lane / G;
  const bool live = c < ncones;
  const int q = live ? dim[c] : 0;
  const long o0 = live ? off[c] : 0;
  const bool mine = live && q >= 1 && q <= kSocBig;  // (longer cones: k_dproj_soc_block)
  const int kind = mine ? (int)cinfo[3 * c] : DP_INSIDE;
  const bool bnd = mine && q > 1 && kind == DP_BOUNDARY;
  double d = 0.;
  if (bnd)
    for (int i = 1 + gl; i < q; i += G) d += vh[o0 + i] * io.u(o0 + i);
  for (int o = G >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, kWave);  // every lane of the wave takes part
  if (!mine) return;
  if (!bnd) {
    for (int i = gl; i < q; i += G) {
      const double ui = io.u(o0 + i);
      io.put(o0 + i, kind == DP_INSIDE ? ui : 0., ui);
    }
    return;
  }
  const double u0 = io.u(o0);
  double top, cz, cw;
  dproj_coef(cinfo[3 * c + 1], cinfo[3 * c + 2], u0, d, top, cz, cw);
  for (int i = 1 + gl; i < q; i += G) {
    const double ui = io.u(o0 + i);
    io.put(o0 + i, cz * vh[o0 + i] + cw * ui, ui);
  }
  if (gl == 0) io.put(o0, top, u0);
}
__global__ __launch_bounds__(kConeThreads) void k_dproj_soc_wave(DprojIo io, const double *__restrict__ vh, const double *__restrict__ cinfo,
                                                                 const int *__restrict__ off, const int *__restrict__ dim, int ncones, int G,
                                                                 const int *done) {
  d_dproj_soc_wave(io, vh, cinfo, off, dim, ncones, G, done);
}
__device__ __forceinline__ void d_dproj_soc_block(DprojIo io, const double *__restrict__ vh, const double *__restrict__ cinfo,
                                                  const int *__restrict__ off, const int *__restrict__ dim,
                                                  const int *__restrict__ big, const int *done) {
  if (done && *done) return;
  __shared__ double sm[kConeThreads / 64];
  __shared__ double bc;
  const int c = big[blockIdx.x];
  const int q = dim[c];
  const long o0 = off[c];
  const int kind = (int)cinfo[3 * c];
  if (kind != DP_BOUNDARY) {  // (uniform over the workgroup)
    for (int i = threadIdx.x; i < q; i += kConeThreads) {
      const double ui = io.u(o0 + i);
      io.put(o0 + i, kind == DP_INSIDE ? ui : 0., ui);
    }
    return;
  }
  double d = 0.;
  for (int i = 1 + threadIdx.x; i < q; i += kConeThreads) d += vh[o0 + i] * io.u(o0 + i);
  d = block_sum<kConeThreads>(d, sm);
  if (threadIdx.x == 0) bc = d;
  __syncthreads();
  const double u0 = io.u(o0);
  double top, cz, cw;
  dproj_coef(cinfo[3 * c + 1], cinfo[3 * c + 2], u0, bc, top, cz, cw);
  for (int i = 1 + threadIdx.x; i < q; i += kConeThreads) {
    const double ui = io.u(o0 + i);
    io.put(o0 + i, cz * vh[o0 + i] + cw * ui, ui);
  }
  if (threadIdx.x == 0) io.put(o0, top, u0);
}
__global__ __launch_bounds__(kConeThreads) void k_dproj_soc_block(DprojIo io, const double *__restrict__ vh, const double *__restrict__ cinfo,
                                                                  const int *__restrict__ off, const int *__restrict__ dim,
                                                                  const int *__restrict__ big, const int *done) {
  d_dproj_soc_block(io, vh, cinfo, off, dim, big, done);
}

// the cone plan the launches below read: the tables of the projections (work.hpp soc_off / soc_dim / soc_big)
struct DprojPlan {
  int z = 0, l = 0, n_soc = 0, n_soc_big = 0, G = 64;
  const int *off = nullptr, *dim = nullptr, *big = nullptr;
  const double *vh = nullptr;  // the fixed point (m)
  double *cinfo = nullptr;     // 3 doubles per SOC
  long m = 0;                  // length of vh
  DprojPsdPlan psd;            // the PSD blocks (dproj_psd.hpp); count == 0: none
  DprojBoxPlan box;            // the box cone (dproj_box_pow.hpp); bsize == 0: none
  DprojSym3Plan sym3;          // the power cones (dproj_box_pow.hpp); count == 0: none
};
inline void launch_dproj_prep(const DprojPlan &p, hipStream_t s) {
  launch_dproj_psd_prep(p.psd, p.vh, p.m, s);
  launch_dbox_prep(p.box, p.vh, s);  // (after the PSD blocks: box.tmp may lie inside psd.tmp_m)
  launch_dsym3_prep(p.sym3, p.vh, s);
  if (p.n_soc <= 0) return;
  hipLaunchKernelGGL(k_dproj_prep_wave, dim3(soc_wave_blocks(p.n_soc, p.G)), dim3(kConeThreads), 0, s, p.vh, p.off, p.dim, p.n_soc, p.G, p.cinfo);
  if (p.n_soc_big > 0) hipLaunchKernelGGL(k_dproj_prep_block, dim3(p.n_soc_big), dim3(kConeThreads), 0, s, p.vh, p.off, p.dim, p.big, p.cinfo);
}
inline void launch_dproj(const DprojPlan &p, const DprojIo &io, const int *done, hipStream_t s) {
  if (p.z + p.l > 0) hipLaunchKernelGGL(k_dproj_zl, dim3(vec_blocks(p.z + p.l)), dim3(kVecThreads), 0, s, io, p.vh, p.z, p.l, done);
  launch_dproj_psd(p.psd, io, done, s);
  launch_dbox(p.box, p.vh, io, done, s);
  launch_dsym3(p.sym3, io, done, s);
  if (p.n_soc <= 0) return;
  hipLaunchKernelGGL(k_dproj_soc_wave, dim3(soc_wave_blocks(p.n_soc, p.G)), dim3(kConeThreads), 0, s, io, p.vh, (const double *)p.cinfo, p.off, p.dim,
                     p.n_soc, p.G, done);
  if (p.n_soc_big > 0)
    hipLaunchKernelGGL(k_dproj_soc_block, dim3(p.n_soc_big), dim3(kConeThreads), 0, s, io, p.vh, (const double *)p.cinfo, p.off, p.dim, p.big, done);
}

}  // namespace scship
