// dproj_box_pow.hpp — W = D Pi_K(v) applied to a vector for the box cone and for the three-row cones (today: the power cones).
//
// Box cone K = {(t, w): t bl <= w <= t bu, t >= 0}, k = bsize - 1 bound rows, at v = (v0, w).  With t* the first entry of Pi_K(v),
//   U = {j: w_j > t* bu_j},  L = {j: w_j < t* bl_j},  F = the other rows,  a_j = bu_j on U, bl_j on L,  h = 1 + sum_{U,L} a_j^2:
//   u = (u0, r):   dt = (u0 + sum_{U,L} a_j r_j) / h  if t* > 0 else 0;   (W u)_0 = dt,   (W u)_j = a_j dt on U and L,   r_j on F.
// The sets are formed with the comparisons of d_proj_box (cones.hpp), so a row sits where the projection put it: an infinite bound is
// never active (t* inf = inf, 0 inf = NaN: both comparisons fail), a zero bound can be (its row's output is 0, not r_j) — which is
// why the apply recomputes the sets from (w_j, bl_j, bu_j, t*) and does not encode "free" in a coefficient.
// The preparation computes t* with the projection's own kernels on a scratch copy (never on the solve's S_BOX_T warm start), then h.
// An apply is ONE dot product and one pass over the rows: one workgroup up to kDboxMultiMin rows (as d_proj_box), above it two
// launches — per-workgroup partial sums, then every workgroup adds the partials in slot order and streams its rows.  All sums have a
// fixed order and there are no atomics: two calls on the same state return the same bits.
//
// Three-row cones: the preparation writes the six entries of the symmetric 3 x 3 block W per cone (I and 0 included), struct of
// arrays W[e * count + c], e = xx, xy, xz, yy, yz, zz; the apply d_dproj_sym3 is a 3 x 3 symmetric product per lane and knows no
// cone.  Power cone pow(a) = {(x, y, z): x^a y^(1-a) >= |z|, x, y >= 0}; entry a >= 0: W = W_pow(a)(v); a < 0: the cone is
// pow(|a|)* and W = I - W_pow(|a|)(-v) (Moreau).  W_pow(a)(v) = I inside the cone, 0 inside the polar cone (the two tests of
// proj_power_cone), else with p = (x, y, sz r) = Pi(v) on phi = x^a y^(1-a) - sz z = 0, sz = sign(v_z):
//   mu = |v_z| - r,   g = (a r / x, (1-a) r / y, -sz),   H_xx = a(a-1) r / x^2,  H_xy = a(1-a) r / (x y),  H_yy = -a(1-a) r / y^2,
//   M = (I - mu H)^{-1},   W = M - (M g)(M g)' / (g' M g).
// proj_power_cone stops its Newton iteration at |f| < 1e-9 and floors x, y at 1e-12: enough inside ADMM, not for a derivative.
// dpow_root carries r to double precision: Newton safeguarded by bisection on [0, |v_z|] until the step no longer changes r.
#pragma once

namespace scship {

// ------------------------------------------------------------------------------------------------ box cone
constexpr int kDboxMultiMin = kBoxMultiMin;  // bsize above this: the two-launch apply (and the multi-launch projection for t*)
enum : int { DB_T = 0, DB_STOP = 1, DB_H = 3, DB_STATE = 4 };  // st[]: t*, the stop flag of k_proj_box_round, h

// the row's set at t: its coefficient, and whether a bound is active (the comparisons of d_proj_box)
__device__ __forceinline__ bool dbox_active(double w, double l, double u, double t, double &a) {
  if (w > t * u) { a = u; return true; }
  if (w < t * l) { a = l; return true; }
  a = 0.;
  return false;
}

// one workgroup: t* by d_proj_box on the copy tmp of the box slice vb, then h
__device__ __forceinline__ void d_dbox_prep(const double *__restrict__ vb, const double *__restrict__ bl, const double *__restrict__ bu,
                                            int bsize, double *tmp, double *st) {
  __shared__ double sm[kBoxThreads / 64];
  for (int j = threadIdx.x; j < bsize; j += kBoxThreads) tmp[j] = vb[j];
  if (threadIdx.x == 0) st[DB_T] = 1.0;  // the cold start of a solve
  __syncthreads();
  d_proj_box(tmp, bl, bu, bsize, st + DB_T, 0, nullptr);
  __syncthreads();
  const double t = tmp[0];
  double hs = 0.;
  for (int j = threadIdx.x; j < bsize - 1; j += kBoxThreads) {
    double a;
    dbox_active(vb[1 + j], bl[j], bu[j], t, a);
    hs += a * a;
  }
  hs = block_sum<kBoxThreads>(hs, sm);
  if (threadIdx.x == 0) {
    st[DB_T] = t;
    st[DB_H] = 1.0 + hs;
  }
}
__global__ __launch_bounds__(kBoxThreads) void k_dbox_prep(const double *__restrict__ vb, const double *__restrict__ bl,
                                                           const double *__restrict__ bu, int bsize, double *tmp, double *st) {
  d_dbox_prep(vb, bl, bu, bsize, tmp, st);
}
// one workgroup: the apply (off = the box cone's first row in the m-vectors of io)
__device__ __forceinline__ void d_dbox(DprojIo io, const double *__restrict__ vb, const double *__restrict__ bl,
                                       const double *__restrict__ bu, int bsize, long off, const double *__restrict__ st, const int *done) {
  if (done && *done) return;
  __shared__ double sm[kBoxThreads / 64];
  __shared__ double bc;
  const double t = st[DB_T], h = st[DB_H];
  double d = 0.;
  for (int j = threadIdx.x; j < bsize - 1; j += kBoxThreads) {
    double a;
    if (dbox_active(vb[1 + j], bl[j], bu[j], t, a)) d += a * io.u(off + 1 + j);
  }
  d = block_sum<kBoxThreads>(d, sm);
  const double u0 = io.u(off);
  if (threadIdx.x == 0) bc = t > 0. ? (u0 + d) / h : 0.;
  __syncthreads();
  const double dt = bc;
  for (int j = threadIdx.x; j < bsize - 1; j += kBoxThreads) {
    double a;
    const double r = io.u(off + 1 + j);
    io.put(off + 1 + j, dbox_active(vb[1 + j], bl[j], bu[j], t, a) ? a * dt : r, r);
  }
  if (threadIdx.x == 0) io.put(off, dt, u0);
}
__global__ __launch_bounds__(kBoxThreads) void k_dbox(DprojIo io, const double *__restrict__ vb, const double *__restrict__ bl,
                                                      const double *__restrict__ bu, int bsize, long off, const double *__restrict__ st,
                                                      const int *done) {
  d_dbox(io, vb, bl, bu, bsize, off, st, done);
}

// ---- the multi-workgroup form (grids of box_multi_wgs(bsize) workgroups of kBoxMultiThreads; any row count: grid-stride) ----
__device__ __forceinline__ void d_dbox_init(double *st) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { st[DB_T] = 1.0; st[DB_STOP] = 0.; }
}
__global__ void k_dbox_init(double *st) { d_dbox_init(st); }
// parts[blockIdx.x] = this workgroup's share of sum a_j r_j (square != 0: of sum a_j^2, io is not read)
__device__ __forceinline__ void d_dbox_part(DprojIo io, const double *__restrict__ vb, const double *__restrict__ bl,
                                            const double *__restrict__ bu, int bsize, long off, const double *__restrict__ st, int square,
                                            double *parts, const int *done) {
  if (done && *done) return;
  __shared__ double sm[kBoxMultiThreads / 64];
  const double t = st[DB_T];
  double d = 0.;
  for (long j = (long)blockIdx.x * kBoxMultiThreads + threadIdx.x; j < bsize - 1; j += (long)gridDim.x * kBoxMultiThreads) {
    double a;
    if (dbox_active(vb[1 + j], bl[j], bu[j], t, a)) d += a * (square ? a : io.u(off + 1 + j));
  }
  d = block_sum<kBoxMultiThreads>(d, sm);
  if (threadIdx.x == 0) parts[blockIdx.x] = d;
}
__global__ __launch_bounds__(kBoxMultiThreads) void k_dbox_part(DprojIo io, const double *__restrict__ vb, const double *__restrict__ bl,
                                                                const double *__restrict__ bu, int bsize, long off,
                                                                const double *__restrict__ st, int square, double *parts, const int *done) {
  d_dbox_part(io, vb, bl, bu, bsize, off, st, square, parts, done);
}
// the partials in slot order (nparts <= kBoxMultiThreads: one per lane, then the fixed tree of block_sum); valid in thread 0
static_assert(kBoxMultiMaxWgs <= kBoxMultiThreads, "dbox_combine: one partial per lane");
__device__ __forceinline__ double dbox_combine(const double *__restrict__ parts, int nparts, double *sm) {
  return block_sum<kBoxMultiThreads>((int)threadIdx.x < nparts ? parts[threadIdx.x] : 0., sm);
}
__device__ __forceinline__ void d_dbox_hfin(const double *__restrict__ parts, int nparts, double *st) {
  __shared__ double sm[kBoxMultiThreads / 64];
  const double hs = dbox_combine(parts, nparts, sm);
  if (threadIdx.x == 0) st[DB_H] = 1.0 + hs;
}
__global__ __launch_bounds__(kBoxMultiThreads) void k_dbox_hfin(const double *__restrict__ parts, int nparts, double *st) {
  d_dbox_hfin(parts, nparts, st);
}
__device__ __forceinline__ void d_dbox_rows(DprojIo io, const double *__restrict__ vb, const double *__restrict__ bl,
                                            const double *__restrict__ bu, int bsize, long off, const double *__restrict__ st,
                                            const double *__restrict__ parts, int nparts, const int *done) {
  if (done && *done) return;
  __shared__ double sm[kBoxMultiThreads / 64];
  __shared__ double bc;
  const double t = st[DB_T], h = st[DB_H];
  const double d = dbox_combine(parts, nparts, sm);
  const double u0 = io.u(off);
  if (threadIdx.x == 0) bc = t > 0. ? (u0 + d) / h : 0.;
  __syncthreads();
  const double dt = bc;
  for (long j = (long)blockIdx.x * kBoxMultiThreads + threadIdx.x; j < bsize - 1; j += (long)gridDim.x * kBoxMultiThreads) {
    double a;
    const double r = io.u(off + 1 + j);
    io.put(off + 1 + j, dbox_active(vb[1 + j], bl[j], bu[j], t, a) ? a * dt : r, r);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) io.put(off, dt, u0);
}
__global__ __launch_bounds__(kBoxMultiThreads) void k_dbox_rows(DprojIo io, const double *__restrict__ vb, const double *__restrict__ bl,
                                                                const double *__restrict__ bu, int bsize, long off,
                                                                const double *__restrict__ st, const double *__restrict__ parts, int nparts,
                                                                const int *done) {
  d_dbox_rows(io, vb, bl, bu, bsize, off, st, parts, nparts, done);
}

// the box cone of a plan.  st: DB_STATE doubles; multi() adds 2 kBoxMultiMaxWgs slots for k_proj_box_round and kBoxMultiMaxWgs for
// the apply's partials (dbox_scratch_doubles), and the ticket.  tmp: bsize doubles nobody reads during the preparation.
struct DprojBoxPlan {
  int bsize = 0;
  long off = 0;
  const double *bl = nullptr, *bu = nullptr;
  double *st = nullptr, *tmp = nullptr;
  unsigned *ticket = nullptr;  // (zero between launches: k_proj_box_round leaves it so)
  bool multi() const { return bsize > kDboxMultiMin; }
  double *round_parts() const { return st + DB_STATE; }
  double *parts() const { return st + DB_STATE + 2 * kBoxMultiMaxWgs; }
};
inline size_t dbox_scratch_doubles(int bsize) { return bsize > kDboxMultiMin ? (size_t)DB_STATE + 3 * kBoxMultiMaxWgs : (size_t)DB_STATE; }

inline void launch_dbox_prep(const DprojBoxPlan &b, const double *vh, hipStream_t s) {
  if (b.bsize <= 0) return;
  const double *vb = vh + b.off;
  if (!b.multi()) {
    hipLaunchKernelGGL(k_dbox_prep, dim3(1), dim3(kBoxThreads), 0, s, vb, b.bl, b.bu, b.bsize, b.tmp, b.st);
    return;
  }
  const int wgs = box_multi_wgs(b.bsize);
  hipLaunchKernelGGL(k_dbox_init, dim3(1), dim3(64), 0, s, b.st);
  for (int round = 0; round < kBoxRounds; ++round)  // (reads vb only: no copy; t* is left in st[DB_T])
    hipLaunchKernelGGL(k_proj_box_round, dim3(wgs), dim3(kBoxMultiThreads), 0, s, vb, b.bl, b.bu, b.bsize, b.st, b.round_parts(), b.ticket, 0,
                       round, (const int *)nullptr);
  hipLaunchKernelGGL(k_dbox_part, dim3(wgs), dim3(kBoxMultiThreads), 0, s, DprojIo{nullptr, nullptr, nullptr, nullptr}, vb, b.bl, b.bu, b.bsize,
                     b.off, (const double *)b.st, 1, b.parts(), (const int *)nullptr);
  hipLaunchKernelGGL(k_dbox_hfin, dim3(1), dim3(kBoxMultiThreads), 0, s, (const double *)b.parts(), wgs, b.st);
}
inline void launch_dbox(const DprojBoxPlan &b, const double *vh, const DprojIo &io, const int *done, hipStream_t s) {
  if (b.bsize <= 0) return;
  const double *vb = vh + b.off;
  if (!b.multi()) {
    hipLaunchKernelGGL(k_dbox, dim3(1), dim3(kBoxThreads), 0, s, io, vb, b.bl, b.bu, b.bsize, b.off, (const double *)b.st, done);
    return;
  }
  const int wgs = box_multi_wgs(b.bsize);
  hipLaunchKernelGGL(k_dbox_part, dim3(wgs), dim3(kBoxMultiThreads), 0, s, io, vb, b.bl, b.bu, b.bsize, b.off, (const double *)b.st, 0, b.parts(),
                     done);
  hipLaunchKernelGGL(k_dbox_rows, dim3(wgs), dim3(kBoxMultiThreads), 0, s, io, vb, b.bl, b.bu, b.bsize, b.off, (const double *)b.st,
                     (const double *)b.parts(), wgs, done);
}

// ------------------------------------------------------------------------------------------------ three-row cones
// x(r) of proj_power_cone without its floor and without the cancellation at xh < 0: the positive root of x^2 - xh x - a (rh - r) r
__device__ __forceinline__ double dpow_x(double r, double xh, double rh, double a) {
  const double q = a * (rh - r) * r, d = sqrt(xh * xh + 4. * q);
  return xh >= 0. ? 0.5 * (xh + d) : 2. * q / (d - xh);
}
// the r of Pi_{pow(a)}(xh, yh, +-rh) for a point outside the cone and its polar: the root of f(r) = x(r)^a y(r)^(1-a) - r on [0, rh]
// (f(0) >= 0 > f(rh)).  Newton from rh / 2 as proj_power_cone, kept inside the bracket by bisection, until the step no longer moves r.
__device__ inline double dpow_root(double xh, double yh, double rh, double a, double &x, double &y) {
  double lo = 0., hi = rh, r = 0.5 * rh;
  for (int it = 0; it < 100; ++it) {
    x = dpow_x(r, xh, rh, a);
    y = dpow_x(r, yh, rh, 1. - a);
    const double xy = pow(x, a) * pow(y, 1. - a), f = xy - r;
    if (f > 0.) lo = r;
    else hi = r;
    const double dxdr = a * (rh - 2. * r) / (2. * x - xh), dydr = (1. - a) * (rh - 2. * r) / (2. * y - yh);
    const double fp = xy * (a * dxdr / x + (1. - a) * dydr / y) - 1.;
    double rn = r - f / fp;
    if (!(rn > lo && rn < hi)) rn = 0.5 * (lo + hi);
    if (rn == r || !(hi - lo > 0.)) break;
    r = rn;
  }
  x = dpow_x(r, xh, rh, a);
  y = dpow_x(r, yh, rh, 1. - a);
  return r;
}
// the six entries of W_pow(a)(v), 0 < a < 1
__device__ inline void dpow_W(const double *v, double a, double *W) {
  const double TOL = 1e-9;  // (the membership tests of proj_power_cone)
  const double xh = v[0], yh = v[1], rh = fabs(v[2]);
  const bool in = xh >= 0 && yh >= 0 && TOL + pow(xh, a) * pow(yh, 1 - a) >= rh;
  const bool polar = !in && xh <= 0 && yh <= 0 && TOL + pow(-xh, a) * pow(-yh, 1 - a) >= rh * pow(a, a) * pow(1 - a, 1 - a);
  W[1] = W[2] = W[4] = 0.;
  if (in || polar) {
    W[0] = W[3] = W[5] = in ? 1. : 0.;
    return;
  }
  if (rh == 0.) {  // a set of measure zero: the derivative of (max(x, 0), max(y, 0), 0)
    W[0] = xh > 0. ? 1. : 0.;
    W[3] = yh > 0. ? 1. : 0.;
    W[5] = 0.;
    return;
  }
  double x, y;
  const double r = dpow_root(xh, yh, rh, a, x, y);
  const double sz = v[2] < 0. ? -1. : 1., mu = rh - r;
  const double gx = a * r / x, gy = (1. - a) * r / y, gz = -sz;
  // I - mu H = [[1 + c / x^2, -c / (x y)], [-c / (x y), 1 + c / y^2]] (+) 1,  c = mu a (1 - a) r >= 0
  const double c = mu * a * (1. - a) * r, cxx = c / (x * x), cyy = c / (y * y), cxy = c / (x * y), det = 1. + cxx + cyy;
  const double mxx = (1. + cyy) / det, mxy = cxy / det, myy = (1. + cxx) / det;
  const double px = mxx * gx + mxy * gy, py = mxy * gx + myy * gy, pz = gz;  // M g
  const double den = gx * px + gy * py + 1.;
  W[0] = mxx - px * px / den;
  W[1] = mxy - px * py / den;
  W[2] = -px * pz / den;
  W[3] = myy - py * py / den;
  W[4] = -py * pz / den;
  W[5] = 1. - 1. / den;
}
// lane per cone: W of the power cones into W[e * ncones + c]  (vp = the fixed point's rows of the power cones)
__device__ __forceinline__ void d_dpow_prep(const double *__restrict__ vp, const double *__restrict__ a, int ncones, double *W) {
  const int c = blockIdx.x * kConeThreads + threadIdx.x;
  if (c >= ncones) return;
  const double ac = a[c];
  const double sg = ac >= 0. ? 1. : -1.;  // a < 0: I - W_pow(|a|)(-v)
  const double v[3] = {sg * vp[3L * c], sg * vp[3L * c + 1], sg * vp[3L * c + 2]};
  double w[6];
  dpow_W(v, fabs(ac), w);
  if (ac < 0.) {
    w[0] = 1. - w[0]; w[3] = 1. - w[3]; w[5] = 1. - w[5];
    w[1] = -w[1]; w[2] = -w[2]; w[4] = -w[4];
  }
#pragma unroll
  for (int e = 0; e < 6; ++e) W[(long)e * ncones + c] = w[e];
}
__global__ __launch_bounds__(kConeThreads) void k_dpow_prep(const double *__restrict__ vp, const double *__restrict__ a, int ncones, double *W) {
  d_dpow_prep(vp, a, ncones, W);
}
// lane per cone: the 3 x 3 symmetric product, rows off + 3 c .. off + 3 c + 2 of the m-vectors of io
__device__ __forceinline__ void d_dproj_sym3(DprojIo io, const double *__restrict__ W, int ncones, long off, const int *done) {
  if (done && *done) return;
  const int c = blockIdx.x * kConeThreads + threadIdx.x;
  if (c >= ncones) return;
  const long o = off + 3L * c;
  const double u0 = io.u(o), u1 = io.u(o + 1), u2 = io.u(o + 2);
  const double xx = W[c], xy = W[(long)ncones + c], xz = W[2L * ncones + c], yy = W[3L * ncones + c], yz = W[4L * ncones + c],
               zz = W[5L * ncones + c];
  io.put(o, xx * u0 + xy * u1 + xz * u2, u0);
  io.put(o + 1, xy * u0 + yy * u1 + yz * u2, u1);
  io.put(o + 2, xz * u0 + yz * u1 + zz * u2, u2);
}
__global__ __launch_bounds__(kConeThreads) void k_dproj_sym3(DprojIo io, const double *__restrict__ W, int ncones, long off, const int *done) {
  d_dproj_sym3(io, W, ncones, off, done);
}

// the three-row cones of a plan: count blocks from row off, W = 6 count doubles; a = the power cones' exponents (the preparation)
struct DprojSym3Plan {
  int count = 0;
  long off = 0;
  const double *a = nullptr;
  double *W = nullptr;
};
inline void launch_dsym3_prep(const DprojSym3Plan &p, const double *vh, hipStream_t s) {
  if (p.count <= 0) return;
  hipLaunchKernelGGL(k_dpow_prep, dim3(ceil_div(p.count, kConeThreads)), dim3(kConeThreads), 0, s, vh + p.off, p.a, p.count, p.W);
}
inline void launch_dsym3(const DprojSym3Plan &p, const DprojIo &io, const int *done, hipStream_t s) {
  if (p.count <= 0) return;
  hipLaunchKernelGGL(k_dproj_sym3, dim3(ceil_div(p.count, kConeThreads)), dim3(kConeThreads), 0, s, io, (const double *)p.W, p.count, p.off, done);
}

}  // namespace scship
