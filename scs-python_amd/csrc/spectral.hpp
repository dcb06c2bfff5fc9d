// spectral.hpp — projections onto the spectral cones: log-det (d), nuclear norm (nuc), ell1, sum of the k largest
// eigenvalues (sl).  Plays the role of SCS's spectral-cone projections (built with use_spectral_cones, R:meson.build:204-217;
// absent).  Slice layouts (DESIGN.md "Spectral cones"):
//   d      (t, v, svec X),  X of order n:   cl{ v > 0, X > 0, t <= v log det(X / v) }
//   nuc    (t, vec X),      X m x n, column-major:  { t >= ||X||_* }
//   ell1   (t, x),          x of length n:  { t >= ||x||_1 }
//   sl     (t, svec X),     X of order n:   { t >= sum of the k largest eigenvalues of X }
// svec is the PSD cone's layout (psd.hpp): lower triangle by column, off-diagonal entries times sqrt(2).
//
// None of these cones is self-dual: the ADMM loop needs Pi_{K*}(w) = w + Pi_K(-w) (Moreau, as cones.hpp does for exp / pow).
// Every kernel takes `dual`, loads sg * w with sg = -1 for the dual, projects onto K and stores (dual ? w + p : p).
//
// Mapping to the machine: ONE launch per cone kind, the grid is the set of cones.
//   ell1      — one wavefront per cone of length <= kSpecEll1WaveMax (four per 256-lane workgroup), one 1024-lane workgroup
//               per longer cone: two launches at most
//   sl, d     — one workgroup per matrix (order <= 64): S and V in LDS, parallel-order cyclic Jacobi (the round-robin schedule
//               rr_pair and the rotation jacobi_rot of psd.hpp) to a fixed tight tolerance, a one-wave projection of the eigenvalue
//               vector, then X+ = V diag(mu) V'
//   nuc       — one workgroup per matrix (min(m, n) <= 64, m n <= 8192): one-sided (Hestenes) Jacobi on the columns of X, or of X'
//               when m < n, in LDS; (t, sigma) through the ell1 routine; X+ = X V diag(sigma+ / sigma) V'
// Every reduction is a fixed shuffle butterfly or a fixed-order block sum: a solve is bit-identical from run to run.
#pragma once
#include "common.hpp"
#include "psd.hpp"

namespace scship {

constexpr int kSpecThreads = 256;
constexpr int kSpecMaxOrder = 64;      // sl, d: order; nuc: min(m, n)
constexpr int kSpecNucMaxElems = 8192; // nuc: m n
constexpr int kSpecLd = kSpecMaxOrder + 1;
constexpr int kSpecMaxSweeps = 40;
constexpr double kSpecOffTol2 = 1e-26;  // two-sided sweeps stop at ||offdiag||_F^2 <= this * ||X||_F^2
constexpr double kSpecOrthTol2 = 1e-28; // one-sided: a column pair is left alone when (y_p'y_q)^2 <= this * |y_p|^2 |y_q|^2

// per-kind metadata: slice offset and up to two sizes (ell1: n | sl: n, k | d: n | nuc: m, n)
struct SpecBatch {
  const int *off;
  const int *a;
  const int *b;
  int count;
};

// LDS of the workgroup kernels (dynamic; the largest member of the launch decides)
inline size_t spec_eig_lds_bytes(int max_order) { return sizeof(double) * 2 * kSpecLd * (size_t)((max_order + 1) & ~1); }
inline size_t spec_nuc_lds_bytes(int max_elems, int max_c) { return sizeof(double) * ((size_t)max_elems + (size_t)kSpecLd * max_c); }

// xor butterflies: every lane of the wave ends with the same bits (IEEE addition is commutative), so the scalar logic below runs
// uniformly on all lanes without a broadcast
__device__ __forceinline__ double spec_wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ __forceinline__ double spec_wmax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ double spec_wmin(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ int spec_wsumi(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// ------------------------------------------------------------------ ell1
// Soft threshold lam of the projection of (t, a) onto {t >= ||a||_1}: a+ = sign(a) max(|a| - lam, 0), t+ = t + lam.
// lam = 0 inside, lam = -t (>= max |a|: everything goes to 0) in the polar cone.  Otherwise the active-set fixed point
// lam <- (sum_{|a_i| > lam} |a_i| - t) / (#{|a_i| > lam} + 1), started from the whole set: lam grows monotonically to the root of
// the piecewise-linear sum max(|a_i| - lam, 0) - t - lam and the set shrinks in every pass but the last (at most n + 1 passes).
template <class Acc>
__device__ double spec_ell1_lambda(Acc a, int n, double t, int lane) {
  double s1 = 0., mx = 0.;
  for (int i = lane; i < n; i += kWave) {
    const double v = fabs(a(i));
    s1 += v;
    mx = fmax(mx, v);
  }
  s1 = spec_wsum(s1);
  mx = spec_wmax(mx);
  if (s1 <= t) return 0.;
  if (mx <= -t) return -t;
  double lam = (s1 - t) / (n + 1);
  int cnt = n;
  for (int it = 0; it <= n; ++it) {
    double sa = 0.;
    int c = 0;
    for (int i = lane; i < n; i += kWave) {
      const double v = fabs(a(i));
      if (v > lam) { sa += v; ++c; }
    }
    sa = spec_wsum(sa);
    c = spec_wsumi(c);
    lam = (sa - t) / (c + 1);
    if (c == cnt) break;
    cnt = c;
  }
  return lam;
}

// Every kernel below is a __device__ body d_X(..., blk) that takes its workgroup index from the caller, plus the one-problem
// kernel k_X that passes blockIdx.x; the grouped solve (batch.hpp) calls the same bodies from its own launch.
__device__ __forceinline__ void d_proj_ell1(double *y, SpecBatch B, int dual, const int *stall, int blk) {
  SCS_STALL_GUARD(stall);
  const int lane = threadIdx.x & 63;
  const int c = blk * (kSpecThreads / kWave) + (threadIdx.x >> 6);
  if (c >= B.count) return;  // (no workgroup barrier below)
  double *x = y + B.off[c];
  const int n = B.a[c];
  const double sg = dual ? -1. : 1.;
  const double t = sg * x[0];
  const double lam = spec_ell1_lambda([&](int i) { return sg * x[1 + i]; }, n, t, lane);
  for (int i = lane; i < n; i += kWave) {
    const double v = sg * x[1 + i];
    const double p = copysign(fmax(fabs(v) - lam, 0.), v);
    x[1 + i] = dual ? x[1 + i] + p : p;
  }
  if (lane == 0) x[0] = dual ? x[0] + (t + lam) : t + lam;
}
__global__ __launch_bounds__(kSpecThreads) void k_proj_ell1(double *y, SpecBatch B, int dual, const int *stall) {
  d_proj_ell1(y, B, dual, stall, (int)blockIdx.x);
}

// Long ell1 cones (n > kSpecEll1WaveMax): one 1024-lane workgroup per cone, the same fixed point with fixed-order block sums.
constexpr int kSpecEll1WaveMax = 2048;
constexpr int kSpecEll1BlockThreads = 1024;
__device__ __forceinline__ void d_proj_ell1_block(double *y, SpecBatch B, int dual, const int *stall, int cidx) {
  SCS_STALL_GUARD(stall);
  constexpr int NT = kSpecEll1BlockThreads;
  __shared__ double sm[NT / kWave];
  __shared__ double bc[2];
  const int tid = threadIdx.x;
  double *x = y + B.off[cidx];
  const int n = B.a[cidx];
  const double sg = dual ? -1. : 1.;
  const double t = sg * x[0];
  double s1 = 0., mx = 0.;
  for (int i = tid; i < n; i += NT) {
    const double v = fabs(x[1 + i]);
    s1 += v;
    mx = fmax(mx, v);
  }
  s1 = block_sum<NT>(s1, sm);
  mx = block_max<NT>(mx, sm);
  if (tid == 0) { bc[0] = s1; bc[1] = mx; }
  __syncthreads();
  s1 = bc[0];
  mx = bc[1];
  __syncthreads();
  double lam;
  if (s1 <= t) {
    lam = 0.;
  } else if (mx <= -t) {
    lam = -t;
  } else {
    lam = (s1 - t) / (n + 1);
    double cnt = n;
    for (int it = 0; it <= n; ++it) {  // as spec_ell1_lambda: the active set shrinks in every pass but the last
      double sa = 0., c = 0.;
      for (int i = tid; i < n; i += NT) {
        const double v = fabs(x[1 + i]);
        if (v > lam) { sa += v; c += 1.; }
      }
      sa = block_sum<NT>(sa, sm);
      c = block_sum<NT>(c, sm);
      if (tid == 0) { bc[0] = (sa - t) / (c + 1.); bc[1] = c; }
      __syncthreads();
      lam = bc[0];
      const bool same = bc[1] == cnt;
      cnt = bc[1];
      __syncthreads();
      if (same) break;
    }
  }
  for (int i = tid; i < n; i += NT) {
    const double v = sg * x[1 + i];
    const double p = copysign(fmax(fabs(v) - lam, 0.), v);
    x[1 + i] = dual ? x[1 + i] + p : p;
  }
  if (tid == 0) x[0] = dual ? x[0] + (t + lam) : t + lam;
}
__global__ __launch_bounds__(kSpecEll1BlockThreads) void k_proj_ell1_block(double *y, SpecBatch B, int dual, const int *stall) {
  d_proj_ell1_block(y, B, dual, stall, (int)blockIdx.x);
}

// ------------------------------------------------------------ eigen-solve
// Parallel-order cyclic Jacobi on the symmetric N x N (N even) matrix S in LDS (leading dimension kSpecLd) by the whole
// workgroup: N - 1 rounds of N/2 disjoint rotations per sweep (psd.hpp rr_pair), each rotation from psd.hpp jacobi_rot.
// On return diag(S) holds the eigenvalues and V (LDS) the eigenvectors as columns.  cs / sn: N/2 doubles each; red: 8 doubles.
__device__ void spec_jacobi(double *S, double *V, int N, double *cs, double *sn, double *red) {
  const int tid = threadIdx.x, H = N / 2, ld = kSpecLd;
  for (int e = tid; e < N * N; e += kSpecThreads) {
    const int j = e / N, i = e - j * N;
    V[i + ld * j] = i == j ? 1. : 0.;
  }
  __syncthreads();
  for (int sweep = 0; sweep < kSpecMaxSweeps; ++sweep) {
    double off = 0., tot = 0.;
    for (int e = tid; e < N * N; e += kSpecThreads) {
      const int j = e / N, i = e - j * N;
      const double a = S[i + ld * j];
      tot += a * a;
      if (i != j) off += a * a;
    }
    off = block_sum<kSpecThreads>(off, red);
    tot = block_sum<kSpecThreads>(tot, red);
    if (tid == 0) red[4] = (off <= kSpecOffTol2 * tot || off == 0.) ? 1. : 0.;
    __syncthreads();
    const bool done = red[4] != 0.;
    __syncthreads();
    if (done) break;
    for (int r = 0; r < N - 1; ++r) {
      if (tid < H) {
        int p, q;
        rr_pair(r, tid, N, p, q);
        const double apq = S[p + ld * q];
        const bool rot = fabs(apq) > 1e-300;
        double c, s;
        jacobi_rot(S[p + ld * p], S[q + ld * q], rot ? apq : 1.0, c, s);
        cs[tid] = rot ? c : 1.;
        sn[tid] = rot ? s : 0.;
      }
      __syncthreads();
      // S <- J' S J: the 2x2 block rows{p,q} x cols{p2,q2} of pairs (k, k2) belongs to one task
      for (int e = tid; e < H * H; e += kSpecThreads) {
        const int k = e / H, k2 = e - k * H;
        int p, q, p2, q2;
        rr_pair(r, k, N, p, q);
        rr_pair(r, k2, N, p2, q2);
        const double c = cs[k], s = sn[k], c2 = cs[k2], s2 = sn[k2];
        const double a0 = S[p + ld * p2], a1 = S[p + ld * q2], a2 = S[q + ld * p2], a3 = S[q + ld * q2];
        const double t1 = c2 * a0 - s2 * a1, t2 = s2 * a0 + c2 * a1;
        const double t3 = c2 * a2 - s2 * a3, t4 = s2 * a2 + c2 * a3;
        S[p + ld * p2] = c * t1 - s * t3;
        S[p + ld * q2] = c * t2 - s * t4;
        S[q + ld * p2] = s * t1 + c * t3;
        S[q + ld * q2] = s * t2 + c * t4;
      }
      for (int e = tid; e < N * H; e += kSpecThreads) {  // V <- V J
        const int k = e / N, i = e - k * N;
        int p, q;
        rr_pair(r, k, N, p, q);
        const double c = cs[k], s = sn[k], vp = V[i + ld * p], vq = V[i + ld * q];
        V[i + ld * p] = c * vp - s * vq;
        V[i + ld * q] = s * vp + c * vq;
      }
      __syncthreads();
    }
  }
}

// -------------------------------------------------- sum of the k largest
// One wave; lane i < n holds lam_i.  (t, lam) onto {t >= sum of the k largest of lam}: mu_i = lam_i - clip(lam_i - c, 0, theta),
// t+ = t + theta.  With lam sorted (lam_1 >= ... >= lam_n) the solution has a top group 1..a (mu = lam - theta), a middle group
// a+1..b (mu = c) and an untouched rest; for each (a, b) the two conditions — the subgradient weights clip(lam - c, 0, theta) / theta
// sum to k, and the top-k sum of mu equals t + theta — are linear in (c, theta).  Every candidate (a = b = k, or a < k < b) is solved
// in closed form and the one that violates its ordering conditions least (first index on ties) wins: exact, no iteration.
// ls, ps: 65 doubles of LDS each (sorted values, prefix sums).  Returns theta; *cc = c.
__device__ double spec_sl_solve(double lam, int n, int k, double t, int lane, double *ls, double *ps, double *cc) {
  double v = lane < n ? lam : -INFINITY;
  for (int size = 2; size <= kWave; size <<= 1)  // bitonic sort, descending
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const double o = __shfl_xor(v, stride, kWave);
      const bool up = (lane & size) == 0 || size == kWave, lower = (lane & stride) == 0;
      v = (lower == up) ? fmax(v, o) : fmin(v, o);
    }
  double s = lane < n ? v : 0.;
  for (int o = 1; o < kWave; o <<= 1) {  // inclusive scan (fixed order per lane)
    const double u = __shfl_up(s, o, kWave);
    if (lane >= o) s += u;
  }
  ls[lane] = v;
  ps[lane + 1] = s;
  if (lane == 0) ps[0] = 0.;
  wave_sync();
  if (ps[k] <= t) { *cc = 0.; return 0.; }  // inside
  auto L = [&](int i) { return ls[i - 1]; };  // 1-based sorted value
  auto cand = [&](int idx, double &c, double &th) {
    double viol;
    if (idx == 0) {  // a = b = k: the top k move down by theta, nothing in between
      th = (ps[k] - t) / (k + 1);
      c = k < n ? L(k + 1) : -INFINITY;
      viol = fmax(0., -th);
      if (k < n) viol = fmax(viol, L(k + 1) - (L(k) - th));
      return viol;
    }
    const int j = idx - 1, a = j / (n - k), b = k + 1 + (j - a * (n - k));
    const double sab = ps[b] - ps[a], r2 = t - ps[a];
    const double d1 = b - a, d2 = k - a, det = -(d1 * (a + 1) + d2 * d2);
    c = (-(a + 1) * sab - d2 * r2) / det;
    th = (d1 * r2 - d2 * sab) / det;
    viol = fmax(0., -th);
    if (a >= 1) viol = fmax(viol, c + th - L(a));
    viol = fmax(viol, L(a + 1) - c - th);
    viol = fmax(viol, c - L(b));
    if (b < n) viol = fmax(viol, L(b + 1) - c);
    return viol;
  };
  const int total = 1 + k * (n - k);
  double best = INFINITY;
  int bi = total;
  for (int idx = lane; idx < total; idx += kWave) {
    double c, th;
    const double vi = cand(idx, c, th);
    if (vi < best) { best = vi; bi = idx; }  // (idx grows: the first minimum of this lane stays)
  }
  for (int o = 32; o > 0; o >>= 1) {  // (violation, index) lexicographic minimum, identical on every lane
    const double ob = __shfl_xor(best, o, kWave);
    const int oi = __shfl_xor(bi, o, kWave);
    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  double c, th;
  cand(bi, c, th);
  *cc = c;
  return th;
}

// ------------------------------------------------------------ log-det
// One wave; lane i < n holds x_i (an eigenvalue).  (t, v, x) onto K_log = cl{ v > 0, x > 0, t <= v sum log(x_i / v) }.
// KKT with multiplier rho >= 0:  t+ = t - rho,  x+_i = (x_i + sqrt(x_i^2 + 4 rho v+)) / 2,  v+ - v + rho (n - L) = 0,
// L = sum log(x+_i / v+), and t+ = v+ L.  For a fixed v+ > 0 the (t, x) part is a projection onto a convex slice: h(rho) =
// v+ L(rho) + rho - t is increasing and concave, its root is found by a Newton iteration safeguarded by a bracket.  The outer
// function G(v+) = v+ - v + rho(v+) (n - L) is the derivative of a strictly convex function of v+ (partial minimisation of the
// squared distance over (t+, x+)): bisection on it, from [0, hi], a bounded number of steps.  A root at v+ -> 0 is the face
// { v = 0, t <= 0, x >= 0 } of the closure; a root with everything -> 0 is the polar cone.  The input is scaled to max-norm 1
// (the cone is a cone: Pi(a w) = a Pi(w)).
struct SpecLogdetOut {
  double t, v, x;
};
__device__ SpecLogdetOut spec_logdet_solve(double x, int n, double t, double v, int lane) {
  const bool live = lane < n;
  const double scale = fmax(fmax(fabs(t), fabs(v)), spec_wmax(live ? fabs(x) : 0.));
  if (scale == 0.) return {0., 0., 0.};
  t /= scale;
  v /= scale;
  x /= scale;
  const double xmin = spec_wmin(live ? x : INFINITY);
  if (v > 0. && xmin > 0. && v * spec_wsum(live ? log(x / v) : 0.) >= t) return {t * scale, v * scale, x * scale};
  auto xp_of = [&](double rho, double vp) {
    const double q = sqrt(x * x + 4. * rho * vp);
    return x >= 0. ? 0.5 * (x + q) : 2. * rho * vp / (q - x);
  };
  // h(rho) and h'(rho) at v+ = vp
  auto h_of = [&](double rho, double vp, double &dh) {
    double lsum = 0., dsum = 0.;
    if (live) {
      const double q = sqrt(x * x + 4. * rho * vp);
      const double xp = x >= 0. ? 0.5 * (x + q) : 2. * rho * vp / (q - x);
      lsum = log(xp / vp);
      dsum = vp / (q * xp);
    }
    lsum = spec_wsum(lsum);
    dsum = spec_wsum(dsum);
    dh = 1. + vp * dsum;
    return vp * lsum + rho - t;
  };
  auto inner = [&](double vp) {
    double dh;
    if (xmin > 0. && h_of(0., vp, dh) >= 0.) return 0.;
    double lo = 0., hi = 1.;
    for (int i = 0; i < 200 && h_of(hi, vp, dh) <= 0.; ++i) { lo = hi; hi *= 2.; }
    double rho = hi;
    for (int it = 0; it < 100; ++it) {
      const double h = h_of(rho, vp, dh);
      if (h > 0.) hi = rho; else lo = rho;
      if (h == 0.) break;
      double rn = rho - h / dh;
      if (!(rn > lo && rn < hi)) rn = 0.5 * (lo + hi);
      const bool stop = fabs(rn - rho) <= 1e-16 * rho || hi - lo <= 1e-16 * hi;
      rho = rn;
      if (stop) break;
    }
    return rho;
  };
  auto G_of = [&](double vp) {
    const double rho = inner(vp);
    const double L = spec_wsum(live ? log(xp_of(rho, vp) / vp) : 0.);
    return vp - v + (rho > 0. ? rho * (n - L) : 0.);
  };
  // bracket [lo, hi] with G(lo) <= 0 < G(hi), then Illinois regula falsi (superlinear, keeps the bracket); while lo is still 0,
  // where G is not defined (the face v = 0), plain bisection
  double lo = 0., hi = fmax(v, 0.) + 1., glo = 0., ghi = G_of(hi);
  for (int i = 0; i < 200 && ghi <= 0.; ++i) { lo = hi; glo = ghi; hi *= 2.; ghi = G_of(hi); }
  double vp = 0.5 * (lo + hi);
  int kept = 0;  // +1: hi kept in the last step(s), -1: lo kept
  for (int it = 0; it < 100 && hi - lo > 1e-16 * hi; ++it) {
    double xn = lo > 0. ? (lo * ghi - hi * glo) / (ghi - glo) : 0.5 * (lo + hi);
    if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
    const double g = G_of(xn);
    const double step = fabs(xn - vp);
    vp = xn;
    if (g == 0.) break;
    if (g > 0.) {
      hi = xn; ghi = g;
      if (kept == -1) glo *= 0.5;
      kept = -1;
    } else {
      lo = xn; glo = g;
      if (kept == 1) ghi *= 0.5;
      kept = 1;
    }
    if (lo > 0. && step <= 1e-16 * xn) break;
  }
  const double rho = inner(vp);
  return {(t - rho) * scale, vp * scale, xp_of(rho, vp) * scale};
}

// kind 0: sl (header t; B.a = n, B.b = k), kind 1: d (header t, v; B.a = n).  One workgroup per matrix.
__device__ __forceinline__ void d_proj_eig_cone(double *y, SpecBatch B, int kind, int dual, const int *stall, int cidx) {
  SCS_STALL_GUARD(stall);
  extern __shared__ double spec_lds[];
  __shared__ double cs[kSpecMaxOrder / 2], sn[kSpecMaxOrder / 2], red[8], mu[kSpecMaxOrder], ls[kWave + 1], ps[kWave + 1], hd[2];
  const int tid = threadIdx.x, ld = kSpecLd;
  const int n = B.a[cidx], N = (n + 1) & ~1, hdr = kind == 1 ? 2 : 1;
  double *S = spec_lds, *V = spec_lds + (size_t)ld * N;
  double *x = y + B.off[cidx];
  const double sg = dual ? -1. : 1., isq2 = 0.70710678118654752440, sq2 = 1.41421356237309504880;
  for (int e = tid; e < N * N; e += kSpecThreads) {
    const int j = e / N, i = e - j * N;
    S[i + ld * j] = 0.;
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += kSpecThreads) {
    const int j = e / n, i = e - j * n;
    if (i < j) continue;
    const long base = (long)j * n - (long)j * (j - 1) / 2;
    double a = sg * x[hdr + base + (i - j)];
    if (i != j) a *= isq2;
    S[i + ld * j] = a;
    S[j + ld * i] = a;
  }
  __syncthreads();
  spec_jacobi(S, V, N, cs, sn, red);
  if (tid < kWave) {
    const double lam = tid < n ? S[tid + ld * tid] : 0.;
    const double t = sg * x[0];
    if (kind == 0) {
      double c;
      const double th = spec_sl_solve(lam, n, B.b[cidx], t, tid, ls, ps, &c);
      if (tid < n) mu[tid] = lam - fmin(fmax(lam - c, 0.), th);
      if (tid == 0) hd[0] = t + th;
    } else {
      const SpecLogdetOut o = spec_logdet_solve(lam, n, t, sg * x[1], tid);
      if (tid < n) mu[tid] = o.x;
      if (tid == 0) { hd[0] = o.t; hd[1] = o.v; }
    }
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += kSpecThreads) {  // X+ = V diag(mu) V', lower triangle
    const int j = e / n, i = e - j * n;
    if (i < j) continue;
    double acc = 0.;
    for (int kk = 0; kk < n; ++kk) acc += V[i + ld * kk] * mu[kk] * V[j + ld * kk];
    const long at = hdr + (long)j * n - (long)j * (j - 1) / 2 + (i - j);
    const double p = i == j ? acc : acc * sq2;
    x[at] = dual ? x[at] + p : p;
  }
  if (tid < hdr) x[tid] = dual ? x[tid] + hd[tid] : hd[tid];
}
__global__ __launch_bounds__(kSpecThreads) void k_proj_eig_cone(double *y, SpecBatch B, int kind, int dual, const int *stall) {
  d_proj_eig_cone(y, B, kind, dual, stall, (int)blockIdx.x);
}

// ------------------------------------------------------- nuclear norm
// One workgroup per matrix.  Y = X (m >= n) or X' (m < n): R x C, R >= C, column-major in LDS.  One-sided Jacobi: a round
// rotates N/2 disjoint column pairs (rr_pair on N = C rounded up to even; a pair with the padding index is skipped) by the
// rotation that diagonalises their 2x2 Gram matrix (jacobi_rot), V <- V J; sweeps until no pair needed a rotation.  Then
// sigma_j = |y_j|, U_j = y_j / sigma_j and X+ = Y diag(sigma+ / sigma) V' (transposed back when m < n).
__device__ __forceinline__ void d_proj_nuc(double *y, SpecBatch B, int dual, const int *stall, int cidx) {
  SCS_STALL_GUARD(stall);
  extern __shared__ double spec_lds[];
  __shared__ double cs[kSpecMaxOrder / 2], sn[kSpecMaxOrder / 2], ratio[kSpecMaxOrder], sig[kSpecMaxOrder], hd[1];
  __shared__ int rotated;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, ld = kSpecLd;
  const int m = B.a[cidx], n = B.b[cidx];
  const bool tr = m < n;
  const int R = tr ? n : m, C = tr ? m : n, N = (C + 1) & ~1, H = N / 2;
  double *Y = spec_lds, *V = spec_lds + (size_t)R * C;
  double *x = y + B.off[cidx];
  const double sg = dual ? -1. : 1.;
  for (int e = tid; e < R * C; e += kSpecThreads) {
    const int j = e / R, i = e - j * R;
    Y[e] = sg * x[1 + (tr ? j + (long)m * i : i + (long)m * j)];
  }
  for (int e = tid; e < C * C; e += kSpecThreads) {
    const int j = e / C, i = e - j * C;
    V[i + ld * j] = i == j ? 1. : 0.;
  }
  __syncthreads();
  for (int sweep = 0; sweep < kSpecMaxSweeps && C > 1; ++sweep) {
    if (tid == 0) rotated = 0;
    __syncthreads();
    for (int r = 0; r < N - 1; ++r) {
      for (int k = wid; k < H; k += kSpecThreads / kWave) {  // a wave per pair: Gram entries by butterflies
        int p, q;
        rr_pair(r, k, N, p, q);
        double al = 0., be = 0., ga = 0.;
        if (q < C)
          for (int i = lane; i < R; i += kWave) {
            const double yp = Y[i + R * p], yq = Y[i + R * q];
            al += yp * yp;
            be += yq * yq;
            ga += yp * yq;
          }
        al = spec_wsum(al);
        be = spec_wsum(be);
        ga = spec_wsum(ga);
        const bool rot = q < C && ga != 0. && ga * ga > kSpecOrthTol2 * al * be;
        double c = 1., s = 0.;
        if (rot) jacobi_rot(al, be, ga, c, s);
        if (lane == 0) {
          cs[k] = c;
          sn[k] = s;
          if (rot) rotated = 1;
        }
      }
      __syncthreads();
      for (int e = tid; e < H * R; e += kSpecThreads) {
        const int k = e / R, i = e - k * R;
        int p, q;
        rr_pair(r, k, N, p, q);
        if (q >= C) continue;
        const double c = cs[k], s = sn[k], yp = Y[i + R * p], yq = Y[i + R * q];
        Y[i + R * p] = c * yp - s * yq;
        Y[i + R * q] = s * yp + c * yq;
      }
      for (int e = tid; e < H * C; e += kSpecThreads) {
        const int k = e / C, i = e - k * C;
        int p, q;
        rr_pair(r, k, N, p, q);
        if (q >= C) continue;
        const double c = cs[k], s = sn[k], vp = V[i + ld * p], vq = V[i + ld * q];
        V[i + ld * p] = c * vp - s * vq;
        V[i + ld * q] = s * vp + c * vq;
      }
      __syncthreads();
    }
    const bool again = rotated != 0;
    __syncthreads();
    if (!again) break;
  }
  for (int j = wid; j < C; j += kSpecThreads / kWave) {
    double ss = 0.;
    for (int i = lane; i < R; i += kWave) ss += Y[i + R * j] * Y[i + R * j];
    ss = spec_wsum(ss);
    if (lane == 0) sig[j] = sqrt(ss);
  }
  __syncthreads();
  if (tid < kWave) {
    const double t = sg * x[0];
    const double lam = spec_ell1_lambda([&](int i) { return sig[i]; }, C, t, tid);
    if (tid < C) {
      const double sj = sig[tid];
      ratio[tid] = sj > 0. ? fmax(sj - lam, 0.) / sj : 0.;
    }
    if (tid == 0) hd[0] = t + lam;
  }
  __syncthreads();
  for (int e = tid; e < m * n; e += kSpecThreads) {
    const int j = e / m, i = e - j * m;
    const int yi = tr ? j : i, vi = tr ? i : j;
    double acc = 0.;
    for (int kk = 0; kk < C; ++kk) acc += Y[yi + R * kk] * ratio[kk] * V[vi + ld * kk];
    x[1 + e] = dual ? x[1 + e] + acc : acc;
  }
  if (tid == 0) x[0] = dual ? x[0] + hd[0] : hd[0];
}
__global__ __launch_bounds__(kSpecThreads) void k_proj_nuc(double *y, SpecBatch B, int dual, const int *stall) {
  d_proj_nuc(y, B, dual, stall, (int)blockIdx.x);
}

}  // namespace scship
