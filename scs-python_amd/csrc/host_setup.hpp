// host_setup.hpp — init-time (one-off, O(nnz)) host work: validation, cone
// bookkeeping, CSC->CSR, symmetric expansion of P and the O(m+n) b/c scaling
// (the matrix equilibration itself runs on the device: normalize_dev.hpp).
//
// Plays the role of scs_source/src/normalize.c + the matrix helpers of
// scs_source/linsys/scs_matrix.c (R:meson.build:192,200; absent).  Algorithm:
// SURVEY App. A.6 — 25 Ruiz (inf-norm) passes + 1 l2 pass on [P A'; A 0], row
// scalings constant inside every non-separable cone, clamped to [1e-4, 1e4];
// then b,c scaled by D,E and a scalar sigma.
//   A_hat = D A E,  P_hat = E P E,  b_hat = sigma D b,  c_hat = sigma E c
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#ifndef USE_SPECTRAL_CONES
#define USE_SPECTRAL_CONES
#endif
#ifndef SCS_HIP_BUILDING_LIBRARY
#define SCS_HIP_BUILDING_LIBRARY
#endif
#include "../../include/scs_hip.h"

namespace scship {

struct HostCsr {
  int rows = 0, cols = 0;
  std::vector<int> rowptr, col;
  std::vector<double> val;
};

// Deep copy of the cone (the glue frees its view right after scs_init, R:scs/scsobject.h:908)
struct HostCone {
  int z = 0, l = 0, bsize = 0, ep = 0, ed = 0;
  std::vector<double> bu, bl, p;
  std::vector<int> q, s, cs;
  // spectral cones (spectral.hpp), after p in the order d, nuc, ell1, sl
  std::vector<int> d, nuc_m, nuc_n, ell1, sl_n, sl_k;
  std::vector<int> boundaries;  // [z+l+bsize, q..., s(s+1)/2..., cs^2..., 3 x (ep+ed+psize), d..., nuc..., ell1..., sl...]
  int m = 0;
  int off_box = 0, off_q = 0, off_s = 0, off_cs = 0, off_ep = 0, off_ed = 0, off_p = 0;
  int off_d = 0, off_nuc = 0, off_ell1 = 0, off_sl = 0;
  bool has_spectral() const { return !d.empty() || !nuc_m.empty() || !ell1.empty() || !sl_n.empty(); }
};

// limits of the spectral kernels (spectral.hpp: everything of one matrix in the LDS of one workgroup); INTEGRATION.md "Limits"
constexpr int kSpectralMaxOrder = 64;       // d, sl: order; nuc: min(m, n)
constexpr int kSpectralNucMaxElems = 8192;  // nuc: m n

// the spectral fields of k (ABI: include/scs_types.h; entry points for consumers built without them pass a cone whose spectral
// fields are zero).  Returns "" or the reason the cone is refused.
inline std::string spectral_cone_error(const ScsCone *k) {
  if (k->dsize < 0 || k->nucsize < 0 || k->ell1_size < 0 || k->sl_size < 0) return "negative spectral cone count";
  if ((k->dsize && !k->d) || (k->nucsize && (!k->nuc_m || !k->nuc_n)) || (k->ell1_size && !k->ell1) ||
      (k->sl_size && (!k->sl_n || !k->sl_k)))
    return "spectral cone count without its array";
  for (int i = 0; i < k->dsize; ++i) {
    if (k->d[i] < 1) return "log-det cone d[" + std::to_string(i) + "] = " + std::to_string(k->d[i]) + ": order must be >= 1";
    if (k->d[i] > kSpectralMaxOrder)
      return "log-det cone d[" + std::to_string(i) + "] = " + std::to_string(k->d[i]) + " exceeds the supported order " +
             std::to_string(kSpectralMaxOrder);
  }
  for (int i = 0; i < k->nucsize; ++i) {
    const long a = k->nuc_m[i], b = k->nuc_n[i];
    const std::string nm = "nuclear-norm cone " + std::to_string(i) + " (" + std::to_string(a) + " x " + std::to_string(b) + ")";
    if (a < 1 || b < 1) return nm + ": sizes must be >= 1";
    if (std::min(a, b) > kSpectralMaxOrder) return nm + ": min(m, n) exceeds " + std::to_string(kSpectralMaxOrder);
    if (a * b > kSpectralNucMaxElems) return nm + ": m n exceeds " + std::to_string(kSpectralNucMaxElems);
  }
  for (int i = 0; i < k->ell1_size; ++i)
    if (k->ell1[i] < 1) return "ell1 cone " + std::to_string(i) + ": length must be >= 1";
  for (int i = 0; i < k->sl_size; ++i) {
    const int n = k->sl_n[i], kk = k->sl_k[i];
    const std::string nm = "sum-of-largest cone " + std::to_string(i) + " (n = " + std::to_string(n) + ", k = " + std::to_string(kk) + ")";
    if (n < 1) return nm + ": order must be >= 1";
    if (n > kSpectralMaxOrder) return nm + ": order exceeds the supported order " + std::to_string(kSpectralMaxOrder);
    if (kk < 1 || kk > n) return nm + ": k must satisfy 1 <= k <= n";
  }
  return "";
}

inline long sd_size(long s) { return s * (s + 1) / 2; }

inline bool build_cone(const ScsCone *k, HostCone &c, std::string *why = nullptr) {
  {
    const std::string e = spectral_cone_error(k);
    if (!e.empty()) {
      if (why) *why = e;
      return false;
    }
  }
  if (k->z < 0 || k->l < 0 || k->bsize < 0 || k->ep < 0 || k->ed < 0) return false;
  if (k->qsize < 0 || k->ssize < 0 || k->psize < 0 || k->cssize < 0) return false;
  c.z = k->z; c.l = k->l; c.bsize = k->bsize; c.ep = k->ep; c.ed = k->ed;
  if (k->bsize > 1) {
    c.bu.assign(k->bu, k->bu + k->bsize - 1);
    c.bl.assign(k->bl, k->bl + k->bsize - 1);
    for (int i = 0; i < k->bsize - 1; ++i)
      if (c.bl[i] > c.bu[i]) return false;
  }
  if (k->qsize) c.q.assign(k->q, k->q + k->qsize);
  if (k->ssize) c.s.assign(k->s, k->s + k->ssize);
  if (k->cssize) c.cs.assign(k->cs, k->cs + k->cssize);
  if (k->psize) c.p.assign(k->p, k->p + k->psize);
  for (int q : c.q) if (q < 0) return false;
  for (int s : c.s) if (s < 0 || s > 8192) return false;   // (psd.hpp kPsdMaxH: 16 * 512)
  for (int s : c.cs) if (s < 0 || s > 4096) return false;  // projected through its 2k x 2k real embedding
  for (double p : c.p) if (!(p >= -1 && p <= 1)) return false;
  long cnt = (long)c.z + c.l;
  c.off_box = (int)cnt; cnt += c.bsize;
  c.off_q = (int)cnt; for (int q : c.q) cnt += q;
  c.off_s = (int)cnt; for (int s : c.s) cnt += sd_size(s);
  c.off_cs = (int)cnt; for (int s : c.cs) cnt += (long)s * s;
  c.off_ep = (int)cnt; cnt += 3L * c.ep;
  c.off_ed = (int)cnt; cnt += 3L * c.ed;
  c.off_p = (int)cnt; cnt += 3L * (long)c.p.size();
  c.d.assign(k->d, k->d + k->dsize);
  c.nuc_m.assign(k->nuc_m, k->nuc_m + k->nucsize);
  c.nuc_n.assign(k->nuc_n, k->nuc_n + k->nucsize);
  c.ell1.assign(k->ell1, k->ell1 + k->ell1_size);
  c.sl_n.assign(k->sl_n, k->sl_n + k->sl_size);
  c.sl_k.assign(k->sl_k, k->sl_k + k->sl_size);
  c.off_d = (int)std::min(cnt, 2000000001L); for (int v : c.d) cnt += sd_size(v) + 2;
  c.off_nuc = (int)std::min(cnt, 2000000001L); for (size_t i = 0; i < c.nuc_m.size(); ++i) cnt += (long)c.nuc_m[i] * c.nuc_n[i] + 1;
  c.off_ell1 = (int)std::min(cnt, 2000000001L); for (int v : c.ell1) cnt += (long)v + 1;
  c.off_sl = (int)std::min(cnt, 2000000001L); for (int v : c.sl_n) cnt += sd_size(v) + 1;
  if (cnt > 2000000000L) return false;
  c.m = (int)cnt;
  c.boundaries.clear();
  c.boundaries.push_back(c.z + c.l + c.bsize);
  for (int q : c.q) c.boundaries.push_back(q);
  for (int s : c.s) c.boundaries.push_back((int)sd_size(s));
  for (int s : c.cs) c.boundaries.push_back(s * s);
  for (int i = 0; i < c.ep + c.ed + (int)c.p.size(); ++i) c.boundaries.push_back(3);
  // none of the spectral cones is invariant under per-row scaling: one boundary (one averaged row scale) per cone
  for (int v : c.d) c.boundaries.push_back((int)sd_size(v) + 2);
  for (size_t i = 0; i < c.nuc_m.size(); ++i) c.boundaries.push_back(c.nuc_m[i] * c.nuc_n[i] + 1);
  for (int v : c.ell1) c.boundaries.push_back(v + 1);
  for (int v : c.sl_n) c.boundaries.push_back((int)sd_size(v) + 1);
  return true;
}

inline bool validate_matrix(const ScsMatrix *A, int m, int n) {
  if (!A || !A->p || A->m != m || A->n != n) return false;
  if (A->p[0] != 0) return false;
  for (int j = 0; j < n; ++j) {
    if (A->p[j + 1] < A->p[j]) return false;
    for (int p = A->p[j]; p < A->p[j + 1]; ++p)
      if (A->i[p] < 0 || A->i[p] >= m) return false;
  }
  return true;
}

// CSC (m x n) -> CSR (m x n); stable counting sort keeps columns ascending inside a row
inline void csc_to_csr(int m, int n, const int *cp, const int *ri, const double *x, HostCsr &out) {
  const long nnz = cp[n];
  out.rows = m; out.cols = n;
  out.rowptr.assign(m + 1, 0);
  out.col.resize(nnz);
  out.val.resize(nnz);
  for (long p = 0; p < nnz; ++p) out.rowptr[ri[p] + 1]++;
  for (int i = 0; i < m; ++i) out.rowptr[i + 1] += out.rowptr[i];
  std::vector<int> next(out.rowptr.begin(), out.rowptr.end() - 1);
  for (int j = 0; j < n; ++j)
    for (int p = cp[j]; p < cp[j + 1]; ++p) {
      const int q = next[ri[p]]++;
      out.col[q] = j;
      out.val[q] = x[p];
    }
}

// upper-triangular CSC P -> full symmetric CSR (n x n), plus its diagonal
inline void sym_expand(int n, const int *cp, const int *ri, const double *x, HostCsr &out, std::vector<double> &diag) {
  out.rows = out.cols = n;
  out.rowptr.assign(n + 1, 0);
  diag.assign(n, 0.0);
  for (int j = 0; j < n; ++j)
    for (int p = cp[j]; p < cp[j + 1]; ++p) {
      const int i = ri[p];
      if (i > j) continue;
      out.rowptr[i + 1]++;
      if (i != j) out.rowptr[j + 1]++;
      else diag[j] += x[p];
    }
  for (int i = 0; i < n; ++i) out.rowptr[i + 1] += out.rowptr[i];
  out.col.resize(out.rowptr[n]);
  out.val.resize(out.rowptr[n]);
  std::vector<int> next(out.rowptr.begin(), out.rowptr.end() - 1);
  // two ordered passes keep every row's columns ascending: first the transposed
  // (strictly-lower) entries (col = i < row = j), then the upper entries (col = j >= row = i)
  for (int j = 0; j < n; ++j)  // lower part of row j: entries (i,j) with i<j, visited with i ascending
    for (int p = cp[j]; p < cp[j + 1]; ++p) {
      const int i = ri[p];
      if (i < j) { const int q = next[j]++; out.col[q] = i; out.val[q] = x[p]; }
    }
  for (int j = 0; j < n; ++j)  // upper part: row i gets column j, j ascending
    for (int p = cp[j]; p < cp[j + 1]; ++p) {
      const int i = ri[p];
      if (i <= j) { const int q = next[i]++; out.col[q] = j; out.val[q] = x[p]; }
    }
}

struct HostScaling {
  std::vector<double> D, E;
  double sigma = 1.0;
};

inline double apply_limit(double x) {
  x = x < 1e-4 ? 1.0 : x;
  return x > 1e4 ? 1e4 : x;
}
inline double safediv_pos(double x, double y) { return y < 1e-18 ? x / 1e-18 : x / y; }

inline void normalize_b_c(HostScaling &sc, double *b, int m, double *c, int n) {
  double nb = 0., nc = 0.;
  for (int i = 0; i < n; ++i) { c[i] *= sc.E[i]; nc = std::max(nc, std::fabs(c[i])); }
  for (int i = 0; i < m; ++i) { b[i] *= sc.D[i]; nb = std::max(nb, std::fabs(b[i])); }
  double sigma = std::max(nc, nb);
  sigma = sigma < 1e-4 ? 1.0 : sigma;
  sigma = sigma > 1e4 ? 1e4 : sigma;
  sigma = safediv_pos(1.0, sigma);
  for (int i = 0; i < n; ++i) c[i] *= sigma;
  for (int i = 0; i < m; ++i) b[i] *= sigma;
  sc.sigma = sigma;
}

}  // namespace scship
