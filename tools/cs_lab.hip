// cs_lab.hip — time and timeline of the column-sorted pass SpMV (spmv_cs.hpp) at the bench workload's shape.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o gpurun_out/cs_lab tools/cs_lab.hip && ./gpurun_out/cs_lab [m] [n] [nnz_per_col]
// LAB_BASE=1: for the K1 (CSR(A)) and K2 (CSR(A'), split layout) shapes the shipped kernel's time, its result check and a per-phase cycle
// breakdown per wave (the kernel's own CS_TL_* s_memtime stamps): prologue, wait-for-gathers + product scatter (+ the stream loads issued
// before the barrier), barrier wait, braid of gathers and LDS row sums, epilogue.  Then the in-kernel combine of split layouts
// (LAB_SKIP_COMBINE=1: not).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include <hip/hip_runtime.h>
#define CS_LAB_TIMELINE 1
__device__ unsigned long long cs_lab_tl[256 * 16 * 8];
#include "../scs-python_amd/csrc/spmv.hpp"
#include "../scs-python_amd/csrc/spmv_cs.hpp"

using namespace scship;
namespace scship { void set_last_error(const std::string &) {} }

struct Csr { int rows = 0, cols = 0; std::vector<int> rowptr, col; std::vector<double> val; };
static void transpose(const Csr &A, Csr &T) {
  T.rows = A.cols; T.cols = A.rows;
  T.rowptr.assign(T.rows + 1, 0);
  const int nnz = A.rowptr[A.rows];
  for (int p = 0; p < nnz; ++p) T.rowptr[A.col[p] + 1]++;
  for (int r = 0; r < T.rows; ++r) T.rowptr[r + 1] += T.rowptr[r];
  T.col.resize(nnz); T.val.resize(nnz);
  std::vector<int> cur(T.rowptr.begin(), T.rowptr.end() - 1);
  for (int r = 0; r < A.rows; ++r)
    for (int p = A.rowptr[r]; p < A.rowptr[r + 1]; ++p) { const int q = cur[A.col[p]]++; T.col[q] = r; T.val[q] = A.val[p]; }
}
template <class T> static T *to_dev(const std::vector<T> &h) {
  T *d; HIP_CHECK(hipMalloc(&d, std::max<size_t>(h.size(), 1) * sizeof(T)));
  HIP_CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
template <class F> static double time_us(F f, int reps) {
  for (int i = 0; i < 3; ++i) f();
  hipEvent_t a, b; HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b));
  HIP_CHECK(hipEventRecord(a, 0));
  for (int i = 0; i < reps; ++i) f();
  HIP_CHECK(hipEventRecord(b, 0)); HIP_CHECK(hipEventSynchronize(b));
  float ms; HIP_CHECK(hipEventElapsedTime(&ms, a, b));
  return ms * 1e3 / reps;
}
static long mismatches(const double *dy, const std::vector<double> &ref) {
  std::vector<double> h(ref.size());
  HIP_CHECK(hipMemcpy(h.data(), dy, ref.size() * 8, hipMemcpyDeviceToHost));
  long bad = 0;
  for (size_t i = 0; i < ref.size(); ++i) bad += std::memcmp(&h[i], &ref[i], 8) != 0;
  return bad;
}

struct EpiRaw2 {
  double *y0, *y1;
  static constexpr int kSums = 0, kMaxs = 0;
  __device__ void operator()(int r, double s, double *, double *) const { y0[r] = s; }
  __device__ void split(int r, double s, int part, double *, double *) const { (part ? y1 : y0)[r] = s; }
};

struct DevCs {
  int *passptr; int2 *pinfo; unsigned *idx; double *val; unsigned long long *meta; CsView v; HostCs hc;
  double *scratch = nullptr; unsigned *ticket = nullptr;
  bool build(const Csr &M, int rpt, int split, bool combine = false) {
    if (!build_cs(M.rowptr.data(), M.col.data(), M.val.data(), M.rows, M.cols, hc, rpt, split)) return false;
    passptr = to_dev(hc.passptr); pinfo = to_dev(hc.pinfo); idx = to_dev(hc.idx); val = to_dev(hc.val); meta = to_dev(hc.meta);
    v = CsView{passptr, pinfo, idx, val, meta, hc.rows, hc.cols, hc.nchunks, hc.R, hc.npass, hc.rpt, hc.split};
    if (combine && split > 1) {
      HIP_CHECK(hipMalloc(&scratch, (size_t)hc.nchunks * split * kCsThreads * hc.rpt * 8));
      HIP_CHECK(hipMalloc(&ticket, (size_t)hc.nchunks * 4));
      HIP_CHECK(hipMemset(ticket, 0, (size_t)hc.nchunks * 4));
      v.scratch = scratch; v.ticket = ticket;
    }
    return true;
  }
  void free() { hipFree(passptr); hipFree(pinfo); hipFree(idx); hipFree(val); hipFree(meta); }
};

static void bench_matrix(const char *name, const Csr &M, int split) {
  std::printf("%s: %d x %d, nnz %d, split %d\n", name, M.rows, M.cols, M.rowptr[M.rows], split);
  std::vector<double> x(M.cols), ref(M.rows);
  std::mt19937_64 g(7);
  std::normal_distribution<double> nd;
  for (auto &v : x) v = nd(g);
  for (int r = 0; r < M.rows; ++r) {
    double s = 0.;
    for (int p = M.rowptr[r]; p < M.rowptr[r + 1]; ++p) s += M.val[p] * x[M.col[p]];
    ref[r] = s;
  }
  double *dx = to_dev(x), *dy, *dy1;
  HIP_CHECK(hipMalloc(&dy, M.rows * sizeof(double)));
  HIP_CHECK(hipMalloc(&dy1, M.rows * sizeof(double)));
  DevCs D;
  if (!D.build(M, 0, split)) { std::printf("  build failed\n"); return; }
  std::printf("  R=%d rpt=%d wgs=%d passes=%d\n", D.hc.R, D.hc.rpt, D.hc.nchunks * D.hc.split, D.hc.npass);
  auto launch = [&] { launch_spmv_cs(D.v, dx, EpiRaw2{dy, dy1}, nullptr, 0, nullptr); };
  {
    HIP_CHECK(hipMemset(dy, 0xff, ref.size() * 8));
    std::printf("  k_spmv_cs_il: %.1f us", time_us(launch, 20));
    if (split == 1) std::printf("  mismatches %ld", mismatches(dy, ref));
    else {
      std::vector<double> h0(ref.size()), h1(ref.size());
      HIP_CHECK(hipMemcpy(h0.data(), dy, ref.size() * 8, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(h1.data(), dy1, ref.size() * 8, hipMemcpyDeviceToHost));
      double err = 0, scl = 0;
      for (size_t i = 0; i < ref.size(); ++i) { err = std::max(err, std::fabs(h0[i] + h1[i] - ref[i])); scl = std::max(scl, std::fabs(ref[i])); }
      std::printf("  max err %.2e (scale %.1f)", err, scl);
    }
    std::printf("\n");
  }
  {
    const int nwg = D.hc.nchunks * D.hc.split, nw = kCsThreads / 64;
    std::vector<unsigned long long> h((size_t)256 * 16 * 8);
    HIP_CHECK(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(cs_lab_tl), h.size() * 8));
    double avg[7] = {0}, mx[7] = {0};
    for (int w = 0; w < nwg * nw; ++w)
      for (int i = 0; i < 7; ++i) { avg[i] += (double)h[(size_t)w * 8 + i]; mx[i] = std::max(mx[i], (double)h[(size_t)w * 8 + i]); }
    const char *names[7] = {"prologue", "wait gathers+scatter(+pre-barrier issue)", "barrier", "braid", "epilogue", "-", "total"};
    std::printf("    timeline, kcycles per wave: ");
    for (int i = 0; i < 7; ++i) if (i != 5) std::printf("%s %.1f (max %.1f)  ", names[i], avg[i] / (nwg * nw) * 1e-3, mx[i] * 1e-3);
    std::printf("\n");
  }
  D.free();
  hipFree(dx); hipFree(dy); hipFree(dy1);
}

// in-kernel combine: correctness of EVERY row over many launches (stale partials of the previous launch sit in the L2s),
// with changing x so that a stale read cannot go unnoticed
static void bench_combine(const char *name, const Csr &M, int split) {
  DevCs D;
  if (!D.build(M, 0, split, true)) { std::printf("%s split %d: build failed\n", name, split); return; }
  std::printf("%s: combine mode split %d  R=%d rpt=%d wgs=%d passes=%d\n", name, split, D.hc.R, D.hc.rpt, D.hc.nchunks * split, D.hc.npass);
  std::mt19937_64 g(11);
  std::normal_distribution<double> nd;
  double *dy; HIP_CHECK(hipMalloc(&dy, M.rows * sizeof(double)));
  long bad_total = 0; double worst = 0;
  std::vector<double> x(M.cols), ref(M.rows), h(M.rows);
  double *dx; HIP_CHECK(hipMalloc(&dx, M.cols * 8));
  for (int rep = 0; rep < 6; ++rep) {
    for (auto &v : x) v = nd(g) * (rep + 1);
    HIP_CHECK(hipMemcpy(dx, x.data(), M.cols * 8, hipMemcpyHostToDevice));
    for (int r = 0; r < M.rows; ++r) { double s = 0.; for (int p = M.rowptr[r]; p < M.rowptr[r + 1]; ++p) s += M.val[p] * x[M.col[p]]; ref[r] = s; }
    HIP_CHECK(hipMemset(dy, 0xff, M.rows * 8));
    for (int k = 0; k < 3; ++k) launch_spmv_cs(D.v, dx, EpiStore{dy, 0}, nullptr, 0, nullptr);
    HIP_CHECK(hipMemcpy(h.data(), dy, M.rows * 8, hipMemcpyDeviceToHost));
    double scl = 0, err = 0;
    for (int r = 0; r < M.rows; ++r) { scl = std::max(scl, std::fabs(ref[r])); const double e = std::fabs(h[r] - ref[r]); if (!(e <= 1e300)) err = 1e300; else err = std::max(err, e); }
    long bad = 0;
    for (int r = 0; r < M.rows; ++r) bad += !(std::fabs(h[r] - ref[r]) <= 1e-12 * scl);
    bad_total += bad; worst = std::max(worst, err / scl);
  }
  auto launch = [&] { launch_spmv_cs(D.v, dx, EpiStore{dy, 0}, nullptr, 0, nullptr); };
  std::printf("  braided + in-kernel combine: %.1f us   rows off by > 1e-12: %ld   worst rel err %.2e\n", time_us(launch, 30), bad_total, worst);
  {
    const int nwg = D.hc.nchunks * D.hc.split, nw = kCsThreads / 64;
    std::vector<unsigned long long> hh((size_t)256 * 16 * 8);
    HIP_CHECK(hipMemcpyFromSymbol(hh.data(), HIP_SYMBOL(cs_lab_tl), hh.size() * 8));
    double avg[7] = {0}, mx[7] = {0};
    for (int w = 0; w < nwg * nw; ++w)
      for (int i = 0; i < 7; ++i) { avg[i] += (double)hh[(size_t)w * 8 + i]; mx[i] = std::max(mx[i], (double)hh[(size_t)w * 8 + i]); }
    const char *names[7] = {"prologue", "wait+scatter", "barrier", "braid", "combine+epilogue", "-", "total"};
    std::printf("    timeline, kcycles per wave: ");
    for (int i = 0; i < 7; ++i) if (i != 5) std::printf("%s %.1f (max %.1f)  ", names[i], avg[i] / (nwg * nw) * 1e-3, mx[i] * 1e-3);
    std::printf("\n");
  }
  {  // the same layout without the combine: partial outputs
    CsView v2 = D.v; v2.scratch = nullptr; v2.ticket = nullptr;
    double *dy1; HIP_CHECK(hipMalloc(&dy1, M.rows * 8));
    auto l2 = [&] { launch_spmv_cs(v2, dx, EpiRaw2{dy, dy1}, nullptr, 0, nullptr); };
    if (split == 2) std::printf("    same layout, partial outputs (no combine): %.1f us\n", time_us(l2, 30));
    hipFree(dy1);
  }
  D.free(); hipFree(dx); hipFree(dy);
}

int main(int argc, char **argv) {
  const int m = argc > 1 ? atoi(argv[1]) : 2000000, n = argc > 2 ? atoi(argv[2]) : 1000000;
  const int k = argc > 3 ? atoi(argv[3]) : 20;
  Csr At;
  At.rows = n; At.cols = m;
  At.rowptr.resize(n + 1);
  std::mt19937_64 g(5);
  std::normal_distribution<double> nd;
  std::vector<int> tmp(k);
  At.rowptr[0] = 0;
  for (int j = 0; j < n; ++j) {
    for (int i = 0; i < k; ++i) tmp[i] = (int)(g() % (unsigned long)m);
    std::sort(tmp.begin(), tmp.end());
    int last = -1;
    for (int i = 0; i < k; ++i)
      if (tmp[i] != last) { At.col.push_back(tmp[i]); At.val.push_back(nd(g)); last = tmp[i]; }
    At.rowptr[j + 1] = (int)At.col.size();
  }
  Csr Ar;
  transpose(At, Ar);
  if (getenv("LAB_BASE")) {
    bench_matrix("K1 shape  CSR(A)", Ar, 1);
    bench_matrix("K2 shape  CSR(A')", At, 2);
  }
  if (getenv("LAB_SKIP_COMBINE")) return 0;
  bench_combine("K1 shape  CSR(A)", Ar, 2);
  bench_combine("K2 shape  CSR(A')", At, 2);
  bench_combine("K2 shape  CSR(A')", At, 4);
  if (Ar.rows <= 1000000) bench_combine("K1 shape  CSR(A)", Ar, 4);
  return 0;
}
