// matrix_update.hpp — scs_hip_update_matrix / scs_hip_update_matrix_device (include/scs_hip.h): new VALUES of A and P on the sparsity
// pattern scs_init was given, written into every resident form of the matrix set, re-equilibrated, and the workspace put back into
// the state scs_init leaves a new workspace in (setup.hpp start_state — the function scs_init itself ends in).
//
// The pattern is unchanged, so every layout decision of scs_init stands; what is needed is, for every stored value slot of every
// resident form, WHERE its value comes from.  Those value maps (work.hpp MatrixSet::ValueMaps; int32, -1 = padding slot) are built at
// the first call — a workspace that never updates its matrix allocates none of this:
//   A' (CSR)            the caller's CSC order itself: a copy
//   A  (CSR)            the transposition's permutation, re-derived from the two resident index arrays (k_map_transpose)
//   P  (full CSR)       two slots per off-diagonal entry of the stored triangle (host_setup.hpp sym_expand), re-derived from the
//                       resident index arrays of the full matrix (k_pf_lowcount, scan, k_map_pf)
//   pass layouts        the builder's partition, cut and slot sort re-run in map-only mode with the layout's own geometry
//                       (setup_cs_dev.hpp DeviceCs::build_value_map), peeled rows and virtual-row pieces included
//   slabs               the resident row offsets and segment pointers walked once more (setup_dev.hpp k_slab_fill_map)
// The layout maps index the equilibrated CSR the layout was built from, and each is CHECKED against the values the layout holds at
// that moment (k_map_check: slot k must hold source[map[k]] bit for bit, padding 0) before anything is overwritten.
//
// A call then is: gather raw values (one launch per matrix) -> device_normalize in place -> gather into the layouts -> diag(P)
// -> zero the iterate state -> start_state.  From the second call on every device block comes from the block pool.
#pragma once
#include <cstdint>

namespace scship {

typedef double vm_d2 __attribute__((ext_vector_type(2)));

// dst[i] = map[i] >= 0 ? src[map[i]] : 0 for i < n; copy_dst[i] = src[i] as well when copy_dst != nullptr (the form whose order IS the
// source's).  The first 4 * nquad elements go four at a time: one 16-byte load of the map, 16-byte stores (the host passes nquad = 0
// when a pointer is not 16-byte aligned).  NT: non-temporal stores — the layout copies are written once and next read by a product.
template <bool NT>
__global__ __launch_bounds__(kVecThreads) void k_vals_gather(double *__restrict__ dst, const int *__restrict__ map,
                                                             const double *__restrict__ src, long n, long nquad,
                                                             double *__restrict__ copy_dst) {
  const long stride = (long)gridDim.x * kVecThreads, t = (long)blockIdx.x * kVecThreads + threadIdx.x;
  for (long q = t; q < nquad; q += stride) {
    const int4 m = reinterpret_cast<const int4 *>(map)[q];
    vm_d2 a, b;
    a.x = m.x >= 0 ? src[m.x] : 0.0;
    a.y = m.y >= 0 ? src[m.y] : 0.0;
    b.x = m.z >= 0 ? src[m.z] : 0.0;
    b.y = m.w >= 0 ? src[m.w] : 0.0;
    vm_d2 *d = reinterpret_cast<vm_d2 *>(dst) + 2 * q;
    if (NT) {
      __builtin_nontemporal_store(a, d);
      __builtin_nontemporal_store(b, d + 1);
    } else {
      d[0] = a;
      d[1] = b;
    }
    if (copy_dst) {
      const vm_d2 *sv = reinterpret_cast<const vm_d2 *>(src) + 2 * q;
      vm_d2 *c = reinterpret_cast<vm_d2 *>(copy_dst) + 2 * q;
      c[0] = sv[0];
      c[1] = sv[1];
    }
  }
  for (long i = 4 * nquad + t; i < n; i += stride) {
    const int p = map[i];
    dst[i] = p >= 0 ? src[p] : 0.0;
    if (copy_dst) copy_dst[i] = src[i];
  }
}

// slot k of a layout must hold source[map[k]] bit for bit (0.0 in a padding slot): the map reproduces the builder's placement
__global__ __launch_bounds__(kVecThreads) void k_map_check(const double *__restrict__ held, const int *__restrict__ map,
                                                           const double *__restrict__ src, long n, long nsrc, int *bad) {
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < n; i += (long)gridDim.x * kVecThreads) {
    const int p = map[i];
    bool ok;
    if (p < 0) ok = held[i] == 0.0;
    else ok = p < nsrc && __double_as_longlong(held[i]) == __double_as_longlong(src[p]);
    if (!ok) atomicExch(bad, 1);
  }
}

// the row of a CSR position q: rowptr[r] <= q < rowptr[r + 1]
__device__ __forceinline__ int vm_row_of(const int *__restrict__ rowptr, int rows, long q) {
  int lo = 0, hi = rows;  // rowptr[lo] <= q < rowptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rowptr[mid] <= q) lo = mid; else hi = mid;
  }
  return lo;
}

// CSR(A) slot q = (row r, column j, the d-th stored entry of that pair) -> its position in CSC(A) = CSR(A'): row j of A', the d-th entry
// with column r.  (Both transpositions, device and host, order a row of A by (column, source position).)  Binary search where the
// row of A' is sorted, a scan where it is not; bad = 1 when there is no such entry.
__global__ __launch_bounds__(kVecThreads) void k_map_transpose(const int *__restrict__ rp, const int *__restrict__ ci, int rows, long nnz,
                                                               const int *__restrict__ trp, const int *__restrict__ tci, int *map, int *bad) {
  for (long q = (long)blockIdx.x * kVecThreads + threadIdx.x; q < nnz; q += (long)gridDim.x * kVecThreads) {
    const int r = vm_row_of(rp, rows, q), j = ci[q];
    int d = 0;
    while (q - d - 1 >= rp[r] && ci[q - d - 1] == j) ++d;
    const int a = trp[j], e = trp[j + 1];
    int lo = a, hi = e;  // first position with tci >= r
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tci[mid] < r) lo = mid + 1; else hi = mid;
    }
    int p = lo + d;
    if (!(p < e && tci[p] == r && (lo == a || tci[lo - 1] != r))) {
      p = -1;
      int k = 0;
      for (int t = a; t < e; ++t)
        if (tci[t] == r && k++ == d) { p = t; break; }
    }
    if (p < 0) atomicExch(bad, 1);
    map[q] = p;
  }
}

// entries of row r of the full symmetric P on or below the diagonal = the entries of column r of the stored (upper) triangle
__global__ __launch_bounds__(kVecThreads) void k_pf_lowcount(const int *__restrict__ rp, const int *__restrict__ ci, int n, int *cnt) {
  for (long r = (long)blockIdx.x * kVecThreads + threadIdx.x; r < n; r += (long)gridDim.x * kVecThreads) {
    int c = 0;
    for (int p = rp[r]; p < rp[r + 1]; ++p) c += ci[p] <= r ? 1 : 0;
    cnt[r] = c;
  }
}
// Full-P slot q = (row r, column c) -> position in the caller's triangle (CSC, columns ascending, up[] = its column pointers as the
// scan of k_pf_lowcount): on or below the diagonal it is entry (c, r) of column r — the k-th entry of row r is the k-th of that column
// (sym_expand fills the lower part of a row in column order) —, above it entry (r, c) of column c, found in row c of the full matrix.
// That pairing needs every column of the triangle in ascending row order (sym_expand writes the off-diagonal entries of a column in the
// caller's order and the diagonal behind them; the rows of the full matrix come out sorted whatever the caller's order was, so nothing
// on the device could tell): scs_init records it (work.hpp MatrixSet::p_update_refusal) and the entry refuses other P before it gets here.
__global__ __launch_bounds__(kVecThreads) void k_map_pf(const int *__restrict__ rp, const int *__restrict__ ci, int n, long nnz,
                                                        const int *__restrict__ up, int *map, int *bad) {
  for (long q = (long)blockIdx.x * kVecThreads + threadIdx.x; q < nnz; q += (long)gridDim.x * kVecThreads) {
    const int r = vm_row_of(rp, n, q), c = ci[q];
    int src = -1;
    if (c <= r) {
      const int k = (int)(q - rp[r]);
      if (k < up[r + 1] - up[r]) src = up[r] + k;
    } else {
      int d = 0;
      while (q - d - 1 >= rp[r] && ci[q - d - 1] == c) ++d;
      const int a = rp[c], e = rp[c + 1];
      int lo = a, hi = e;  // first position of row c with column >= r
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ci[mid] < r) lo = mid + 1; else hi = mid;
      }
      const int k = lo - a + d;
      if (lo + d < e && ci[lo + d] == r && k < up[c + 1] - up[c]) src = up[c] + k;
    }
    if (src < 0) atomicExch(bad, 1);
    map[q] = src;
  }
}

}  // namespace scship

// while alive, device blocks released on this thread go to the block pool (common.hpp DevPool): only where the stream is idle at every release
struct PoolReleaseScope {
  PoolReleaseScope() { ++t_pool_release; }
  ~PoolReleaseScope() { --t_pool_release; }
  PoolReleaseScope(const PoolReleaseScope &) = delete;
  PoolReleaseScope &operator=(const PoolReleaseScope &) = delete;
};

static void vm_gather(double *dst, const DevBuf<int> &map, const double *src, long n, double *copy_dst, bool nontemporal, hipStream_t s) {
  if (n <= 0) return;
  auto al16 = [](const void *p) { return ((uintptr_t)p & 15u) == 0; };
  const bool vec = al16(dst) && al16(map.p) && (!copy_dst || (al16(copy_dst) && al16(src)));
  const long nquad = vec ? n / 4 : 0;
  const dim3 grid(vec_blocks(n)), block(kVecThreads);
  if (nontemporal) hipLaunchKernelGGL(k_vals_gather<true>, grid, block, 0, s, dst, (const int *)map.p, src, n, nquad, copy_dst);
  else hipLaunchKernelGGL(k_vals_gather<false>, grid, block, 0, s, dst, (const int *)map.p, src, n, nquad, copy_dst);
}

// the layout copies of one matrix: M's pass layout was built from T (the other orientation's CSR; P: its own), its slab from its own CSR
struct VmLayout {
  DeviceCsr *M;
  const DeviceCsr *T;
  DevBuf<int> *cs_map, *slab_map;
};

// The value maps of the two CSR forms, in the caller's order: ar (CSR(A) slot -> position in the caller's CSC values) and pf (full
// CSR(P) slot -> position in the caller's triangle).  Each is built once per matrix set, by whichever comes first: the first
// scs_hip_update_matrix (both) or the first derivative that perturbs A or P (perturb.hpp: the one it needs).  The caller has selected
// the device and keeps the arena out of the way.  Throws — with the map released — when a map cannot be derived.
static void build_csr_value_maps(ScsHipWork *w, bool want_a, bool want_p, const char *who) {
  MatrixSet &ms = *w->mats;
  MatrixSet::ValueMaps &vm = ms.vmaps;
  std::lock_guard<std::mutex> lock(ms.maps_mu);  // (clones share the set)
  want_a = want_a && !vm.ar.p;
  want_p = want_p && !vm.pf.p;
  if (!want_a && !want_p) return;
  hipStream_t s = w->stream;
  DevBuf<int> bad;
  bad.alloc_zero(1, s);
  auto verdict = [&](const char *what) {
    int b = 0;
    HIP_CHECK(hipMemcpyAsync(&b, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (b) throw std::runtime_error(std::string(who) + ": the value map of " + what + " does not reproduce the resident layout");
  };
  DeviceCsr &At = ms.At, &Ar = ms.Ar, &Pf = ms.Pf;
  if (want_a) {
    try {
      if (At.nnz != ms.a_nnz_in || Ar.nnz != At.nnz) throw std::runtime_error(std::string(who) + ": the resident forms of A do not hold nnz(A) values");
      vm.ar.alloc((size_t)std::max(Ar.nnz, 1L));
      if (Ar.nnz > 0)
        hipLaunchKernelGGL(k_map_transpose, dim3(vec_blocks(Ar.nnz)), dim3(kVecThreads), 0, s, (const int *)Ar.rowptr.p, (const int *)Ar.col.p, Ar.rows,
                           (long)Ar.nnz, (const int *)At.rowptr.p, (const int *)At.col.p, vm.ar.p, bad.p);
      verdict("A (CSR)");
    } catch (...) {
      (void)hipStreamSynchronize(s);
      vm.ar.release();
      throw;
    }
  }
  if (want_p) {
    try {
      const int n = Pf.rows;
      DevBuf<int> cnt, up, tmp;
      cnt.alloc((size_t)n);
      up.alloc((size_t)n + 1);
      tmp.alloc_zero((size_t)(n / kScanTile + 4), s);
      hipLaunchKernelGGL(k_pf_lowcount, dim3(vec_blocks(n)), dim3(kVecThreads), 0, s, (const int *)Pf.rowptr.p, (const int *)Pf.col.p, n, cnt.p);
      device_exclusive_scan(cnt.p, up.p, n, tmp.p, s);
      int total = 0;
      HIP_CHECK(hipMemcpyAsync(&total, up.p + n, sizeof(int), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if ((long)total != ms.p_nnz_in)  // (cannot happen for a P the entry lets through: the host check of scs_init counted the same)
        throw std::runtime_error(std::string(who) + ": P was given with " + std::to_string(ms.p_nnz_in) + " entries of which " +
                                 std::to_string(total) + " lie in the upper triangle: its values cannot be updated in place");
      vm.pf.alloc((size_t)std::max(Pf.nnz, 1L));
      if (Pf.nnz > 0)
        hipLaunchKernelGGL(k_map_pf, dim3(vec_blocks(Pf.nnz)), dim3(kVecThreads), 0, s, (const int *)Pf.rowptr.p, (const int *)Pf.col.p, n, (long)Pf.nnz,
                           (const int *)up.p, vm.pf.p, bad.p);
      verdict("P (full CSR)");  // (synchronises: cnt / up / tmp are locals)
    } catch (...) {
      (void)hipStreamSynchronize(s);
      vm.pf.release();
      throw;
    }
  }
}

// The value maps of the set (first call).  Throws — with nothing of the matrices touched — when a map cannot be derived or does not
// reproduce what the layout holds.
static void build_value_maps(ScsHipWork *w) {
  MatrixSet &ms = *w->mats;
  MatrixSet::ValueMaps &vm = ms.vmaps;
  hipStream_t s = w->stream;
  DevBuf<int> bad;
  bad.alloc_zero(1, s);
  auto verdict = [&](const char *what) {
    int b = 0;
    HIP_CHECK(hipMemcpyAsync(&b, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (b) throw std::runtime_error(std::string("scs_hip_update_matrix: the value map of ") + what + " does not reproduce the resident layout");
  };
  try {
    DeviceCsr &At = ms.At, &Ar = ms.Ar, &Pf = ms.Pf;
    build_csr_value_maps(w, true, w->has_P, "scs_hip_update_matrix");  // (a derivative with dA / dP may have built them: kept)
    const VmLayout lay[3] = {{&At, &Ar, &vm.at_cs, &vm.at_slab}, {&Ar, &At, &vm.ar_cs, &vm.ar_slab}, {&Pf, &Pf, &vm.pf_cs, &vm.pf_slab}};
    for (int k = 0; k < (w->has_P ? 3 : 2); ++k) {
      DeviceCsr &M = *lay[k].M;
      const DeviceCsr &T = *lay[k].T;
      if (M.cs.ok) {
        if (!M.build_cs_value_map(T, s, *lay[k].cs_map, ms.opt))
          throw std::runtime_error("scs_hip_update_matrix: the pass layout could not be re-derived with the geometry scs_init chose");
        hipLaunchKernelGGL(k_map_check, dim3(vec_blocks((long)M.cs.val.n)), dim3(kVecThreads), 0, s, (const double *)M.cs.val.p,
                           (const int *)lay[k].cs_map->p, (const double *)T.val.p, (long)M.cs.val.n, (long)T.nnz, bad.p);
        verdict("a column-sorted pass layout");
      }
      if (M.has_slab) {
        M.build_slab_value_map(s, *lay[k].slab_map);
        hipLaunchKernelGGL(k_map_check, dim3(vec_blocks((long)M.s_val.n)), dim3(kVecThreads), 0, s, (const double *)M.s_val.p,
                           (const int *)lay[k].slab_map->p, (const double *)M.val.p, (long)M.s_val.n, (long)M.nnz, bad.p);
        verdict("an L2-blocked slab layout");
      }
    }
  } catch (...) {
    HIP_CHECK(hipStreamSynchronize(s));
    for (DevBuf<int> *b : {&vm.ar, &vm.pf, &vm.at_cs, &vm.ar_cs, &vm.pf_cs, &vm.at_slab, &vm.ar_slab, &vm.pf_slab}) b->release();
    throw;
  }
  vm.built = true;
  if (ms.opt.debug & DBG_SETUP)  // SCS_HIP_DEBUG=setup: what was mapped (the tests read the layout kinds off this line)
    std::fprintf(stderr, "[scs-hip] value maps: CSR(A) %zu, CSR(P) %zu; pass layouts A' %zu, A %zu, P %zu slots (peeled rows %d, %d, %d; pieces %d, %d, %d); "
                 "slabs A' %zu, A %zu, P %zu slots\n", vm.ar.n, vm.pf.n, vm.at_cs.n, vm.ar_cs.n, vm.pf_cs.n,
                 ms.At.cs_virt_lp > 0 ? 0 : ms.At.npeel, ms.Ar.cs_virt_lp > 0 ? 0 : ms.Ar.npeel, ms.Pf.cs_virt_lp > 0 ? 0 : ms.Pf.npeel,
                 ms.At.cs.ok ? ms.At.cs.npieces : 0, ms.Ar.cs.ok ? ms.Ar.cs.npieces : 0, ms.Pf.cs.ok ? ms.Pf.cs.npieces : 0,
                 vm.at_slab.n, vm.ar_slab.n, vm.pf_slab.n);
}

// what alloc_zero left in a new workspace, and the host-side per-workspace state of a workspace that has not solved yet
static void zero_state(ScsHipWork *w) {
  hipStream_t s = w->stream;
  auto zero = [&](void *p, size_t bytes) {
    if (p && bytes) HIP_CHECK(hipMemsetAsync(p, 0, bytes, s));
  };
  for (DevBuf<double> *b : {&w->v, &w->v_prev, &w->u, &w->ut, &w->rsk, &w->diag_r, &w->g, &w->h, &w->cg_b, &w->cg_p, &w->cg_r, &w->cg_Gp, &w->cg_M,
                            &w->ws, &w->tmp_m, &w->solx, &w->soly, &w->sols, &w->part, &w->part2, &w->part_v, &w->sc, &w->out, &w->px,
                            &w->psd_scratch, &w->cs_stage, &w->box_parts})
    zero(b->p, sizeof(double) * b->n);
  zero(w->fl.p, sizeof(int) * w->fl.n);
  zero(w->cg_ticket.p, sizeof(unsigned) * w->cg_ticket.n);
  zero(w->box_ticket.p, sizeof(unsigned) * w->box_ticket.n);
  w->scale = w->stgs.scale;
  w->setup_failed = false;
  w->diag_r_structured = false;
  w->sol_on_device = false;
  w->v_norm_fresh = false;
  w->last_cg_iters = 8;
  for (int &c : w->cg_hist) c = 8;
  w->cg_hist_pos = 0;
  w->r = Residuals{};
  w->cg_res_min = w->psd_res_min = 0;
  w->tot_cg_iters = 0;
  w->pipe_stalls = 0;
}

// Ax / Px: nnz(A) / nnz(P) values in the order of the CSC arrays scs_init was given (host pointers, or — dev — device pointers of the
// workspace's device), nullptr = keep.  The caller holds w->mtx and the scratch turn, has selected the device and refused bad arguments.
static void update_matrix_impl(ScsHipWork *w, const double *Ax, const double *Px, bool dev) {
  const double t0 = now_ms();
  MatrixSet &ms = *w->mats;
  MatrixSet::ValueMaps &vm = ms.vmaps;
  hipStream_t s = w->stream;
  HIP_CHECK(hipStreamSynchronize(s));
  ArenaScope no_arena(nullptr);  // (what this allocates outlives no arena chunk: exact-size blocks)
  // Temporaries come back from the pool next call.  The scope ends behind device_normalize: every release inside it — the locals of
  // build_value_maps, of the layout builders' map mode and of device_normalize — follows a stream synchronise of the function that owns
  // the block.  What start_state launches (the cold PCG, the G^-1 build of a workspace that does not defer them) releases as in scs_init.
  std::unique_ptr<PoolReleaseScope> pool(new PoolReleaseScope());
  if (!vm.built) build_value_maps(w);
  if ((w->b_host_stale || w->c_host_stale)) w->refresh_host_bc(true, true);  // the state restarts from the CURRENT b, c: their host mirrors

  // ---- the raw values on the device ----
  // with `normalize` and a P, updating one matrix re-equilibrates both: the set keeps the raw values of both from here on
  const bool keep_raw = w->normalized && w->has_P;
  const long annz = ms.a_nnz_in, pnnz = ms.p_nnz_in;
  auto stage = [&](DevBuf<double> &raw, bool &set, const double *given, const std::vector<double> &host0, long cnt) -> const double * {
    if (cnt <= 0) return nullptr;
    if (given && dev && !keep_raw) return given;
    if (!given && !keep_raw) return nullptr;
    if (!raw.p) raw.alloc((size_t)cnt);
    if (given) HIP_CHECK(hipMemcpyAsync(raw.p, given, sizeof(double) * cnt, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    else if (!set) {
      if ((long)host0.size() != cnt) throw std::runtime_error("scs_hip_update_matrix: the values of the kept matrix are not available");
      HIP_CHECK(hipMemcpyAsync(raw.p, host0.data(), sizeof(double) * cnt, hipMemcpyHostToDevice, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));  // (host sources are the caller's or about to be dropped)
    set = keep_raw;
    return raw.p;
  };
  const double *ax = stage(vm.raw_a, vm.raw_a_set, Ax, ms.ax0, annz);
  const double *px = w->has_P ? stage(vm.raw_p, vm.raw_p_set, Px, ms.px0, pnnz) : nullptr;
  if (keep_raw) { std::vector<double>().swap(ms.ax0); std::vector<double>().swap(ms.px0); }

  // ---- raw values into the CSR forms: one launch per matrix ----
  if (ax) vm_gather(ms.Ar.val.p, vm.ar, ax, ms.Ar.nnz, ms.At.val.p, /*nontemporal=*/false, s);
  if (px) vm_gather(ms.Pf.val.p, vm.pf, px, ms.Pf.nnz, nullptr, /*nontemporal=*/false, s);
  // ---- equilibrate in place, as scs_init ----
  if (w->normalized) {
    device_normalize(ms.At, ms.Ar, w->has_P ? &ms.Pf : nullptr, w->cone, ms.D, ms.E, s, ms.opt.norm_fuse);
    adopt_equilibration(w);
  }
  pool.reset();
  // ---- the layout copies, from the equilibrated CSR they were built from ----
  const bool a_new = ax != nullptr, p_new = px != nullptr;
  if (a_new) {
    if (ms.At.cs.ok) vm_gather(ms.At.cs.val.p, vm.at_cs, ms.Ar.val.p, (long)ms.At.cs.val.n, nullptr, true, s);
    if (ms.Ar.cs.ok) vm_gather(ms.Ar.cs.val.p, vm.ar_cs, ms.At.val.p, (long)ms.Ar.cs.val.n, nullptr, true, s);
    if (ms.At.has_slab) vm_gather(ms.At.s_val.p, vm.at_slab, ms.At.val.p, (long)ms.At.s_val.n, nullptr, true, s);
    if (ms.Ar.has_slab) vm_gather(ms.Ar.s_val.p, vm.ar_slab, ms.Ar.val.p, (long)ms.Ar.s_val.n, nullptr, true, s);
  }
  if (p_new) {
    if (ms.Pf.cs.ok) vm_gather(ms.Pf.cs.val.p, vm.pf_cs, ms.Pf.val.p, (long)ms.Pf.cs.val.n, nullptr, true, s);
    if (ms.Pf.has_slab) vm_gather(ms.Pf.s_val.p, vm.pf_slab, ms.Pf.val.p, (long)ms.Pf.s_val.n, nullptr, true, s);
    hipLaunchKernelGGL(k_csr_diag, dim3(vec_blocks(w->n)), dim3(kVecThreads), 0, s, ms.Pf.rowptr.p, ms.Pf.col.p, ms.Pf.val.p, w->n, ms.Pdiag.p);
  }
  // ---- the state scs_init leaves ----
  zero_state(w);
  start_state(w, [](const char *) {});
  HIP_CHECK(hipGetLastError());
  w->setup_time = now_ms() - t0;
}
