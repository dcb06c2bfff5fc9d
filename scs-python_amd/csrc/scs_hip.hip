// scs_hip.hip — libscs_hip.so: device-resident SCS ADMM loop for MI355X (gfx950).
//
// Replaces, for the hot path only, the absent SCS C core behind the reference's
// glue: scs_init / scs_solve / scs_update / scs_finish (R:scs/scsobject.h:903,986,
// 1217,1240), i.e. scs_source/src/scs.c + linsys/gpu/indirect (R:meson.build:195,
// 303-304).  Not a port: the reference's GPU backend keeps only the CG mat-vecs on
// the device (cuSPARSE/cuBLAS) and round-trips rhs/solution over PCIe every
// iteration; here the whole iteration — KKT solve, cone
// projections, Anderson acceleration, residuals — stays in HBM, and only a few
// scalars per iteration plus the final x,y,s cross PCIe.
//
// Iteration, state v, R = diag(diag_r):
//   u_t = (R+Q)^{-1} R v   : PCG on (R_x + P + A' R_y^{-1} A), then tau from a quadratic
//   u   = Pi_{R^n x K* x R+}(2 u_t - v)
//   rsk = R (v + u - 2 u_t)   (only when residuals are needed)
//   v  += alpha (u - u_t)
#include <atomic>
#include <cstddef>
#include <chrono>
#include <csignal>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

#include "options.hpp"
#include "aa.hpp"
#include "common.hpp"
#include "cones.hpp"
#include "host_setup.hpp"
#include "normalize_dev.hpp"
#include "psd.hpp"
#include "spectral.hpp"
#include "dense.hpp"
#include "setup_dev.hpp"
#include "setup_cs_dev.hpp"
#include "spmv.hpp"
#include "vec.hpp"
#include "device_io.hpp"
#include "dproj.hpp"
#include "lsqr.hpp"

#include "runtime.hpp"
#include "device_csr.hpp"
#include "work.hpp"
#include "io.hpp"
#include "setup.hpp"
#include "loop.hpp"
#include "batch.hpp"
#include "matrix_update.hpp"
#include "perturb.hpp"
#include "diff.hpp"
#include "refine.hpp"
#include "spmv_lanes.hpp"
#include "diff_batch.hpp"
#include "refine_batch.hpp"
#include "grad_shared.hpp"

// ================================================================ C ABI
// A consumer compiled without USE_SPECTRAL_CONES hands over a ScsCone that ends at psize: the plain entry points copy that
// prefix and nothing beyond it (the spectral fields of the copy are zero).
static ScsCone short_cone(const ScsCone *k) {
  ScsCone c;
  std::memset(&c, 0, sizeof(c));
  if (k) std::memcpy(&c, k, offsetof(ScsCone, d));
  return c;
}

extern "C" {

ScsWork *scs_init(const ScsData *d, const ScsCone *k, const ScsSettings *stgs) {
  try {
    set_last_error("");
    const ScsCone kk = short_cone(k);
    return init_impl(d, k ? &kk : nullptr, stgs);
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return nullptr;
  }
}

ScsWork *scs_hip_init_linsys(const ScsData *d, const ScsCone *k, const ScsSettings *stgs, int linsys) {
  try {
    set_last_error("");
    const ScsCone kk = short_cone(k);
    return init_impl(d, k ? &kk : nullptr, stgs, linsys);
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return nullptr;
  }
}

// the entries for consumers built with USE_SPECTRAL_CONES (include/scs_hip.h): the whole struct
ScsWork *scs_init_spectral(const ScsData *d, const ScsCone *k, const ScsSettings *stgs) {
  try {
    set_last_error("");
    return init_impl(d, k, stgs);
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return nullptr;
  }
}

ScsWork *scs_hip_init_linsys_spectral(const ScsData *d, const ScsCone *k, const ScsSettings *stgs, int linsys) {
  try {
    set_last_error("");
    return init_impl(d, k, stgs, linsys);
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return nullptr;
  }
}
ScsWork *scs_hip_clone(ScsWork *w) {
  try {
    set_last_error("");
    return clone_impl(w);
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return nullptr;
  }
}
int scs_hip_shares_matrix(const ScsWork *a, const ScsWork *b) { return a && b && a->mats == b->mats ? 1 : 0; }
int scs_hip_linsys_kind(const ScsWork *w) { return w ? (w->dense() ? 2 : 1) : 0; }

// A vector of a failed solve is NaN: on the host, or — device endpoints — on the device (best effort: the failure may be the device's)
static void fill_failed(ScsHipWork *w, ScsSolution *sol, bool dev_io) {
  if (!dev_io) {
    fill_nan(sol->x, w->n);
    fill_nan(sol->y, w->m);
    fill_nan(sol->s, w->m);
    return;
  }
  if (hipSetDevice(w->device) != hipSuccess) return;
  const double *ptr[3] = {sol->x, sol->y, sol->s};
  const long len[3] = {w->n, w->m, w->m};
  for (int k = 0; k < 3; ++k)
    if (ptr[k]) hipLaunchKernelGGL(k_fill, dim3(vec_blocks(len[k])), dim3(kVecThreads), 0, w->stream, (double *)ptr[k], (double)NAN, len[k]);
  (void)hipStreamSynchronize(w->stream);
  (void)hipGetLastError();
}

// scs_solve and scs_hip_solve_device: one loop, the endpoints on the host or (dev_io) on the device
static scs_int solve_entry(ScsWork *w, ScsSolution *sol, ScsInfo *info, scs_int warm_start, bool dev_io) {
  try {
    set_last_error("");
    const double scale_entry = w->scale;  // (nothing of the environment is read here: the workspace has its snapshot, options.hpp)
    try {
      return solve_impl(w, sol, info, warm_start, dev_io);
    } catch (const SpinTimeout &) {
      // not a failure of the problem: restart without the spinning kernels (the caller's sol is untouched until a solve finishes)
      ++g_spin_fallbacks;
      {
        std::lock_guard<std::mutex> lock(w->mtx);
        HIP_CHECK(hipSetDevice(w->device));
        w->spin_fallback(scale_entry);
      }
      return solve_impl(w, sol, info, warm_start, dev_io);
    }
  } catch (const std::exception &e) {
    set_last_error(e.what());
    info->status_val = SCS_FAILED;
    std::snprintf(info->status, sizeof(info->status), "failure");
    fill_failed(w, sol, dev_io);
    return SCS_FAILED;
  }
}

scs_int scs_solve(ScsWork *w, ScsSolution *sol, ScsInfo *info, scs_int warm_start) {
  if (!w || !sol || !info) return SCS_FAILED;
  return solve_entry(w, sol, info, warm_start, /*dev_io=*/false);
}

// ---- device-resident endpoints (include/scs_hip.h; csrc/device_io.hpp) ----
// a caller's vector must be device memory of the workspace's device: a host address handed to a kernel is a GPU fault, not an error code
static void check_device_vector(const void *p, int device, const char *who, const char *name) {
  hipPointerAttribute_t a;
  std::memset(&a, 0, sizeof(a));
  const hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) (void)hipGetLastError();
  if (e != hipSuccess || a.type != hipMemoryTypeDevice)
    throw std::runtime_error(std::string(who) + ": " + name + " is not a device address");
  if (a.device != device)
    throw std::runtime_error(std::string(who) + ": " + name + " lives on device " + std::to_string(a.device) + ", the workspace on device " +
                             std::to_string(device));
}
static void check_device_solution(const ScsHipWork *w, const double *x, const double *y, const double *s, scs_int warm_start, const char *who) {
  if (warm_start && (!x || !y || !s)) throw std::runtime_error(std::string(who) + ": a warm start needs x_dev, y_dev and s_dev");
  if (x) check_device_vector(x, w->device, who, "x_dev");
  if (y) check_device_vector(y, w->device, who, "y_dev");
  if (s) check_device_vector(s, w->device, who, "s_dev");
}

scs_int scs_hip_update_device(ScsWork *w, const scs_float *b_dev, const scs_float *c_dev) {
  if (!w) return -1;
  try {
    set_last_error("");
    if (b_dev) check_device_vector(b_dev, w->device, "scs_hip_update_device", "b_dev");
    if (c_dev) check_device_vector(c_dev, w->device, "scs_hip_update_device", "c_dev");
    std::lock_guard<std::mutex> lock(w->mtx);
    HIP_CHECK(hipSetDevice(w->device));
    ScsHipWork::ScratchTurn turn(w);
    w->diff_mark_stale();
    w->update_device(b_dev, c_dev);
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}

scs_int scs_hip_solve_device(ScsWork *w, scs_float *x_dev, scs_float *y_dev, scs_float *s_dev, ScsInfo *info, scs_int warm_start) {
  if (!w || !info) return -1;
  try {
    set_last_error("");
    check_device_solution(w, x_dev, y_dev, s_dev, warm_start, "scs_hip_solve_device");
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
  ScsSolution sol{x_dev, y_dev, s_dev};
  return solve_entry(w, &sol, info, warm_start, /*dev_io=*/true);
}
int scs_hip_work_device(const ScsWork *w) { return w ? w->device : -1; }

// Grouped solve of `count` workspaces (include/scs_hip.h): members that can share launches — same shape, CSR-stream
// layouts, one-launch cone kernels (GroupSolve::member_ok / same_shape) — advance in lock step through the grouped
// kernels of batch.hpp; the others are solved by scs_solve's own loop.  Every info[i] / sol[i] is filled exactly as
// scs_solve(w[i], sol[i], info[i], warm_start) would (iterates are bit-identical).
// A shape class is one group (cut into near-equal parts above kGroupMax members), and the groups of a call run one after the other on
// the calling thread: several concurrently driven groups were built, measured and lost.
// o: the options of THIS call (solve_batch_entry) — the group-level ones, batch.hpp GroupSolve::opt.
static scs_int solve_one_group(ScsWork **works, ScsSolution **sols, ScsInfo **infos, const std::vector<int> &idx, scs_int warm_start,
                               std::string &err, bool dev_io, const Options &o) {
  if (idx.size() == 1) {
    const int i = idx[0];
    const scs_int st = solve_entry(works[i], sols[i], infos[i], warm_start, dev_io);
    if (st == SCS_FAILED) { err = scs_hip_last_error(); return -1; }
    return 0;
  }
  scs_int rc = 0;
  std::vector<std::unique_lock<std::mutex>> locks;
  std::vector<hipStream_t> saved;
  GroupSolve gs(o);
  //  every member starts out "unfinished": the catch block below marks exactly those the solve did not finish, also when
  // the exception comes before the members' begin_solve cleared their infos (caller memory); member mutexes are taken in ADDRESS
  // order, so two concurrent batches that share workspaces in different orders cannot deadlock (the Python glue sorts too)
  for (int j : idx) {
    std::memset(infos[j], 0, sizeof(ScsInfo));
    infos[j]->status_val = SCS_UNFINISHED;
  }
  try {
    {
      std::vector<int> order(idx);
      std::sort(order.begin(), order.end(), [&](int a, int b) { return std::less<ScsHipWork *>()(works[a], works[b]); });
      for (int j : order) locks.emplace_back(works[j]->mtx);
    }
    HIP_CHECK(hipSetDevice(works[idx[0]]->device));
    gs.s = works[idx[0]]->stream;
    gs.dev_io = dev_io;
    for (int j : idx) {
      gs.W.push_back(works[j]); gs.sols.push_back(sols[j]); gs.infos.push_back(infos[j]);
      saved.push_back(works[j]->stream);
      works[j]->stream = gs.s;  // every member's kernels go to the group's stream for the duration of the solve
      works[j]->aa.stream = gs.s;
    }
    gs.build();
    gs.run(warm_start);
  } catch (const std::exception &e) {
    err = e.what();
    rc = -1;
    (void)hipStreamSynchronize(gs.s);
    for (int j : idx)
      if (infos[j]->status[0] == 0) {  // (finish_solve writes the status string: empty = this member never got there)
        infos[j]->status_val = SCS_FAILED;
        std::snprintf(infos[j]->status, sizeof(infos[j]->status), "failure");
        fill_failed(works[j], sols[j], dev_io);
      }
  }
  for (size_t k = 0; k < saved.size(); ++k) {
    works[idx[k]]->stream = saved[k];
    works[idx[k]]->aa.stream = saved[k];
  }
  return rc;
}

// The jobs of a batch: shape classes of members that can share launches (GroupSolve::member_ok / same_shape), in the order of
// their first member, each cut into contiguous, near-equal parts; a job of one member is solved by scs_solve.  Both
// scs_hip_solve_batch and scs_hip_batch_plan take their groups from here (a function of the workspaces alone).
constexpr int kGroupMax = 1024;  // members of one group
static std::vector<std::vector<int>> plan_batch(ScsWork *const *works, int count) {
  std::vector<std::vector<int>> jobs;
  std::vector<char> taken((size_t)count, 0);
  for (int i = 0; i < count; ++i) {
    if (taken[(size_t)i]) continue;
    taken[(size_t)i] = 1;
    std::vector<int> cls{i};
    if (GroupSolve::member_ok(works[i]))
      for (int j = i + 1; j < count; ++j)
        if (!taken[(size_t)j] && GroupSolve::member_ok(works[j]) && GroupSolve::same_shape(works[i], works[j])) {
          taken[(size_t)j] = 1;
          cls.push_back(j);
        }
    const int S = (int)cls.size();
    const int k = (S + kGroupMax - 1) / kGroupMax;
    for (int part = 0; part < k; ++part) {  // contiguous, near-equal parts
      const int lo = (int)((long)S * part / k), hi = (int)((long)S * (part + 1) / k);
      jobs.emplace_back(cls.begin() + lo, cls.begin() + hi);
    }
  }
  return jobs;
}

// What scs_hip_solve_batch(works, .., count, ..) would do with each member (include/scs_hip.h): group_of[i] = the index of its
// group, -1 for a member solved alone.  Returns the number of groups, -1 on bad arguments.
int scs_hip_batch_plan(ScsWork **works, scs_int count, scs_int *group_of) {
  if (!works || !group_of || count < 0) return -1;
  set_last_error("");
  for (int i = 0; i < count; ++i) {
    if (!works[i]) { set_last_error("scs_hip_batch_plan: null entry"); return -1; }
    for (int j = 0; j < i; ++j)
      if (works[j] == works[i]) { set_last_error("scs_hip_batch_plan: a workspace appears twice"); return -1; }
  }
  int groups = 0;
  for (const std::vector<int> &job : plan_batch(works, (int)count)) {
    const int id = job.size() > 1 ? groups++ : -1;
    for (int i : job) group_of[i] = id;
  }
  return groups;
}

// scs_hip_solve_batch and scs_hip_solve_batch_device: the same jobs, the endpoints on the host or (dev_io) on the device
static scs_int solve_batch_entry(ScsWork **works, ScsSolution **sols, ScsInfo **infos, scs_int count, scs_int warm_start, bool dev_io) {
  InterruptListener ctrlc;  // for the whole call: members solved one after the other all see the same Ctrl-C
  refresh_options();
  const Options &o = opts();  // the group-level options of this call (per-workspace ones stay what each member was created with)
  std::vector<std::vector<int>> jobs = plan_batch(works, (int)count);
  std::stable_sort(jobs.begin(), jobs.end(), [](const std::vector<int> &a, const std::vector<int> &b) { return a.size() > b.size(); });
  scs_int rc = 0;
  std::string first_err;
  (void)hipSetDevice(current_device());
  for (const std::vector<int> &job : jobs) {
    std::string err;
    if (solve_one_group(works, sols, infos, job, warm_start, err, dev_io, o) != 0) {
      rc = -1;
      if (first_err.empty()) first_err = err;
    }
  }
  if (rc != 0) set_last_error(first_err);
  return rc;
}

scs_int scs_hip_solve_batch(ScsWork **works, ScsSolution **sols, ScsInfo **infos, scs_int count, scs_int warm_start) {
  if (!works || !sols || !infos || count < 0) return -1;
  set_last_error("");
  for (int i = 0; i < count; ++i) {
    if (!works[i] || !sols[i] || !infos[i]) { set_last_error("scs_hip_solve_batch: null entry"); return -1; }
    for (int j = 0; j < i; ++j)
      if (works[j] == works[i]) { set_last_error("scs_hip_solve_batch: a workspace appears twice"); return -1; }
  }
  return solve_batch_entry(works, sols, infos, count, warm_start, /*dev_io=*/false);
}

scs_int scs_hip_solve_batch_device(ScsWork **works, scs_float **x_dev, scs_float **y_dev, scs_float **s_dev, ScsInfo **infos, scs_int count,
                                   scs_int warm_start) {
  if (!works || !infos || count < 0) return -1;
  set_last_error("");
  std::vector<ScsSolution> sols((size_t)count);
  std::vector<ScsSolution *> solp((size_t)count);
  try {
    if (warm_start && (!x_dev || !y_dev || !s_dev)) throw std::runtime_error("scs_hip_solve_batch_device: a warm start needs x_dev, y_dev and s_dev");
    for (int i = 0; i < count; ++i) {
      if (!works[i] || !infos[i]) throw std::runtime_error("scs_hip_solve_batch_device: null entry");
      for (int j = 0; j < i; ++j)
        if (works[j] == works[i]) throw std::runtime_error("scs_hip_solve_batch_device: a workspace appears twice");
      sols[(size_t)i] = ScsSolution{x_dev ? x_dev[i] : nullptr, y_dev ? y_dev[i] : nullptr, s_dev ? s_dev[i] : nullptr};
      solp[(size_t)i] = &sols[(size_t)i];
      check_device_solution(works[i], sols[(size_t)i].x, sols[(size_t)i].y, sols[(size_t)i].s, warm_start, "scs_hip_solve_batch_device");
    }
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
  return solve_batch_entry(works, solp.data(), infos, count, warm_start, /*dev_io=*/true);
}

scs_int scs_update(ScsWork *w, scs_float *b, scs_float *c) {
  if (!w) return -1;
  try {
    std::lock_guard<std::mutex> lock(w->mtx);
    HIP_CHECK(hipSetDevice(w->device));
    ScsHipWork::ScratchTurn turn(w);
    w->diff_mark_stale();
    const int n = w->n, m = w->m;
    if ((!b && w->b_host_stale) || (!c && w->c_host_stale)) w->refresh_host_bc(!b, !c);  // (a kept vector that a device update replaced)
    if (b) { w->b_orig.assign(b, b + m); w->b_host_stale = false; w->b_raw_fresh = false; }
    if (c) { w->c_orig.assign(c, c + n); w->c_host_stale = false; w->c_raw_fresh = false; }
    w->nm_b_orig = w->nm_c_orig = 0;
    for (double x : w->b_orig) w->nm_b_orig = std::max(w->nm_b_orig, std::fabs(x));
    for (double x : w->c_orig) w->nm_c_orig = std::max(w->nm_c_orig, std::fabs(x));
    std::vector<double> bn(w->b_orig), cn(w->c_orig);
    if (w->normalized) normalize_b_c(w->scal, bn.data(), m, cn.data(), n);
    std::vector<double> hh(w->l, 0.0);
    std::copy(cn.begin(), cn.end(), hh.begin());
    std::copy(bn.begin(), bn.end(), hh.begin() + n);
    w->h.upload(hh.data(), w->l, w->stream);
    if (w->normalized) {  // sigma changed: refresh the un-normalisation factors
      std::vector<double> di(m), ei(n);
      for (int i = 0; i < m; ++i) di[i] = 1.0 / (w->scal.D[i] * w->scal.sigma);
      for (int i = 0; i < n; ++i) ei[i] = 1.0 / (w->scal.E[i] * w->scal.sigma);
      w->Dinv.upload(di.data(), m, w->stream);
      w->Einv.upload(ei.data(), n, w->stream);
    }
    HIP_CHECK(hipStreamSynchronize(w->stream));
    if (w->setup_pending) w->finish_pending_setup();  // (a workspace that has not solved yet: R, the preconditioner or G^{-1}, and g in one go)
    else w->update_work_cache();
    HIP_CHECK(hipStreamSynchronize(w->stream));
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}

// ---- matrix values on the resident layouts (include/scs_hip.h; csrc/matrix_update.hpp) ----
// every refusal of an ARGUMENT comes before device work; all leave the workspace as it was (a value map that does not reproduce a
// resident layout is found by device work, at the first call: matrix_update.hpp build_value_maps)
static scs_int update_matrix_entry(ScsWork *w, const scs_float *Ax, const scs_float *Px, bool dev, const char *who) {
  if (!w) {
    set_last_error(std::string(who) + ": null workspace");
    return -1;
  }
  try {
    set_last_error("");
    if (!Ax && !Px) return 0;
    if (Px && !w->has_P) throw std::runtime_error(std::string(who) + ": values of P for a workspace created without P");
    // (Ax alone too: the first call maps every resident form, and with `normalize` new values of A re-equilibrate P from its raw values)
    if (w->has_P && !w->mats->p_update_refusal.empty()) throw std::runtime_error(std::string(who) + ": " + w->mats->p_update_refusal);
    if (dev) {
      if (Ax) check_device_vector(Ax, w->device, who, "Ax_dev");
      if (Px) check_device_vector(Px, w->device, who, "Px_dev");
    }
    std::lock_guard<std::mutex> lock(w->mtx);
    if (w->mats.use_count() > 1)
      throw std::runtime_error(std::string(who) + ": the matrix set is shared by " + std::to_string(w->mats.use_count()) +
                               " workspaces (live clones read it): finish the clones first");
    HIP_CHECK(hipSetDevice(w->device));
    ScsHipWork::ScratchTurn turn(w);
    w->diff_mark_stale();
    update_matrix_impl(w, Ax, Px, dev);
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}
scs_int scs_hip_update_matrix(ScsWork *w, const scs_float *Ax, const scs_float *Px) {
  return update_matrix_entry(w, Ax, Px, /*dev=*/false, "scs_hip_update_matrix");
}
scs_int scs_hip_update_matrix_device(ScsWork *w, const scs_float *Ax_dev, const scs_float *Px_dev) {
  return update_matrix_entry(w, Ax_dev, Px_dev, /*dev=*/true, "scs_hip_update_matrix_device");
}

// ---- derivatives of the last solve (include/scs_hip.h; csrc/diff.hpp) ----
// every refusal comes before device work and leaves the workspace as it was.  dev: the pointers are device pointers; else host
// pointers, staged into device buffers around the same path.
// why the matrix perturbations of a forward call cannot be taken ("" = they can)
static std::string pert_refusal(const ScsHipWork *w, const DiffCall &call) {
  if (call.adjoint) return "";
  if (call.pert[0] && w->At.nnz != w->mats->a_nnz_in) return "the resident A' does not hold nnz(A) values: dAx cannot be applied";
  if (call.pert[1]) {
    if (!w->has_P) return "dPx for a workspace created without P";
    if (!w->mats->p_update_refusal.empty()) return w->mats->p_update_refusal;
  }
  return "";
}
// the device-pointer checks of a call's vectors, under the names the entry's header gives them
static void diff_check_device(const ScsHipWork *w, const DiffCall &call, const char *who) {
  for (int k = 0; k < 2; ++k)
    if (call.pert[k]) check_device_vector(call.pert[k], w->device, who, (std::string(DiffCall::pert_name(k)) + "_dev").c_str());
  for (int k = 0; k < 3; ++k)
    if (call.in[k]) check_device_vector(call.in[k], w->device, who, (std::string(call.in_name(k)) + "_dev").c_str());
  for (int k = 0; k < 4; ++k)
    if (call.out[k]) check_device_vector(call.out[k], w->device, who, (std::string(call.out_name(k)) + "_dev").c_str());
}
// The refusal ladder of one call on one workspace (the caller holds w->mtx): the first step that applies throws "<who>: <reason>".
// who = the entry's name, or "<entry>: member i" in a batch, whose members must all live on `batch_device` (< 0: a call of its own).
static void diff_check(const ScsHipWork *w, const DiffCall &call, bool dev, const std::string &who, int batch_device = -1) {
  std::string why = diff_refusal(w);
  if (why.empty() && batch_device >= 0 && w->device != batch_device) why = "the members of a batch live on one device";
  if (why.empty() && call.adjoint && call.out[2] && w->At.nnz != w->mats->a_nnz_in)
    why = "the resident A' does not hold nnz(A) values: dAx cannot be gathered";
  if (why.empty() && call.adjoint && call.out[3]) why = !w->has_P ? "dPx for a workspace created without P" : w->mats->p_update_refusal;
  if (why.empty()) why = pert_refusal(w, call);
  if (!why.empty()) throw std::runtime_error(who + ": " + why);
  if (dev) diff_check_device(w, call, who.c_str());
}
// The host twin of one call: device copies of `in` and `pert`, device blocks for `out`.  stage() queues the uploads and returns the
// device-side call, fetch() queues the downloads; the caller synchronises the stream once after all uploads and once after all
// downloads, and holds an ArenaScope(nullptr).
struct DiffStage {
  DevBuf<double> bin[3], bout[4], bpert[2];
  DiffCall host;
  DiffCall stage(const ScsHipWork *w, const DiffCall &call, hipStream_t s) {
    host = call;
    DiffCall dc = call;
    for (int k = 0; k < 3; ++k)
      if (call.in[k]) {
        bin[k].upload(call.in[k], (size_t)call.in_len(w, k), s);
        dc.in[k] = bin[k].p;
      }
    for (int k = 0; k < 2; ++k)
      if (call.pert[k]) {
        bpert[k].upload(call.pert[k], (size_t)std::max(DiffCall::pert_len(w, k), 1L), s);
        dc.pert[k] = bpert[k].p;
      }
    for (int k = 0; k < 4; ++k)
      if (call.out[k]) {
        bout[k].alloc((size_t)std::max(call.out_len(w, k), 1L));
        dc.out[k] = bout[k].p;
      }
    return dc;
  }
  void fetch(const ScsHipWork *w, hipStream_t s) const {
    for (int k = 0; k < 4; ++k)
      if (host.out[k]) bout[k].download(host.out[k], (size_t)host.out_len(w, k), s);
  }
};
static scs_int diff_entry(ScsWork *w, DiffCall call, const ScsHipDiffOpts *o, ScsHipDiffInfo *info, bool dev, const char *who) {
  if (!w) {
    set_last_error(std::string(who) + ": null workspace");
    return -1;
  }
  try {
    set_last_error("");
    std::lock_guard<std::mutex> lock(w->mtx);
    diff_check(w, call, dev, who);
    HIP_CHECK(hipSetDevice(w->device));
    ScsHipWork::ScratchTurn turn(w);
    if (dev) {
      diff_impl(w, call, o, info);
      return 0;
    }
    ArenaScope no_arena(nullptr);
    DiffStage st;
    const DiffCall dc = st.stage(w, call, w->stream);
    HIP_CHECK(hipStreamSynchronize(w->stream));
    diff_impl(w, dc, o, info);
    st.fetch(w, w->stream);
    HIP_CHECK(hipStreamSynchronize(w->stream));
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}
static DiffCall adjoint_call(const scs_float *gx, const scs_float *gy, const scs_float *gs, scs_float *db, scs_float *dc, scs_float *dAx,
                             scs_float *dPx) {
  DiffCall c;
  c.adjoint = true;
  c.in[0] = gx; c.in[1] = gy; c.in[2] = gs;
  c.out[0] = db; c.out[1] = dc; c.out[2] = dAx; c.out[3] = dPx;
  return c;
}
static DiffCall derivative_call(const scs_float *db, const scs_float *dc, const scs_float *dAx, const scs_float *dPx, scs_float *dx,
                                scs_float *dy, scs_float *ds) {
  DiffCall c;
  c.adjoint = false;
  c.in[0] = db; c.in[1] = dc;
  c.pert[0] = dAx; c.pert[1] = dPx;
  c.out[0] = dx; c.out[1] = dy; c.out[2] = ds;
  return c;
}
scs_int scs_hip_adjoint_device(ScsWork *w, const scs_float *gx_dev, const scs_float *gy_dev, const scs_float *gs_dev, scs_float *db_dev,
                               scs_float *dc_dev, scs_float *dAx_dev, scs_float *dPx_dev, const ScsHipDiffOpts *opts, ScsHipDiffInfo *info) {
  return diff_entry(w, adjoint_call(gx_dev, gy_dev, gs_dev, db_dev, dc_dev, dAx_dev, dPx_dev), opts, info, /*dev=*/true, "scs_hip_adjoint_device");
}
scs_int scs_hip_adjoint(ScsWork *w, const scs_float *gx, const scs_float *gy, const scs_float *gs, scs_float *db, scs_float *dc, scs_float *dAx,
                        scs_float *dPx, const ScsHipDiffOpts *opts, ScsHipDiffInfo *info) {
  return diff_entry(w, adjoint_call(gx, gy, gs, db, dc, dAx, dPx), opts, info, /*dev=*/false, "scs_hip_adjoint");
}
scs_int scs_hip_derivative_full_device(ScsWork *w, const scs_float *db_dev, const scs_float *dc_dev, const scs_float *dAx_dev,
                                       const scs_float *dPx_dev, scs_float *dx_dev, scs_float *dy_dev, scs_float *ds_dev,
                                       const ScsHipDiffOpts *opts, ScsHipDiffInfo *info) {
  return diff_entry(w, derivative_call(db_dev, dc_dev, dAx_dev, dPx_dev, dx_dev, dy_dev, ds_dev), opts, info, /*dev=*/true,
                    "scs_hip_derivative_full_device");
}
scs_int scs_hip_derivative_full(ScsWork *w, const scs_float *db, const scs_float *dc, const scs_float *dAx, const scs_float *dPx, scs_float *dx,
                                scs_float *dy, scs_float *ds, const ScsHipDiffOpts *opts, ScsHipDiffInfo *info) {
  return diff_entry(w, derivative_call(db, dc, dAx, dPx, dx, dy, ds), opts, info, /*dev=*/false, "scs_hip_derivative_full");
}
// (one path: the entries without matrix perturbations are the full ones with NULL dAx / dPx, under their own name in a refusal)
scs_int scs_hip_derivative_device(ScsWork *w, const scs_float *db_dev, const scs_float *dc_dev, scs_float *dx_dev, scs_float *dy_dev,
                                  scs_float *ds_dev, const ScsHipDiffOpts *opts, ScsHipDiffInfo *info) {
  return diff_entry(w, derivative_call(db_dev, dc_dev, nullptr, nullptr, dx_dev, dy_dev, ds_dev), opts, info, /*dev=*/true, "scs_hip_derivative_device");
}
scs_int scs_hip_derivative(ScsWork *w, const scs_float *db, const scs_float *dc, scs_float *dx, scs_float *dy, scs_float *ds,
                           const ScsHipDiffOpts *opts, ScsHipDiffInfo *info) {
  return diff_entry(w, derivative_call(db, dc, nullptr, nullptr, dx, dy, ds), opts, info, /*dev=*/false, "scs_hip_derivative");
}

// dP x + dA' y (n) and dA x (m) at the resident solution: the perturbation products of the full derivative on their own (perturb.hpp)
static scs_int data_perturbation_entry(ScsWork *w, const scs_float *dAx, const scs_float *dPx, scs_float *out_c, scs_float *out_b, bool dev,
                                       const char *who) {
  if (!w) {
    set_last_error(std::string(who) + ": null workspace");
    return -1;
  }
  try {
    set_last_error("");
    const DiffCall call = derivative_call(nullptr, nullptr, dAx, dPx, nullptr, nullptr, nullptr);
    std::lock_guard<std::mutex> lock(w->mtx);
    std::string why = diff_refusal(w);
    if (why.empty()) why = pert_refusal(w, call);
    if (!why.empty()) throw std::runtime_error(std::string(who) + ": " + why);
    if (dev) {
      diff_check_device(w, call, who);  // (dAx, dPx: the call holds nothing else)
      if (out_c) check_device_vector(out_c, w->device, who, "out_c_dev");
      if (out_b) check_device_vector(out_b, w->device, who, "out_b_dev");
    }
    HIP_CHECK(hipSetDevice(w->device));
    ScsHipWork::ScratchTurn turn(w);
    hipStream_t s = w->stream;
    const size_t n = (size_t)w->n, m = (size_t)w->m;
    ArenaScope no_arena(nullptr);
    DevBuf<double> ba, bp, bc, bb;
    const double *da = dAx, *dp = dPx;
    double *oc = out_c, *ob = out_b;
    if (!dev) {
      if (dAx) { ba.upload(dAx, (size_t)std::max(DiffCall::pert_len(w, 0), 1L), s); da = ba.p; }
      if (dPx) { bp.upload(dPx, (size_t)std::max(DiffCall::pert_len(w, 1), 1L), s); dp = bp.p; }
      if (out_c) { bc.alloc(n); oc = bc.p; }
      if (out_b) { bb.alloc(m); ob = bb.p; }
      HIP_CHECK(hipStreamSynchronize(s));
    }
    diff_alloc(w);
    pert_alloc(w, da != nullptr, dp != nullptr, who);
    pert_launch(w, da, dp, nullptr, nullptr, 1.0, oc, ob, s);
    HIP_CHECK(hipGetLastError());
    if (!dev) {
      if (out_c) bc.download(out_c, n, s);
      if (out_b) bb.download(out_b, m, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}
scs_int scs_hip_data_perturbation_device(ScsWork *w, const scs_float *dAx_dev, const scs_float *dPx_dev, scs_float *out_c_dev,
                                         scs_float *out_b_dev) {
  return data_perturbation_entry(w, dAx_dev, dPx_dev, out_c_dev, out_b_dev, /*dev=*/true, "scs_hip_data_perturbation_device");
}
scs_int scs_hip_data_perturbation(ScsWork *w, const scs_float *dAx, const scs_float *dPx, scs_float *out_c, scs_float *out_b) {
  return data_perturbation_entry(w, dAx, dPx, out_c, out_b, /*dev=*/false, "scs_hip_data_perturbation");
}

// ---- grouped derivatives (include/scs_hip.h; csrc/diff_batch.hpp) ----
// The jobs of a derivative batch: classes of members that can share launches (GroupDiff::member_ok / same_shape, and the same request
// for dAx / dPx), in the order of their first member; a job of one member goes through diff_impl.
static std::vector<std::vector<int>> plan_diff_batch(ScsWork *const *works, int count, const std::vector<int> &want) {
  std::vector<std::vector<int>> jobs;
  std::vector<char> taken((size_t)count, 0);
  for (int i = 0; i < count; ++i) {
    if (taken[(size_t)i]) continue;
    taken[(size_t)i] = 1;
    std::vector<int> cls{i};
    if (GroupDiff::member_ok(works[i]))
      for (int j = i + 1; j < count && (int)cls.size() < kGroupMax; ++j)
        if (!taken[(size_t)j] && want[(size_t)j] == want[(size_t)i] && GroupDiff::member_ok(works[j]) && GroupDiff::same_shape(works[i], works[j])) {
          taken[(size_t)j] = 1;
          cls.push_back(j);
        }
    jobs.push_back(cls);
  }
  return jobs;
}
static bool diff_batch_members_ok(ScsWork *const *works, scs_int count, const char *who) {
  if (!works || count <= 0) {
    set_last_error(std::string(who) + ": count must be positive and w non-NULL");
    return false;
  }
  for (int i = 0; i < count; ++i) {
    if (!works[i]) { set_last_error(std::string(who) + ": member " + std::to_string(i) + ": null workspace"); return false; }
    for (int j = 0; j < i; ++j)
      if (works[j] == works[i]) { set_last_error(std::string(who) + ": member " + std::to_string(i) + ": a workspace appears twice"); return false; }
  }
  return true;
}

int scs_hip_diff_batch_plan(ScsWork **works, scs_int count, int want_dA, int want_dP, scs_int *group_of) {
  if (!group_of) return -1;
  set_last_error("");
  if (!diff_batch_members_ok(works, count, "scs_hip_diff_batch_plan")) return -1;
  const std::vector<int> want((size_t)count, (want_dA ? 1 : 0) | (want_dP ? 2 : 0));
  int groups = 0;
  for (const std::vector<int> &job : plan_diff_batch(works, (int)count, want)) {
    const int id = job.size() > 1 ? groups++ : -1;
    for (int i : job) group_of[i] = id;
  }
  return groups;
}
long scs_hip_diff_group_launches(void) { return g_diff_group_launches.load(); }
long scs_hip_diff_group_syncs(void) { return g_diff_group_syncs.load(); }

// the two outputs of scs_hip_adjoint_shared[_device]: ONE vector each for all members (csrc/grad_shared.hpp); nullptr = not wanted
struct SharedSum {
  scs_float *dA = nullptr, *dP = nullptr;
};
// dev: the members' pointers are device pointers; else host pointers, staged around the same path (same bits).  sum: the members share
// one matrix set and carry no dAx / dPx of their own; after they are differentiated as ever, the sums of their matrix gradients go to *sum.
static scs_int diff_batch_entry(ScsWork **works, std::vector<DiffCall> calls, const ScsHipDiffOpts *o, ScsHipDiffInfo **infos, scs_int count,
                                bool dev, const char *who, const SharedSum *sum = nullptr) {
  set_last_error("");
  if (!diff_batch_members_ok(works, count, who)) return -1;
  if (sum && !sum->dA && !sum->dP) {
    set_last_error(std::string(who) + ": dAx_sum and dPx_sum are both NULL: nothing to sum");
    return -1;
  }
  const bool adjoint = calls[0].adjoint;  // (count >= 1: one call per member)
  std::vector<std::unique_lock<std::mutex>> locks;
  std::vector<hipStream_t> saved;
  std::vector<int> restored;
  scs_int rc = 0;
  try {
    {  // member mutexes in ADDRESS order (as solve_one_group)
      std::vector<int> order((size_t)count);
      std::iota(order.begin(), order.end(), 0);
      std::sort(order.begin(), order.end(), [&](int a, int b) { return std::less<ScsHipWork *>()(works[a], works[b]); });
      for (int j : order) locks.emplace_back(works[j]->mtx);
    }
    // every member's refusal ladder, before any device work
    std::vector<int> want((size_t)count, 0);
    for (int i = 0; i < count; ++i) {
      const DiffCall &call = calls[(size_t)i];
      const std::string member = std::string(who) + ": member " + std::to_string(i);
      if (sum) {  // the ladder of a member that asks for what the sums hold (the sum outputs stand in its dAx / dPx slots)
        DiffCall asked = call;
        asked.out[2] = sum->dA; asked.out[3] = sum->dP;
        diff_check(works[i], asked, dev, member, works[0]->device);
        if (!scs_hip_shares_matrix(works[i], works[0]))
          throw std::runtime_error(member + ": does not share the matrix set of member 0 (scs_hip_clone): the matrix gradients of different matrices cannot be summed");
      } else {
        diff_check(works[i], call, dev, member, works[0]->device);
      }
      want[(size_t)i] = adjoint ? ((call.out[2] ? 1 : 0) | (call.out[3] ? 2 : 0)) : ((call.pert[0] ? 1 : 0) | (call.pert[1] ? 2 : 0));
    }
    HIP_CHECK(hipSetDevice(works[0]->device));
    hipStream_t s = works[0]->stream;
    ArenaScope no_arena(nullptr);
    std::vector<DiffStage> stages(dev ? 0 : (size_t)count);  // host twins: every member's vectors
    DevBuf<double> sum_a, sum_p;                               // ... and the two sums
    GradSumJob gsum;
    if (sum) {
      ScsHipWork *w0 = works[0];
      gsum.n = w0->n; gsum.m = w0->m;
      gsum.a_rp = w0->At.rowptr.p; gsum.a_ci = w0->At.col.p; gsum.a_nnz = (long)w0->At.nnz;
      gsum.dA = sum->dA; gsum.dP = sum->dP;
      if (sum->dP) {
        diff_build_tri(w0);  // (it may still refuse: before any member is differentiated)
        gsum.p_rp = w0->Pf.rowptr.p; gsum.p_ci = w0->Pf.col.p; gsum.p_up = w0->diff.tri_up.p; gsum.p_nnz = w0->mats->p_nnz_in;
      }
      if (!dev) {
        if (sum->dA) { sum_a.alloc((size_t)std::max(gsum.a_nnz, 1L)); gsum.dA = sum_a.p; }
        if (sum->dP) { sum_p.alloc((size_t)std::max(gsum.p_nnz, 1L)); gsum.dP = sum_p.p; }
      }
    }
    if (!dev) {
      for (int i = 0; i < count; ++i) calls[(size_t)i] = stages[(size_t)i].stage(works[i], calls[(size_t)i], s);
      HIP_CHECK(hipStreamSynchronize(s));
    }
    for (const std::vector<int> &job : plan_diff_batch(works, (int)count, want)) {
      if (job.size() == 1) {
        ScsHipWork *w = works[job[0]];
        ScsHipWork::ScratchTurn turn(w);
        diff_impl(w, calls[(size_t)job[0]], o, infos ? infos[job[0]] : nullptr);
        continue;
      }
      GroupDiff gd;
      gd.adjoint = adjoint;
      gd.s = s;
      for (int j : job) {  // every member's kernels go to the group's stream for the duration of the call
        saved.push_back(works[j]->stream);
        restored.push_back(j);
        works[j]->stream = s;
      }
      for (int j : job) {
        diff_alloc(works[j]);
        if (adjoint && calls[(size_t)j].out[3]) diff_build_tri(works[j]);
        if (calls[(size_t)j].perturbs()) pert_alloc(works[j], calls[(size_t)j].pert[0] != nullptr, calls[(size_t)j].pert[1] != nullptr, who);
        gd.W.push_back(works[j]);
        gd.calls.push_back(calls[(size_t)j]);
        gd.infos.push_back(infos ? infos[j] : nullptr);
      }
      gd.run(o);
      for (size_t k = 0; k < restored.size(); ++k) works[restored[k]]->stream = saved[k];
      saved.clear();
      restored.clear();
    }
    if (sum) {  // every member's db, dc lie in its own scratch (DiffWiring: tA, tP), its solution in solx, soly: all members, in index order
      std::vector<const double *> X, Y, DB, DC;
      for (int i = 0; i < count; ++i) {
        const ScsHipWork *w = works[i];
        X.push_back(w->solx.p); Y.push_back(w->soly.p); DB.push_back(w->diff.tA.p); DC.push_back(w->diff.tP.p);
      }
      grad_sum_run(gsum, X, Y, DB, DC, s);
      if (!dev) {
        if (sum->dA) sum_a.download(sum->dA, (size_t)gsum.a_nnz, s);
        if (sum->dP) sum_p.download(sum->dP, (size_t)gsum.p_nnz, s);
      }
    }
    if (!dev) {
      for (int i = 0; i < count; ++i) stages[(size_t)i].fetch(works[i], s);
      HIP_CHECK(hipStreamSynchronize(s));
    }
  } catch (const std::exception &e) {
    set_last_error(e.what());
    rc = -1;
  }
  for (size_t k = 0; k < restored.size(); ++k) works[restored[k]]->stream = saved[k];
  return rc;
}
static const scs_float *at_or_null(const scs_float **a, int i) { return a ? a[i] : nullptr; }
static scs_float *at_or_null(scs_float **a, int i) { return a ? a[i] : nullptr; }
static scs_int adjoint_batch_entry(ScsWork **w, const scs_float **gx, const scs_float **gy, const scs_float **gs, scs_float **db, scs_float **dc,
                                   scs_float **dAx, scs_float **dPx, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count, bool dev,
                                   const char *who) {
  std::vector<DiffCall> calls;
  for (int i = 0; i < count; ++i)
    calls.push_back(adjoint_call(at_or_null(gx, i), at_or_null(gy, i), at_or_null(gs, i), at_or_null(db, i), at_or_null(dc, i),
                                 at_or_null(dAx, i), at_or_null(dPx, i)));
  return diff_batch_entry(w, calls, opts, info, count, dev, who);
}
// the members as scs_hip_adjoint_batch[_device] takes them with dAx = dPx = NULL, then the two sums
static scs_int adjoint_shared_entry(ScsWork **w, const scs_float **gx, const scs_float **gy, const scs_float **gs, scs_float **db, scs_float **dc,
                                    scs_float *dAx_sum, scs_float *dPx_sum, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count,
                                    bool dev, const char *who) {
  std::vector<DiffCall> calls;
  for (int i = 0; i < count; ++i)
    calls.push_back(adjoint_call(at_or_null(gx, i), at_or_null(gy, i), at_or_null(gs, i), at_or_null(db, i), at_or_null(dc, i), nullptr, nullptr));
  const SharedSum sum{dAx_sum, dPx_sum};
  return diff_batch_entry(w, calls, opts, info, count, dev, who, &sum);
}
static scs_int derivative_batch_entry(ScsWork **w, const scs_float **db, const scs_float **dc, const scs_float **dAx, const scs_float **dPx,
                                      scs_float **dx, scs_float **dy, scs_float **ds, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info,
                                      scs_int count, bool dev, const char *who) {
  std::vector<DiffCall> calls;
  for (int i = 0; i < count; ++i)
    calls.push_back(derivative_call(at_or_null(db, i), at_or_null(dc, i), at_or_null(dAx, i), at_or_null(dPx, i), at_or_null(dx, i),
                                    at_or_null(dy, i), at_or_null(ds, i)));
  return diff_batch_entry(w, calls, opts, info, count, dev, who);
}
scs_int scs_hip_adjoint_batch_device(ScsWork **w, const scs_float **gx_dev, const scs_float **gy_dev, const scs_float **gs_dev, scs_float **db_dev,
                                     scs_float **dc_dev, scs_float **dAx_dev, scs_float **dPx_dev, const ScsHipDiffOpts *opts,
                                     ScsHipDiffInfo **info, scs_int count) {
  return adjoint_batch_entry(w, gx_dev, gy_dev, gs_dev, db_dev, dc_dev, dAx_dev, dPx_dev, opts, info, count, /*dev=*/true, "scs_hip_adjoint_batch_device");
}
scs_int scs_hip_adjoint_batch(ScsWork **w, const scs_float **gx, const scs_float **gy, const scs_float **gs, scs_float **db, scs_float **dc,
                              scs_float **dAx, scs_float **dPx, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count) {
  return adjoint_batch_entry(w, gx, gy, gs, db, dc, dAx, dPx, opts, info, count, /*dev=*/false, "scs_hip_adjoint_batch");
}
scs_int scs_hip_adjoint_shared_device(ScsWork **w, const scs_float **gx_dev, const scs_float **gy_dev, const scs_float **gs_dev, scs_float **db_dev,
                                      scs_float **dc_dev, scs_float *dAx_sum_dev, scs_float *dPx_sum_dev, const ScsHipDiffOpts *opts,
                                      ScsHipDiffInfo **info, scs_int count) {
  return adjoint_shared_entry(w, gx_dev, gy_dev, gs_dev, db_dev, dc_dev, dAx_sum_dev, dPx_sum_dev, opts, info, count, /*dev=*/true,
                              "scs_hip_adjoint_shared_device");
}
scs_int scs_hip_adjoint_shared(ScsWork **w, const scs_float **gx, const scs_float **gy, const scs_float **gs, scs_float **db, scs_float **dc,
                               scs_float *dAx_sum, scs_float *dPx_sum, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count) {
  return adjoint_shared_entry(w, gx, gy, gs, db, dc, dAx_sum, dPx_sum, opts, info, count, /*dev=*/false, "scs_hip_adjoint_shared");
}
scs_int scs_hip_derivative_batch_device(ScsWork **w, const scs_float **db_dev, const scs_float **dc_dev, scs_float **dx_dev, scs_float **dy_dev,
                                        scs_float **ds_dev, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count) {
  return derivative_batch_entry(w, db_dev, dc_dev, nullptr, nullptr, dx_dev, dy_dev, ds_dev, opts, info, count, /*dev=*/true,
                                "scs_hip_derivative_batch_device");
}
scs_int scs_hip_derivative_full_batch_device(ScsWork **w, const scs_float **db_dev, const scs_float **dc_dev, const scs_float **dAx_dev,
                                             const scs_float **dPx_dev, scs_float **dx_dev, scs_float **dy_dev, scs_float **ds_dev,
                                             const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count) {
  return derivative_batch_entry(w, db_dev, dc_dev, dAx_dev, dPx_dev, dx_dev, dy_dev, ds_dev, opts, info, count, /*dev=*/true,
                                "scs_hip_derivative_full_batch_device");
}
scs_int scs_hip_derivative_full_batch(ScsWork **w, const scs_float **db, const scs_float **dc, const scs_float **dAx, const scs_float **dPx,
                                      scs_float **dx, scs_float **dy, scs_float **ds, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info,
                                      scs_int count) {
  return derivative_batch_entry(w, db, dc, dAx, dPx, dx, dy, ds, opts, info, count, /*dev=*/false, "scs_hip_derivative_full_batch");
}
scs_int scs_hip_derivative_batch(ScsWork **w, const scs_float **db, const scs_float **dc, scs_float **dx, scs_float **dy, scs_float **ds,
                                 const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count) {
  return derivative_batch_entry(w, db, dc, nullptr, nullptr, dx, dy, ds, opts, info, count, /*dev=*/false, "scs_hip_derivative_batch");
}

// ---- Newton polish of the resident solution (include/scs_hip.h; csrc/refine.hpp) ----
// locking, device selection and the scratch turn are diff_entry's; every refusal comes before device work
static scs_int refine_entry(ScsWork *w, ScsSolution *sol, const ScsHipRefineOpts *o, ScsHipRefineInfo *info, bool dev, const char *who) {
  if (!w) {
    set_last_error(std::string(who) + ": null workspace");
    return -1;
  }
  try {
    set_last_error("");
    std::lock_guard<std::mutex> lock(w->mtx);
    std::string why = diff_refusal(w);
    if (why.empty() && o && o->tol != o->tol) why = "tol is NaN";
    if (!why.empty()) throw std::runtime_error(std::string(who) + ": " + why);
    if (dev && sol) {
      if (sol->x) check_device_vector(sol->x, w->device, who, "sol_dev->x");
      if (sol->y) check_device_vector(sol->y, w->device, who, "sol_dev->y");
      if (sol->s) check_device_vector(sol->s, w->device, who, "sol_dev->s");
    }
    HIP_CHECK(hipSetDevice(w->device));
    ScsHipWork::ScratchTurn turn(w);
    refine_impl(w, o, info);
    if (sol && dev) {
      w->hand_over_solution(sol);
    } else if (sol) {
      if (sol->x) w->solx.download(sol->x, w->n, w->stream);
      if (sol->y) w->soly.download(sol->y, w->m, w->stream);
      if (sol->s) w->sols.download(sol->s, w->m, w->stream);
      HIP_CHECK(hipStreamSynchronize(w->stream));
    }
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}
scs_int scs_hip_refine(ScsWork *w, ScsSolution *sol, const ScsHipRefineOpts *opts, ScsHipRefineInfo *info) {
  return refine_entry(w, sol, opts, info, /*dev=*/false, "scs_hip_refine");
}
scs_int scs_hip_refine_device(ScsWork *w, ScsSolution *sol_dev, const ScsHipRefineOpts *opts, ScsHipRefineInfo *info) {
  return refine_entry(w, sol_dev, opts, info, /*dev=*/true, "scs_hip_refine_device");
}

// ---- the polish of a batch (include/scs_hip.h; csrc/refine_batch.hpp) ----
// Locking, stream redirection and grouping are diff_batch_entry's (plan_diff_batch with no matrix gradients requested); the refusals
// and each member's hand-over are refine_entry's.
static scs_int refine_batch_entry(ScsWork **works, ScsSolution **sols, const ScsHipRefineOpts *o, ScsHipRefineInfo **infos, scs_int count, bool dev,
                                  const char *who) {
  set_last_error("");
  if (!diff_batch_members_ok(works, count, who)) return -1;
  std::vector<std::unique_lock<std::mutex>> locks;
  std::vector<hipStream_t> saved;
  std::vector<int> restored;
  scs_int rc = 0;
  try {
    {  // member mutexes in ADDRESS order (as diff_batch_entry)
      std::vector<int> order((size_t)count);
      std::iota(order.begin(), order.end(), 0);
      std::sort(order.begin(), order.end(), [&](int a, int b) { return std::less<ScsHipWork *>()(works[a], works[b]); });
      for (int j : order) locks.emplace_back(works[j]->mtx);
    }
    // every member's refusals, before any device work
    for (int i = 0; i < count; ++i) {
      const ScsHipWork *w = works[i];
      const std::string member = std::string(who) + ": member " + std::to_string(i);
      std::string why = diff_refusal(w);
      if (why.empty() && w->device != works[0]->device) why = "the members of a batch live on one device";
      if (why.empty() && o && o->tol != o->tol) why = "tol is NaN";
      if (!why.empty()) throw std::runtime_error(member + ": " + why);
      const ScsSolution *sol = sols ? sols[i] : nullptr;
      if (dev && sol) {
        if (sol->x) check_device_vector(sol->x, w->device, member.c_str(), "sol_dev->x");
        if (sol->y) check_device_vector(sol->y, w->device, member.c_str(), "sol_dev->y");
        if (sol->s) check_device_vector(sol->s, w->device, member.c_str(), "sol_dev->s");
      }
    }
    HIP_CHECK(hipSetDevice(works[0]->device));
    hipStream_t s = works[0]->stream;
    const std::vector<int> want((size_t)count, 0);
    for (const std::vector<int> &job : plan_diff_batch(works, (int)count, want)) {
      if (job.size() == 1) {
        ScsHipWork *w = works[job[0]];
        ScsHipWork::ScratchTurn turn(w);
        refine_impl(w, o, infos ? infos[job[0]] : nullptr);
        continue;
      }
      GroupRefine gr;
      gr.gd.s = s;
      for (int j : job) {  // every member's kernels go to the group's stream for the duration of the call
        saved.push_back(works[j]->stream);
        restored.push_back(j);
        works[j]->stream = s;
      }
      for (int j : job) {
        refine_alloc(works[j]);
        gr.gd.W.push_back(works[j]);
        gr.infos.push_back(infos ? infos[j] : nullptr);
      }
      gr.run(o);
      for (size_t k = 0; k < restored.size(); ++k) works[restored[k]]->stream = saved[k];
      saved.clear();
      restored.clear();
    }
    // the hand-over of refine_entry, member by member
    for (int i = 0; i < count; ++i) {
      ScsHipWork *w = works[i];
      ScsSolution *sol = sols ? sols[i] : nullptr;
      if (!sol) continue;
      if (dev) {
        w->hand_over_solution(sol);
      } else {
        if (sol->x) w->solx.download(sol->x, w->n, w->stream);
        if (sol->y) w->soly.download(sol->y, w->m, w->stream);
        if (sol->s) w->sols.download(sol->s, w->m, w->stream);
        HIP_CHECK(hipStreamSynchronize(w->stream));
      }
    }
  } catch (const std::exception &e) {
    set_last_error(e.what());
    rc = -1;
  }
  for (size_t k = 0; k < restored.size(); ++k) works[restored[k]]->stream = saved[k];
  return rc;
}
scs_int scs_hip_refine_batch(ScsWork **w, ScsSolution **sol, const ScsHipRefineOpts *opts, ScsHipRefineInfo **info, scs_int count) {
  return refine_batch_entry(w, sol, opts, info, count, /*dev=*/false, "scs_hip_refine_batch");
}
scs_int scs_hip_refine_batch_device(ScsWork **w, ScsSolution **sol_dev, const ScsHipRefineOpts *opts, ScsHipRefineInfo **info, scs_int count) {
  return refine_batch_entry(w, sol_dev, opts, info, count, /*dev=*/true, "scs_hip_refine_batch_device");
}

// ---- several directions at one solution (include/scs_hip.h; lanes: csrc/lsqr.hpp, csrc/diff_batch.hpp, csrc/spmv_lanes.hpp) ----
int scs_hip_diff_lane_tile(int tile) {
  if (tile == 4 || tile == 8) return g_diff_lane_tile.exchange(tile);
  return g_diff_lane_tile.load();
}
// base: the call of direction 0 — row 0 of every array.  Direction k reads and writes row k.
static scs_int diff_multi_entry(ScsWork *w, scs_int K, DiffCall base, const ScsHipDiffOpts *o, ScsHipDiffInfo *infos, bool dev, const char *who) {
  if (!w) {
    set_last_error(std::string(who) + ": null workspace");
    return -1;
  }
  try {
    set_last_error("");
    std::lock_guard<std::mutex> lock(w->mtx);
    diff_check(w, base, /*dev=*/false, who);
    if (K < 1) throw std::runtime_error(std::string(who) + ": K = " + std::to_string((long)K) + ": at least one direction");
    if (K > kDiffLanesMax)
      throw std::runtime_error(std::string(who) + ": K = " + std::to_string((long)K) + " exceeds the limit of " + std::to_string(kDiffLanesMax) +
                               " directions per call");
    if (dev) diff_check_device(w, base, who);
    HIP_CHECK(hipSetDevice(w->device));
    ScsHipWork::ScratchTurn turn(w);
    hipStream_t s = w->stream;
    ArenaScope no_arena(nullptr);
    const size_t SK = (size_t)K;
    DevBuf<double> bin[3], bout[4];
    const DiffCall host = base;
    if (!dev) {  // the host twin: K rows of every array through the staging of the single entries (DiffStage), in one copy each
      for (int k = 0; k < 3; ++k)
        if (host.in[k]) {
          bin[k].upload(host.in[k], SK * (size_t)host.in_len(w, k), s);
          base.in[k] = bin[k].p;
        }
      for (int k = 0; k < 4; ++k)
        if (host.out[k]) {
          bout[k].alloc(std::max(SK * (size_t)host.out_len(w, k), (size_t)1));
          base.out[k] = bout[k].p;
        }
      HIP_CHECK(hipStreamSynchronize(s));
    }
    std::vector<DiffCall> calls(SK, base);
    for (size_t k = 0; k < SK; ++k) {
      for (int i = 0; i < 3; ++i)
        if (base.in[i]) calls[k].in[i] = base.in[i] + k * (size_t)base.in_len(w, i);
      for (int i = 0; i < 4; ++i)
        if (base.out[i]) calls[k].out[i] = base.out[i] + k * (size_t)base.out_len(w, i);
    }
    if (GroupDiff::member_ok(w)) {
      diff_alloc_lanes(w, (int)K);
      if (base.adjoint && base.out[3]) diff_build_tri(w);
      GroupDiff gd;
      gd.adjoint = base.adjoint;
      gd.s = s;
      gd.one_work = true;
      for (int k = 0; k < (int)K; ++k) {
        gd.W.push_back(w);
        gd.lane.push_back(k);
        gd.calls.push_back(calls[(size_t)k]);
        gd.infos.push_back(infos ? infos + k : nullptr);
      }
      gd.run(o);
    } else {  // layouts the lock-step path does not cover: one direction after the other on lane 0, same bits
      for (int k = 0; k < (int)K; ++k) diff_impl(w, calls[(size_t)k], o, infos ? infos + k : nullptr);
    }
    if (!dev) {
      for (int k = 0; k < 4; ++k)
        if (host.out[k]) bout[k].download(host.out[k], SK * (size_t)host.out_len(w, k), s);
      HIP_CHECK(hipStreamSynchronize(s));
    }
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}
scs_int scs_hip_adjoint_multi_device(ScsWork *w, scs_int K, const scs_float *GX_dev, const scs_float *GY_dev, const scs_float *GS_dev,
                                     scs_float *DB_dev, scs_float *DC_dev, scs_float *DAx_dev, scs_float *DPx_dev, const ScsHipDiffOpts *opts,
                                     ScsHipDiffInfo *infos) {
  return diff_multi_entry(w, K, adjoint_call(GX_dev, GY_dev, GS_dev, DB_dev, DC_dev, DAx_dev, DPx_dev), opts, infos, /*dev=*/true,
                          "scs_hip_adjoint_multi_device");
}
scs_int scs_hip_adjoint_multi(ScsWork *w, scs_int K, const scs_float *GX, const scs_float *GY, const scs_float *GS, scs_float *DB, scs_float *DC,
                              scs_float *DAx, scs_float *DPx, const ScsHipDiffOpts *opts, ScsHipDiffInfo *infos) {
  return diff_multi_entry(w, K, adjoint_call(GX, GY, GS, DB, DC, DAx, DPx), opts, infos, /*dev=*/false, "scs_hip_adjoint_multi");
}
scs_int scs_hip_derivative_multi_device(ScsWork *w, scs_int K, const scs_float *DB_dev, const scs_float *DC_dev, scs_float *DX_dev,
                                        scs_float *DY_dev, scs_float *DS_dev, const ScsHipDiffOpts *opts, ScsHipDiffInfo *infos) {
  return diff_multi_entry(w, K, derivative_call(DB_dev, DC_dev, nullptr, nullptr, DX_dev, DY_dev, DS_dev), opts, infos, /*dev=*/true,
                          "scs_hip_derivative_multi_device");
}
scs_int scs_hip_derivative_multi(ScsWork *w, scs_int K, const scs_float *DB, const scs_float *DC, scs_float *DX, scs_float *DY, scs_float *DS,
                                 const ScsHipDiffOpts *opts, ScsHipDiffInfo *infos) {
  return diff_multi_entry(w, K, derivative_call(DB, DC, nullptr, nullptr, DX, DY, DS), opts, infos, /*dev=*/false, "scs_hip_derivative_multi");
}

void scs_finish(ScsWork *w) {
  if (!w) return;
  try {
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
  } catch (...) {
  }
  delete w;
}

void scs_set_default_settings(ScsSettings *s) {
  // defaults: R:README.md:98-104 (AA); R:test/test_warm_start_consistency.py:228-241 (scale, rho_x, alpha);
  // banner R:notebooks/scs_benchmarks.ipynb cell 2 (eps, max_iters, normalize, adaptive_scale)
  s->normalize = 1;
  s->scale = 0.1;
  s->adaptive_scale = 1;
  s->rho_x = 1e-6;
  s->max_iters = 100000;
  s->eps_abs = 1e-4;
  s->eps_rel = 1e-4;
  s->eps_infeas = 1e-7;
  s->alpha = 1.5;
  s->time_limit_secs = 0.;
  s->verbose = 1;
  s->warm_start = 0;
  s->acceleration_lookback = 10;
  s->acceleration_interval = 10;
  s->acceleration_type_1 = 1;
  s->acceleration_regularization = 1e-8;
  s->acceleration_relaxation = 1.0;
  s->write_data_filename = nullptr;
  s->log_csv_filename = nullptr;
}

const char *scs_version(void) { return "3.2.11"; }
size_t scs_sizeof_int(void) { return sizeof(scs_int); }
size_t scs_sizeof_float(void) { return sizeof(scs_float); }

int scs_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int scs_hip_set_device(int dev) {
  int n = scs_hip_device_count();
  if (dev < 0 || dev >= n) return -1;
  g_default_device.store(dev);
  return 0;
}
int scs_hip_set_thread_device(int dev) {
  if (dev < 0) { t_device = -1; return 0; }
  if (dev >= scs_hip_device_count()) return -1;
  t_device = dev;
  return 0;
}
int scs_hip_labs_build(void) { return kLabsBuild ? 1 : 0; }
int scs_hip_mem_info(size_t *free_bytes, size_t *total_bytes) {
  if (scs_hip_device_count() <= 0) return -1;
  size_t f = 0, t = 0;
  if (hipSetDevice(current_device()) != hipSuccess || hipMemGetInfo(&f, &t) != hipSuccess) return -1;
  if (free_bytes) *free_bytes = f + DevPool::inst().held_bytes();
  if (total_bytes) *total_bytes = t;
  return 0;
}
const char *scs_hip_last_error(void) { return g_last_error.c_str(); }

/* reps back-to-back launches of K1, of K2 and (QPs) of K3 on the solver's own stream and resident data, one HIP event
 * pair around each batch (event overhead amortised); out = {K1 avg ms, K2 avg ms, K3 avg ms inside the CG step's sequence, K3 back to back}
 * (K3: 0 without P) */
int scs_hip_time_matvec(ScsWork *w, int reps, double *out) {
  if (!w || !out || reps <= 0) return -1;
  try {
    std::lock_guard<std::mutex> lock(w->mtx);
    HIP_CHECK(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    ScsHipWork::ScratchTurn turn(w);
    w->finish_pending_setup();  // (R lives in the products)
    // the products exactly as the CG step of this workspace launches them
    for (int i = 0; i < 2; ++i) w->matvec(w->cg_p.p, nullptr);
    HIP_CHECK(hipEventRecord(w->ev[0], s));
    for (int i = 0; i < reps; ++i) launch_spmv(w->Ar.view(), w->cg_p.p, EpiDivR{w->tmp_m.p, w->rdy()}, nullptr, s);
    HIP_CHECK(hipEventRecord(w->ev[1], s));
    for (int i = 0; i < reps; ++i)
      launch_spmv(w->At.view(), w->tmp_m.p, EpiGp{w->cg_Gp.p, w->cg_p.p, w->rdx(), w->has_P ? 1 : 0, w->part.p, w->gp2()}, nullptr, s);
    HIP_CHECK(hipEventRecord(w->ev[2], s));
    HIP_CHECK(hipEventSynchronize(w->ev[2]));
    float a = 0, b = 0, c = 0;
    HIP_CHECK(hipEventElapsedTime(&a, w->ev[0], w->ev[1]));
    HIP_CHECK(hipEventElapsedTime(&b, w->ev[1], w->ev[2]));
    float c2 = 0;
    if (w->has_P) {  // K3: Gp = P p (csrc/spmv*.hpp on the full symmetric CSR of P, epilogue EpiStore)
      // (i) back to back: Pf alone (224 MB at the bench's target_qp) stays in the 256 MB Infinity Cache between launches — flattering;
      HIP_CHECK(hipEventRecord(w->ev[0], s));
      for (int i = 0; i < reps; ++i) launch_spmv(w->Pf.view(), w->cg_p.p, EpiStore{w->cg_Gp.p, 0}, nullptr, s);
      HIP_CHECK(hipEventRecord(w->ev[1], s));
      // (ii) as the CG step runs it, between K1 and K2, which stream 240 MB each: (K1, K3, K2) x reps minus (K1, K2) x reps
      for (int i = 0; i < reps; ++i) w->matvec(w->cg_p.p, nullptr);
      HIP_CHECK(hipEventRecord(w->ev[2], s));
      HIP_CHECK(hipEventSynchronize(w->ev[2]));
      HIP_CHECK(hipEventElapsedTime(&c, w->ev[0], w->ev[1]));
      float t_all = 0, t_12 = 0;
      HIP_CHECK(hipEventElapsedTime(&t_all, w->ev[1], w->ev[2]));
      HIP_CHECK(hipEventRecord(w->ev[0], s));
      for (int i = 0; i < reps; ++i) {
        launch_spmv(w->Ar.view(), w->cg_p.p, EpiDivR{w->tmp_m.p, w->rdy()}, nullptr, s);
        launch_spmv(w->At.view(), w->tmp_m.p, EpiGp{w->cg_Gp.p, w->cg_p.p, w->rdx(), 1, w->part.p, w->gp2()}, nullptr, s);
      }
      HIP_CHECK(hipEventRecord(w->ev[1], s));
      HIP_CHECK(hipEventSynchronize(w->ev[1]));
      HIP_CHECK(hipEventElapsedTime(&t_12, w->ev[0], w->ev[1]));
      c2 = t_all - t_12;
    }
    out[0] = a / reps;
    out[1] = b / reps;
    out[2] = c2 / reps;
    out[3] = c / reps;
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}

int scs_hip_solution_to_device(ScsWork *w, scs_float *x_dev, scs_float *y_dev, scs_float *s_dev) {
  if (!w) return -1;
  try {
    std::lock_guard<std::mutex> lock(w->mtx);
    if (!w->sol_on_device) throw std::runtime_error("no solution yet: call scs_solve first");
    HIP_CHECK(hipSetDevice(w->device));
    if (x_dev) HIP_CHECK(hipMemcpyAsync(x_dev, w->solx.p, sizeof(double) * w->n, hipMemcpyDeviceToDevice, w->stream));
    if (y_dev) HIP_CHECK(hipMemcpyAsync(y_dev, w->soly.p, sizeof(double) * w->m, hipMemcpyDeviceToDevice, w->stream));
    if (s_dev) HIP_CHECK(hipMemcpyAsync(s_dev, w->sols.p, sizeof(double) * w->m, hipMemcpyDeviceToDevice, w->stream));
    HIP_CHECK(hipStreamSynchronize(w->stream));
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}

void scs_hip_set_mark(ScsWork *w, int iter) {
  if (w) w->mark_iter = iter;
}
void scs_hip_get_mark(const ScsWork *w, double *out) {
  if (!w || !out) return;
  out[0] = w->mark_ms; out[1] = (double)w->mark_cg; out[2] = (double)w->mark_aa_calls; out[3] = (double)w->mark_aa_accept;
}

/* bench.py --workload config4_psd: average duration of one batched PSD projection (K9, all s-cones of the problem) on the
 * solver's own stream and resident state — the current dual iterate is copied to a scratch vector and projected `reps`
 * times (warm-started eigenvectors, as inside the ADMM loop); the copies are timed separately and subtracted.
 * out[4] = {ms per projection, number of matrices, largest order, flops of a LAPACK-style eigensolve of them all
 * (16/3 n^3 + 2 n^3 per matrix)}.  Returns 0 on success, 1 when the problem has no PSD cone. */
long scs_hip_spin_fallbacks(void) { return g_spin_fallbacks.load(); }
long scs_hip_tiled_launches(void) { return g_tiled_launches.load(); }

void scs_hip_trim_pool(void) { DevPool::inst().trim(); }
void scs_hip_pool_stats(ScsHipPoolStats *out) { if (out) DevPool::inst().stats(out); }

int scs_hip_psd_refine_stats(ScsWork *w, double *out, int cap) {
  if (!w || !out || cap < 0) return -1;
  try {
    std::lock_guard<std::mutex> lock(w->mtx);
    HIP_CHECK(hipSetDevice(w->device));
    HIP_CHECK(hipStreamSynchronize(w->stream));
    const int cnt = std::min(cap, w->n_psd_big);
    for (int c = 0; c < cnt; ++c) {
      double st[kPsdStateDoubles];
      const long at = w->psd_woff_h[(size_t)c] + psd_scratch_doubles(w->psd_order_h[(size_t)c]) - kPsdStateDoubles;
      HIP_CHECK(hipMemcpy(st, w->psd_scratch.p + at, sizeof st, hipMemcpyDeviceToHost));
      out[8 * c + 0] = st[9];
      out[8 * c + 1] = st[10];
      out[8 * c + 2] = st[8];
      out[8 * c + 3] = st[11];
      out[8 * c + 4] = st[7];
      out[8 * c + 5] = st[12];
      out[8 * c + 6] = st[13];
      out[8 * c + 7] = st[14];
    }
    return cnt;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}

int scs_hip_time_psd(ScsWork *w, int reps, double *out) {
  if (!w || !out || reps <= 0) return -1;
  try {
    std::lock_guard<std::mutex> lock(w->mtx);
    HIP_CHECK(hipSetDevice(w->device));
    if (w->n_psd <= 0) return 1;
    hipStream_t s = w->stream;
    const size_t bytes = sizeof(double) * w->m;
    auto copy = [&] { HIP_CHECK(hipMemcpyAsync(w->tmp_m.p, w->u.p + w->n, bytes, hipMemcpyDeviceToDevice, s)); };
    for (int i = 0; i < 2; ++i) { copy(); w->launch_psd(w->tmp_m.p, w->psd_off.p, w->psd_order.p, w->psd_woff.p, w->n_psd, w->n_psd_big); }
    HIP_CHECK(hipEventRecord(w->ev[0], s));
    for (int i = 0; i < reps; ++i) copy();
    HIP_CHECK(hipEventRecord(w->ev[1], s));
    for (int i = 0; i < reps; ++i) { copy(); w->launch_psd(w->tmp_m.p, w->psd_off.p, w->psd_order.p, w->psd_woff.p, w->n_psd, w->n_psd_big); }
    HIP_CHECK(hipEventRecord(w->ev[2], s));
    HIP_CHECK(hipEventSynchronize(w->ev[2]));
    float a = 0, b = 0;
    HIP_CHECK(hipEventElapsedTime(&a, w->ev[0], w->ev[1]));
    HIP_CHECK(hipEventElapsedTime(&b, w->ev[1], w->ev[2]));
    double flops = 0.;
    int mx = 0;
    for (int sd : w->cone.s) { flops += (16. / 3. + 2.) * (double)sd * sd * sd; mx = std::max(mx, sd); }
    out[0] = (b - a) / reps;
    out[1] = (double)w->cone.s.size();
    out[2] = (double)mx;
    out[3] = flops;
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}

int scs_hip_time_dproj(ScsWork *w, int reps, double *out) {
  if (!w || !out || reps <= 0) return -1;
  try {
    set_last_error("");
    std::lock_guard<std::mutex> lock(w->mtx);
    const std::string why = diff_refusal(w);
    if (!why.empty()) throw std::runtime_error("scs_hip_time_dproj: " + why);
    HIP_CHECK(hipSetDevice(w->device));
    ScsHipWork::ScratchTurn turn(w);
    hipStream_t s = w->stream;
    const int m = w->m;
    diff_alloc(w);
    DiffScratch &d = w->diff;
    const double *D = w->normalized ? w->D.p : nullptr;
    hipLaunchKernelGGL(k_dproj_vhat, dim3(vec_blocks(m)), dim3(kVecThreads), 0, s, (const double *)w->sols.p, (const double *)w->soly.p, D,
                       w->normalized ? w->scal.sigma : 1.0, m, d.vhat.p);
    const DprojPlan plan = diff_plan(w);  // (of which vh, box and sym3 are read below)
    // the two-launch form needs the partial slots whatever the size: scratch of this call when the workspace holds the short state
    ArenaScope no_arena(nullptr);
    DevBuf<double> st_big;
    DevBuf<unsigned> ticket;
    DprojBoxPlan multi = plan.box;
    if (plan.box.bsize > 0 && !plan.box.multi()) {
      st_big.alloc((size_t)DB_STATE + 3 * kBoxMultiMaxWgs);
      ticket.alloc_zero(1, s);
      multi.st = st_big.p; multi.ticket = ticket.p;
    }
    launch_dbox_prep(plan.box, plan.vh, s);
    launch_dsym3_prep(plan.sym3, plan.vh, s);
    if (st_big.p) HIP_CHECK(hipMemcpyAsync(st_big.p, plan.box.st, sizeof(double) * DB_STATE, hipMemcpyDeviceToDevice, s));
    const DprojIo io{d.uh.p + w->n, nullptr, d.dW.p, d.dWmI.p};  // (any m-vector serves as u)
    HIP_CHECK(hipMemsetAsync(d.uh.p, 0, sizeof(double) * ((size_t)w->n + m), s));
    auto timed = [&](auto &&body) {
      for (int i = 0; i < 2; ++i) body();
      HIP_CHECK(hipEventRecord(w->ev[0], s));
      for (int i = 0; i < reps; ++i) body();
      HIP_CHECK(hipEventRecord(w->ev[1], s));
      HIP_CHECK(hipEventSynchronize(w->ev[1]));
      HIP_CHECK(hipGetLastError());
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, w->ev[0], w->ev[1]));
      return (double)ms / reps;
    };
    for (int i = 0; i < 8; ++i) out[i] = 0.;
    const DprojBoxPlan &b = plan.box;
    if (b.bsize > 1) {
      const double *vb = plan.vh + b.off;
      const int wgs = box_multi_wgs(b.bsize);
      out[0] = timed([&] { hipLaunchKernelGGL(k_dbox, dim3(1), dim3(kBoxThreads), 0, s, io, vb, b.bl, b.bu, b.bsize, b.off, (const double *)b.st,
                                              (const int *)nullptr); });
      out[1] = timed([&] {
        hipLaunchKernelGGL(k_dbox_part, dim3(wgs), dim3(kBoxMultiThreads), 0, s, io, vb, b.bl, b.bu, b.bsize, b.off, (const double *)multi.st, 0,
                           multi.parts(), (const int *)nullptr);
        hipLaunchKernelGGL(k_dbox_rows, dim3(wgs), dim3(kBoxMultiThreads), 0, s, io, vb, b.bl, b.bu, b.bsize, b.off, (const double *)multi.st,
                           (const double *)multi.parts(), wgs, (const int *)nullptr);
      });
      // one projection of the same cone, in the form a solve uses at this size, on the scratch copy and this call's own t
      double *tw = multi.st + DB_STOP + 1;  // (a free slot of the state)
      const double one = 1.0;
      HIP_CHECK(hipMemcpyAsync(tw, &one, sizeof(double), hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (b.bsize > kBoxMultiMin)
        out[2] = timed([&] {
          for (int round = 0; round < kBoxRounds; ++round)
            hipLaunchKernelGGL(k_proj_box_round, dim3(wgs), dim3(kBoxMultiThreads), 0, s, vb, b.bl, b.bu, b.bsize, multi.st, multi.round_parts(),
                               multi.ticket, 0, round, (const int *)nullptr);
          hipLaunchKernelGGL(k_proj_box_apply, dim3(wgs), dim3(kBoxMultiThreads), 0, s, b.tmp, b.bl, b.bu, b.bsize, multi.st, 0, (const int *)nullptr);
        });
      else
        out[2] = timed([&] { hipLaunchKernelGGL(k_proj_box, dim3(1), dim3(kBoxThreads), 0, s, b.tmp, b.bl, b.bu, b.bsize, tw, 0, (const int *)nullptr); });
      out[3] = (double)b.bsize;
    }
    const DprojSym3Plan &p3 = plan.sym3;
    if (p3.count > 0) {
      out[4] = timed([&] { launch_dsym3(p3, io, nullptr, s); });
      out[5] = timed([&] { launch_dsym3_prep(p3, plan.vh, s); });
      HIP_CHECK(hipMemcpyAsync(d.dW.p + p3.off, plan.vh + p3.off, sizeof(double) * 3 * (size_t)p3.count, hipMemcpyDeviceToDevice, s));
      out[6] = timed([&] { hipLaunchKernelGGL(k_proj_pow_primal, dim3(ceil_div(p3.count, kConeThreads)), dim3(kConeThreads), 0, s, d.dW.p + p3.off, p3.a,
                                              p3.count, (const int *)nullptr); });
      out[7] = (double)p3.count;
    }
    HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return -1;
  }
}

void scs_hip_set_profiling(ScsWork *w, int on) {
  if (w) w->profile = on != 0;
}
void scs_hip_kernel_times(const ScsWork *w, double *out) {
  if (!w || !out) return;
  out[0] = w->prof_ms[0]; out[1] = (double)w->prof_n[0];
  out[2] = w->prof_ms[1]; out[3] = (double)w->prof_n[1];
  out[4] = (double)w->At.nnz; out[5] = (double)w->Ar.nwg(); out[6] = (double)w->At.nwg();
  out[7] = w->has_P ? (double)w->Pf.nnz : 0.0;
  out[8] = w->prof_cone_ms; out[9] = (double)w->prof_cone_n;
  out[10] = w->prof_ms[2]; out[11] = (double)w->prof_n[2];
}

#include "lab_entries.hpp"

}  // extern "C"

