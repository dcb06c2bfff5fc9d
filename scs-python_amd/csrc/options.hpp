// options.hpp — every environment variable the library reads, in ONE place (round 6).
//
// The product has 17 runtime knobs (INTEGRATION.md "Runtime knobs"; the Python loader adds SCS_HIP_LIB, SCS_HIP_RUNTIME and shares
// SCS_HIP_RUNTIME_ENV).  They are parsed HERE (refresh_options(): a test may change the environment between two workspaces of one
// process), never at the point of use, and every reader is handed the struct it reads:
//   per workspace   scs_init takes opts() once, right after refresh_options(), and the matrix set keeps that snapshot (work.hpp
//                   MatrixSet::opt, ScsHipWork::opt).  Layouts, cone pipelines, the Anderson factorisation, run-ahead and diagnostics of
//                   the workspace read it for good; scs_hip_clone shares the set and with it the snapshot; scs_hip_update_matrix re-derives
//                   layouts under it.  A solve re-reads nothing: no setenv and no other thread's scs_init changes a live workspace.
//   per batch call  what spans workspaces — SCS_HIP_DEBUG=group, SCS_HIP_SHARED_TILE (labs) — is read once by scs_hip_solve_batch
//                   (and its device twin) and handed down (batch.hpp GroupSolve::opt); the kernel-level entry points (lab_entries.hpp) hand
//                   theirs to the temporary objects they build.
//   process-wide    SCS_HIP_STREAMS, SCS_HIP_POOL_MB, SCS_HIP_CTRLC, SCS_HIP_RUNTIME_ENV (read once where they are used) and, labs,
//                   SCS_HIP_POOL_POISON (the block pool is the process's: common.hpp DevPool::get reads the global).
// Everything else that rounds 1-5 could switch at run time — the experiments that lost and still have code (cooperative launches, the
// in-kernel combine of split layouts ...) and the lab switches of the kernels — is a compile-time default in
// the product and only reads the environment in the `-DSCS_HIP_LABS` build (scs-python_amd/Makefile `make labs` -> libscs_hip_labs.so,
// used by tools/ and by the tests marked `labs`).  Four closed experiments of the CG path, the older schedules of the column-sorted
// SpMV and the lab switches nothing set any more have no code: DESIGN.md §4, its column-sorted SpMV section and "Retired lab switches".
#pragma once
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

extern char **environ;

namespace scship {

enum : unsigned { DBG_PIPE = 1u, DBG_GROUP = 2u, DBG_SETUP = 4u, DBG_TOL = 8u };

struct Options {
  // ------------------------------------------------------------------ product knobs (per workspace; `debug` group: per batch call)
  bool pipeline = true;        // SCS_HIP_PIPELINE=0: the host looks at the CG flags in every iteration (no run-ahead)
  int pipe_chunk = 0;          // SCS_HIP_PIPELINE=N (N >= 2): run-ahead with CG chunks of N steps (tests: forces stalls)
  bool host_setup = false;     // SCS_HIP_SETUP=host: transposition / layout builders on the host (fallback, entry-for-entry identical)
  bool lazy_setup = true;      // SCS_HIP_LAZY_SETUP=0: small problems finish R, the preconditioner / G^-1 and g inside scs_init
  bool cs = true;              // SCS_HIP_CS=0: never the column-sorted pass layout (slab / CSR-stream kernels)
  long cs_min_nnz = 1L << 20;  // SCS_HIP_CS=N (N >= 2): the pass layout from N nonzeros on (tests on small matrices)
  bool cs_split = true;        // SCS_HIP_CS_SPLIT=0: one workgroup per row chunk for A' too (bit-exact sequential row sums)
  bool slab = true;            // SCS_HIP_SLAB=0: no L2-blocked slab copy (and no pass layout): the plain CSR-stream kernel
  bool aa_gram = false;        // SCS_HIP_AA=gram: Anderson acceleration through the Gram matrix + host LU instead of the TSQR
  int psd_split = -1;          // SCS_HIP_PSD_SPLIT=0|1: force the one-launch / the split pipeline of the PSD projection
  int psd_mc = -1;             // SCS_HIP_PSD_MC=G: workgroups per matrix of the multi-CU sweep kernel (1: never spin)
  bool psd_refine = true;      // SCS_HIP_PSD_REFINE=0: strict Jacobi sweeps only (bit-identical to the one-launch kernel)
  bool psd_tol_adaptive = true;  // SCS_HIP_PSD_TOL=fixed: sweeps always to 1e-8
  int spin_budget_log2 = 25;   // SCS_HIP_SPIN_BUDGET_LOG2: barrier polls before a spinning kernel gives up (tests: 0)
  bool linsys_dense = false;   // SCS_HIP_LINSYS=dense: the bare C entry scs_init builds the dense direct solver
  unsigned debug = 0;          // SCS_HIP_DEBUG=pipe,group,setup,tol: diagnostics on stderr
  // (process-wide, read once where they are used: SCS_HIP_STREAMS, SCS_HIP_POOL_MB, SCS_HIP_CTRLC, SCS_HIP_RUNTIME_ENV)

  // ------------------------------------------------------------------ labs (compile-time defaults in the product)
  bool psd_coop = false;       // hipLaunchCooperativeKernel for the multi-CU sweeps: ~2 ms per launch in a warm process
  bool cs_combine = false;     // in-kernel combine of split layouts: eats the gather gain
  int cs_rpt = 0, cs_split_a = 0, cs_split_at = 0;
  bool cs_peel = true, cs_virt = true;
  bool cg_fuse = true, norm_fuse = true, soc_psd_fuse = true;
  double psd_tol_k = 1e-2;
  bool psd_la = true, psd_mc_nocheck = false;
  bool pool_poison = false;     // (process-wide: the block pool is shared by every workspace)
  bool shared_tile = false;    // SCS_HIP_SHARED_TILE=1: members of a group on one matrix set read it once per tile of four (batch.hpp
                               // k_spmv_stream_tiled) instead of per-member launches over the shared storage; not measured to win yet

  static bool is0(const char *e) { return e && e[0] == '0'; }
  static bool is1(const char *e) { return e && e[0] == '1'; }
  static Options parse() {
    Options o;
    if (const char *e = getenv("SCS_HIP_PIPELINE")) {
      const int v = atoi(e);
      o.pipeline = !is0(e);
      o.pipe_chunk = v >= 2 ? v : 0;
    }
    if (const char *e = getenv("SCS_HIP_SETUP")) o.host_setup = e[0] == 'h';
    o.lazy_setup = !is0(getenv("SCS_HIP_LAZY_SETUP"));
    if (const char *e = getenv("SCS_HIP_CS")) {
      const long v = atol(e);
      o.cs = !is0(e);
      if (v >= 2) o.cs_min_nnz = v;
    }
    o.cs_split = !is0(getenv("SCS_HIP_CS_SPLIT"));
    o.slab = !is0(getenv("SCS_HIP_SLAB"));
    if (const char *e = getenv("SCS_HIP_AA")) o.aa_gram = e[0] == 'g';
    if (const char *e = getenv("SCS_HIP_PSD_SPLIT")) o.psd_split = e[0] == '1' ? 1 : 0;
    if (const char *e = getenv("SCS_HIP_PSD_MC")) o.psd_mc = atoi(e);
    o.psd_refine = !is0(getenv("SCS_HIP_PSD_REFINE"));
    if (const char *e = getenv("SCS_HIP_PSD_TOL")) o.psd_tol_adaptive = e[0] != 'f';
    if (const char *e = getenv("SCS_HIP_SPIN_BUDGET_LOG2")) { const int v = atoi(e); o.spin_budget_log2 = v < 0 ? 0 : (v > 40 ? 40 : v); }
    if (const char *e = getenv("SCS_HIP_LINSYS")) o.linsys_dense = e[0] == 'd' || e[0] == 'D';
    if (const char *e = getenv("SCS_HIP_DEBUG")) {
      if (strstr(e, "pipe")) o.debug |= DBG_PIPE;
      if (strstr(e, "group")) o.debug |= DBG_GROUP;
      if (strstr(e, "setup")) o.debug |= DBG_SETUP;
      if (strstr(e, "tol")) o.debug |= DBG_TOL;
      if (strstr(e, "all")) o.debug = ~0u;
    }
#ifdef SCS_HIP_LABS
    auto pos_int = [](const char *name, int dflt) { const char *e = getenv(name); const int v = e ? atoi(e) : 0; return v > 0 ? v : dflt; };
    auto pos_dbl = [](const char *name, double dflt) { const char *e = getenv(name); const double v = e ? atof(e) : 0.; return v > 0. ? v : dflt; };
    o.psd_coop = is1(getenv("SCS_HIP_PSD_COOP"));
    o.cs_combine = is1(getenv("SCS_HIP_CS_COMBINE"));
    { const int v = pos_int("SCS_HIP_CS_RPT", 0); o.cs_rpt = (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) ? v : 0; }  // full chunks of 1024 * rpt rows
    o.cs_split_a = pos_int("SCS_HIP_CS_SPLIT_A", 0);
    o.cs_split_at = pos_int("SCS_HIP_CS_SPLIT_AT", 0);
    o.cs_peel = !is0(getenv("SCS_HIP_CS_PEEL"));
    o.cs_virt = !is0(getenv("SCS_HIP_CS_VIRT"));
    o.cg_fuse = !is0(getenv("SCS_HIP_CG_FUSE"));
    o.norm_fuse = !is0(getenv("SCS_HIP_NORM_FUSE"));
    o.soc_psd_fuse = !is0(getenv("SCS_HIP_SOC_PSD_FUSE"));
    o.psd_tol_k = pos_dbl("SCS_HIP_PSD_TOL_K", 1e-2);
    o.psd_la = !is0(getenv("SCS_HIP_PSD_LA"));
    o.psd_mc_nocheck = getenv("SCS_HIP_PSD_MC_NOCHECK") != nullptr;
    o.pool_poison = is1(getenv("SCS_HIP_POOL_POISON"));
    if (const char *e = getenv("SCS_HIP_SHARED_TILE")) o.shared_tile = e[0] != '0';
#endif
    return o;
  }
};

// The current options live behind an atomic pointer: readers (opts(), anywhere, any thread) never see a half-written struct, and a
// reference they hold stays valid — a superseded struct is never freed (a few hundred bytes per CHANGE of the environment, which only
// tests make).
inline std::atomic<const Options *> &options_ptr() {
  static std::atomic<const Options *> p{new Options(Options::parse())};
  return p;
}
// what the NEXT workspace / batch call / kernel-level call takes its snapshot from (the environment as it was at the last
// refresh_options()).  Called in the bodies of the entry points only: everything below them reads the reference it was handed.
inline const Options &opts() { return *options_ptr().load(std::memory_order_acquire); }
// re-read the environment: first thing in scs_init, the batch entries and the kernel-level entry points that read options.  A new
// struct is only published when an SCS_HIP_* variable changed since the last call, so concurrent scs_init calls under one
// environment publish nothing.
inline void refresh_options() {
  static std::mutex m;
  static std::string last = "\x01";  // (never equal to a real signature: the first call publishes what it parsed)
  std::lock_guard<std::mutex> lk(m);  // (before the walk: two threads must not publish in the opposite order of what they read)
  std::string sig;
  for (char **e = environ; e && *e; ++e)
    if (std::strncmp(*e, "SCS_HIP_", 8) == 0) { sig += *e; sig += '\n'; }
  if (sig != last) {
    options_ptr().store(new Options(Options::parse()), std::memory_order_release);
    last = sig;
  }
}
#ifdef SCS_HIP_LABS
constexpr bool kLabsBuild = true;
#else
constexpr bool kLabsBuild = false;
#endif

}  // namespace scship
