// work.hpp — ScsHipWork: the workspace behind the C-ABI handle (device buffers, cone metadata and launches, spin chain, per-solve state); its member functions continue in the .inl files included at the end of the struct
// (one of the units csrc/scs_hip.hip is assembled from — ONE translation unit, in this order: runtime.hpp, device_csr.hpp, work.hpp
// [+ work_linsys.inl, work_admm.inl, work_residuals.inl, work_solve_ends.inl], io.hpp, setup.hpp, loop.hpp, batch.hpp, the C ABI in scs_hip.hip,
// lab_entries.hpp; split out of the 3 800-line file of rounds 1-5 in round 6 — VERDICT r05 item 6 — without moving a line of code)
#pragma once
using namespace scship;

static void write_csv_row(FILE *f, int iter, const Residuals &r, double scale, const double *diffs, double aa_norm,
                          double time_s);

// A spinning multi-workgroup kernel (k_psd_sweep_mc) gave up at a barrier: scs_solve restarts the solve without it
struct SpinTimeout : std::runtime_error {
  using std::runtime_error::runtime_error;
};
static std::atomic<long> g_spin_fallbacks{0};  // scs_hip_spin_fallbacks(): tests
// Spinning kernels need ALL their workgroups on the device at once.  One workspace alone sizes its grid for that; two workspaces of a
// device that launch such grids on different streams at the same time (threads with their own SCS objects: R:test/test_thread_safety.py:78-93)
// could each get half of theirs placed and wait for the other half for good.  So inside a process the spinning launches of a device
// form a chain: once more than one workspace of the device uses them, each launch waits for the event recorded behind the previous one
// (hipStreamWaitEvent: nothing on the host waits) and leaves its own.  A lone user pays nothing.
struct SpinChain {
  std::mutex mu;
  int users = 0;
  hipEvent_t last = nullptr;
  hipStream_t last_stream = nullptr;
};
static SpinChain &spin_chain(int device) {
  static SpinChain c[64];
  return c[device & 63];
}

// ============================================================== shared matrix set
// What a workspace holds that is a function of A, P, the cone boundaries and `normalize` alone: the resident layouts of A', A and P,
// the diagonal of P and the equilibration vectors.  It is written by scs_init and read-only from then on, so scs_hip_clone hands the
// SAME set to the workspace it makes: a clone allocates per-solve state only.  Reference-counted (std::shared_ptr); whichever user
// dies last releases it, inside its own pool window (~ScsHipWork).
struct MatrixSet {
  // the options the layouts were built under (options.hpp: taken once by scs_init; a superseded struct is never freed).  Whatever
  // re-derives a layout (matrix_update.hpp) and every workspace on the set — scs_hip_clone — reads this one, never the global.
  const Options &opt;
  explicit MatrixSet(const Options &o) : opt(o) {}
  std::shared_ptr<Arena> home;  // the arena of the workspace that built the set (FIRST member: destroyed last — the buffers below may live in it)
  DeviceCsr At, Ar, Pf;
  DevBuf<double> Pdiag, D, E;
  // what scs_hip_clone rebuilds the state of scs_init from: the data and settings scs_init was called with (scs_update moves b_orig / c_orig)
  std::vector<double> b0, c0, bl0, bu0;
  ScsSettings stgs0{};
  // scs_hip_update_matrix (matrix_update.hpp): nothing of this exists until the first call (ar / pf: or until the first derivative that
  // perturbs A / P, perturb.hpp, which builds the one it needs and no layout map; `built` = ALL maps of the set exist).  One int32 source index per stored value
  // slot of every resident form but A' (whose values ARE the caller's CSC order): -1 marks a padding slot.  ar / pf index the caller's
  // arrays, the layout maps the equilibrated CSR they were built from (cs of A': CSR(A); cs of A: CSR(A'); cs of P and every slab: own CSR).
  struct ValueMaps {
    bool built = false;
    DevBuf<int> ar, pf, at_cs, ar_cs, pf_cs, at_slab, ar_slab, pf_slab;
    // the caller's values as they arrived (staging of the host entry; with `normalize` and a P also the copy a later call that keeps
    // one matrix re-equilibrates from)
    DevBuf<double> raw_a, raw_p;
    bool raw_a_set = false, raw_p_set = false;
    size_t bytes() const {
      return sizeof(int) * (ar.n + pf.n + at_cs.n + ar_cs.n + pf_cs.n + at_slab.n + ar_slab.n + pf_slab.n) + sizeof(double) * (raw_a.n + raw_p.n);
    }
  } vmaps;
  long a_nnz_in = 0, p_nnz_in = 0;  // lengths of the value arrays scs_init was given (P: the triangle as passed)
  // why Px cannot be taken ("" = it can): the map of the full CSR(P) (matrix_update.hpp k_map_pf) pairs the k-th entry of a column of the
  // caller's triangle with the k-th lower entry of that row of the full matrix, which holds for an upper triangle with ascending
  // row indices in every column only.  scs_init accepts other P (entries below the diagonal are ignored, columns may be unsorted).
  std::string p_update_refusal;
  // host copies of those values, kept only where a matrix update may need them: `normalize` with a P (updating one matrix re-equilibrates
  // both from their raw values); moved to raw_a / raw_p by the first update
  std::vector<double> ax0, px0;
  // The column-sorted layouts keep scratch of a product inside the layout (partial row sums of split chunks, piece sums of virtual rows,
  // combine tickets).  Workspaces that share such a set take turns: one solve / update at a time (small problems — CSR-stream — have none).
  std::mutex scratch_mu;
  std::mutex maps_mu;  // around the one-time build of vmaps.ar / vmaps.pf (matrix_update.hpp build_csr_value_maps: clones may race for it)
  bool has_scratch() const { return At.cs.ok || Ar.cs.ok || Pf.cs.ok; }
};

// ============================================================== workspace
struct ScsHipWork {
  // first member = destroyed last: ends the window in which this workspace's device blocks go to the block pool (common.hpp DevPool)
  struct PoolWindowEnd {
    bool armed = false;
    ~PoolWindowEnd() { if (armed) --t_pool_release; }
  } pool_window_end;
  std::shared_ptr<Arena> arena;  // small problems: all device buffers of the workspace come from here (FIRST member: destroyed last; the matrix set holds it too)
  std::shared_ptr<MatrixSet> mats;  // behind the arena: released before it, inside the pool window
  explicit ScsHipWork(const Options &o) : mats(std::make_shared<MatrixSet>(o)) {}     // scs_init, the kernel-level entry points
  explicit ScsHipWork(std::shared_ptr<MatrixSet> shared) : mats(std::move(shared)) {}  // scs_hip_clone
  const Options &opt = mats->opt;  // the ONE options snapshot of this workspace, for its whole life: no member reads the process-global one
  struct ScratchTurn {  // around everything that launches products of this workspace's matrices outside a grouped solve
    std::unique_lock<std::mutex> lk;
    explicit ScratchTurn(ScsHipWork *w) { if (w->mats->has_scratch()) lk = std::unique_lock<std::mutex>(w->mats->scratch_mu); }
  };
  int device = 0;  // the HIP device this workspace (stream, buffers, events) lives on
  int n = 0, m = 0;
  long l = 0;
  ScsSettings stgs{};
  double scale = 0.1;
  HostCone cone;
  HostScaling scal;
  bool normalized = false, has_P = false;
  std::vector<double> b_orig, c_orig;
  double nm_b_orig = 0, nm_c_orig = 0;
  double setup_time = 0;
  std::string log_csv_filename, write_data_filename;

  hipStream_t stream = nullptr;
  bool pooled_stream = false, stream_shared = false;  // pooled_stream: a real workspace (scs_init: g_streams); the stack workspaces of the kernel-level entry points borrow theirs
  void *pinned_block = nullptr;  // all pinned host scalars / flags of the workspace (g_pinned)
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // [3]: behind K3 in a sampled CG step of a problem with P
  double *h_pin = nullptr;  // pinned scalars
  int *h_flags = nullptr;   // pinned flags
  double *h_params = nullptr, *d_params = nullptr;  // mapped pinned per-iteration scalars (P_*), slot in use (2 slots)
  double *h_params_base = nullptr, *d_params_base = nullptr;
  // run-ahead mode (see F_STALL in vec.hpp): plain iterations are enqueued whole and one ahead of the host's view
  // (both from `opt`, for real workspaces only: setup.hpp init_streams_and_pinned)
  bool pipelined = false;
  int pipe_chunk_override = 0, pipe_stalls = 0;  // tests: SCS_HIP_PIPELINE=N forces CG chunks of N steps (=> stalls)
  const int *stall = nullptr;      // fl + F_STALL while a run-ahead iteration is being enqueued, else nullptr
  int *stall_fl = nullptr;         // fl (or nullptr): k_tau_dots raises the stall, k_cone_pre parks the CG kernels
  int *h_flags_slot[2] = {nullptr, nullptr};
  hipEvent_t ev_iter[2] = {nullptr, nullptr};
  hipEvent_t ev_prof[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};  // in-situ K1 / K2 (/ K3) samples of the run-ahead loop
  int prof_step[2] = {-1, -1};  // CG step (0-based) bracketed by ev_prof[slot], -1 = none
  hipEvent_t ev_cone[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // in-situ: the cone kernels of a queued iteration
  bool cone_sampled[2] = {false, false};
  double prof_cone_ms = 0;
  long prof_cone_n = 0;

  // (the matrix set: shared with the clones of this workspace)
  DeviceCsr &At = mats->At;  // CSR(A') == caller's CSC(A): rows n, cols m   (x-space outputs)
  DeviceCsr &Ar = mats->Ar;  // CSR(A): rows m, cols n                        (y-space outputs)
  DeviceCsr &Pf = mats->Pf;  // full symmetric CSR(P)
  DevBuf<double> &Pdiag = mats->Pdiag;
  DevBuf<double> &D = mats->D, &E = mats->E;

  DevBuf<double> v, v_prev, u, ut, rsk, g, h, diag_r, Dinv, Einv;  // (Dinv / Einv carry sigma, which follows b and c: per workspace)
  DevBuf<double> cg_b, cg_p, cg_r, cg_Gp, cg_M, tmp_m, ws, px;
  DevBuf<double> part, part2, sc, out;  // part2: partials of k_cg_update (read by k_cg_dir while `part` is reused), of k_prep
  DevBuf<double> part_v;                // sum-of-squares partials of v for the next k_prep
  bool v_norm_fresh = false;
  DevBuf<int> fl;
  DevBuf<double> solx, soly, sols;
  bool sol_on_device = false;  // solx/soly/sols hold the final (x, y, s) of the last solve
  // derivatives of the solve (diff.hpp): whether solx / soly / sols can be differentiated — 0: no solve yet, 1: the last solve ended
  // solved and nothing changed since, 2: it did not end solved, 3: b, c or the matrix changed since (the resident solution is stale) —
  // and the scratch of those calls (nothing is allocated before the first one)
  int diff_state = 0, last_status_val = 0;
  void diff_mark_stale() { if (diff_state == 1) diff_state = 3; }
  DiffScratch diff;
  // device-resident endpoints (device_io.hpp, scs_hip_update_device): the caller's b / c as they arrived, allocated by the first device
  // update.  A vector lives where it was last written: *_raw_fresh = the device copy is current, *_host_stale = b_orig / c_orig is not
  // (scs_update with one NULL argument refreshes the mirror it keeps: refresh_host_bc)
  DevBuf<double> b_raw, c_raw;
  DevBuf<unsigned> io_ticket;  // k_bc_load's arrival counter (0 between launches)
  bool b_raw_fresh = false, c_raw_fresh = false, b_host_stale = false, c_host_stale = false;
  // large solutions leave through a pinned mirror owned by the workspace (the caller's arrays are never handed to the runtime,
  // see scs_hip_runtime_env): three DMA copies in flight, each array moved on by a few host threads as soon as it has landed
  double *sol_pin = nullptr;
  bool sol_pin_refused = false;
  hipEvent_t sol_ev[3] = {nullptr, nullptr, nullptr};
  static constexpr size_t kSolMirrorMin = (size_t)1 << 20;  // bytes of x | y | s from which the mirror is used
  static void spread_memcpy(void *dst, const void *src, size_t bytes) {
    const int nt = bytes >= ((size_t)8 << 20) ? 4 : 1;
    if (nt == 1) { std::memcpy(dst, src, bytes); return; }
    const size_t part = (bytes / nt + 4095) & ~(size_t)4095;
    std::thread th[3];
    for (int t = 1; t < nt; ++t) {
      const size_t o = std::min(bytes, part * t), c = std::min(bytes - o, part);
      th[t - 1] = std::thread([=] { if (c) std::memcpy((char *)dst + o, (const char *)src + o, c); });
    }
    std::memcpy(dst, src, std::min(bytes, part));
    for (int t = 1; t < nt; ++t) th[t - 1].join();
  }
  void ensure_solution_mirror() {  // (scs_init calls this: pinning 40 MB costs milliseconds)
    const size_t bytes = sizeof(double) * ((size_t)n + 2 * (size_t)m);
    if (sol_pin || sol_pin_refused || bytes < kSolMirrorMin) return;
    if (hipHostMalloc((void **)&sol_pin, bytes, hipHostMallocDefault) != hipSuccess) {  // (no pinned memory left: the runtime's own staging)
      (void)hipGetLastError();
      sol_pin = nullptr;
      sol_pin_refused = true;
      return;
    }
    for (auto &e : sol_ev) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  void download_solution(ScsSolution *sol) {
    ensure_solution_mirror();
    if (!sol_pin) {
      solx.download(sol->x, n, stream);
      soly.download(sol->y, m, stream);
      sols.download(sol->s, m, stream);
      HIP_CHECK(hipStreamSynchronize(stream));
      return;
    }
    double *hx = sol_pin, *hy = sol_pin + n, *hs = sol_pin + n + m;
    solx.download(hx, n, stream); HIP_CHECK(hipEventRecord(sol_ev[0], stream));
    soly.download(hy, m, stream); HIP_CHECK(hipEventRecord(sol_ev[1], stream));
    sols.download(hs, m, stream); HIP_CHECK(hipEventRecord(sol_ev[2], stream));
    HIP_CHECK(hipEventSynchronize(sol_ev[0])); spread_memcpy(sol->x, hx, sizeof(double) * n);
    HIP_CHECK(hipEventSynchronize(sol_ev[1])); spread_memcpy(sol->y, hy, sizeof(double) * m);
    HIP_CHECK(hipEventSynchronize(sol_ev[2])); spread_memcpy(sol->s, hs, sizeof(double) * m);
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  int part_len = 0;

  // cones
  DevBuf<int> soc_off, soc_dim, soc_big;
  int n_soc = 0, n_soc_big = 0, soc_G = 64;  // soc_G: lanes per cone in k_proj_soc_wave (cones.hpp soc_group)
  DevBuf<double> pow_a, box_bl, box_bu;
  DevBuf<double> box_bl_orig, box_bu_orig, box_parts;
  DevBuf<unsigned> cg_ticket;  // k_cg_update_dir's arrival counter (0 between launches)
  DevBuf<unsigned> box_ticket;  // the caller's bounds (the working copies follow the row scaling): footer diagnostics
  DevBuf<int> psd_off, psd_order;    // orders > kPsdSmallMax first (n_psd_big of them), then the small ones
  DevBuf<long> psd_woff;
  std::vector<long> psd_woff_h;  // host copies (scs_hip_psd_refine_stats)
  std::vector<int> psd_order_h;
  DevBuf<double> psd_scratch;
  int n_psd = 0, n_psd_big = 0;
  // split mode of the block kernel (psd.hpp): worth it when the large matrices alone leave most CUs idle
  static constexpr int kPsdSplitRounds = 2;  // x kPsdLogSweeps = 6 sweeps: a cold start needs ~9; the LAST round is the one behind the refinement stage
  bool psd_split = false;
  int psd_max_np = 0, psd_max_tiles = 0;
  // complex PSD cones: projected through the packed 2k x 2k real embedding held in cs_stage (psd.hpp)
  DevBuf<int> cs_off, cs_order, cs_poff, cs_porder;  // same ordering: embeddings of order > kPsdSmallMax first
  DevBuf<long> cs_soff, cs_woff;
  DevBuf<double> cs_stage;
  int n_cs = 0, n_cs_big = 0;
  // spectral cones (spectral.hpp): one SpecBatch per kind, uploaded by upload_cone_meta; everything else lives in LDS
  DevBuf<int> spec_meta;  // [ell1 off | n] [long ell1 off | n] [sl off | n | k] [d off | n] [nuc off | m | n]
  SpecBatch spec_ell1{}, spec_ell1_long{}, spec_sl{}, spec_d{}, spec_nuc{};
  size_t spec_sl_lds = 0, spec_d_lds = 0, spec_nuc_lds = 0;
  // one launch per kind (ell1: one for the short and one for the long cones), whatever the number of cones
  void launch_spectral(double *y, int dual) {
    if (spec_d.count > 0)
      hipLaunchKernelGGL(k_proj_eig_cone, dim3(spec_d.count), dim3(kSpecThreads), spec_d_lds, stream, y, spec_d, 1, dual, stall);
    if (spec_nuc.count > 0)
      hipLaunchKernelGGL(k_proj_nuc, dim3(spec_nuc.count), dim3(kSpecThreads), spec_nuc_lds, stream, y, spec_nuc, dual, stall);
    if (spec_ell1.count > 0)
      hipLaunchKernelGGL(k_proj_ell1, dim3(ceil_div(spec_ell1.count, kSpecThreads / kWave)), dim3(kSpecThreads), 0, stream, y, spec_ell1,
                         dual, stall);
    if (spec_ell1_long.count > 0)
      hipLaunchKernelGGL(k_proj_ell1_block, dim3(spec_ell1_long.count), dim3(kSpecEll1BlockThreads), 0, stream, y, spec_ell1_long, dual, stall);
    if (spec_sl.count > 0)
      hipLaunchKernelGGL(k_proj_eig_cone, dim3(spec_sl.count), dim3(kSpecThreads), spec_sl_lds, stream, y, spec_sl, 0, dual, stall);
  }

  // batched PSD projection of `count` packed matrices (the first `big` of order > kPsdSmallMax): K9 + its one-wave variant
  void launch_psd(double *base, const int *off, const int *order, const long *woff, int count, int big) {
    if (big > 0) {
      PsdBatch B{off, order, woff, big};
      if (psd_split) {
        // few large matrices: sweeps (A only) -> V updates over 16-row strips on the idle CUs -> reconstruction
        const int gper = psd_gemm_tasks(std::max(psd_max_tiles, 1));  // tasks (= workgroups of one wavefront) per matrix, dealt to the XCDs in runs
        const dim3 gg(psd_gemm_grid(gper, big)), gb(kPsdGemmThreads);
        const dim3 gt(psd_xcd_grid(std::max(psd_max_tiles, 1), big));
        // front: unpack, V = I / V' on many CUs; orders 0 / 1 and the periodic re-orthogonalisation of V in the one-workgroup kernel
        hipLaunchKernelGGL(k_psd_front, gt, dim3(kPsdFrontThreads), 0, stream,
                           (const double *)base, B, psd_scratch.p, psd_warm, stall);
        hipLaunchKernelGGL(k_proj_psd<3>, dim3(big), dim3(kPsdThreads), kPsdLdsBytes, stream, base, B, psd_scratch.p, psd_warm, 0, stall, psd_tol2,
                           psd_refine_default(false), 0);
        hipLaunchKernelGGL(k_psd_gemm<PSD_G1>, gg, gb, 0, stream, base, B, psd_scratch.p, psd_warm, stall, gper);
        hipLaunchKernelGGL(k_psd_gemm<PSD_G2>, gg, gb, 0, stream, base, B, psd_scratch.p, psd_warm, stall, gper);
        int mc = !fl.p ? 1 : psd_mc_members(big);  // (the multi-CU kernel polls the workspace's error flag at its barriers)
        // Round 5: GEMM-only refinement of the sign split instead of the last Jacobi sweep(s) (psd.hpp psd_stop_test).
        // SCS_HIP_PSD_REFINE=0: strict sweeps only (bit-identical to the one-launch kernel)
        PsdRefineCfg R = psd_refine_default(opt.psd_refine);
        if ((size_t)32 * psd_max_np * sizeof(double) > 160 * 1024) R.on = 0;  // k_psd_apply_q keeps two 16-row strips in LDS
        std::unique_ptr<SpinLink> link;
        if (mc > 1) link.reset(new SpinLink(this));  // spinning launches of this device, one grid at a time (SpinChain)
        for (int round = 0; round < kPsdSplitRounds; ++round) {
          const int post = (R.on && round == kPsdSplitRounds - 1) ? 1 : 0;
          if (post) {
            // the refinement stage (psd.hpp psd_stop_test): matrices the sweeps left REFINABLE get the mixed-sign part of S = V'AV
            // removed by GEMMs; the round behind it re-tests them (and goes on sweeping whatever is not done: nothing is lost)
            hipLaunchKernelGGL(k_psd_gemm<PSD_COMM>, gg, gb, 0, stream, base, B, psd_scratch.p, psd_warm, stall, gper);
            hipLaunchKernelGGL(k_psd_gemm<PSD_KK>, gg, gb, 0, stream, base, B, psd_scratch.p, psd_warm, stall, gper);
            hipLaunchKernelGGL(k_psd_gemm<PSD_T>, gg, gb, 0, stream, base, B, psd_scratch.p, psd_warm, stall, gper);
            hipLaunchKernelGGL(k_psd_gemm<PSD_S1>, gg, gb, 0, stream, base, B, psd_scratch.p, psd_warm, stall, gper);
            hipLaunchKernelGGL(k_psd_apply_q, gt, dim3(kPsdApplyThreads), (size_t)32 * psd_max_np * sizeof(double), stream, B,
                               psd_scratch.p, stall);
          }
          if (mc > 1) {  // sweeps of one matrix over `mc` CUs (k_psd_sweep_mc): cooperative launch, spinning barriers
            double *scr = psd_scratch.p;
            int G = mc, rnd = round;
            int *err = fl.p + F_PERSIST_ERR;
            const int *st = stall;
            int la = opt.psd_la ? 1 : 0;  // (labs switch) one barrier per step
            const double *tl = psd_tol2;
            PsdRefineCfg Rr = R;
            int pst = post;
            long budget = 1L << opt.spin_budget_log2;  // barrier polls before a member gives up (SCS_HIP_SPIN_BUDGET_LOG2; tests: 0)
            void *args[] = {&B, &scr, &rnd, &G, &la, &err, &st, &tl, &Rr, &pst, &budget};
            // Round 4: ORDINARY launch by default.  hipLaunchCooperativeKernel guarantees co-residency of the grid, but on this runtime it costs
            // ~0.1 ms per launch in a fresh process and ~2 ms per launch once the process has driven other workspaces / streams before (config 4 as
            // the second workload of a bench run: 224 iters/s in the steady window and 245 over a whole solve against 462 / 521 with the ordinary
            // launch; cold window 495 vs 522; tools/dbg/c4_after.py, profiles/r04_psd_coop.txt).  The ordinary launch is safe for the same reason the
            // cooperative one is accepted: the grid is sized to fit the device at one workgroup per CU (psd_mc_cap, occupancy query), the
            // dispatcher places workgroups in order, and a kernel of another stream that holds CUs finishes without waiting for this one — a group
            // whose members are late spins within its budget (F_PERSIST_ERR otherwise: an error, not a hang).  (labs) SCS_HIP_PSD_COOP=1: cooperative launch.
            if (opt.psd_coop) {
              const hipError_t e = hipLaunchCooperativeKernel(reinterpret_cast<const void *>(k_psd_sweep_mc), dim3((unsigned)psd_mc_grid(big, mc)),
                                                             dim3(kPsdThreads), args, (unsigned)kPsdMcLdsBytes, stream);
              if (e != hipSuccess) {  // the runtime cannot co-schedule the grid (it only refuses the FIRST round: nothing ran yet)
                (void)hipGetLastError();
                if (round > 0) HIP_CHECK(e);
                psd_mc_cap = 0;  // from now on: one workgroup per matrix
                mc = 1;
              }
            } else  // ordinary launch (rocprofv3 7.2 crashes at exit after a cooperative launch)
              hipLaunchKernelGGL(k_psd_sweep_mc, dim3((unsigned)psd_mc_grid(big, mc)), dim3(kPsdThreads), kPsdMcLdsBytes, stream, B, scr, rnd, G,
                                 la, err, st, tl, Rr, pst, budget);
          }
          if (mc <= 1)
          hipLaunchKernelGGL(k_proj_psd<1>, dim3(big), dim3(kPsdThreads), kPsdLdsBytes, stream, base, B, psd_scratch.p, psd_warm, round, stall, psd_tol2,
                             R, post);
          hipLaunchKernelGGL(k_psd_apply_v, gt, dim3(kPsdApplyThreads), (size_t)16 * psd_max_np * sizeof(double),
                             stream, B, psd_scratch.p, stall);
        }
        link.reset();
        hipLaunchKernelGGL(k_psd_fmap, gt, dim3(256), 0, stream, B, psd_scratch.p, stall);
        hipLaunchKernelGGL(k_psd_gemm<PSD_R1>, gg, gb, 0, stream, base, B, psd_scratch.p, psd_warm, stall, gper);
        hipLaunchKernelGGL(k_psd_gemm<PSD_R2>, gg, gb, 0, stream, base, B, psd_scratch.p, psd_warm, stall, gper);
      } else {
        hipLaunchKernelGGL(k_proj_psd<0>, dim3(big), dim3(kPsdThreads), kPsdLdsBytes, stream, base, B, psd_scratch.p, psd_warm, 0, stall, psd_tol2,
                           psd_refine_default(false), 0);
      }
    }
    if (count > big) {
      // small matrices (order <= 32): four wavefronts per matrix (psd.hpp d_proj_psd_small4)
      PsdBatch B{off + big, order + big, woff + big, count - big};
      hipLaunchKernelGGL(k_proj_psd_small4, dim3(count - big), dim3(kPsdSmallThreads), 0, stream, base, B, psd_scratch.p, psd_warm, stall,
                         psd_tol2);
    }
  }
  // Members (CUs) per matrix for the split-mode sweeps: as many as fit when every matrix gets the same number and a
  // group stays inside one XCD (grid = 8 * G * ceil(count / 8) workgroups, all co-resident: cooperative launch).
  // SCS_HIP_PSD_MC=G forces G (0 / 1: the one-workgroup sweep kernel).
  int psd_mc_cap = -1;  // co-resident workgroups of k_psd_sweep_mc on this device (0: no cooperative launch)
  bool spin_user = false;
  hipEvent_t ev_spin = nullptr;
  void spin_register() {  // before this workspace's first spinning launch
    if (spin_user) return;
    SpinChain &c = spin_chain(device);
    bool others;
    {
      std::lock_guard<std::mutex> lk(c.mu);
      others = ++c.users >= 2;
    }
    spin_user = true;
    HIP_CHECK(hipEventCreateWithFlags(&ev_spin, hipEventDisableTiming));
    if (others) HIP_CHECK(hipDeviceSynchronize());  // what the others launched before they had to leave events is done now
  }
  void spin_unregister() {
    if (!spin_user) return;
    SpinChain &c = spin_chain(device);
    {
      std::lock_guard<std::mutex> lk(c.mu);
      --c.users;
      if (c.last == ev_spin) c.last = nullptr;
    }
    if (ev_spin) (void)hipEventDestroy(ev_spin);
    ev_spin = nullptr;
    spin_user = false;
  }
  // around the spinning launches of one call (held while they are enqueued: the chain is a total order)
  struct SpinLink {
    ScsHipWork *w;
    SpinChain &c;
    std::unique_lock<std::mutex> lk;
    explicit SpinLink(ScsHipWork *w_) : w(w_), c(spin_chain(w_->device)) {
      w->spin_register();
      lk = std::unique_lock<std::mutex>(c.mu);
      if (c.users >= 2 && c.last && c.last_stream != w->stream) HIP_CHECK(hipStreamWaitEvent(w->stream, c.last, 0));
    }
    ~SpinLink() {
      if (c.users >= 2 && hipEventRecord(w->ev_spin, w->stream) == hipSuccess) {
        c.last = w->ev_spin;
        c.last_stream = w->stream;
      }
    }
  };
  int psd_mc_members(int big) {
    if (psd_mc_cap < 0) {
      int coop = 0, per_cu = 0, cus = 0;
      (void)hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, device);
      (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(k_psd_sweep_mc), kPsdThreads, kPsdMcLdsBytes) != hipSuccess)
        per_cu = 0;
      psd_mc_cap = coop ? std::min(per_cu, 1) * cus : 0;  // one member per CU: the pivot solves want a SIMD each
    }
    const int groups = 8 * ((big + 7) / 8);
    // at least ~3 pivots per member and step: below that the barriers cost more than the spread saves
    // (tools/psd_mc_lab.sh: order 200 x 50, G = 4: 3.57 -> 2.24 ms per projection; order 64 x 100, G = 2: 0.29 -> 0.42 ms)
    const int pivots = psd_max_np / (2 * kPsdB);
    int G = std::min(std::min(psd_mc_cap / groups, kPsdMcMaxG), pivots / 3);
    if (opt.psd_mc >= 0) {  // SCS_HIP_PSD_MC at the workspace's creation (-1: pick)
      G = opt.psd_mc;
      if (G > kPsdMcMaxG || ((long)G * groups > (long)psd_mc_cap && !opt.psd_mc_nocheck)) G = 1;  // ((labs) NOCHECK: tests of the refused launch)
    }
    return std::max(G, 1);
  }
  // stopping level of the PSD sweeps (psd.hpp psd_offtol2): inside the ADMM loop the iteration's P_PSD_TOL2, else nullptr = fixed 1e-8
  const double *psd_tol2 = nullptr;
  // ... and only while no Anderson extrapolation can happen yet (the history is still filling: iteration < lookback x interval;
  // always, without acceleration): plain ADMM tolerates inexact projections, the secant model of the acceleration does not —
  // with interval 1 and type-II steps a golden infeasible instance stalled for good (tools/dbg/psd_tol_infeas.py).
  double psd_tol2_for(int iter) const {
    const bool plain_phase = aa.mem <= 0 || (long)iter < (long)aa.mem * stgs.acceleration_interval;
    return plain_phase ? psd_tol2_of(psd_res_min) : kPsdOffTol2;
  }
  static constexpr double kPsdTolMax = 1e-3;  // the loosest level the sweeps ever stop at
  double psd_tol2_of(double level) const {  // level = what note_check_residuals left in psd_res_min
    if (!opt.psd_tol_adaptive) return kPsdOffTol2;  // SCS_HIP_PSD_TOL=fixed: A/B
    const double t = std::min(std::max(level, 1e-8), kPsdTolMax);
    return t * t;
  }
  int psd_warm = 1;  // warm-start the eigen-solves from the previous call's eigenvectors (0 in the one-shot test entry)

  // AA (aa.hpp): f = v (map output), x = v_prev (map input); the safeguard verdict rides along with the CG flags
  DeviceAa aa;
  double aa_norm = 0;
  int rejected_accel = 0, accepted_accel = 0;

  // per-solve state
  Residuals r;
  double sum_log_scale_factor = 0;
  int n_log_scale_factor = 0, last_scale_update_iter = 0, scale_updates = 0;
  long tot_cg_iters = 0;
  int last_cg_iters = 8;
  int cg_hist[8] = {8, 8, 8, 8, 8, 8, 8, 8}, cg_hist_pos = 0;  // CG steps of the last 8 linear solves (chunk sizing)
  void note_cg_iters(int it) { cg_hist[cg_hist_pos++ & 7] = it; }
  // largest step count of the last kChunkWindow linear solves: what a queued iteration's CG chunk is sized
  // for.  Round 4: 3 instead of 8 — in the cold-start phase the counts FALL from iteration to iteration, and a window of 8 kept
  // enqueuing the counts of eight iterations ago: 36 % of the K1 / K2 launches of the bench window were early-exit launches
  // (profiles/r03_bench_kernel_trace.txt: 3581 launched, 2309 with work).
  static constexpr int kChunkWindow = 3;
  int recent_cg_max() const {
    int mx = 1;
    for (int k = 1; k <= kChunkWindow; ++k) mx = std::max(mx, cg_hist[(cg_hist_pos - k) & 7]);
    return mx;
  }
  int recent_cg_q3() const {  // third quartile of the last 8 linear solves (the grouped loop's prediction: a short round is cheap there)
    int h[8];
    std::copy(cg_hist, cg_hist + 8, h);
    std::sort(h, h + 8);
    return std::max(1, h[5]);
  }
  double cg_res_min = 0;
  // what the PSD stopping level follows (psd_tol2_of): the smallest of the residuals ANY termination test looks at —
  // primal / dual residual and, for a problem drifting towards a certificate, the certificate's own residuals
  double psd_res_min = 0;
  void note_check_residuals() {
    cg_res_min = std::min(r.nm_pri_n, r.nm_dual_n);
    psd_res_min = opt.psd_tol_k * cg_res_min;  // ((labs) SCS_HIP_PSD_TOL_K; see psd.hpp psd_offtol2 for why 1e-2)
    if (std::isfinite(r.res_infeas)) psd_res_min = std::min(psd_res_min, r.res_infeas);
    // (an unboundedness certificate needs BOTH of its residuals small; |Px| / -c'x is identically 0 for an LP)
    if (std::isfinite(r.res_unbdd_a) && std::isfinite(r.res_unbdd_p)) psd_res_min = std::min(psd_res_min, std::max(r.res_unbdd_a, r.res_unbdd_p));
  }
  // live kernel timing (HIP events on the launch stream, one sampled CG step per chunk)
  bool profile = false;
  double prof_ms[3] = {0, 0, 0};  // K1 (A p), K2 (A' z + R_x p [+ P p]), K3 (P p; problems with P)
  long prof_n[3] = {0, 0, 0};
  // one sampled CG step: events [0] K1 [1] (K3 [3]) K2 [2]
  void note_cg_sample(hipEvent_t *e) {
    float a = 0, b = 0, c = 0;
    if (hipEventElapsedTime(&a, e[0], e[1]) != hipSuccess) return;
    if (has_P) {
      if (hipEventElapsedTime(&c, e[1], e[3]) != hipSuccess || hipEventElapsedTime(&b, e[3], e[2]) != hipSuccess) return;
      prof_ms[2] += c; prof_n[2]++;
    } else if (hipEventElapsedTime(&b, e[1], e[2]) != hipSuccess) {
      return;
    }
    prof_ms[0] += a; prof_n[0]++;
    prof_ms[1] += b; prof_n[1]++;
  }
  // bench.py: a timestamp INSIDE a solve (scs_hip_set_mark): when iteration mark_iter is about to start the stream is
  // drained and the elapsed time / counters are recorded, so a window that starts past the cold start can be timed
  int mark_iter = -1;
  double mark_ms = -1;
  long mark_cg = 0;
  int mark_aa_calls = 0, mark_aa_accept = 0;
  std::mutex mtx;

  ~ScsHipWork() {
    // nothing of this workspace is in flight once its stream is idle: its blocks may be handed to the next workspace without hipFree
    // (real workspaces only: the stack workspaces of the kernel-level entry points borrow a stream that is gone by now)
    if (stream && pooled_stream && hipStreamSynchronize(stream) == hipSuccess) {
      pool_window_end.armed = true;
      ++t_pool_release;
    }
    spin_unregister();
    if (pinned_block) {
      g_pinned.release(pinned_block);
    } else {  // (stack workspaces of the kernel-level entry points allocate what they need themselves)
      if (h_pin) (void)hipHostFree(h_pin);
      if (h_flags) (void)hipHostFree(h_flags);
      if (h_params_base) (void)hipHostFree(h_params_base);
      for (auto &hf : h_flags_slot) if (hf) (void)hipHostFree(hf);
    }
    if (sol_pin) (void)hipHostFree(sol_pin);
    for (auto &e : sol_ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : ev_iter) if (e) (void)hipEventDestroy(e);
    for (auto &es : ev_prof) for (auto &e : es) if (e) (void)hipEventDestroy(e);
    for (auto &es : ev_cone) for (auto &e : es) if (e) (void)hipEventDestroy(e);
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    if (stream && pooled_stream) g_streams.release(device, stream);
  }

#include "work_linsys.inl"
#include "work_admm.inl"
#include "work_residuals.inl"
#include "work_solve_ends.inl"
};
