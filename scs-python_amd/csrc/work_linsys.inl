// work_linsys.inl — members of ScsHipWork (work.hpp): the linear solve of an ADMM iteration — dense direct path, the K1 / K2 / K3 products, PCG
// (fused start, steps, run_cg), the standalone KKT solve and g = KKT^-1 h
  // -------------------------------------------------------------- helpers
  int vb(long nelem) const { return vec_blocks(nelem); }

  // ---- dense direct linsys (dense.hpp; linsys == 1): G^{-1} = (R_x + P + A' R_y^{-1} A)^{-1} resident in HBM, rebuilt whenever R changes
  int linsys = 0;  // 0: indirect (PCG), 1: dense direct
  DevBuf<double> dn_G, dn_Pk, dn_L, dn_Rt;
  int dn_NP = 0, dense_factorisations = 0;
  bool dense() const { return linsys == 1; }
  DenseMat dense_mat() const { return DenseMat{dn_G.p, dn_Pk.p, dn_L.p, dn_Rt.p, n, dn_NP}; }
  DenseSrc dense_src() const {
    return DenseSrc{At.rowptr.p, At.col.p, At.val.p, Ar.rowptr.p, Ar.col.p, Ar.val.p, has_P ? Pf.rowptr.p : nullptr,
                    has_P ? Pf.col.p : nullptr, has_P ? Pf.val.p : nullptr, diag_r.p};
  }
  void dense_alloc() {
    dn_NP = dense_np(n);
    dn_G.alloc((size_t)dn_NP * dn_NP);
    dn_Pk.alloc((size_t)kDenseB * kDenseB);
    dn_L.alloc((size_t)dn_NP * kDenseB);
    dn_Rt.alloc((size_t)dn_NP * kDenseB);
  }
  void dense_gemv(const double *b, double *x, const int *st) {
    hipLaunchKernelGGL(k_dense_gemv, dim3(dense_gemv_blocks(n)), dim3(kDenseThreads), 0, stream, (const double *)dn_G.p, dn_NP, n, b, x, st);
  }
  // Dense workspaces finish their setup — R, G^{-1}, g = KKT^{-1} [c; -b] — at the first solve (or update) instead of inside scs_init:
  // a batch of them then forms and inverts all its matrices in ONE batched sweep (GroupSolve::run), 66 launches for the whole group
  // instead of 66 launch-bound ones per member (SCS_HIP_LAZY_SETUP=0: inside scs_init).
  bool setup_pending = false, setup_failed = false;
  std::string setup_failed_msg(int member = -1) const {
    return std::string("hip_dense: the inverse of the reduced KKT matrix is not finite") +
           (member >= 0 ? " (member " + std::to_string(member) + " of the batch)" : "") +
           " (a vanishing pivot block — column-rank-deficient A with a tiny rho_x?); use LinearSolver.HIP_INDIRECT for this problem";
  }
  void finish_pending_setup() {
    if (setup_failed) throw std::runtime_error(setup_failed_msg());  //  a failed setup stays failed: no solve on a non-finite inverse
    if (!setup_pending) return;
    const double t0 = now_ms();
    set_diag_r();
    update_work_cache();
    HIP_CHECK(hipStreamSynchronize(stream));
    setup_pending = false;
    setup_time += now_ms() - t0;
    if (dense()) {
      //  the Gauss-Jordan sweep of the dense path does not pivot and checks nothing on the way: at least the solve it has just
      // been used for, g = KKT^-1 [c; -b], must be finite (g' R g is on the device already: one double)
      double gg = 0.;
      HIP_CHECK(hipMemcpyAsync(&gg, sc.p + S_GG, sizeof(double), hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
      if (!std::isfinite(gg)) {
        setup_failed = true;
        throw std::runtime_error(setup_failed_msg());
      }
    }
  }
  void dense_refactor() {  // diag_r must be current on the stream
    dense_factor(dense_src(), dense_mat(), stream);
    ++dense_factorisations;
  }

  void set_diag_r() {
    diag_r_structured = true;
    hipLaunchKernelGGL(k_set_diag_r, dim3(vb(l)), dim3(kVecThreads), 0, stream, diag_r.p, n, m, cone.z, stgs.rho_x, scale);
    if (dense()) { dense_refactor(); return; }
    hipLaunchKernelGGL(k_precond, dim3(vb(n)), dim3(kVecThreads), 0, stream, At.rowptr.p, At.col.p, At.val.p, diag_r.p,
                       has_P ? Pdiag.p : (const double *)nullptr, cg_M.p, n);
  }

  // R_x / R_y as the SpMV epilogues take them: two scalars inside the ADMM workspace (set_diag_r built diag_r), the
  // vector for the standalone KKT entry point (arbitrary diag_r)
  // (SCS_HIP_PIPELINE=0, the host-synchronous loop, reads the vector too: set_diag_r updates it in place at every scale update)
  bool diag_r_structured = false;
  bool r_scalars() const { return diag_r_structured && pipelined; }
  RDiag rdx() const { return r_scalars() ? RDiag(stgs.rho_x, stgs.rho_x, 0) : RDiag(diag_r.p); }
  RDiag rdy() const { return r_scalars() ? RDiag(1.0 / (1000. * scale), 1.0 / scale, cone.z) : RDiag(diag_r.p + n); }
  // Gp = (R_x + P + A' R_y^{-1} A) x ; partial p.Gp into part[0..At.nblk)
  // step_counter != nullptr marks the A product of a CG step (its workgroup 0 advances the step parity)
  // second half of Gp when A' has the split layout (EpiGp::split): Gp = cg_Gp + gp2()
  double *gp2() const { return At.cs.ok && At.cs.split > 1 && !At.cs.combine() ? At.cs_part1.p : nullptr; }
  void matvec(const double *x, const int *done, int *step_counter = nullptr) {
    launch_spmv(Ar.view(), x, EpiDivR{tmp_m.p, rdy()}, done, stream, step_counter);
    if (has_P) launch_spmv(Pf.view(), x, EpiStore{cg_Gp.p, 0}, done, stream);
    launch_spmv(At.view(), tmp_m.p, EpiGp{cg_Gp.p, x, rdx(), has_P ? 1 : 0, part.p, gp2()}, done, stream);
  }

  void read_flags() {
    HIP_CHECK(hipGetLastError());  // launches are not checked one by one: a refused one is caught here
    HIP_CHECK(hipMemcpyAsync(h_flags, fl.p, sizeof(int) * F_COUNT, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    process_pending_flags();
  }

  void process_pending_flags() {
    if (h_flags[F_PERSIST_ERR]) throw SpinTimeout("a spinning multi-workgroup kernel (PSD sweeps) timed out at its barrier");
    if (aa.pending_safeguard) {
      const bool bad = h_flags[F_SAFE_BAD] != 0;
      aa.safeguard_verdict(bad);
      if (bad) rejected_accel++;
      else accepted_accel++;
    }
  }

  // ---- enqueue helpers ----
  void enqueue_cg_start(double *xout, const double *warm) {
    const int nb = vb(n);
    if (warm) matvec(warm, nullptr);
    hipLaunchKernelGGL(k_cg_init, dim3(nb), dim3(kVecThreads), 0, stream, cg_b.p, cg_Gp.p, warm, cg_M.p, xout, cg_r.p, cg_p.p,
                       n, warm ? 1 : 0, fl.p, part.p, (const double *)gp2());
    hipLaunchKernelGGL(k_fin_cg_init, dim3(1), dim3(kVecThreads), 0, stream, part.p, nb, 0, sc.p, fl.p);
    HIP_CHECK(hipMemsetAsync(fl.p + F_ITERS, 0, sizeof(int), stream));
  }
  // yacc != nullptr: carry y += alpha R_y^{-1} A p along (ADMM path, see k_prep).  evs: three events around the two products (in-situ
  // kernel timing of one step: bench.py's roofline)
  void enqueue_cg_step(double *xout, double *yacc, hipEvent_t *evs = nullptr) {
    const int nb = vb(std::max(n, yacc ? m : 0));
    if (evs) {
      HIP_CHECK(hipEventRecord(evs[0], stream));
      launch_spmv(Ar.view(), cg_p.p, EpiDivR{tmp_m.p, rdy()}, fl.p + F_DONE, stream, fl.p + F_STEP);
      HIP_CHECK(hipEventRecord(evs[1], stream));
      if (has_P) {
        launch_spmv(Pf.view(), cg_p.p, EpiStore{cg_Gp.p, 0}, fl.p + F_DONE, stream);
        HIP_CHECK(hipEventRecord(evs[3], stream));
      }
      launch_spmv(At.view(), tmp_m.p, EpiGp{cg_Gp.p, cg_p.p, rdx(), has_P ? 1 : 0, part.p, gp2()}, fl.p + F_DONE, stream);
      HIP_CHECK(hipEventRecord(evs[2], stream));
    } else
    matvec(cg_p.p, fl.p + F_DONE, fl.p + F_STEP);
    if (cg_fuse()) {  // small systems: update + direction as one launch (vec.hpp k_cg_update_dir; same bits)
      hipLaunchKernelGGL(k_cg_update_dir, dim3(nb), dim3(kVecThreads), 0, stream, xout, cg_r.p, cg_p.p, (const double *)cg_Gp.p,
                         (const double *)cg_M.p, n, yacc, (const double *)tmp_m.p, m, (const double *)part.p, At.nwg(), sc.p, fl.p, part2.p,
                         (const double *)gp2(), cg_ticket.p);
      return;
    }
    hipLaunchKernelGGL(k_cg_update, dim3(nb), dim3(kVecThreads), 0, stream, xout, cg_r.p, cg_p.p, cg_Gp.p, cg_M.p, n, yacc,
                       tmp_m.p, m, part.p, At.nwg(), sc.p, fl.p, part2.p, (const double *)gp2());
    hipLaunchKernelGGL(k_cg_dir, dim3(vb(n)), dim3(kVecThreads), 0, stream, cg_p.p, cg_r.p, cg_M.p, n, part2.p, nb, sc.p, fl.p);
  }
  // SCS_HIP_CG_FUSE=0: always two launches
  bool cg_fuse() const { return opt.cg_fuse && n <= kCgFuseMaxN; }  // ((labs switch) SCS_HIP_CG_FUSE)

  // PCG on cg_b (rhs, length n); solution accumulates in xout.  S_TOL / F_DONE must be set on device.
  // Returns CG iterations taken.
  // mode 0: enqueue the CG start here; 1: the start is already enqueued (not synced);
  // 2: the start and some steps already ran and the flags are on the host (recover_stalled_iteration): go on from h_flags.
  int run_cg(double *xout, const double *warm, int max_its, int mode = 0) {
    int done_iters = 0;
    const bool started = mode == 2;
    if (mode == 0) enqueue_cg_start(xout, warm);
    else if (started) done_iters = h_flags[F_ITERS];
    bool finished = started && (h_flags[F_DONE] || done_iters >= max_its);  // (mode 2: nothing may be left to do)
    double *yacc = (xout == ut.p) ? ut.p + n : nullptr;  // ADMM path carries the y block along the recurrence
    int chunk = started ? std::max(2, std::min(std::max(done_iters / 2, 4), 64)) : std::max(1, std::min(last_cg_iters + 2, 64));  // a host round trip costs ~30 us, an unused CG step four ~1 us launches
    while (!finished) {
      const int iters_before = done_iters;
      const int sample_it = chunk / 2;  // a mid-chunk step: not the one right behind the host sync
      for (int it = 0; it < chunk; ++it) enqueue_cg_step(xout, yacc, (profile && it == sample_it) ? ev : nullptr);
      read_flags();
      if (profile && h_flags[F_ITERS] - iters_before > sample_it) note_cg_sample(ev);  // the sampled step really ran
      done_iters = h_flags[F_ITERS];
      finished = h_flags[F_DONE] || done_iters >= max_its;
      chunk = std::max(2, std::min(std::max(done_iters / 2, 4), 64));
    }
    last_cg_iters = done_iters;
    if (xout == ut.p) note_cg_iters(done_iters);  // (not the cold KKT solves of init / scale updates)
    tot_cg_iters += done_iters;
    return done_iters;
  }

  // standalone KKT solve on a device vector rhs (length n+m), cold start, fixed tolerance
  int kkt_solve(double *rhs, double tol) {
    hipLaunchKernelGGL(k_kkt_prep, dim3(vb(m)), dim3(kVecThreads), 0, stream, rhs, diag_r.p, tmp_m.p, n, m);
    launch_spmv(At.view(), tmp_m.p, EpiRhs{cg_b.p, rhs}, nullptr, stream);
    HIP_CHECK(hipMemsetAsync(part.p, 0, sizeof(double), stream));
    hipLaunchKernelGGL(k_fin_tol, dim3(1), dim3(kVecThreads), 0, stream, part.p, 1, 0.0, 1.0, tol, 0, (const double *)nullptr, sc.p,
                       fl.p);
    int its = 0;
    if (dense()) dense_gemv(cg_b.p, ws.p, nullptr);
    else its = run_cg(ws.p, nullptr, 10 * n);  // solution in ws
    launch_spmv(Ar.view(), ws.p, EpiStore{tmp_m.p, 0}, nullptr, stream);
    hipLaunchKernelGGL(k_kkt_y, dim3(vb(m)), dim3(kVecThreads), 0, stream, rhs, tmp_m.p, diag_r.p, n, m);
    HIP_CHECK(hipMemcpyAsync(rhs, ws.p, sizeof(double) * n, hipMemcpyDeviceToDevice, stream));
    return its;
  }

  // g = (R + M)^{-1} [c; -b];  cache g'Rg
  void update_work_cache() {
    hipLaunchKernelGGL(k_g_rhs, dim3(vb((long)n + m)), dim3(kVecThreads), 0, stream, g.p, h.p, n, m);
    kkt_solve(g.p, 1e-12);
    const int nb = vb(l - 1);
    hipLaunchKernelGGL(k_gg, dim3(nb), dim3(kVecThreads), 0, stream, g.p, diag_r.p, l - 1, part.p);
    hipLaunchKernelGGL(k_fin_store_sum, dim3(1), dim3(kVecThreads), 0, stream, part.p, nb, sc.p, (int)S_GG);
  }

