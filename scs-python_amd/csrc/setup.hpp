// setup.hpp — scs_init: cone metadata upload and init_impl (validation, uploads, layouts, equilibration, vectors, AA workspace, R / preconditioner / g)
// (one of the units csrc/scs_hip.hip is assembled from — ONE translation unit, in this order: runtime.hpp, device_csr.hpp, work.hpp
// [+ work_linsys.inl, work_admm.inl, work_residuals.inl, work_solve_ends.inl], io.hpp, setup.hpp, loop.hpp, batch.hpp, the C ABI in scs_hip.hip,
// lab_entries.hpp; split out of the 3 800-line file of rounds 1-5 in round 6 — VERDICT r05 item 6 — without moving a line of code)
#pragma once
// ================================================================ init
static void upload_cone_meta(ScsHipWork *w) {
  hipStream_t s = w->stream;
  const HostCone &c = w->cone;
  std::vector<int> off, dim, big;
  int o = c.off_q, max_small = 0;
  for (size_t i = 0; i < c.q.size(); ++i) {
    off.push_back(o);
    dim.push_back(c.q[i]);
    if (c.q[i] > kSocBig) big.push_back((int)i);
    else max_small = std::max(max_small, (int)c.q[i]);
    o += c.q[i];
  }
  w->n_soc = (int)off.size();
  w->soc_G = soc_group(max_small);
  w->n_soc_big = (int)big.size();
  if (w->n_soc) { w->soc_off.upload(off.data(), off.size(), s); w->soc_dim.upload(dim.data(), dim.size(), s); }
  if (w->n_soc_big) w->soc_big.upload(big.data(), big.size(), s);
  if (!c.p.empty()) w->pow_a.upload(c.p.data(), c.p.size(), s);
  if (c.bsize > 1) {
    w->box_bl.upload(c.bl.data(), c.bl.size(), s);
    w->box_bu.upload(c.bu.data(), c.bu.size(), s);
    if (!w->box_bl_orig.p) {  // (scs_init uploaded the originals before the row scaling; the standalone entry points have none)
      w->box_bl_orig.upload(c.bl.data(), c.bl.size(), s);
      w->box_bu_orig.upload(c.bu.data(), c.bu.size(), s);
    }
  }
  std::vector<int> poff, pord;
  std::vector<long> woff;
  long wtot = 0;
  for (int pass = 0; pass < 2; ++pass) {  // pass 0: orders > kPsdSmallMax (block kernel), pass 1: the one-wave kernel's
    o = c.off_s;
    for (int sdim : c.s) {
      if ((sdim > kPsdSmallMax) == (pass == 0)) {
        poff.push_back(o);
        pord.push_back(sdim);
        woff.push_back(wtot);
        wtot += psd_scratch_doubles(sdim);
      }
      o += (int)sd_size(sdim);
    }
    if (pass == 0) w->n_psd_big = (int)poff.size();
  }
  w->n_psd = (int)poff.size();
  if (w->n_psd) {
    w->psd_off.upload(poff.data(), poff.size(), s);
    w->psd_order.upload(pord.data(), pord.size(), s);
    w->psd_woff.upload(woff.data(), woff.size(), s);
    w->psd_woff_h = woff;
    w->psd_order_h = pord;
  }
  std::vector<int> coff, cord, cpoff, cpord;
  std::vector<long> csoff, cwoff;
  long stot = 0;
  for (int pass = 0; pass < 2; ++pass) {
    o = c.off_cs;
    for (int k : c.cs) {
      if ((2 * k > kPsdSmallMax) == (pass == 0)) {
        coff.push_back(o);
        cord.push_back(k);
        csoff.push_back(stot);
        cpoff.push_back((int)stot);
        cpord.push_back(2 * k);
        cwoff.push_back(wtot);
        wtot += psd_scratch_doubles(2 * k);
        stot += sd_size(2 * k);
      }
      o += k * k;
    }
    if (pass == 0) w->n_cs_big = (int)coff.size();
  }
  w->n_cs = (int)coff.size();
  if (w->n_cs) {
    w->cs_off.upload(coff.data(), coff.size(), s);
    w->cs_order.upload(cord.data(), cord.size(), s);
    w->cs_soff.upload(csoff.data(), csoff.size(), s);
    w->cs_poff.upload(cpoff.data(), cpoff.size(), s);
    w->cs_porder.upload(cpord.data(), cpord.size(), s);
    w->cs_woff.upload(cwoff.data(), cwoff.size(), s);
    w->cs_stage.alloc_zero((size_t)std::max(stot, 1L), s);
  }
  if (w->n_psd || w->n_cs) w->psd_scratch.alloc_zero((size_t)std::max(wtot, 1L), s);
  if (c.has_spectral()) {  // spectral cones: offsets and sizes per kind in one block (spectral.hpp SpecBatch)
    std::vector<int> meta;
    auto put = [&](const std::vector<int> &v) { const size_t at = meta.size(); meta.insert(meta.end(), v.begin(), v.end()); return at; };
    std::vector<int> off;
    int max_sl = 0, max_d = 0, max_rc = 0, max_c = 0;
    std::vector<int> loff, ln, sn;
    o = c.off_ell1;
    for (int v : c.ell1) {
      (v > kSpecEll1WaveMax ? loff : off).push_back(o);
      (v > kSpecEll1WaveMax ? ln : sn).push_back(v);
      o += v + 1;
    }
    const size_t e_off = put(off), e_n = put(sn), el_off = put(loff), el_n = put(ln);
    off.clear();
    o = c.off_sl;
    for (int v : c.sl_n) { off.push_back(o); o += (int)sd_size(v) + 1; max_sl = std::max(max_sl, v); }
    const size_t s_off = put(off), s_n = put(c.sl_n), s_k = put(c.sl_k);
    off.clear();
    o = c.off_d;
    for (int v : c.d) { off.push_back(o); o += (int)sd_size(v) + 2; max_d = std::max(max_d, v); }
    const size_t d_off = put(off), d_n = put(c.d);
    off.clear();
    o = c.off_nuc;
    for (size_t i = 0; i < c.nuc_m.size(); ++i) {
      off.push_back(o);
      o += c.nuc_m[i] * c.nuc_n[i] + 1;
      max_rc = std::max(max_rc, c.nuc_m[i] * c.nuc_n[i]);
      max_c = std::max(max_c, std::min(c.nuc_m[i], c.nuc_n[i]));
    }
    const size_t u_off = put(off), u_m = put(c.nuc_m), u_n = put(c.nuc_n);
    w->spec_meta.upload(meta.data(), meta.size(), s);
    const int *mp = w->spec_meta.p;
    w->spec_ell1 = SpecBatch{mp + e_off, mp + e_n, nullptr, (int)sn.size()};
    w->spec_ell1_long = SpecBatch{mp + el_off, mp + el_n, nullptr, (int)ln.size()};
    w->spec_sl = SpecBatch{mp + s_off, mp + s_n, mp + s_k, (int)c.sl_n.size()};
    w->spec_d = SpecBatch{mp + d_off, mp + d_n, nullptr, (int)c.d.size()};
    w->spec_nuc = SpecBatch{mp + u_off, mp + u_m, mp + u_n, (int)c.nuc_m.size()};
    w->spec_sl_lds = spec_eig_lds_bytes(max_sl);
    w->spec_d_lds = spec_eig_lds_bytes(max_d);
    w->spec_nuc_lds = spec_nuc_lds_bytes(max_rc, max_c);
  }
  {
    int big_total = 0, max_order = 0;
    for (int sdim : c.s)
      if (sdim > kPsdSmallMax) { ++big_total; max_order = std::max(max_order, sdim); }
    for (int k : c.cs)
      if (2 * k > kPsdSmallMax) { ++big_total; max_order = std::max(max_order, 2 * k); }
    w->psd_max_np = (int)psd_np(std::max(max_order, 2));
    w->psd_max_tiles = w->psd_max_np / 16;
    // split mode: one CU per matrix would leave at least half of the GPU idle.  Its V update keeps a 16-row strip of V in LDS
    // (16 x NP doubles): orders above 1280 do not fit and take the one-workgroup-per-matrix kernel (any order up to 16 kPsdMaxH)
    w->psd_split = big_total > 0 && big_total <= 128 && (size_t)16 * w->psd_max_np * sizeof(double) <= 160 * 1024;
    if (w->opt.psd_split >= 0) w->psd_split = big_total > 0 && w->opt.psd_split == 1;  // SCS_HIP_PSD_SPLIT: A/B and tests
  }
  HIP_CHECK(hipStreamSynchronize(s));
}

// first chunk of a workspace arena: ~40 doubles per row / column of vectors + the Anderson history + 3 matrix layouts of 12 B per nonzero
// (annz = 0: a clone, which holds no matrix), rounded up to a power of two
static size_t arena_first_chunk(long l, long lookback, long annz) {
  const long mem = std::max(0L, lookback);
  const size_t est = (size_t)(8 * (40 + 3 * mem) * l + 3 * 12 * annz + (256 << 10));
  size_t c = 256 << 10;
  while (c < est && c < Arena::kChunkBytes) c <<= 1;
  return c;
}

// the stream, events and pinned host block of a workspace (scs_init and scs_hip_clone)
static void init_streams_and_pinned(ScsHipWork *w) {
  w->pipelined = w->opt.pipeline;     // SCS_HIP_PIPELINE=0: the host looks at the CG flags in every iteration
  w->pipe_chunk_override = w->opt.pipe_chunk;
  w->stream = g_streams.acquire(w->device, &w->stream_shared);
  w->pooled_stream = true;
  for (auto &e : w->ev) HIP_CHECK(hipEventCreate(&e));
  {  // one pinned, device-mapped block: [h_pin 256 f64 | AA h_pin 256 f64 | params 2 x P_COUNT f64 | flags 3 x F_COUNT i32]
    char *blk = (char *)g_pinned.acquire();
    w->pinned_block = blk;
    std::memset(blk, 0, kPinnedBlockBytes);
    w->h_pin = (double *)blk;
    w->aa.h_pin = (double *)blk + 256;
    w->aa.owns_pin = false;
    w->h_params_base = (double *)blk + 512;
    w->h_flags = (int *)((double *)blk + 512 + 2 * P_COUNT);
    w->h_flags_slot[0] = w->h_flags + F_COUNT;
    w->h_flags_slot[1] = w->h_flags + 2 * F_COUNT;
    static_assert((512 + 2 * P_COUNT) * sizeof(double) + 3 * F_COUNT * sizeof(int) <= kPinnedBlockBytes, "pinned block too small");
    HIP_CHECK(hipHostGetDevicePointer((void **)&w->d_params_base, w->h_params_base, 0));
  }
  w->h_params = w->h_params_base;
  w->d_params = w->d_params_base;
  for (int i = 0; i < 2; ++i) HIP_CHECK(hipEventCreateWithFlags(&w->ev_iter[i], hipEventDisableTiming));
}

// The host mirrors of D and E and the box bounds that follow the row scaling (bl_j <- bl_j D_{j+1} / D_0, from the CALLER's bounds in the
// matrix set): behind every device_normalize — scs_init's and scs_hip_update_matrix's
static void adopt_equilibration(ScsHipWork *w) {
  hipStream_t s = w->stream;
  const int n = w->n, m = w->m;
  w->scal.D.resize(m);
  w->scal.E.resize(n);
  w->D.download(w->scal.D.data(), m, s);
  w->E.download(w->scal.E.data(), n, s);
  HIP_CHECK(hipStreamSynchronize(s));
  if (w->cone.bsize > 1) {
    const double *Db = &w->scal.D[w->cone.off_box];
    const std::vector<double> &bl0 = w->mats->bl0, &bu0 = w->mats->bu0;
    for (int j = 0; j < w->cone.bsize - 1; ++j) {
      w->cone.bu[j] = (bu0[j] >= 1e15) ? INFINITY : Db[j + 1] * bu0[j] / Db[0];
      w->cone.bl[j] = (bl0[j] <= -1e15) ? -INFINITY : Db[j + 1] * bl0[j] / Db[0];
    }
  }
}

// The part of scs_init's state that is a function of the resident matrices, D / E and the CURRENT b and c: h, sigma, Dinv / Einv, the
// working box bounds, the box cone's t, an empty Anderson history and (unless deferred) R, the preconditioner or G^{-1}, and g.
// scs_init, scs_hip_clone (through init_state) and scs_hip_update_matrix all end in this one function.
template <class Mark>
static void start_state(ScsHipWork *w, Mark &&mark) {
  hipStream_t s = w->stream;
  const int n = w->n, m = w->m;
  const long l = w->l;
  {
    std::vector<double> hh(l, 0.0);
    std::copy(w->c_orig.begin(), w->c_orig.end(), hh.begin());
    std::copy(w->b_orig.begin(), w->b_orig.end(), hh.begin() + n);
    w->h.upload(hh.data(), l, s);
    HIP_CHECK(hipStreamSynchronize(s));
  }
  if (w->normalized) {
    w->scal.sigma = device_normalize_b_c(w->h, n, m, w->D, w->E, w->part, w->h_pin, s);
    std::vector<double> di(m), ei(n);
    for (int i = 0; i < m; ++i) di[i] = 1.0 / (w->scal.D[i] * w->scal.sigma);
    for (int i = 0; i < n; ++i) ei[i] = 1.0 / (w->scal.E[i] * w->scal.sigma);
    w->Dinv.upload(di.data(), m, s);
    w->Einv.upload(ei.data(), n, s);
    HIP_CHECK(hipStreamSynchronize(s));
  }
  if (w->cone.bsize > 1) {  // the working bounds (they follow the row scaling: adopt_equilibration)
    w->box_bl.upload(w->cone.bl.data(), w->cone.bl.size(), s);
    w->box_bu.upload(w->cone.bu.data(), w->cone.bu.size(), s);
  }
  {
    const double one = 1.0;
    HIP_CHECK(hipMemcpyAsync(w->sc.p + S_BOX_T, &one, sizeof(double), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  w->aa.reset(); w->aa.success = 0; w->aa.pending_safeguard = false; w->aa.st = ScsAaStats{};
  mark("b/c scaling, box bounds, AA reset");
  // ---- R, preconditioner (or G^{-1}), pre-solved g ----
  {
    // Round 5, late: the indirect path defers it too (SCS_HIP_LAZY_SETUP=0: inside scs_init) — its cold PCG for g is ~50 steps = 150 dependent
    // launches, three quarters of the dispatch chain of a small problem's scs_init; a batch runs it as ONE grouped cold solve (batch.hpp
    // apply_scale_updates, the path of an adaptive-scale update: bit-identical to the solo one), a lone workspace at its first solve.
    // (small problems only, n + m <= 32768: there the chain is what scs_init costs; a large problem keeps its cold solve out of scs_solve)
    const bool small_indirect = !w->dense() && (long)n + m <= 32768;
    w->setup_pending = (w->dense() || small_indirect) && w->opt.lazy_setup;  // (a clone defers what its parent deferred)
  }
  if (!w->setup_pending) {
    w->set_diag_r();
    w->update_work_cache();
  }
  HIP_CHECK(hipStreamSynchronize(s));
  mark("R, preconditioner, g = KKT^-1 h");
}

// Everything of scs_init behind the matrix set: vectors, cone metadata, the Anderson workspace (the allocations), then start_state.
// scs_hip_clone runs exactly this on the shared set, from the b, c and settings scs_init got.
template <class Mark>
static void init_state(ScsHipWork *w, Mark &&mark) {
  hipStream_t s = w->stream;
  const int n = w->n, m = w->m;
  // ---- vectors ----
  const long l = w->l;
  for (DevBuf<double> *b : {&w->v, &w->v_prev, &w->u, &w->ut, &w->rsk, &w->diag_r}) b->alloc_zero(l, s);
  w->g.alloc_zero(l, s);
  w->h.alloc_zero(l, s);
  for (DevBuf<double> *b : {&w->cg_b, &w->cg_p, &w->cg_r, &w->cg_Gp, &w->cg_M, &w->ws}) b->alloc_zero(n, s);
  w->cg_ticket.alloc_zero(1, s);
  w->tmp_m.alloc_zero(m, s);
  w->ensure_solution_mirror();
  w->solx.alloc_zero(n, s);
  w->soly.alloc_zero(m, s);
  w->sols.alloc_zero(m, s);
  // (x 8 until round 3: the residual epilogues leave 9 and 10 values per workgroup — with more than 1638 workgroups, i.e. the CSR-stream
  // layout of a matrix beyond ~3.4 M nonzeros, their partials ran past the buffer: a memory fault at 9419 row blocks)
  w->part_len = std::max({w->At.nblk, w->Ar.nblk, w->At.nwg(), w->Ar.nwg(), w->has_P ? std::max(w->Pf.nblk, w->Pf.nwg()) : 0, kMaxVecBlocks}) *
                kMaxEpiReductions;
  w->part.alloc_zero(w->part_len, s);
  w->part2.alloc_zero(2 * kMaxVecBlocks, s);
  w->part_v.alloc_zero(kMaxVecBlocks, s);
  w->sc.alloc_zero(S_COUNT, s);
  w->out.alloc_zero(256, s);
  w->fl.alloc_zero(F_COUNT, s);
  upload_cone_meta(w);
  // ---- AA workspace ----
  w->aa.init(l, w->stgs.acceleration_lookback, w->stgs.acceleration_type_1, w->stgs.acceleration_regularization,
             w->stgs.acceleration_relaxation, /*safeguard_factor=*/1.0, /*max_weight_norm=*/1e10, s, w->opt.aa_gram);
  if (w->dense()) w->dense_alloc();
  mark("vectors, cones, AA workspace");
  start_state(w, mark);
}

static ScsHipWork *init_impl(const ScsData *d, const ScsCone *k, const ScsSettings *stgs, int linsys = 0) {
  const double t0 = now_ms();
  refresh_options();  // the environment as it is NOW ...
  const Options &o = opts();  // ... and the snapshot this workspace, its matrix set and its clones keep for good (options.hpp)
  if (linsys == 0) linsys = o.linsys_dense ? 2 : 1;
  if (linsys != 1 && linsys != 2) throw std::runtime_error("unknown linear-system solver kind");
  if (!d || !k || !stgs) throw std::runtime_error("null argument");
  if (d->m <= 0 || d->n <= 0 || !d->A || !d->b || !d->c) throw std::runtime_error("invalid data dimensions");
  if (!validate_matrix(d->A, d->m, d->n)) throw std::runtime_error("invalid A matrix");
  if (d->P && !validate_matrix(d->P, d->n, d->n)) throw std::runtime_error("invalid P matrix");
  if (!(stgs->max_iters > 0) || !(stgs->eps_abs >= 0) || !(stgs->eps_rel >= 0) || !(stgs->eps_infeas >= 0) ||
      !(stgs->alpha > 0 && stgs->alpha < 2) || !(stgs->rho_x > 0) || !(stgs->scale > 0) ||
      !(stgs->acceleration_interval > 0) || stgs->acceleration_lookback < 0 ||
      !(stgs->time_limit_secs >= 0))
    throw std::runtime_error("invalid settings");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    throw std::runtime_error("libscs_hip: no HIP device available (this backend has no CPU fallback)");
  HIP_CHECK(hipSetDevice(current_device()));

  std::unique_ptr<ScsHipWork> w(new ScsHipWork(o));
  w->device = current_device();
  {
    std::string why;
    if (!build_cone(k, w->cone, &why)) throw std::runtime_error(why.empty() ? "invalid cone" : "invalid cone: " + why);
  }
  if (w->cone.m != d->m) throw std::runtime_error("cone dimensions do not match m");
  const int n = d->n, m = d->m;
  if (linsys == 2 && n > kDenseMaxN)
    throw std::runtime_error("hip_dense: n = " + std::to_string(n) + " exceeds " + std::to_string(kDenseMaxN) +
                             " (the explicit inverse of the reduced KKT matrix would need " + std::to_string((long)n * n * 8 / 1000000) +
                             " MB); use the indirect solver");
  w->linsys = linsys == 2 ? 1 : 0;
  w->n = n; w->m = m; w->l = (long)n + m + 1;
  w->stgs = *stgs;
  if (stgs->write_data_filename) w->write_data_filename = stgs->write_data_filename;
  if (stgs->log_csv_filename) w->log_csv_filename = stgs->log_csv_filename;
  w->stgs.write_data_filename = nullptr;
  w->stgs.log_csv_filename = nullptr;
  w->scale = stgs->scale;
  w->has_P = d->P != nullptr;
  if (!w->write_data_filename.empty()) write_problem_data(w->write_data_filename.c_str(), d, k, stgs);
  w->b_orig.assign(d->b, d->b + m);
  w->c_orig.assign(d->c, d->c + n);
  for (double x : w->b_orig) w->nm_b_orig = std::max(w->nm_b_orig, std::fabs(x));
  for (double x : w->c_orig) w->nm_c_orig = std::max(w->nm_c_orig, std::fabs(x));
  w->mats->b0 = w->b_orig;  // (host copies for scs_hip_clone: a clone starts from what scs_init was given)
  w->mats->c0 = w->c_orig;
  w->mats->bl0 = w->cone.bl;
  w->mats->bu0 = w->cone.bu;
  w->mats->stgs0 = w->stgs;
  w->mats->a_nnz_in = d->A->p[n];
  w->mats->p_nnz_in = d->P ? d->P->p[n] : 0;
  if (d->P) {  // (O(nnz(P)) over arrays validate_matrix has just walked)
    bool below = false, unsorted = false;
    for (int j = 0; j < n; ++j)
      for (scs_int p = d->P->p[j]; p < d->P->p[j + 1]; ++p) {
        below |= d->P->i[p] > j;
        unsorted |= p > d->P->p[j] && d->P->i[p] < d->P->i[p - 1];
      }
    if (below) w->mats->p_update_refusal = "P was given to scs_init with entries below the diagonal (they were ignored): its values cannot be updated in place";
    else if (unsorted) w->mats->p_update_refusal = "P was given to scs_init with row indices that do not ascend inside a column: its values cannot be updated in place";
  }
  if (d->P && stgs->normalize) {  // (scs_hip_update_matrix with one matrix kept re-equilibrates both: work.hpp MatrixSet::ax0)
    w->mats->ax0.assign(d->A->x, d->A->x + w->mats->a_nnz_in);
    w->mats->px0.assign(d->P->x, d->P->x + w->mats->p_nnz_in);
  }

  init_streams_and_pinned(w.get());
  hipStream_t s = w->stream;
  // small problems (config 5: a batch of them) take their device memory from one arena (common.hpp) instead of ~100
  // separate allocations
  {
    const long annz = d->A->p[n];
    if (annz <= (1L << 18) && w->l <= (1L << 17)) {
      w->arena.reset(new Arena());
      w->mats->home = w->arena;  // (the set's buffers live in it: it stays until the last user of the set is gone)
      w->arena->stream = s;
      w->arena->first_chunk = arena_first_chunk(w->l, stgs->acceleration_lookback, annz);
    }
  }
  ArenaScope arena_scope(w->arena.get());
  const bool setup_timing = (o.debug & DBG_SETUP) != 0;  // SCS_HIP_DEBUG=setup: where does scs_init spend its time
  double t_mark = now_ms();
  auto mark = [&](const char *what) {
    if (!setup_timing) return;
    HIP_CHECK(hipStreamSynchronize(s));
    const double t = now_ms();
    std::fprintf(stderr, "[scs-hip setup] %-34s %8.1f ms\n", what, t - t_mark);
    t_mark = t;
  };
  mark("validation, cone, host copies");

  // ---- matrices to HBM (raw): CSC(A) as CSR(A'), explicit CSR(A), full CSR(P) ----
  w->normalized = stgs->normalize != 0;
  // Device path (default): upload the caller's CSC once, transpose and (after the equilibration) build the
  // L2-blocked copies on the device; the host builders remain for SCS_HIP_SETUP=host and for rows too long to sort.
  const bool host_build = o.host_setup;
  bool slabs_pending = false;
  w->At.upload(n, m, d->A->p, d->A->i, d->A->x, s, o, /*allow_slab=*/host_build);
  mark("A' upload (+ slab build on the host)");
  HostCsr ar, pf;  // host copies of the index arrays: only filled on the host paths
  if (host_build || !w->Ar.transpose_from(w->At, s)) {
    csc_to_csr(m, n, d->A->p, d->A->i, d->A->x, ar);
    mark("CSC -> CSR on the host");
    w->Ar.upload(m, n, ar.rowptr.data(), ar.col.data(), ar.val.data(), s, o, /*allow_slab=*/host_build);
    mark("A upload (+ slab build on the host)");
    slabs_pending = !host_build;
  } else {
    mark("CSC -> CSR on the device");
    slabs_pending = true;
  }
  if (w->has_P) {
    std::vector<double> pdiag;
    sym_expand(n, d->P->p, d->P->i, d->P->x, pf, pdiag);
    w->Pf.upload(n, n, pf.rowptr.data(), pf.col.data(), pf.val.data(), s, o, /*allow_slab=*/host_build);
    w->px.alloc_zero(n, s);
  }
  if (w->cone.bsize > 1) {  // the caller's box bounds, before the row scaling touches the working copies
    w->box_bl_orig.upload(w->cone.bl.data(), w->cone.bl.size(), s);
    w->box_bu_orig.upload(w->cone.bu.data(), w->cone.bu.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));
  }
  // ---- K12: equilibrate on the device, in place in all resident layouts ----
  if (w->normalized) {
    device_normalize(w->At, w->Ar, w->has_P ? &w->Pf : nullptr, w->cone, w->D, w->E, s, o.norm_fuse);
    adopt_equilibration(w.get());
  }
  mark("equilibration (device)");
  for (DeviceCsr *M : {&w->At, &w->Ar, &w->Pf}) M->refresh_slab(s, true);
  if (slabs_pending) {
    // large matrices: column-sorted pass copy (spmv_cs.hpp), each built from the other orientation's CSR;
    // the L2-blocked slab copy only where the pattern does not fit that format
    // A' products feed the CG update, which takes Gp as the sum of two partial vectors: two workgroups per chunk
    if (!w->At.build_cs_dev(w->Ar, s, /*kind=*/1, o)) w->At.build_slab_dev(s, o);
    if (!w->Ar.build_cs_dev(w->At, s, /*kind=*/0, o)) w->Ar.build_slab_dev(s, o);
    if (w->has_P && !w->Pf.build_cs_dev(w->Pf, s, /*kind=*/2, o)) w->Pf.build_slab_dev(s, o);
  }
  if (host_build) {  // SCS_HIP_SETUP=host: the column-sorted copies from the host builder, on the equilibrated values
    std::vector<double> hv;
    auto host_cs = [&](DeviceCsr &M, const int *rp, const int *ci, int kind) {
      if (!M.cs_wanted_here(o)) return;
      hv.resize((size_t)M.nnz);
      M.val.download(hv.data(), (size_t)M.nnz, s);
      HIP_CHECK(hipStreamSynchronize(s));
      M.build_cs_host(rp, ci, hv.data(), s, kind, o);
    };
    host_cs(w->At, d->A->p, d->A->i, 1);
    host_cs(w->Ar, ar.rowptr.data(), ar.col.data(), 0);
    if (w->has_P) host_cs(w->Pf, pf.rowptr.data(), pf.col.data(), 2);
  }
  mark("column-sorted / L2-blocked copies, value refresh");
  if (w->has_P) {  // diagonal of the (scaled) P for the Jacobi preconditioner
    w->Pdiag.alloc_zero(n, s);
    hipLaunchKernelGGL(k_csr_diag, dim3(vec_blocks(n)), dim3(kVecThreads), 0, s, w->Pf.rowptr.p, w->Pf.col.p, w->Pf.val.p, n,
                       w->Pdiag.p);
  }
  init_state(w.get(), mark);
  w->setup_time = now_ms() - t0;
  return w.release();
}

// scs_hip_clone: a workspace in the state scs_init left `src` in — its original b, c and settings, cold start — on src's matrix set.
// The matrix part of scs_init is complete when scs_init returns (only R, the preconditioner / G^{-1} and g are ever deferred, and
// those are per-solve state), so there is nothing to finish first.
static ScsHipWork *clone_impl(ScsHipWork *src) {
  const double t0 = now_ms();
  if (!src) throw std::runtime_error("null argument");
  std::lock_guard<std::mutex> lock(src->mtx);
  HIP_CHECK(hipSetDevice(src->device));
  std::unique_ptr<ScsHipWork> w(new ScsHipWork(src->mats));  // (the set carries the parent's options snapshot: nothing of the environment is read)
  const MatrixSet &ms = *w->mats;
  w->device = src->device;
  w->cone = src->cone;  // (box bounds already follow the row scaling; nothing changes them after scs_init)
  w->n = src->n; w->m = src->m; w->l = src->l;
  w->linsys = src->linsys;
  w->stgs = ms.stgs0;   // (file names are not inherited: write_data_filename was served by scs_init, a log file has one writer)
  w->scale = w->stgs.scale;
  w->has_P = src->has_P;
  w->normalized = src->normalized;
  w->scal.D = src->scal.D;
  w->scal.E = src->scal.E;
  w->b_orig = ms.b0;
  w->c_orig = ms.c0;
  for (double x : w->b_orig) w->nm_b_orig = std::max(w->nm_b_orig, std::fabs(x));
  for (double x : w->c_orig) w->nm_c_orig = std::max(w->nm_c_orig, std::fabs(x));
  init_streams_and_pinned(w.get());
  hipStream_t s = w->stream;
  const int n = w->n;
  if (src->arena) {  // as the parent: its own arena, sized without the matrix layouts
    w->arena.reset(new Arena());
    w->arena->stream = s;
    w->arena->first_chunk = arena_first_chunk(w->l, w->stgs.acceleration_lookback, 0);
  }
  ArenaScope arena_scope(w->arena.get());
  ScsHipWork::ScratchTurn turn(w.get());
  if (w->has_P) w->px.alloc_zero(n, s);
  if (w->cone.bsize > 1) {  // the caller's box bounds (footer diagnostics)
    w->box_bl_orig.upload(ms.bl0.data(), ms.bl0.size(), s);
    w->box_bu_orig.upload(ms.bu0.data(), ms.bu0.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));
  }
  init_state(w.get(), [](const char *) {});
  w->setup_time = now_ms() - t0;
  return w.release();
}
