// device_csr.hpp — a matrix resident in HBM in every layout the mat-vec kernels read (CSR, slab, column-sorted passes) and its builders; the equilibration driver; the residual record
// (one of the units csrc/scs_hip.hip is assembled from — ONE translation unit, in this order: runtime.hpp, device_csr.hpp, work.hpp
// [+ work_linsys.inl, work_admm.inl, work_residuals.inl, work_solve_ends.inl], io.hpp, setup.hpp, loop.hpp, batch.hpp, the C ABI in scs_hip.hip,
// lab_entries.hpp; split out of the 3 800-line file of rounds 1-5 in round 6 — VERDICT r05 item 6 — without moving a line of code)
#pragma once
namespace scship {

// ---------------------------------------------------------------- device CSR
struct DeviceCsr {
  DevBuf<int> rowptr, col;
  DevBuf<int4> rowblk;
  DevBuf<double> val;
  int rows = 0, cols = 0, nblk = 0;
  long nnz = 0;
  // optional L2-blocked copy (spmv.hpp) used by the mat-vec kernels when the gather vector exceeds L2
  bool has_slab = false;
  DevBuf<int> s_segptr, s_col, s_perm;  // s_perm: source index of every slab entry in CSR order (-1 = padding)
  DevBuf<unsigned short> s_roff;
  DevBuf<double> s_val;
  int s_nchunks = 0, s_S = 0, s_R = 0, s_max_seg = 0;
  int s_shift = 0;  // log2 of the slab width the copy was built with (matrix_update.hpp re-derives the value map from it)
  // optional column-sorted pass copy (spmv_cs.hpp); preferred over the slab copy when both could be built
  DeviceCs cs;
  // rows too long for the layout's count fields are peeled off it (spmv_cs.hpp CsView::peel) and done over the plain CSR
  DevBuf<unsigned> peel_mask;
  DevBuf<int4> peel_blk;
  int npeel = 0, npeel_long = 0;
  long peel_nnz = 0;  // nonzeros in the peeled rows
  int cs_virt_lp = 0;  // piece length the virtual-row layout was accepted with (0: no virtual rows); matrix_update.hpp re-plans with it
  // Every builder below takes the options the layouts are built under (`o`: the matrix set's snapshot, work.hpp MatrixSet::opt — or a
  // kernel-level entry point's own): what a value map is later re-derived from must be what the layout was built with.
  // host: mark rows longer than `thresh`; one row block {row, row + 1, first nonzero, end} each.  false: nothing to peel
  bool make_peel(const int *rp_host, int thresh, hipStream_t s, const Options &o) {
    peel_mask.release(); peel_blk.release(); npeel = 0; npeel_long = 0; peel_nnz = 0;
    if (!o.cs_peel) return false;  // (labs) A/B: reject such patterns as round 1 did
    std::vector<int4> blk;
    std::vector<unsigned> mask;
    for (int r = 0; r < rows; ++r)
      if (rp_host[r + 1] - rp_host[r] > thresh) {
        if (mask.empty()) mask.assign(((size_t)rows + 31) / 32, 0u);
        mask[r >> 5] |= 1u << (r & 31);
        blk.push_back(int4{r, r + 1, rp_host[r], rp_host[r + 1]});
      }
    if (blk.empty()) return false;
    // the longest rows first (those > kPeelLongRow get a whole workgroup each in k_spmv_peeled; starting the long ones early
    // keeps the tail of the launch short), ties in row order: a fixed order, so the reduction partials are deterministic
    std::stable_sort(blk.begin(), blk.end(), [](const int4 &a, const int4 &b) { return a.w - a.z > b.w - b.z; });
    npeel_long = 0;
    for (const int4 &b : blk) { npeel_long += (b.w - b.z > kPeelLongRow) ? 1 : 0; peel_nnz += b.w - b.z; }
    npeel = (int)blk.size();
    peel_mask.upload(mask.data(), mask.size(), s);
    peel_blk.upload(blk.data(), blk.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));
    return true;
  }
  // ---- virtual rows (spmv_cs.hpp CsView::Rr): long rows cut into pieces that ride in the passes ----
  using VirtPlan = CsVirtPlan;
  // rows longer than max(lp, what a count field holds) nonzeros -> ceil(len / lp) pieces (rows a field holds stay whole and keep
  // the oracle's summation order; a piece's run is added by ONE lane, so pieces are short whatever the field would hold);
  // fills the peel mask / row blocks {row, row + 1, first piece, end}
  bool plan_virtual(const int *rp, int lp, VirtPlan &P, hipStream_t s, const Options &o) {
    clear_peel();
    if (!cs_plan_virtual(rp, rows, lp, std::max(lp, peel_threshold(1, o)), P, o.cs_rpt)) return false;
    npeel = (int)P.blk.size();
    npeel_long = 0;  // (a row's pieces are few: one wavefront adds them)
    peel_nnz = P.long_nnz;
    peel_mask.upload(P.mask.data(), P.mask.size(), s);
    peel_blk.upload(P.blk.data(), P.blk.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));
    return true;
  }
  void adopt_virtual(const VirtPlan &P, hipStream_t s) {
    cs.rows = rows;
    cs.Rr = P.Rr; cs.Rp = P.Rp; cs.npieces = P.V;
    cs.tpart.alloc_zero((size_t)P.V, s);
  }
  bool build_virtual_dev(const DeviceCsr &T, const int *rp, int lp, hipStream_t s, const Options &o) {
    VirtPlan P;
    if (!plan_virtual(rp, lp, P, s, o)) return false;
    DevBuf<int2> d_info;
    DevBuf<int> vslot;
    d_info.upload(P.rowinfo.data(), P.rowinfo.size(), s);
    vslot.alloc((size_t)nnz);
    hipLaunchKernelGGL(k_cs_vslot, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, s, T.rowptr.p, T.col.p, cols, (long)nnz, rowptr.p, col.p,
                       d_info.p, P.Rr, P.Rp, P.R, vslot.p);
    HIP_CHECK(hipStreamSynchronize(s));  // (P.rowinfo is read by the upload)
    const bool built = cs.build_from_transpose(P.nchunks * P.R, cols, T.rowptr.p, vslot.p, T.val.p, nnz, s, 1, nullptr, P.R, P.rpt);
    if (o.debug & DBG_SETUP)
      std::fprintf(stderr, "[scs-hip] column-sorted layout %d x %d: rows longer than %d in pieces of <= %d (%d rows, %ld of %ld nonzeros, %d pieces; chunks of %d + %d slots, %d rows per lane): %s\n",
                   rows, cols, std::max(lp, peel_threshold(1, o)), lp, npeel, peel_nnz, (long)nnz, P.V, P.Rr, P.Rp, P.rpt, built ? "built" : "a count field overflowed");
    if (!built) { clear_peel(); return false; }
    adopt_virtual(P, s);
    cs_virt_lp = lp;
    return true;
  }
  bool build_virtual_host(const int *rp, const int *ci, const double *v, int lp, hipStream_t s, HostCs &h, const Options &o) {
    VirtPlan P;
    if (!plan_virtual(rp, lp, P, s, o)) return false;
    if (!build_cs_virtual(rp, ci, v, rows, cols, P, h)) { clear_peel(); return false; }
    virt_host_plan = P;
    cs_virt_lp = lp;
    return true;
  }
  VirtPlan virt_host_plan;
  // pieces per pass to aim for (x the passes a chunk is expected to have = the piece length): smaller pieces, more slots
  std::vector<int> virt_piece_lengths() const {
    const long npass_est = std::max<long>(1, (long)nnz / kCsTargetWgs / kCsPass);
    std::vector<int> out;
    for (int per_pass : {24, 12, 6}) out.push_back((int)std::min<long>(per_pass * npass_est, 1L << 20));
    return out;
  }
  static constexpr int kPeelLadder[] = {32, 16, 8, 4, 2, 1};  // multiples of the count field's capacity tried as the peel threshold
  int peel_threshold(int split, const Options &o) const {
    int R, rpt;
    cs_pick_geometry(rows, R, rpt, split, o.cs_rpt);
    return cs_peel_threshold(rpt);
  }
  DevBuf<double> cs_part0, cs_part1;  // cs.split == 2 without the in-kernel combine: partial row sums (spmv.hpp EpiPartial / EpiGp::split)
  // Workgroups per row chunk.  kind: 0 = A (y-space products), 1 = A' (x-space products), 2 = P.  Taller chunks mean more
  // nonzeros per 128-byte line of the gather vector, i.e. fewer lines per gather instruction — the quantity that bounds
  // these kernels — at the price of partial row sums.  Default: only A' is split, in two, and hands its two partial
  // vectors to the CG update (EpiGp::split: Gp is linear in them) or to k_epi_finish — no combine pass.
  // SCS_HIP_CS_COMBINE=1: the partial sums of up to 4 parts are added INSIDE the kernel by the
  // last workgroup of a chunk to arrive, so every product — A too — may be split (SCS_HIP_CS_SPLIT_A / _AT).
  // Measured at the bench size (tools/cs_lab.hip): the 48 MB of partial-sum traffic and the 16-rows-per-lane row sums
  // eat the gather gain (A: 91.5 us unsplit, 95 us split in two + combine; A': 93 us two partial vectors, 100 us four
  // parts + combine) => off by default.
  // SCS_HIP_CS_SPLIT=0: one workgroup per row chunk everywhere (bit-exact sequential row sums; A/B)
  int cs_pick_split(int kind, const Options &o) const {
    if (!o.cs_split || o.cs_rpt > 0) return 1;
    if (!o.cs_combine) {  // (labs: the in-kernel combine)
      if (kind != 1) return 1;
      int R, rpt;
      cs_pick_geometry(rows, R, rpt, 2);
      return rpt <= 8 ? 2 : 1;
    }
    { const int v = kind == 0 ? o.cs_split_a : kind == 1 ? o.cs_split_at : 0; if (v == 1 || v == 2 || v == 4) return v; }
    for (int sp : {4, 2}) {
      int R, rpt;
      cs_pick_geometry(rows, R, rpt, sp);
      if ((long)R * (kCsTargetWgs / sp) >= rows && rpt <= 16 && R >= 64 * sp) return sp;  // the chunks still cover all rows in one wave of workgroups
    }
    return 1;
  }
  void cs_after_build(hipStream_t s, const Options &o) {
    cs_part0.release(); cs_part1.release();
    if (!cs.ok || cs.split <= 1) return;
    if (o.cs_combine) cs.enable_combine(s);
    else { cs_part0.alloc_zero((size_t)rows, s); cs_part1.alloc_zero((size_t)rows, s); }
  }
  // T = this matrix transposed (device CSR with the CURRENT values); host: build from this matrix's own host arrays.
  // the pass layout is used at all: SCS_HIP_CS=0 keeps the slab kernel, SCS_HIP_SLAB=0 the CSR-stream kernel (A/B measurements)
  bool cs_wanted_here(const Options &o) const { return o.cs && o.slab && cs_wanted(rows, nnz, o.cs_min_nnz); }
  bool build_cs_dev(const DeviceCsr &T, hipStream_t s, int kind, const Options &o) {
    cs.release();
    peel_mask.release(); peel_blk.release(); npeel = 0; npeel_long = 0;
    if (!cs_wanted_here(o)) return false;
    bool ok = false;
    const int sp = cs_pick_split(kind, o);
    std::vector<int> rp((size_t)rows + 1);  // row lengths decide what is peeled (O(rows) at init)
    rowptr.download(rp.data(), rp.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));
    // For every split candidate: first WITHOUT peeling — what the count fields limit is a row's nonzeros inside ONE
    // pass, and a long row whose columns are spread out (a uniformly denser matrix: 100 nonzeros per row over 1e6
    // columns) has ~1 per pass — then, if a count overflowed, with the rows longer than a count field peeled off; and
    // a layout whose peeled rows hold most of the nonzeros is not kept (the side launch would be the product).
    auto attempt = [&](int split) {
      clear_peel();
      if (cs.build_from_transpose(rows, cols, T.rowptr.p, T.col.p, T.val.p, nnz, s, split, nullptr, 0, o.cs_rpt)) return true;
      // the long rows cut into pieces that ride in the passes (one workgroup per chunk: split 1) ...
      if (o.cs_virt)  // (labs) SCS_HIP_CS_VIRT=0: long rows go to the CSR-stream side launch whole (round 2)
        for (int lp : virt_piece_lengths())
          if (build_virtual_dev(T, rp.data(), lp, s, o)) return true;
      // ... or, failing that, peeled as FEW rows as the count fields allow: a row of 500 nonzeros has ~50 in each of its chunk's ten passes and
      // rides in them (its gathers share lines with the other rows' there); thresholds from 32 x the field down to the field
      for (int mult : kPeelLadder) {
        if (!make_peel(rp.data(), peel_threshold(split, o) * mult, s, o)) continue;  // (no row that long: next rung)
        if (peel_nnz > (nnz / 5) * 3) { clear_peel(); return false; }
        const bool built = cs.build_from_transpose(rows, cols, T.rowptr.p, T.col.p, T.val.p, nnz, s, split, peel_mask.p, 0, o.cs_rpt);
        if (o.debug & DBG_SETUP)
          std::fprintf(stderr, "[scs-hip] column-sorted layout %d x %d, split %d: rows longer than %d peeled (%d rows, %ld of %ld nonzeros): %s\n",
                       rows, cols, split, peel_threshold(split, o) * mult, npeel, peel_nnz, (long)nnz, built ? "built" : "a count field overflowed");
        if (built) return true;
      }
      clear_peel();
      return false;
    };
    if (sp > 1) ok = attempt(sp);
    if (!ok) ok = attempt(1);
    if (!ok) clear_peel();
    cs_after_build(s, o);
    return ok;
  }
  void clear_peel() { peel_mask.release(); peel_blk.release(); npeel = 0; npeel_long = 0; peel_nnz = 0; cs_virt_lp = 0; }
  bool build_cs_host(const int *rp, const int *ci, const double *v, hipStream_t s, int kind, const Options &o) {
    cs.release();
    peel_mask.release(); peel_blk.release(); npeel = 0; npeel_long = 0;
    if (!cs_wanted_here(o)) return false;
    HostCs h;
    bool ok = false, virt_host = false;
    const int sp = cs_pick_split(kind, o);
    auto attempt = [&](int split) {  // same policy as build_cs_dev: unpeeled first, then the long rows peeled, capped
      clear_peel();
      if (build_cs(rp, ci, v, rows, cols, h, o.cs_rpt, split, nullptr)) return true;
      if (o.cs_virt)
        for (int lp : virt_piece_lengths())
          if (build_virtual_host(rp, ci, v, lp, s, h, o)) { virt_host = true; return true; }
      for (int mult : kPeelLadder) {
        const int thresh = peel_threshold(split, o) * mult;
        if (!make_peel(rp, thresh, s, o)) continue;
        if (peel_nnz > (nnz / 5) * 3) { clear_peel(); return false; }
        std::vector<unsigned> mk(((size_t)rows + 31) / 32, 0u);
        for (int r = 0; r < rows; ++r)
          if (rp[r + 1] - rp[r] > thresh) mk[r >> 5] |= 1u << (r & 31);
        if (build_cs(rp, ci, v, rows, cols, h, o.cs_rpt, split, mk.data())) return true;
      }
      clear_peel();
      return false;
    };
    if (sp > 1) ok = attempt(sp);
    if (!ok) ok = attempt(1);
    if (!ok) { clear_peel(); return false; }
    cs.from_host(h, s);
    if (virt_host) adopt_virtual(virt_host_plan, s);
    cs_after_build(s, o);
    return true;
  }
  void set_rowblocks(const int *rp_host, hipStream_t s) {
    std::vector<int4> rb = build_rowblocks(rp_host, rows);
    nblk = (int)rb.size();
    rowblk.upload(rb.data(), rb.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));  // rb is a local
  }
  // (o.host_setup — SCS_HIP_SETUP=host — builds the slab copy on the host: fallback / A-B / tests)
  void upload(int rows_, int cols_, const int *rp, const int *ci, const double *v, hipStream_t s, const Options &o, bool allow_slab = true) {
    rows = rows_; cols = cols_; nnz = rp[rows_];
    rowptr.upload(rp, rows + 1, s);
    col.upload(ci, nnz, s);
    val.upload(v, nnz, s);
    set_rowblocks(rp, s);
    has_slab = false;
    if (allow_slab && slab_wanted(rows, cols) && o.slab) {  // SCS_HIP_SLAB=0 forces the plain CSR-stream kernel (A/B measurements)
      if (!o.host_setup) {
        build_slab_dev(s, o);
      } else {
        HostSlab hs;
        std::vector<int> src;
        if (build_slab(rp, ci, v, rows, cols, hs, &src)) {
          s_perm.upload(src.data(), src.size(), s);
          s_segptr.upload(hs.segptr.data(), hs.segptr.size(), s);
          s_roff.upload(hs.roff.data(), hs.roff.size(), s);
          s_col.upload(hs.col.data(), hs.col.size(), s);
          s_val.upload(hs.val.data(), hs.val.size(), s);
          s_nchunks = hs.nchunks; s_S = hs.S; s_R = hs.R; s_max_seg = hs.max_seg; s_shift = kSlabShift;
          has_slab = true;
          HIP_CHECK(hipStreamSynchronize(s));  // hs is a local
        }
      }
    }
    HIP_CHECK(hipStreamSynchronize(s));
  }
  // this = src' on the device (setup_dev.hpp).  false: a row is too long for the one-lane sort (caller falls back).
  bool transpose_from(const DeviceCsr &src, hipStream_t s) {
    rows = src.cols; cols = src.rows; nnz = src.nnz;
    rowptr.alloc_zero((size_t)rows + 1, s);
    col.alloc_zero((size_t)std::max(nnz, 1L), s);
    val.alloc_zero((size_t)std::max(nnz, 1L), s);
    DevBuf<int> cursor, perm, tmp, flag;
    cursor.alloc_zero((size_t)rows + 1, s);
    perm.alloc_zero((size_t)std::max(nnz, 1L), s);
    tmp.alloc_zero((size_t)(rows / kScanTile + 4), s);
    flag.alloc_zero(1, s);
    if (nnz > 0) hipLaunchKernelGGL(k_count_index, dim3(vec_blocks(nnz)), dim3(kVecThreads), 0, s, src.col.p, nnz, cursor.p);
    device_exclusive_scan(cursor.p, rowptr.p, rows, tmp.p, s);
    HIP_CHECK(hipMemcpyAsync(cursor.p, rowptr.p, sizeof(int) * rows, hipMemcpyDeviceToDevice, s));
    // small matrices: a wavefront per row (setup_dev.hpp; the same result, a shorter link in the dispatch chain of a small scs_init)
    const bool per_wave = std::max(rows, src.rows) <= kTransposeWaveRows;
    if (per_wave) {
      const int wpb = kVecThreads / 64;
      hipLaunchKernelGGL(k_transpose_scatter_w, dim3(std::max(1, std::min(ceil_div(src.rows, wpb), kMaxVecBlocks))), dim3(kVecThreads), 0, s, src.rowptr.p,
                         src.col.p, src.rows, cursor.p, col.p, perm.p);
      hipLaunchKernelGGL(k_sort_rows_w, dim3(std::max(1, std::min(ceil_div(rows, wpb), kMaxVecBlocks))), dim3(kVecThreads), 0, s, rowptr.p, col.p, perm.p, rows,
                         flag.p);
    } else {
      hipLaunchKernelGGL(k_transpose_scatter, dim3(vec_blocks(src.rows)), dim3(kVecThreads), 0, s, src.rowptr.p, src.col.p, src.rows,
                         cursor.p, col.p, perm.p);
      hipLaunchKernelGGL(k_sort_rows, dim3(vec_blocks(rows)), dim3(kVecThreads), 0, s, rowptr.p, col.p, perm.p, rows, flag.p);
    }
    if (nnz > 0) hipLaunchKernelGGL(k_gather_f64, dim3(vec_blocks(nnz)), dim3(kVecThreads), 0, s, val.p, src.val.p, perm.p, nnz);
    int too_long = 0;
    std::vector<int> rp((size_t)rows + 1);
    HIP_CHECK(hipMemcpyAsync(&too_long, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    rowptr.download(rp.data(), rp.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));
    if (too_long) return false;
    set_rowblocks(rp.data(), s);
    has_slab = false;
    return true;
  }
  // L2-blocked copy of the CURRENT csr arrays, built on the device (same layout as spmv.hpp build_slab)
  void build_slab_dev(hipStream_t s, const Options &o) {
    has_slab = false;
    if (!slab_wanted(rows, cols) || !o.slab) return;
    SlabGeom g;
    g.rows = rows; g.cols = cols; g.R = slab_pick_rows(rows); g.shift = kSlabShift;
    g.S = (int)(((long)cols + (1L << g.shift) - 1) >> g.shift);
    g.nchunks = (rows + g.R - 1) / g.R;
    const long nseg = (long)g.nchunks * g.S;
    DevBuf<int> seg_size, tmp, flag;
    seg_size.alloc_zero((size_t)nseg + 1, s);
    tmp.alloc_zero((size_t)(nseg / kScanTile + 4), s);
    flag.alloc_zero(1, s);
    s_roff.alloc_zero((size_t)nseg * (g.R + kSlabRoffPad), s);
    s_segptr.alloc_zero((size_t)nseg + 1, s);
    hipLaunchKernelGGL(k_slab_count, dim3(vec_blocks(rows)), dim3(kVecThreads), 0, s, rowptr.p, col.p, g, s_roff.p, flag.p);
    hipLaunchKernelGGL(k_slab_scan, dim3((unsigned)nseg), dim3(kScanThreads), 0, s, g, s_roff.p, seg_size.p, flag.p);
    device_exclusive_scan(seg_size.p, s_segptr.p, nseg, tmp.p, s);
    std::vector<int> sizes((size_t)nseg);
    int total = 0, overflow = 0;
    HIP_CHECK(hipMemcpyAsync(sizes.data(), seg_size.p, sizeof(int) * nseg, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&total, s_segptr.p + nseg, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&overflow, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    long check = 0;
    int max_seg = 0;
    for (int v : sizes) { check += v; max_seg = std::max(max_seg, v); }
    if (overflow || check != (long)total || check > 2000000000L) {  // uint16 offsets or int32 positions do not fit: no slab copy
      s_roff.release(); s_segptr.release();
      return;
    }
    s_col.alloc_zero((size_t)std::max(total, 1), s);
    s_val.alloc_zero((size_t)std::max(total, 1), s);
    hipLaunchKernelGGL(k_slab_fill, dim3(vec_blocks(rows)), dim3(kVecThreads), 0, s, rowptr.p, col.p, val.p, g, s_roff.p, s_segptr.p,
                       s_col.p, s_val.p);
    hipLaunchKernelGGL(k_slab_pad, dim3(vec_blocks(nseg)), dim3(kVecThreads), 0, s, g, s_roff.p, s_segptr.p, s_col.p, s_val.p);
    HIP_CHECK(hipStreamSynchronize(s));
    s_nchunks = g.nchunks; s_S = g.S; s_R = g.R; s_max_seg = max_seg; s_shift = g.shift;
    has_slab = true;
  }
  // ---- value maps of the EXISTING layout copies (matrix_update.hpp): where every stored value slot takes its value from ----
  // pass layout: positions in T.val (T = the CSR the layout was built from), through the builder re-run in map-only mode with the
  // layout's own geometry — the resident peel mask, or the row slots of the virtual rows re-planned with the accepted piece length
  bool build_cs_value_map(const DeviceCsr &T, hipStream_t s, DevBuf<int> &map, const Options &o) const {
    if (!cs.ok) return false;
    if (cs_virt_lp <= 0) return cs.build_value_map(T.rowptr.p, T.col.p, nnz, s, npeel > 0 ? peel_mask.p : nullptr, map);
    std::vector<int> rp((size_t)rows + 1);
    rowptr.download(rp.data(), rp.size(), s);
    HIP_CHECK(hipStreamSynchronize(s));
    VirtPlan P;
    if (!cs_plan_virtual(rp.data(), rows, cs_virt_lp, std::max(cs_virt_lp, peel_threshold(1, o)), P, o.cs_rpt)) return false;
    if (P.R != cs.R || P.rpt != cs.rpt || P.nchunks != cs.nchunks || P.Rr != cs.Rr || P.Rp != cs.Rp || P.V != cs.npieces) return false;
    DevBuf<int2> d_info;
    DevBuf<int> vslot;
    d_info.upload(P.rowinfo.data(), P.rowinfo.size(), s);
    vslot.alloc((size_t)nnz);
    hipLaunchKernelGGL(k_cs_vslot, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, s, T.rowptr.p, T.col.p, cols, (long)nnz, rowptr.p, col.p,
                       d_info.p, P.Rr, P.Rp, P.R, vslot.p);
    HIP_CHECK(hipStreamSynchronize(s));  // (P.rowinfo is read by the upload)
    return cs.build_value_map(T.rowptr.p, vslot.p, nnz, s, nullptr, map);  // (synchronises: vslot is a local)
  }
  // slab copy: positions in this matrix's own CSR values, through the resident row offsets and segment pointers
  void build_slab_value_map(hipStream_t s, DevBuf<int> &map) const {
    map.alloc(s_val.n);
    HIP_CHECK(hipMemsetAsync(map.p, 0xFF, sizeof(int) * std::max<size_t>(s_val.n, 1), s));  // -1: padding
    SlabGeom g;
    g.rows = rows; g.cols = cols; g.R = s_R; g.shift = s_shift; g.S = s_S; g.nchunks = s_nchunks;
    hipLaunchKernelGGL(k_slab_fill_map, dim3(vec_blocks(rows)), dim3(kVecThreads), 0, s, rowptr.p, col.p, g, s_roff.p, s_segptr.p, map.p);
    HIP_CHECK(hipStreamSynchronize(s));
  }
  SpmvMat view() const {
    SpmvMat M;
    M.csr = CsrView{rowptr.p, col.p, val.p, rowblk.p, rows, cols, nblk, nnz};
    M.use_slab = has_slab;
    if (has_slab) M.slab = SlabView{s_segptr.p, s_roff.p, s_col.p, s_val.p, rows, cols, s_nchunks, s_S, s_R, s_max_seg};
    M.use_cs = cs.ok;
    if (cs.ok) {
      M.cs = cs.view(); M.part0 = cs_part0.p; M.part1 = cs_part1.p;
      M.cs.peel = npeel > 0 ? peel_mask.p : nullptr;
      M.peel_blk = peel_blk.p;
      M.npeel = npeel;
      M.nlong = npeel_long;
    }
    return M;
  }
  int nwg() const { return cs.ok ? (cs.combine() ? cs.nchunks : cs.nchunks * cs.split) + peel_wgs_for(npeel, npeel_long) : has_slab ? s_nchunks : nblk; }
  // after the CSR values were rescaled on the device: refresh the slab copy and drop the index map
  void refresh_slab(hipStream_t s, bool drop_perm) {
    if (!has_slab || s_perm.n == 0) return;  // (device-built slabs are made from the already equilibrated values)
    const long cnt = (long)s_val.n;
    hipLaunchKernelGGL(k_gather_vals, dim3(vec_blocks(cnt)), dim3(kVecThreads), 0, s, s_val.p, val.p, s_perm.p, cnt);
    if (drop_perm) {
      HIP_CHECK(hipStreamSynchronize(s));
      s_perm.release();
    }
  }
};

// K12 on the device: equilibrate the three resident layouts in place; D (m) and E (n) accumulate the scalings.
// fused_finish = Options::norm_fuse ((labs) SCS_HIP_NORM_FUSE=0: the four launches of rounds 1-4; A/B, same bits)
static void device_normalize(DeviceCsr &At, DeviceCsr &Ar, DeviceCsr *Pf, const HostCone &cone, DevBuf<double> &D,
                             DevBuf<double> &E, hipStream_t s, bool fused_finish) {
  const int m = Ar.rows, n = At.rows;
  DevBuf<double> Dt, Et, Ep;
  Dt.alloc(m);
  Et.alloc(n);
  if (Pf) Ep.alloc(n);
  D.alloc(m);
  E.alloc(n);
  hipLaunchKernelGGL(k_fill, dim3(vec_blocks(m)), dim3(kVecThreads), 0, s, D.p, 1.0, (long)m);
  hipLaunchKernelGGL(k_fill, dim3(vec_blocks(n)), dim3(kVecThreads), 0, s, E.p, 1.0, (long)n);
  // non-separable cone blocks (everything after the z/l/box rows)
  // (every block behind the separable rows, the one-row ones too: normalize_dev.hpp k_pass_finish)
  std::vector<int> boff, blen;
  const int prefix = (int)std::min<long>(cone.boundaries[0], m);
  long count = cone.boundaries[0];
  for (size_t i = 1; i < cone.boundaries.size(); ++i) {
    if (cone.boundaries[i] >= 1) { boff.push_back((int)count); blen.push_back(cone.boundaries[i]); }
    count += cone.boundaries[i];
  }
  DevBuf<int> dboff, dblen;
  const int nblocks = (int)boff.size();
  if (nblocks) { dboff.upload(boff.data(), boff.size(), s); dblen.upload(blen.data(), blen.size(), s); }
  // norms of pass p+1 come out of the rescale sweep of pass p (k_rescale_norm); the very first norms need their own sweep
  DevBuf<double> Dn, En;
  Dn.alloc(m);
  En.alloc(n);
  auto sweep = [&](DeviceCsr &M, const double *rs, const double *cs, int l2, double *out) {
    if (M.nblk > 0)
      hipLaunchKernelGGL(k_rescale_norm, dim3(M.nblk), dim3(kSpmvThreads), 0, s, M.view().csr, M.val.p, rs, cs, l2, out);
  };
  // (the sweeps of a pass are independent of each other: one launch for all of them, normalize_dev.hpp k_rescale_norm3)
  auto sweeps = [&](const double *Dfac, const double *Efac, int l2, double *Dout, double *Eout, double *Pout) {
    if (!fused_finish) {
      sweep(Ar, Dfac, Efac, l2, Dout);
      sweep(At, Efac, Dfac, l2, Eout);
      if (Pf) sweep(*Pf, Efac, Efac, l2, Pout);
      return;
    }
    const int n1 = Ar.nblk, n2 = At.nblk, n3 = Pf ? Pf->nblk : 0;
    if (n1 + n2 + n3 <= 0) return;
    const CsrView v1 = Ar.view().csr, v2 = At.view().csr, v3 = Pf ? Pf->view().csr : v1;
    hipLaunchKernelGGL(k_rescale_norm3, dim3(n1 + n2 + n3), dim3(kSpmvThreads), 0, s, v1, Ar.val.p, Dfac, Efac, Dout, n1, v2, At.val.p, Efac, Dfac, Eout, n2,
                       v3, Pf ? Pf->val.p : (double *)nullptr, Efac, Efac, Pout, l2);
  };
  sweeps(nullptr, nullptr, 0, Dt.p, Et.p, Pf ? Ep.p : nullptr);
  for (int pass = 0; pass < 26; ++pass) {
    const int l2 = pass >= 25 ? 1 : 0;
    const int l2_next = pass + 1 >= 26 ? -1 : (pass + 1 >= 25 ? 1 : 0);
    if (Pf) hipLaunchKernelGGL(k_combine, dim3(vec_blocks(n)), dim3(kVecThreads), 0, s, Et.p, Ep.p, n, l2);
    if (fused_finish) {
      const int nbD = prefix > 0 ? vec_blocks(prefix) : 0, nbE = vec_blocks(n), nbB = ceil_div(nblocks, kVecThreads / 64);
      hipLaunchKernelGGL(k_pass_finish, dim3(nbD + nbE + nbB), dim3(kVecThreads), 0, s, Dt.p, D.p, prefix, Et.p, E.p, n, (const int *)dboff.p,
                         (const int *)dblen.p, nblocks, l2, nbD, nbE);
    } else {
      if (l2) {
        hipLaunchKernelGGL(k_sqrt_inplace, dim3(vec_blocks(m)), dim3(kVecThreads), 0, s, Dt.p, m);
        hipLaunchKernelGGL(k_sqrt_inplace, dim3(vec_blocks(n)), dim3(kVecThreads), 0, s, Et.p, n);
      }
      if (nblocks)
        hipLaunchKernelGGL(k_enforce_blocks, dim3(ceil_div(nblocks, kVecThreads / 64)), dim3(kVecThreads), 0, s, Dt.p, dboff.p,
                           dblen.p, nblocks, l2);
      hipLaunchKernelGGL(k_invsqrt_acc, dim3(vec_blocks(m)), dim3(kVecThreads), 0, s, Dt.p, D.p, m);
      hipLaunchKernelGGL(k_invsqrt_acc, dim3(vec_blocks(n)), dim3(kVecThreads), 0, s, Et.p, E.p, n);
    }
    sweeps(Dt.p, Et.p, l2_next, Dn.p, En.p, Pf ? Ep.p : nullptr);
    std::swap(Dt.p, Dn.p);
    std::swap(Et.p, En.p);
  }
  HIP_CHECK(hipStreamSynchronize(s));  // Dt/Et/Ep and the block arrays are locals
}

// b_hat = sigma D b, c_hat = sigma E c on the device vector h = [c; b]; returns sigma
static double device_normalize_b_c(DevBuf<double> &h, int n, int m, const DevBuf<double> &D, const DevBuf<double> &E,
                                   DevBuf<double> &part, double *h_pin, hipStream_t s) {
  const int nbn = vec_blocks(n), nbm = vec_blocks(m);
  hipLaunchKernelGGL(k_scale_by_vec, dim3(nbn), dim3(kVecThreads), 0, s, h.p, E.p, n, part.p);
  hipLaunchKernelGGL(k_scale_by_vec, dim3(nbm), dim3(kVecThreads), 0, s, h.p + n, D.p, m, part.p + kMaxVecBlocks);
  std::vector<double> pm(2 * kMaxVecBlocks, 0.0);
  HIP_CHECK(hipMemcpyAsync(pm.data(), part.p, sizeof(double) * 2 * kMaxVecBlocks, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  double nc = 0., nb = 0.;
  for (int i = 0; i < nbn; ++i) nc = std::max(nc, pm[i]);
  for (int i = 0; i < nbm; ++i) nb = std::max(nb, pm[kMaxVecBlocks + i]);
  double sigma = std::max(nc, nb);
  sigma = sigma < 1e-4 ? 1.0 : sigma;
  sigma = sigma > 1e4 ? 1e4 : sigma;
  sigma = safediv_pos(1.0, sigma);
  hipLaunchKernelGGL(k_scale_scalar, dim3(vec_blocks((long)n + m)), dim3(kVecThreads), 0, s, h.p, sigma, (long)n + m);
  (void)h_pin;
  return sigma;
}

struct Residuals {
  int last_iter = -1;
  double tau = 0, kap = 0;
  double nm_pri_n = 0, nm_dual_n = 0;  // normalised ||Ax+s-b tau||, ||Px+A'y+c tau||
  double nm_ax_s_btau = 0, nm_ax_s = 0, nm_ax = 0, nm_s = 0;
  double nm_px_aty_ctau = 0, nm_px = 0, nm_aty = 0;
  double bty_tau = 0, ctx_tau = 0, xt_p_x_tau = 0;
  double bty = 0, ctx = 0, xt_p_x = 0, gap = 0, pobj = 0, dobj = 0;
  double res_pri = 0, res_dual = 0, res_infeas = NAN, res_unbdd_a = NAN, res_unbdd_p = NAN;
  // extras for the CSV log (normalised space and 2-norms)
  double sq_pri_n = 0, sq_pri_o = 0, sq_dual_n = 0, sq_dual_o = 0, nm_ax_s_n = 0, nm_px_n = 0, nm_aty_n = 0;
  double bty_tau_n = 0, ctx_tau_n = 0, xt_p_x_tau_n = 0, kap_n = 0;
};

}  // namespace scship
