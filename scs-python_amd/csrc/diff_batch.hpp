// diff_batch.hpp — grouped derivative: G equally shaped, solved workspaces are differentiated in lock step, ONE launch per kernel of
// the LSQR iteration for the whole group (include/scs_hip.h: scs_hip_adjoint_batch[_device], scs_hip_derivative_batch[_device]).
//
// The reason is the one of batch.hpp: a small problem's LSQR iteration is 10-16 dependent launches of ~5 us, a hardware queue retires
// them one after the other, so K members differentiated in turn are bound by the command queue.  The means are the ones of batch.hpp
// too: every kernel of diff.hpp / lsqr.hpp / dproj.hpp / dproj_psd.hpp is a __device__ body with its one-problem entry k_X and the
// generic entry k_grouped<d_X, ..> (blockIdx.y = member, blockIdx.x = what the one-problem launch uses, arguments from a per-member
// record).  Same code, same block decomposition, same partial sums => every member's outputs, iteration count, stopping rule and
// residual figures are bit-identical to a call of its own (tests/test_adjoint_batch_gpu.py).
//
// GroupDiff::run and diff_impl are the two ways to issue one call, and they read the same definitions (diff.hpp): the limits
// (DiffLimits), the cone plan (diff_plan), the buffer assignments and the order of a product's pieces (DiffWiring, DiffProduct), the
// host control of the iteration (lsqr_drive) and the reported figures (diff_fill_info).  What differs is only that diff_impl launches
// k_X with a member's arguments where run writes them into the member's record of the table of d_X.  The members share the iteration
// index k (a launch-level argument of the two LSQR kernels: k_grouped_k); a member that has converged drops out of the member list,
// and until the host has seen its flag its kernels return at once on its own done flag.  Per chunk of iterations ONE gather launch
// and ONE copy of G x LF_COUNT ints cross the host.  Each member keeps its own DiffScratch; the group owns the argument tables, the
// member lists and the two gathered blocks, and gives its device blocks back to the block pool when the call ends.
//
// A member is a (workspace, lane) pair (lsqr.hpp DiffLane).  In a batch every member is lane 0 of a workspace of its own.  In a multi
// call (scs_hip_adjoint_multi: K directions at ONE solution, one_work) the members are lanes 0 .. K-1 of one workspace: the preparation
// runs for member 0 alone (it writes what belongs to the solution), every other table holds one record per lane as ever, and the three
// SpMVs of a product go through k_spmv_stream_lanes (spmv_lanes.hpp), which reads the one matrix once per tile of lanes.  Iteration
// state, stopping rule, done flag and the member list work per lane exactly as they work per workspace.
#pragma once

namespace scship {

// a table body whose FIRST argument is launch-level (the same for every member): the LSQR iteration index
template <auto Fn, int Threads, class... A>
__global__ __launch_bounds__(Threads) void k_grouped_k(const Pack<A...> *tab, const int *list, int k) {
  pack_call(Fn, tab[list[blockIdx.y]], k);
}
template <auto Fn, int Threads, class... A> GTable<Fn, Threads, A...> gtable_k_of(void (*)(int, A...));
#define SCS_GTABLE_K(threads, ...) decltype(gtable_k_of<__VA_ARGS__, threads>(__VA_ARGS__))
template <auto Fn, int Threads, class... A>
inline void launch_grouped_k(const GTable<Fn, Threads, A...> &t, const int *list, int cnt, int k, hipStream_t s) {
  if (!t.used || cnt <= 0 || t.gx <= 0) return;
  hipLaunchKernelGGL((k_grouped_k<Fn, Threads, A...>), dim3((unsigned)t.gx, (unsigned)cnt), dim3(Threads), t.lds, s,
                     (const Pack<A...> *)t.dev.p, list, k);
}

static std::atomic<long> g_diff_group_launches{0};  // scs_hip_diff_group_launches(): tests, tools/adjoint_batch_bench.py
static std::atomic<long> g_diff_group_syncs{0};     // scs_hip_diff_group_syncs(): host synchronisations of the groups (tools/refine_batch_timing.py)
// lanes of one workspace per workgroup of the lanes' product (spmv_lanes.hpp): 4 or 8.  4 by the table of profiles/adjoint_multi.txt
// (the measured problems have few row blocks: at tile 8 half as many workgroups each serve twice the lanes in turn, and a call of
// K >= 8 lanes took 1.2 - 1.4 times as long); scs_hip_diff_lane_tile() moves it for tools/adjoint_multi_bench.py, which measures both.
static std::atomic<int> g_diff_lane_tile{4};

constexpr size_t kDiffPsdBorrowMax = (size_t)256 << 20;  // K9-layout scratch borrowed at once by the grouped decomposition (bytes)

struct GroupDiff {
  // A member is (workspace, lane): a batch has G workspaces on their lane 0; a multi call (scs_hip_adjoint_multi, one_work) has ONE
  // solved workspace whose K directions are the members W[g] = w, lane[g] = g.  Then the preparation — what belongs to the solution —
  // runs for member 0 alone, and the three products of a DiffProduct read the matrix once per lane tile (spmv_lanes.hpp).
  std::vector<ScsHipWork *> W;
  std::vector<int> lane;  // empty: every member on lane 0
  bool one_work = false;
  std::vector<DiffCall> calls;
  std::vector<ScsHipDiffInfo *> infos;
  bool adjoint = true;
  int G = 0, n = 0, m = 0;
  long N = 0;
  bool has_P = false;
  hipStream_t s = nullptr;

  // one apply of W (dproj.hpp launch_dproj) over the group
  struct DprojTabs {
    SCS_GTABLE(kVecThreads, d_dproj_zl) zl;
    SCS_GTABLE(kDprojPsdThreads, d_dproj_psd_fused) psd;
    SCS_GTABLE(kConeThreads, d_dproj_soc_wave) soc;
    SCS_GTABLE(kConeThreads, d_dproj_soc_block) soc_big;
    SCS_GTABLE(kBoxThreads, d_dbox) box;  // (one workgroup: a box above kDboxMultiMin keeps its member solo, member_ok)
    SCS_GTABLE(kConeThreads, d_dproj_sym3) sym3;
    void size(const DprojPlan &p, size_t G) {
      if (p.z + p.l > 0) { zl.resize(G); zl.gx = vec_blocks(p.z + p.l); }
      if (p.psd.n_small > 0) { psd.resize(G); psd.gx = ceil_div(p.psd.n_small, kDprojPsdThreads / 64); psd.lds = kDprojPsdFusedLds; }
      if (p.n_soc > 0) { soc.resize(G); soc.gx = soc_wave_blocks(p.n_soc, p.G); }
      if (p.n_soc > 0 && p.n_soc_big > 0) { soc_big.resize(G); soc_big.gx = p.n_soc_big; }
      if (p.box.bsize > 0) { box.resize(G); box.gx = 1; }
      if (p.sym3.count > 0) { sym3.resize(G); sym3.gx = ceil_div(p.sym3.count, kConeThreads); }
    }
    void set(int g, const DprojPlan &p, const DprojIo &io, const int *done) {
      if (zl.used) zl.set(g, io, p.vh, p.z, p.l, done);
      if (psd.used) psd.set(g, io, p.psd, done);
      if (soc.used) soc.set(g, io, p.vh, (const double *)p.cinfo, p.off, p.dim, p.n_soc, p.G, done);
      if (soc_big.used) soc_big.set(g, io, p.vh, (const double *)p.cinfo, p.off, p.dim, p.big, done);
      if (box.used) box.set(g, io, p.vh + p.box.off, p.box.bl, p.box.bu, p.box.bsize, p.box.off, (const double *)p.box.st, done);
      if (sym3.used) sym3.set(g, io, (const double *)p.sym3.W, p.sym3.count, p.sym3.off, done);
    }
  };
  // one product of the operator over the group: every member's DiffProduct (diff.hpp), which also says in which order the pieces go
  struct ProdTabs {
    DprojTabs dp;
    SCS_GTABLE(kSpmvThreads, d_spmv_stream<EpiStore>) ar, at, pf;
    bool transposed = false;
    void set(int g, const ScsHipWork *w, const DprojPlan &plan, const DiffProduct &p, const int *done) {
      transposed = p.transposed;
      dp.set(g, plan, p.io, done);
      ar.set(g, csr_of(w->Ar), p.ar.in, p.ar.out, done, nullptr);
      at.set(g, csr_of(w->At), p.at.in, p.at.out, done, nullptr);
      if (w->has_P) pf.set(g, csr_of(w->Pf), p.pf.in, p.pf.out, done, nullptr);
    }
  };

  SCS_GTABLE(kVecThreads, d_dproj_vhat) t_vhat;
  SCS_GTABLE(kConeThreads, d_dproj_prep_wave) t_prep_wave;
  SCS_GTABLE(kConeThreads, d_dproj_prep_block) t_prep_block;
  SCS_GTABLE(kBoxThreads, d_dbox_prep) t_box_prep;
  SCS_GTABLE(kConeThreads, d_dpow_prep) t_pow_prep;
  SCS_GTABLE(kVecThreads, d_copy_f64) t_psd_copy, t_copy_out0, t_copy_out1, t_gather_st;
  SCS_GTABLE(kPsdThreads, d_proj_psd<0>) t_psd_eig;
  SCS_GTABLE(kDprojPsdThreads, d_dproj_psd_gather) t_psd_gather;
  SCS_GTABLE(kVecThreads, d_adj_in) t_adj_in;
  SCS_GTABLE(kVecThreads, d_fwd_in) t_fwd_in;
  SCS_GTABLE(kPertThreads, d_pert_rows) t_pert[3];  // forward with dA / dP (perturb.hpp): dA' y, dA x, dP x — in the order of pert_products
  SCS_GTABLE(kVecThreads, d_pert_eff) t_pert_eff;
  SCS_GTABLE(kVecThreads, d_lsqr_start) t_start;
  SCS_GTABLE_K(kVecThreads, d_lsqr_v) t_lsqr_v;
  SCS_GTABLE_K(kVecThreads, d_lsqr_u) t_lsqr_u;
  SCS_GTABLE(kVecThreads, d_adj_out) t_adj_out;
  SCS_GTABLE(kVecThreads, d_fwd_out) t_fwd_out;
  SCS_GTABLE(kVecThreads, d_grad_a) t_grad_a;
  SCS_GTABLE(kVecThreads, d_grad_p) t_grad_p;
  SCS_GTABLE(kVecThreads, d_copy_i32) t_gather_fl;
  DprojTabs rhs1, rhs2;  // adjoint: W gs, (W - I) gy;  forward: rhs1 = the final apply
  ProdTabs pv, pu;       // the product step_v consumes (input uh) and the one step_u consumes (input vh)

  DevBuf<int> flags_d, lists_d;   // G x LF_COUNT;  [identity | active]
  DevBuf<double> st_d;            // G x L_COUNT
  int *flags_h = nullptr, *lists_h = nullptr;  // (pinned: every copy here is asynchronous)
  double *st_h = nullptr;
  const int *all_d = nullptr;                  // the identity list
  int *active_d = nullptr, *active_h = nullptr;  // the members LSQR still iterates (lsqr_run compacts it)
  std::vector<DprojPlan> plans;
  long launches = 0, syncs = 0;
  int lane_tile = 4;

  ~GroupDiff() {
    if (s && hipStreamSynchronize(s) == hipSuccess) {  // the stream is drained: the group's device blocks are the pool's
      ++t_pool_release;
      for_tables([](auto &t) { t.dev.release(); });
      flags_d.release(); lists_d.release(); st_d.release();
      --t_pool_release;
    }
    g_diff_group_launches.fetch_add(launches, std::memory_order_relaxed);
    g_diff_group_syncs.fetch_add(syncs, std::memory_order_relaxed);
    if (flags_h) (void)hipHostFree(flags_h);
    if (lists_h) (void)hipHostFree(lists_h);
    if (st_h) (void)hipHostFree(st_h);
  }

  // Can this workspace be differentiated inside a group?  The CSR-stream layouts (every product is one launch whose grid follows from
  // the row blocks) and PSD blocks on the fused apply; the five-launch tile path stays with diff_impl.
  static bool member_ok(const ScsHipWork *w) {
    if (w->At.cs.ok || w->Ar.cs.ok || w->At.has_slab || w->Ar.has_slab) return false;
    if (w->has_P && (w->Pf.cs.ok || w->Pf.has_slab)) return false;
    for (int o : w->psd_order_h)
      if (o > kDprojPsdFusedMax) return false;
    if (w->cone.bsize > kDboxMultiMin) return false;  // the multi-launch box apply (and the 25 rounds of its preparation)
    return true;
  }
  // the part of GroupSolve::same_shape the derivative depends on
  static bool same_shape(const ScsHipWork *a, const ScsHipWork *b) {
    const HostCone &x = a->cone, &y = b->cone;
    return a->device == b->device && a->n == b->n && a->m == b->m && a->has_P == b->has_P && a->normalized == b->normalized &&
           x.z == y.z && x.l == y.l && x.bsize == y.bsize && x.q == y.q && x.s == y.s && x.p.size() == y.p.size();
  }

  template <class F> void for_dproj(DprojTabs &d, F &&f) { f(d.zl); f(d.psd); f(d.box); f(d.sym3); f(d.soc); f(d.soc_big); }
  template <class F> void for_tables(F &&f) {
    f(t_vhat); f(t_prep_wave); f(t_prep_block); f(t_box_prep); f(t_pow_prep); f(t_psd_copy); f(t_copy_out0); f(t_copy_out1); f(t_gather_st); f(t_psd_eig);
    f(t_psd_gather); f(t_adj_in); f(t_fwd_in); f(t_pert[0]); f(t_pert[1]); f(t_pert[2]); f(t_pert_eff); f(t_start); f(t_lsqr_v); f(t_lsqr_u); f(t_adj_out); f(t_fwd_out); f(t_grad_a);
    f(t_grad_p); f(t_gather_fl);
    for (DprojTabs *d : {&rhs1, &rhs2, &pv.dp, &pu.dp}) for_dproj(*d, f);
    for (ProdTabs *p : {&pv, &pu}) { f(p->ar); f(p->at); f(p->pf); }
  }
  template <class T> void go(const T &t, const int *list, int count) {
    t.launch(list, count, s);
    if (t.used && count > 0 && t.gx > 0) ++launches;
  }
  template <class T> void go_k(const T &t, const int *list, int count, int k) {
    launch_grouped_k(t, list, count, k, s);
    if (t.used && count > 0 && t.gx > 0) ++launches;
  }
  void go_dproj(const DprojTabs &d, const int *list, int count) {  // (the order of launch_dproj)
    go(d.zl, list, count);
    go(d.psd, list, count);
    go(d.box, list, count);
    go(d.sym3, list, count);
    go(d.soc, list, count);
    go(d.soc_big, list, count);
  }
  template <class T> void go_spmv(const T &t, const int *list, int count) {
    if (!one_work) return go(t, list, count);
    launch_lanes(t, list, count, lane_tile, s);
    if (t.used && count > 0 && t.gx > 0) ++launches;
  }
  void go_prod(const ProdTabs &p, const int *list, int count) {  // (the order of a DiffProduct)
    if (!p.transposed) go_dproj(p.dp, list, count);
    go_spmv(p.ar, list, count);
    if (p.transposed) go_dproj(p.dp, list, count);
    go_spmv(p.at, list, count);
    go_spmv(p.pf, list, count);
  }
  void sync() {
    HIP_CHECK(hipGetLastError());  // (launches are not checked one by one)
    HIP_CHECK(hipStreamSynchronize(s));
    ++syncs;
  }
  static CsrView csr_of(const DeviceCsr &M) {
    CsrView V = M.view().csr;
    V.pstride = V.nblk;
    return V;
  }

  // The member lists and the gathered blocks of a group of G members: the identity list and the active list, uploaded.
  void alloc_lists() {
    HIP_CHECK(hipHostMalloc((void **)&flags_h, sizeof(int) * LF_COUNT * G));
    HIP_CHECK(hipHostMalloc((void **)&lists_h, sizeof(int) * 2 * G));
    HIP_CHECK(hipHostMalloc((void **)&st_h, sizeof(double) * L_COUNT * G));
    flags_d.alloc((size_t)LF_COUNT * G);
    st_d.alloc((size_t)L_COUNT * G);
    lists_d.alloc((size_t)2 * G);
    for (int g = 0; g < G; ++g) lists_h[g] = lists_h[G + g] = g;
    HIP_CHECK(hipMemcpyAsync(lists_d.p, lists_h, sizeof(int) * 2 * G, hipMemcpyHostToDevice, s));
    all_d = lists_d.p;
    active_d = lists_d.p + G;
    active_h = lists_h + G;
  }
  // ---- LSQR as a piece of its own: GroupDiff::run solves once over all members, GroupRefine (refine_batch.hpp) once per Newton step
  // over the members that still step.  The tables (the caller sets the products' gx from its members' row blocks and uploads) ...
  void size_lsqr(const DprojPlan &p0, size_t SG, int nbN) {
    t_start.resize(SG); t_lsqr_v.resize(SG); t_lsqr_u.resize(SG);
    t_start.gx = t_lsqr_v.gx = t_lsqr_u.gx = nbN;
    for (ProdTabs *p : {&pv, &pu}) {
      p->dp.size(p0, SG);
      p->ar.resize(SG); p->at.resize(SG);
      if (has_P) p->pf.resize(SG);
    }
    t_gather_fl.resize(SG); t_gather_fl.gx = 1;
  }
  // ... member g's records: the same whatever the direction, over the wiring's two products on lane d of w
  void set_lsqr(int g, const ScsHipWork *w, DiffLane &d, const DprojPlan &plan, const DiffWiring &wr, int nbN, double tol) {
    const int *done = d.fl.p + LF_DONE;
    t_start.set(g, d.uh.p, wr.start_add[0], wr.start_add[1], n, N, d.x.p, d.w.p, d.partU.p, d.st.p, d.fl.p);
    pv.set(g, w, plan, wr.pv, done);
    pu.set(g, w, plan, wr.pu, done);
    t_lsqr_v.set(g, wr.pv.read, d.vh.p, (const double *)d.w.p, d.x.p, n, N, (const double *)d.partU.p, nbN, d.partV.p, d.partX.p, d.st.p, d.fl.p);
    t_lsqr_u.set(g, wr.pu.read, d.uh.p, (const double *)d.vh.p, d.w.p, n, N, (const double *)d.partV.p, (const double *)d.partX.p, nbN,
                 d.partU.p, d.st.p, d.fl.p, tol);
    t_gather_fl.set(g, (const int *)d.fl.p, flags_d.p + (size_t)g * LF_COUNT, (int)LF_COUNT);
  }
  // ... and the solve: the members active_h[0 .. na), each from the right-hand side in its uh to the answer in its x, in chunks of
  // iterations between looks at the gathered flags.  list_changed: the caller rewrote the pinned active list (after a synchronisation
  // of the stream), the device's copy follows before the first launch.  Leaves every member's flag block in flags_h.
  void lsqr_run(int na, bool list_changed, long cap) {
    auto push_list = [&] {  // the pinned active list was rewritten or compacted: the device's copy follows before the next launch
      if (list_changed) HIP_CHECK(hipMemcpyAsync(active_d, active_h, sizeof(int) * (size_t)na, hipMemcpyHostToDevice, s));
      list_changed = false;
    };
    push_list();
    go(t_start, active_d, na);
    auto step_v = [&](int k) { go_prod(pv, active_d, na); go_k(t_lsqr_v, active_d, na, k); };
    auto step_u = [&](int k) {  // (the first launches after every look at the flags)
      push_list();
      go_prod(pu, active_d, na);
      go_k(t_lsqr_u, active_d, na, k);
    };
    lsqr_drive(cap, step_u, step_v, [&] {
      // Only the members still iterating are gathered, but the whole of flags_d comes back.  That is safe: a member's row of flags_d
      // is written by this gather alone, and a member is in the gather of the look that first finds it done — after which its device
      // block no longer changes (d_lsqr_v / d_lsqr_u return on the done flag), so the row it left is its final one.  Rows of members
      // outside this solve (GroupRefine: members that stopped stepping) hold the flags of the last solve they took part in; callers read
      // the rows of the members they passed in and no others.  Finished members leave the active list.
      go(t_gather_fl, active_d, na);
      HIP_CHECK(hipMemcpyAsync(flags_h, flags_d.p, sizeof(int) * LF_COUNT * G, hipMemcpyDeviceToHost, s));
      sync();  // (the pinned list may be rewritten)
      int keep = 0;
      for (int i = 0; i < na; ++i)
        if (!flags_h[(size_t)active_h[i] * LF_COUNT + LF_DONE]) active_h[keep++] = active_h[i];
      list_changed = list_changed || keep != na;
      na = keep;
      return na == 0;
    });
  }

  // The caller holds every member's mutex, has selected the device, refused bad arguments (diff_check) and run diff_alloc /
  // diff_build_tri / pert_alloc for every member.  All pointers are device pointers.
  void run(const ScsHipDiffOpts *o) {
    const double t0 = now_ms();
    G = (int)W.size();
    ScsHipWork *w0 = W[0];
    n = w0->n; m = w0->m; N = (long)n + m; has_P = w0->has_P;
    const DiffLimits lim(o, N);
    const int nbN = vec_blocks(N);
    const bool want_dA = adjoint && calls[0].out[2], want_dP = adjoint && calls[0].out[3];
    ArenaScope no_arena(nullptr);
    lane_tile = g_diff_lane_tile.load() == 8 ? 8 : 4;
    const int GP = one_work ? 1 : G;  // members that prepare: the first of each workspace

    alloc_lists();

    // ---- the members' cone plans ----
    plans.clear();
    for (ScsHipWork *w : W) plans.push_back(diff_plan(w));
    const DprojPlan &p0 = plans[0];
    const size_t SG = (size_t)G;

    // ---- tables ----
    t_vhat.resize(SG); t_vhat.gx = vec_blocks(m);
    if (p0.n_soc > 0) { t_prep_wave.resize(SG); t_prep_wave.gx = soc_wave_blocks(p0.n_soc, p0.G); }
    if (p0.n_soc > 0 && p0.n_soc_big > 0) { t_prep_block.resize(SG); t_prep_block.gx = p0.n_soc_big; }
    if (p0.box.bsize > 0) { t_box_prep.resize(SG); t_box_prep.gx = 1; }
    if (p0.sym3.count > 0) { t_pow_prep.resize(SG); t_pow_prep.gx = ceil_div(p0.sym3.count, kConeThreads); }
    // the decomposition borrows K9-layout scratch for a slice of the members at a time (stream order protects its reuse)
    const size_t per_member = (size_t)std::max(p0.psd.scratch_doubles, 1L);
    const int slice = (int)std::max<size_t>(1, std::min<size_t>((size_t)GP, kDiffPsdBorrowMax / (per_member * sizeof(double))));
    DevBuf<double> psd_scratch;
    if (p0.psd.count > 0) {
      psd_scratch.alloc(per_member * (size_t)slice);
      t_psd_copy.resize(SG); t_psd_copy.gx = vec_blocks(m);
      t_psd_eig.resize(SG); t_psd_eig.gx = p0.psd.count; t_psd_eig.lds = kPsdLdsBytes;
      t_psd_gather.resize(SG); t_psd_gather.gx = p0.psd.count;
    }
    if (adjoint) {
      t_adj_in.resize(SG); t_adj_in.gx = nbN;
      rhs1.size(p0, SG); rhs2.size(p0, SG);
      t_adj_out.resize(SG); t_adj_out.gx = nbN;
      t_copy_out0.resize(SG); t_copy_out0.gx = vec_blocks(m);
      t_copy_out1.resize(SG); t_copy_out1.gx = vec_blocks(n);
      if (want_dA) t_grad_a.resize(SG);
      if (want_dP) t_grad_p.resize(SG);
    } else {
      t_fwd_in.resize(SG); t_fwd_in.gx = nbN;
      if (calls[0].perturbs()) {  // (the members of a group agree in which of dA / dP they pass: plan_diff_batch)
        for (int k = 0; k < (calls[0].pert[0] ? 2 : 0) + (calls[0].pert[1] ? 1 : 0); ++k) { t_pert[k].resize(SG); t_pert[k].gx = 0; }
        t_pert_eff.resize(SG); t_pert_eff.gx = nbN;
      }
      rhs1.size(p0, SG);
      t_fwd_out.resize(SG); t_fwd_out.gx = nbN;
    }
    size_lsqr(p0, SG, nbN);
    t_gather_st.resize(SG); t_gather_st.gx = 1;

    int gx_ar = 0, gx_at = 0, gx_pf = 0, gx_ga = 0, gx_gp = 0;
    const PsdRefineCfg refine_off = psd_refine_default(false);
    for (int g = 0; g < G; ++g) {
      ScsHipWork *w = W[(size_t)g];
      const int ln = lane.empty() ? 0 : lane[(size_t)g];
      DiffLane &d = w->diff.lane(ln);
      const DiffCall &a = calls[(size_t)g];
      const DprojPlan &plan = plans[(size_t)g];
      const double *D = w->normalized ? w->D.p : nullptr, *E = w->normalized ? w->E.p : nullptr;
      const double sigma = w->normalized ? w->scal.sigma : 1.0;
      gx_ar = std::max(gx_ar, w->Ar.view().csr.nblk);
      gx_at = std::max(gx_at, w->At.view().csr.nblk);
      if (has_P) gx_pf = std::max(gx_pf, w->Pf.view().csr.nblk);
      t_vhat.set(g, (const double *)w->sols.p, (const double *)w->soly.p, D, sigma, m, w->diff.vhat.p);
      if (t_prep_wave.used) t_prep_wave.set(g, plan.vh, plan.off, plan.dim, plan.n_soc, plan.G, plan.cinfo);
      if (t_prep_block.used) t_prep_block.set(g, plan.vh, plan.off, plan.dim, plan.big, plan.cinfo);
      if (t_box_prep.used) t_box_prep.set(g, plan.vh + plan.box.off, plan.box.bl, plan.box.bu, plan.box.bsize, plan.box.tmp, plan.box.st);
      if (t_pow_prep.used) t_pow_prep.set(g, plan.vh + plan.sym3.off, plan.sym3.a, plan.sym3.count, plan.sym3.W);
      if (t_psd_eig.used) {
        double *scr = psd_scratch.p + per_member * (size_t)(g % slice);
        t_psd_copy.set(g, plan.vh, plan.psd.tmp_m, (long)m);
        t_psd_eig.set(g, plan.psd.tmp_m, PsdBatch{plan.psd.off, plan.psd.order, plan.psd.woff, plan.psd.count}, scr, /*allow_warm=*/0, 0,
                      (const int *)nullptr, plan.psd.tol2, refine_off, 0);
        t_psd_gather.set(g, plan.psd, (const double *)scr, plan.vh);
      }
      const DiffWiring wr = diff_wiring(w, a, ln);
      // right-hand side and results: the kernels of the call's direction
      if (adjoint) {
        t_adj_in.set(g, a.in[0], a.in[1], a.in[2], D, E, sigma, n, m, d.uh.p, wr.gyh, wr.gsh);
        rhs1.set(g, plan, wr.rhs_gs, nullptr);
        rhs2.set(g, plan, wr.rhs_gy, nullptr);
        t_adj_out.set(g, (const double *)d.x.p, D, E, sigma, n, m, wr.dc, wr.db);
        t_copy_out0.set(g, (const double *)wr.db, a.out[0], a.out[0] ? (long)m : 0L);
        t_copy_out1.set(g, (const double *)wr.dc, a.out[1], a.out[1] ? (long)n : 0L);
        if (want_dA) {
          t_grad_a.set(g, (const int *)w->At.rowptr.p, (const int *)w->At.col.p, w->At.rows, (long)w->At.nnz, (const double *)w->solx.p,
                       (const double *)w->soly.p, (const double *)wr.dc, (const double *)wr.db, a.out[2]);
          gx_ga = std::max(gx_ga, vec_blocks((long)w->At.nnz));
        }
        if (want_dP) {
          t_grad_p.set(g, (const int *)w->Pf.rowptr.p, (const int *)w->Pf.col.p, n, (long)w->Pf.nnz, (const int *)w->diff.tri_up.p,
                       (const double *)w->solx.p, (const double *)wr.dc, a.out[3]);
          gx_gp = std::max(gx_gp, vec_blocks((long)w->Pf.nnz));
        }
      } else {
        if (wr.eff_c) {  // the launches of pert_launch (perturb.hpp)
          PertProduct pr[3];
          const int cnt = pert_products(w, a.pert[0], a.pert[1], pr);
          for (int k = 0; k < cnt; ++k) {
            t_pert[k].set(g, pr[k].rp, pr[k].ci, pr[k].map, pr[k].val, pr[k].vec, pr[k].rows, pr[k].lg, pr[k].out);
            t_pert[k].gx = std::max(t_pert[k].gx, pr[k].blocks());
          }
          t_pert_eff.set(g, a.in[1], a.in[0], a.pert[1] ? (const double *)d.tP.p : nullptr, a.pert[0] ? (const double *)d.tAt.p : nullptr,
                         a.pert[0] ? (const double *)d.tA.p : nullptr, -1.0, n, m, wr.eff_c, wr.eff_b);
        }
        t_fwd_in.set(g, wr.db_in, wr.dc_in, D, E, sigma, n, m, d.uh.p);
        rhs1.set(g, plan, wr.fin, nullptr);
        t_fwd_out.set(g, (const double *)d.x.p, (const double *)d.dW.p, (const double *)d.dWmI.p, D, E, sigma, n, m, a.out[0], a.out[1], a.out[2]);
      }
      set_lsqr(g, w, d, plan, wr, nbN, lim.tol);
      t_gather_st.set(g, (const double *)d.st.p, st_d.p + (size_t)g * L_COUNT, (long)L_COUNT);
    }
    for (ProdTabs *p : {&pv, &pu}) { p->ar.gx = gx_ar; p->at.gx = gx_at; p->pf.gx = gx_pf; }
    t_grad_a.gx = gx_ga; t_grad_p.gx = gx_gp;
    for_tables([&](auto &t) { t.upload(s); });

    // ---- the fixed point and the cone records ----
    go(t_vhat, all_d, GP);
    if (t_psd_eig.used) {
      for (int lo = 0; lo < GP; lo += slice) {
        const int cnt = std::min(slice, GP - lo);
        go(t_psd_copy, all_d + lo, cnt);
        go(t_psd_eig, all_d + lo, cnt);
        go(t_psd_gather, all_d + lo, cnt);
      }
      sync();  // one synchronisation for the group: the borrowed scratch is the pool's again
      ++t_pool_release;
      psd_scratch.release();
      --t_pool_release;
    }
    go(t_box_prep, all_d, GP);  // (the order of launch_dproj_prep: after the PSD blocks, whose tmp_m holds box.tmp)
    go(t_pow_prep, all_d, GP);
    go(t_prep_wave, all_d, GP);
    go(t_prep_block, all_d, GP);

    // ---- right-hand side into uh, x = w = 0 ----
    if (adjoint) {
      go(t_adj_in, all_d, G);
      go_dproj(rhs1, all_d, G);
      go_dproj(rhs2, all_d, G);
    } else {
      for (auto &t : t_pert) go(t, all_d, G);
      go(t_pert_eff, all_d, G);
      go(t_fwd_in, all_d, G);
    }
    // ---- LSQR over all members (the identity list is on the device) ----
    lsqr_run(G, false, lim.cap);
    go(t_gather_st, all_d, G);
    HIP_CHECK(hipMemcpyAsync(st_h, st_d.p, sizeof(double) * L_COUNT * G, hipMemcpyDeviceToHost, s));

    // ---- results ----
    if (adjoint) {
      go(t_adj_out, all_d, G);
      go(t_copy_out0, all_d, G);
      go(t_copy_out1, all_d, G);
      go(t_grad_a, all_d, G);
      go(t_grad_p, all_d, G);
    } else {
      go_dproj(rhs1, all_d, G);
      go(t_fwd_out, all_d, G);
    }
    sync();
    const double dt = now_ms() - t0;
    for (int g = 0; g < G; ++g) diff_fill_info(infos[(size_t)g], flags_h + (size_t)g * LF_COUNT, st_h + (size_t)g * L_COUNT, lim.cap, dt);
  }
};

}  // namespace scship
