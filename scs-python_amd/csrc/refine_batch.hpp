// refine_batch.hpp — grouped Newton polish: G equally shaped, solved workspaces are refined in lock step, ONE launch per kernel for the
// group and ONE host synchronisation per evaluation of F^ for the group (include/scs_hip.h: scs_hip_refine_batch[_device]).
//
// The reason is the one of diff_batch.hpp: a refine of a small problem is a few dozen dependent launches plus a read-back per
// evaluation, so K members refined in turn are bound by the command queue and by K x (evaluations + LSQR looks) synchronisations.  The
// means are the same too: the bodies d_X of refine.hpp, dproj*.hpp, spmv.hpp and lsqr.hpp through the grouped entries (blockIdx.y =
// member, arguments from the member's record), the LSQR solve through GroupDiff::lsqr_run.  Same code, same block decomposition, same
// partial sums => every member's x, y, s and info (but time_ms, which is the group's) have the bits of scs_hip_refine on that member alone
// (tests/test_refine_batch_gpu.py).
//
// The control flow of refine_impl lives on the host, per member, over lists.  Members differ in the number of steps, of halvings and
// in why they stop, so the group keeps a STEPPING list (members that have not stopped) and, inside a step, a SEARCHING list (members
// whose line search has not ended).  At halving round h every member still searching has t = 2^-h exactly: t is a launch-level
// argument (k_grouped_t).  d_refine_finish writes every member's state block into one stacked block of the group, one copy into pinned
// memory and one synchronisation serve the whole list, and the host applies the Armijo test per member: accepted members leave the
// searching list and go through d_refine_accept at once (it reads dW / dWmI of that trial's evaluation; the member is not evaluated
// again before), a member that runs out of halvings stops with 3.  Compacted lists are uploaded before their next use; a pinned list is
// only rewritten after a synchronisation that followed its last upload (every evaluation ends in one).  Every loop is bounded on the
// host: a pass of the stepping loop gives every member in it one more step or takes it out, and no member takes more than max_steps.
#pragma once

namespace scship {

// d_refine_trial with the step length first: the launch-level argument of k_grouped_t
__device__ __forceinline__ void d_refine_trial_t(double t, const double *__restrict__ bx, const double *__restrict__ bv,
                                                 const double *__restrict__ d, int n, int m, double *tx, double *tv) {
  d_refine_trial(bx, bv, d, t, n, m, tx, tv);
}
// a table body whose FIRST argument is launch-level and a double (k_grouped_k of diff_batch.hpp, with the step length for the index)
template <auto Fn, int Threads, class... A>
__global__ __launch_bounds__(Threads) void k_grouped_t(const Pack<A...> *tab, const int *list, double t) {
  pack_call(Fn, tab[list[blockIdx.y]], t);
}
template <auto Fn, int Threads, class... A> GTable<Fn, Threads, A...> gtable_t_of(void (*)(double, A...));
#define SCS_GTABLE_T(threads, ...) decltype(gtable_t_of<__VA_ARGS__, threads>(__VA_ARGS__))
template <auto Fn, int Threads, class... A>
inline void launch_grouped_t(const GTable<Fn, Threads, A...> &t, const int *list, int cnt, double v, hipStream_t s) {
  if (!t.used || cnt <= 0 || t.gx <= 0) return;
  hipLaunchKernelGGL((k_grouped_t<Fn, Threads, A...>), dim3((unsigned)t.gx, (unsigned)cnt), dim3(Threads), t.lds, s,
                     (const Pack<A...> *)t.dev.p, list, v);
}

struct GroupRefine {
  GroupDiff gd;  // the members (gd.W), the stream, the LSQR piece, the launch count
  std::vector<ScsHipRefineInfo *> infos;

  // launch_dproj_prep over the group, at one of the two points of a member (the base plan or the trial plan)
  struct PrepTabs {
    SCS_GTABLE(kVecThreads, d_copy_f64) psd_copy;
    SCS_GTABLE(kPsdThreads, d_proj_psd<0>) psd_eig;
    SCS_GTABLE(kDprojPsdThreads, d_dproj_psd_gather) psd_gather;
    SCS_GTABLE(kBoxThreads, d_dbox_prep) box;
    SCS_GTABLE(kConeThreads, d_dpow_prep) pow;
    SCS_GTABLE(kConeThreads, d_dproj_prep_wave) wave;
    SCS_GTABLE(kConeThreads, d_dproj_prep_block) block;
    void size(const DprojPlan &p, size_t G, int m) {
      if (p.psd.count > 0) {
        psd_copy.resize(G); psd_copy.gx = vec_blocks(m);
        psd_eig.resize(G); psd_eig.gx = p.psd.count; psd_eig.lds = kPsdLdsBytes;
        psd_gather.resize(G); psd_gather.gx = p.psd.count;
      }
      if (p.box.bsize > 0) { box.resize(G); box.gx = 1; }
      if (p.sym3.count > 0) { pow.resize(G); pow.gx = ceil_div(p.sym3.count, kConeThreads); }
      if (p.n_soc > 0) { wave.resize(G); wave.gx = soc_wave_blocks(p.n_soc, p.G); }
      if (p.n_soc > 0 && p.n_soc_big > 0) { block.resize(G); block.gx = p.n_soc_big; }
    }
    void set(int g, const DprojPlan &p, int m) {
      if (psd_copy.used) psd_copy.set(g, p.vh, p.psd.tmp_m, (long)m);
      if (box.used) box.set(g, p.vh + p.box.off, p.box.bl, p.box.bu, p.box.bsize, p.box.tmp, p.box.st);
      if (pow.used) pow.set(g, p.vh + p.sym3.off, p.sym3.a, p.sym3.count, p.sym3.W);
      if (wave.used) wave.set(g, p.vh, p.off, p.dim, p.n_soc, p.G, p.cinfo);
      if (block.used) block.set(g, p.vh, p.off, p.dim, p.big, p.cinfo);
    }
    // the two records that read the borrowed scratch: set anew when the pool hands out another block (evaluate)
    void set_scratch(int g, const DprojPlan &p, double *scr) {
      psd_eig.set(g, p.psd.tmp_m, PsdBatch{p.psd.off, p.psd.order, p.psd.woff, p.psd.count}, scr, /*allow_warm=*/0, 0, (const int *)nullptr,
                  p.psd.tol2, psd_refine_default(false), 0);
      psd_gather.set(g, p.psd, (const double *)scr, p.vh);
    }
  };
  // one evaluation of F^ at the base (0) or the trial (1) point: what differs between the two is the plan's vh and the x^ read
  struct EvalTabs {
    PrepTabs prep;
    GroupDiff::DprojTabs apply;
    SCS_GTABLE(kSpmvThreads, d_spmv_stream<EpiStore>) ar, pf;
    SCS_GTABLE(kVecThreads, d_refine_residual) resid;
    const double *scratch_at = nullptr;  // the borrowed block the PSD records point into
  } ev[2];
  SCS_GTABLE(kSpmvThreads, d_spmv_stream<EpiStore>) t_at;  // A^' y^: y^ lies in dWmI at either point
  SCS_GTABLE(kVecThreads, d_refine_start) t_start;
  SCS_GTABLE(kVecThreads, d_refine_finish) t_finish;
  SCS_GTABLE_T(kVecThreads, d_refine_trial_t) t_trial;
  SCS_GTABLE(kVecThreads, d_refine_accept) t_accept;

  DevBuf<int> lists_d;   // [searching | accepted]
  DevBuf<double> st_d;   // G x RS_COUNT: the stacked state blocks
  int *lists_h = nullptr;
  double *st_h = nullptr;
  std::vector<DprojPlan> plans[2];
  size_t per_member = 1;
  int slice = 1;

  template <class F> void for_tables(F &&f) {
    for (EvalTabs &e : ev) {
      f(e.prep.psd_copy); f(e.prep.psd_eig); f(e.prep.psd_gather); f(e.prep.box); f(e.prep.pow); f(e.prep.wave); f(e.prep.block);
      gd.for_dproj(e.apply, f);
      f(e.ar); f(e.pf); f(e.resid);
    }
    f(t_at); f(t_start); f(t_finish); f(t_trial); f(t_accept);
  }
  ~GroupRefine() {
    if (gd.s && hipStreamSynchronize(gd.s) == hipSuccess) {  // the stream is drained: the group's device blocks are the pool's
      ++t_pool_release;
      for_tables([](auto &t) { t.dev.release(); });
      lists_d.release(); st_d.release();
      --t_pool_release;
    }
    if (lists_h) (void)hipHostFree(lists_h);
    if (st_h) (void)hipHostFree(st_h);
  }
  void sync() { gd.sync(); }

  // F^ of the members list[0 .. cnt) at their base or trial point: -F^ into uh, the figures into the member's block of st_h
  void evaluate(int which, const int *list_d, const int *list_h, int cnt) {
    EvalTabs &e = ev[which];
    hipStream_t s = gd.s;
    if (e.prep.psd_eig.used) {
      // the decomposition borrows K9-layout scratch for a slice of the members at a time, at every evaluation (stream order protects
      // its reuse between the chunks; members of one chunk have slots of their own)
      DevBuf<double> scratch;
      scratch.alloc(per_member * (size_t)slice);
      if (scratch.p != e.scratch_at) {  // (the records were last uploaded before a synchronisation: they may be rewritten)
        for (int g = 0; g < gd.G; ++g) e.prep.set_scratch(g, plans[which][(size_t)g], scratch.p + per_member * (size_t)(g % slice));
        e.prep.psd_eig.upload(s);
        e.prep.psd_gather.upload(s);
        e.scratch_at = scratch.p;
      }
      std::vector<char> slot((size_t)slice);
      for (int lo = 0; lo < cnt;) {
        std::fill(slot.begin(), slot.end(), 0);
        int hi = lo;
        while (hi < cnt && !slot[(size_t)(list_h[hi] % slice)]) slot[(size_t)(list_h[hi++] % slice)] = 1;
        gd.go(e.prep.psd_copy, list_d + lo, hi - lo);
        gd.go(e.prep.psd_eig, list_d + lo, hi - lo);
        gd.go(e.prep.psd_gather, list_d + lo, hi - lo);
        lo = hi;
      }
      sync();  // one synchronisation for the list: the borrowed scratch is the pool's again
      ++t_pool_release;
      scratch.release();
      --t_pool_release;
    }
    gd.go(e.prep.box, list_d, cnt);  // (the order of launch_dproj_prep)
    gd.go(e.prep.pow, list_d, cnt);
    gd.go(e.prep.wave, list_d, cnt);
    gd.go(e.prep.block, list_d, cnt);
    gd.go_dproj(e.apply, list_d, cnt);
    gd.go(e.ar, list_d, cnt);
    gd.go(t_at, list_d, cnt);
    gd.go(e.pf, list_d, cnt);
    gd.go(e.resid, list_d, cnt);
    gd.go(t_finish, list_d, cnt);
    HIP_CHECK(hipMemcpyAsync(st_h, st_d.p, sizeof(double) * RS_COUNT * gd.G, hipMemcpyDeviceToHost, s));
    sync();
  }

  // The caller holds every member's mutex, has selected the device, refused what diff_refusal refuses and run refine_alloc for every
  // member.  Leaves every member's best accepted point in its solx / soly / sols (untouched when no step of it was accepted).
  void run(const ScsHipRefineOpts *o) {
    const double t0 = now_ms();
    hipStream_t s = gd.s;
    const int G = gd.G = (int)gd.W.size();
    ScsHipWork *w0 = gd.W[0];
    const int n = gd.n = w0->n, m = gd.m = w0->m;
    const long N = gd.N = (long)n + m;
    gd.has_P = w0->has_P;
    gd.adjoint = false;
    const RefineLimits lim(o);
    const DiffLimits llim(&lim.lsqr, N);
    const int nbN = vec_blocks(N);
    const size_t SG = (size_t)G;
    ArenaScope no_arena(nullptr);

    gd.alloc_lists();
    HIP_CHECK(hipHostMalloc((void **)&lists_h, sizeof(int) * 2 * G));
    HIP_CHECK(hipHostMalloc((void **)&st_h, sizeof(double) * RS_COUNT * G));
    lists_d.alloc(2 * SG);
    st_d.alloc((size_t)RS_COUNT * SG);
    int *search_h = lists_h, *accept_h = lists_h + G;
    int *search_d = lists_d.p, *accept_d = lists_d.p + G;

    // ---- the members' cone plans over the base and over the trial point: the same records, read against the v^ they were prepared at
    for (ScsHipWork *w : gd.W) {
      DprojPlan pb = diff_plan(w), pt = pb;
      pb.vh = w->diff.refine.bv.p;
      pt.vh = w->diff.refine.tv.p;
      plans[0].push_back(pb);
      plans[1].push_back(pt);
    }
    const DprojPlan &p0 = plans[0][0];
    per_member = (size_t)std::max(p0.psd.scratch_doubles, 1L);
    slice = (int)std::max<size_t>(1, std::min<size_t>(SG, kDiffPsdBorrowMax / (per_member * sizeof(double))));

    // ---- tables ----
    for (EvalTabs &e : ev) {
      e.prep.size(p0, SG, m);
      e.apply.size(p0, SG);
      e.ar.resize(SG);
      if (gd.has_P) e.pf.resize(SG);
      e.resid.resize(SG); e.resid.gx = nbN;
    }
    t_at.resize(SG);
    t_start.resize(SG); t_trial.resize(SG); t_accept.resize(SG);
    t_start.gx = t_trial.gx = t_accept.gx = nbN;
    t_finish.resize(SG); t_finish.gx = 1;
    gd.size_lsqr(p0, SG, nbN);

    DiffCall fwd;
    fwd.adjoint = false;
    int gx_ar = 0, gx_at = 0, gx_pf = 0;
    for (int g = 0; g < G; ++g) {
      ScsHipWork *w = gd.W[(size_t)g];
      DiffScratch &d = w->diff;
      DiffScratch::Refine &r = d.refine;
      const double *D = w->normalized ? w->D.p : nullptr, *E = w->normalized ? w->E.p : nullptr;
      const double sigma = w->normalized ? w->scal.sigma : 1.0;
      gx_ar = std::max(gx_ar, w->Ar.view().csr.nblk);
      gx_at = std::max(gx_at, w->At.view().csr.nblk);
      if (gd.has_P) gx_pf = std::max(gx_pf, w->Pf.view().csr.nblk);
      t_start.set(g, (const double *)w->solx.p, (const double *)w->soly.p, (const double *)w->sols.p, D, E, sigma, n, m, r.bx.p, r.bv.p);
      for (int k = 0; k < 2; ++k) {
        EvalTabs &e = ev[k];
        const DprojPlan &plan = plans[k][(size_t)g];
        const double *xh = k == 0 ? r.bx.p : r.tx.p;
        e.prep.set(g, plan, m);
        e.apply.set(g, plan, DprojIo{plan.vh, nullptr, d.dW.p, d.dWmI.p}, nullptr);
        e.ar.set(g, GroupDiff::csr_of(w->Ar), xh, EpiStore{d.tA.p, 0}, (const int *)nullptr, nullptr);
        if (gd.has_P) e.pf.set(g, GroupDiff::csr_of(w->Pf), xh, EpiStore{d.tP.p, 0}, (const int *)nullptr, nullptr);
        e.resid.set(g, RefineEval{xh, d.dW.p, d.dWmI.p, w->has_P ? d.tP.p : nullptr, d.tAt.p, d.tA.p, w->h.p, D, E, sigma}, n, m, d.uh.p,
                    r.part.p);
      }
      t_at.set(g, GroupDiff::csr_of(w->At), (const double *)d.dWmI.p, EpiStore{d.tAt.p, 0}, (const int *)nullptr, nullptr);
      t_finish.set(g, (const double *)r.part.p, nbN, sigma, lim.tol, st_d.p + (size_t)g * RS_COUNT);
      t_trial.set(g, (const double *)r.bx.p, (const double *)r.bv.p, (const double *)d.x.p, n, m, r.tx.p, r.tv.p);
      t_accept.set(g, (const double *)r.tx.p, (const double *)r.tv.p, (const double *)d.dW.p, (const double *)d.dWmI.p, D, E, sigma, n, m, r.bx.p,
                   r.bv.p, w->solx.p, w->soly.p, w->sols.p);
      // the Newton system J d = -F^ over the member's BASE plan, wired as refine_impl wires it
      gd.set_lsqr(g, w, d, plans[0][(size_t)g], diff_wiring(w, fwd), nbN, llim.tol);
    }
    for (EvalTabs &e : ev) { e.ar.gx = gx_ar; e.pf.gx = gx_pf; }
    t_at.gx = gx_at;
    for (GroupDiff::ProdTabs *p : {&gd.pv, &gd.pu}) { p->ar.gx = gx_ar; p->at.gx = gx_at; p->pf.gx = gx_pf; }
    for_tables([&](auto &t) { t.upload(s); });
    gd.for_tables([&](auto &t) { t.upload(s); });

    // ---- the starting point and F^ there ----
    struct Member {
      double cur[RS_COUNT], first[RS_COUNT];
      int steps = 0, halvings = 0, stop = 0;
      long lsqr_iters = 0;
    };
    std::vector<Member> M(SG);
    gd.go(t_start, gd.all_d, G);
    sync();  // (the tables are on the device: evaluate may rewrite the records of the borrowed scratch)
    for (int g = 0; g < G; ++g) search_h[g] = g;
    evaluate(0, gd.all_d, search_h, G);
    std::vector<int> stepping;
    for (int g = 0; g < G; ++g) {
      Member &mb = M[(size_t)g];
      std::copy(st_h + (size_t)g * RS_COUNT, st_h + (size_t)(g + 1) * RS_COUNT, mb.cur);
      std::copy(mb.cur, mb.cur + RS_COUNT, mb.first);
      mb.stop = mb.cur[RS_CONV] != 0. ? 1 : 0;
      if (!mb.stop) stepping.push_back(g);
    }

    // ---- Newton steps: every pass gives each member of the stepping list one more step, or takes it out ----
    for (int pass = 0; pass < lim.max_steps && !stepping.empty(); ++pass) {
      int ns = (int)stepping.size();
      std::copy(stepping.begin(), stepping.end(), gd.active_h);
      gd.lsqr_run(ns, true, llim.cap);  // uh = -F^ of the base point in, the step (dx ; dv) in x out
      for (int g : stepping) M[(size_t)g].lsqr_iters += std::min((long)gd.flags_h[(size_t)g * LF_COUNT + LF_ITERS], llim.cap);
      std::copy(stepping.begin(), stepping.end(), search_h);
      HIP_CHECK(hipMemcpyAsync(search_d, search_h, sizeof(int) * (size_t)ns, hipMemcpyHostToDevice, s));
      std::vector<int> next;
      double t = 1.0;
      for (int h = 0; h <= kRefineHalvings && ns > 0; ++h, t *= 0.5) {
        launch_grouped_t(t_trial, search_d, ns, t, s);
        ++gd.launches;
        evaluate(1, search_d, search_h, ns);
        int keep = 0, na = 0;
        for (int i = 0; i < ns; ++i) {
          const int g = search_h[i];
          Member &mb = M[(size_t)g];
          const double *tri = st_h + (size_t)g * RS_COUNT;
          if (tri[RS_PHI] < (1. - kRefineArmijo * t) * mb.cur[RS_PHI]) {  // (a NaN merit compares false)
            std::copy(tri, tri + RS_COUNT, mb.cur);
            ++mb.steps;
            if (mb.cur[RS_CONV] != 0.) mb.stop = 1;
            else if (mb.steps >= lim.max_steps) mb.stop = 2;
            else next.push_back(g);
            accept_h[na++] = g;
          } else {
            if (h < kRefineHalvings) ++mb.halvings;
            search_h[keep++] = g;
          }
        }
        if (na > 0) {  // the accepted trials become base points and resident solutions, before anything else touches their dW / dWmI
          HIP_CHECK(hipMemcpyAsync(accept_d, accept_h, sizeof(int) * (size_t)na, hipMemcpyHostToDevice, s));
          gd.go(t_accept, accept_d, na);
        }
        if (keep != ns && keep > 0) HIP_CHECK(hipMemcpyAsync(search_d, search_h, sizeof(int) * (size_t)keep, hipMemcpyHostToDevice, s));
        ns = keep;
      }
      for (int i = 0; i < ns; ++i) M[(size_t)search_h[i]].stop = 3;  // no t gave a decrease
      std::sort(next.begin(), next.end());  // (the order of the members, whatever round each was accepted in)
      stepping.swap(next);
    }
    sync();
    const double dt = now_ms() - t0;
    for (int g = 0; g < G; ++g) {
      ScsHipRefineInfo *info = infos[(size_t)g];
      if (!info) continue;
      const Member &mb = M[(size_t)g];
      info->steps = mb.steps; info->halvings = mb.halvings; info->lsqr_iters = (scs_int)mb.lsqr_iters; info->stop = mb.stop;
      info->merit_before = mb.first[RS_PHI]; info->merit_after = mb.cur[RS_PHI];
      info->res_pri_before = mb.first[RS_PRI]; info->res_dual_before = mb.first[RS_DUAL]; info->gap_before = mb.first[RS_GAP];
      info->res_pri = mb.cur[RS_PRI]; info->res_dual = mb.cur[RS_DUAL]; info->gap = mb.cur[RS_GAP];
      info->pobj = mb.cur[RS_XPX] / 2. + mb.cur[RS_CTX];
      info->dobj = -mb.cur[RS_XPX] / 2. - mb.cur[RS_BTY];
      info->time_ms = dt;
    }
  }
};

}  // namespace scship
