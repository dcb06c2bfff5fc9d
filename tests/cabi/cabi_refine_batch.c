/* Plain-C consumer of scs_hip_refine_batch / scs_hip_refine_batch_device (include/scs_hip.h).  The QP with an SOC of cabi_refine.c
 * (m = 6, n = 3) with three different right-hand sides is solved at eps = 1e-4 on three workspaces and on three twins.  The twins are
 * polished by three calls of scs_hip_refine, the workspaces by ONE call of the batch entry; infos and solutions are compared with
 * memcmp / ==.  A third set goes through the device entry on hipMalloc'ed vectors.  NULL sol / info arrays and NULL entries are
 * accepted; a refused member leaves -1 and its index in the message.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_refine_batch.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
 * Exit code 0 on success, 2 without a device; prints one line per check. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "scs_hip.h"

enum { M = 6, N = 3, ANNZ = 6, PNNZ = 4, K = 3 };

static int fails = 0;
static void expect(const char *what, int ok) {
  printf("%s -> %s\n", what, ok ? "ok" : "FAIL");
  fails += !ok;
}
static scs_float *dev_alloc(size_t count) {
  scs_float *d = NULL;
  if (hipMalloc((void **)&d, count * sizeof(scs_float)) != hipSuccess) { printf("hipMalloc failed\n"); exit(3); }
  return d;
}
static int same_info(const ScsHipRefineInfo *a, const ScsHipRefineInfo *b) {  /* all but time_ms */
  return a->steps == b->steps && a->halvings == b->halvings && a->lsqr_iters == b->lsqr_iters && a->stop == b->stop &&
         a->merit_before == b->merit_before && a->merit_after == b->merit_after && a->res_pri_before == b->res_pri_before &&
         a->res_dual_before == b->res_dual_before && a->gap_before == b->gap_before && a->res_pri == b->res_pri && a->res_dual == b->res_dual &&
         a->gap == b->gap && a->pobj == b->pobj && a->dobj == b->dobj;
}

static scs_int Ai[ANNZ] = {0, 4, 1, 5, 2, 3}, Ap[N + 1] = {0, 2, 4, 6};
static scs_float Ax[ANNZ] = {1.0, -1.0, 1.0, -1.0, 1.0, -0.1};
static scs_int Pi[PNNZ] = {0, 0, 1, 2}, Pp[N + 1] = {0, 1, 3, 4};
static scs_float Px[PNNZ] = {1.0, 0.2, 1.0, 0.5};
static scs_float B[K][M] = {{1.5, 1.5, 1.0, 2.0, 0.0, 0.0}, {1.4, 1.6, 0.9, 2.1, 0.0, 0.0}, {1.7, 1.2, 1.1, 1.8, 0.0, 0.0}};
static scs_float Cv[K][N] = {{-3.0, -2.5, -1.0}, {-2.8, -2.7, -0.9}, {-3.2, -2.2, -1.2}};

/* workspace i of a set: problem i, solved at 1e-4 (NULL: a failure, reported) */
static ScsWork *solved(int i) {
  scs_int q[1] = {3};
  ScsMatrix A = {Ax, Ai, Ap, M, N}, P = {Px, Pi, Pp, N, N};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  st.eps_abs = st.eps_rel = 1e-4;
  ScsCone k;
  memset(&k, 0, sizeof(k));
  k.l = 3;
  k.q = q;
  k.qsize = 1;
  ScsData d = {M, N, &A, &P, B[i], Cv[i]};
  ScsWork *w = scs_init(&d, &k, &st);
  if (!w) { printf("scs_init failed: %s\n", scs_hip_last_error()); return NULL; }
  scs_float x[N], y[M], s[M];
  ScsSolution sol = {x, y, s};
  ScsInfo info;
  if (scs_solve(w, &sol, &info, 0) != SCS_SOLVED) { printf("solve %d did not end solved\n", i); scs_finish(w); return NULL; }
  return w;
}

int main(void) {
  if (scs_hip_device_count() < 1) {
    printf("no HIP device\n");
    return 2;
  }
  ScsWork *w[K], *twin[K], *third[K];
  for (int i = 0; i < K; ++i) {
    w[i] = solved(i); twin[i] = solved(i); third[i] = solved(i);
    if (!w[i] || !twin[i] || !third[i]) return 3;
  }
  const double tol = 1e-10;
  ScsHipRefineOpts opts = {tol, 0, 0., 0};

  /* the reference: three solo calls on the twins */
  scs_float xs[K][N], ys[K][M], ss[K][M];
  ScsHipRefineInfo solo[K];
  for (int i = 0; i < K; ++i) {
    ScsSolution sol = {xs[i], ys[i], ss[i]};
    expect("solo scs_hip_refine on a twin", scs_hip_refine(twin[i], &sol, &opts, &solo[i]) == 0 && solo[i].stop == 1 && solo[i].steps >= 1);
  }

  /* the grouping, then one call for the three */
  scs_int group_of[K];
  expect("the three form one group", scs_hip_diff_batch_plan(w, K, 0, 0, group_of) == 1 && group_of[0] == 0 && group_of[1] == 0 && group_of[2] == 0);
  scs_float xb[K][N], yb[K][M], sb[K][M];
  ScsSolution sols[K];
  ScsSolution *solp[K];
  ScsHipRefineInfo got[K];
  ScsHipRefineInfo *infop[K];
  for (int i = 0; i < K; ++i) {
    sols[i].x = xb[i]; sols[i].y = yb[i]; sols[i].s = sb[i];
    solp[i] = &sols[i];
    infop[i] = &got[i];
  }
  const long before = scs_hip_diff_group_launches();
  scs_int rc = scs_hip_refine_batch(w, solp, &opts, infop, K);
  printf("scs_hip_refine_batch: rc %d (%s), steps %d %d %d, grouped launches %ld\n", (int)rc, scs_hip_last_error(), (int)got[0].steps,
         (int)got[1].steps, (int)got[2].steps, scs_hip_diff_group_launches() - before);
  expect("scs_hip_refine_batch", rc == 0);
  expect("the call went through grouped launches", scs_hip_diff_group_launches() > before);
  for (int i = 0; i < K; ++i) {
    expect("batch: x identical", memcmp(xb[i], xs[i], sizeof(xs[i])) == 0);
    expect("batch: y identical", memcmp(yb[i], ys[i], sizeof(ys[i])) == 0);
    expect("batch: s identical", memcmp(sb[i], ss[i], sizeof(ss[i])) == 0);
    expect("batch: info identical", same_info(&got[i], &solo[i]));
  }

  /* the device entry on the third set */
  ScsSolution sd[K];
  ScsSolution *sdp[K];
  ScsHipRefineInfo gd[K];
  ScsHipRefineInfo *gdp[K];
  for (int i = 0; i < K; ++i) {
    sd[i].x = dev_alloc(N); sd[i].y = dev_alloc(M); sd[i].s = dev_alloc(M);
    sdp[i] = &sd[i];
    gdp[i] = &gd[i];
  }
  sdp[1] = NULL;  /* a NULL entry: member 1 is refined, nothing is copied out */
  gdp[2] = NULL;
  rc = scs_hip_refine_batch_device(third, sdp, &opts, gdp, K);
  expect("scs_hip_refine_batch_device with a NULL sol entry and a NULL info entry", rc == 0);
  for (int i = 0; i < K; i += 2) {
    scs_float x2[N], y2[M], s2[M];
    if (hipMemcpy(x2, sd[i].x, sizeof(x2), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(y2, sd[i].y, sizeof(y2), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(s2, sd[i].s, sizeof(s2), hipMemcpyDeviceToHost) != hipSuccess) {
      printf("hipMemcpy failed\n");
      return 3;
    }
    expect("device entry: x, y, s identical", memcmp(x2, xs[i], sizeof(x2)) == 0 && memcmp(y2, ys[i], sizeof(y2)) == 0 && memcmp(s2, ss[i], sizeof(s2)) == 0);
  }
  expect("device entry: info identical", same_info(&gd[0], &solo[0]) && same_info(&gd[1], &solo[1]));
  /* member 1 was polished all the same: a second call finds nothing to do there */
  ScsHipRefineInfo again;
  expect("the member without a sol entry was refined", scs_hip_refine(third[1], NULL, &opts, &again) == 0 && again.steps == 0 && again.stop == 1);
  ScsSolution hostsol = {xb[0], yb[0], sb[0]};
  ScsSolution *mixed[K] = {&sd[0], &hostsol, &sd[2]};
  rc = scs_hip_refine_batch_device(third, mixed, &opts, NULL, K);
  printf("host pointers in member 1: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("host pointers are refused by the device entry, by member", rc == -1 && strstr(scs_hip_last_error(), "member 1") != NULL &&
                                                                         strstr(scs_hip_last_error(), "not a device address") != NULL);

  /* NULL arrays */
  expect("NULL sol, opts and info are accepted", scs_hip_refine_batch(w, NULL, NULL, NULL, K) == 0);

  /* a refused member: -1, its index, and nobody was touched */
  scs_int q[1] = {3};
  ScsMatrix A = {Ax, Ai, Ap, M, N}, P = {Px, Pi, Pp, N, N};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  ScsCone k;
  memset(&k, 0, sizeof(k));
  k.l = 3; k.q = q; k.qsize = 1;
  ScsData d = {M, N, &A, &P, B[0], Cv[0]};
  ScsWork *fresh = scs_init(&d, &k, &st);
  ScsWork *with_unsolved[K] = {w[0], w[1], fresh};
  for (int i = 0; i < K; ++i) got[i].stop = -7;
  rc = scs_hip_refine_batch(with_unsolved, solp, &opts, infop, K);
  printf("an unsolved member: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("an unsolved member is refused with its index", rc == -1 && strstr(scs_hip_last_error(), "member 2") != NULL &&
                                                           strstr(scs_hip_last_error(), "no solve yet") != NULL);
  expect("and no info was written", got[0].stop == -7 && got[1].stop == -7 && got[2].stop == -7);
  ScsWork *twice[K] = {w[0], w[1], w[0]};
  expect("a workspace that appears twice is refused", scs_hip_refine_batch(twice, NULL, &opts, NULL, K) == -1 &&
                                                        strstr(scs_hip_last_error(), "member 2") != NULL);
  expect("count 0 is refused", scs_hip_refine_batch(w, NULL, &opts, NULL, 0) == -1);
  scs_float x[N], y[M], s[M];
  ScsSolution sol = {x, y, s};
  ScsInfo info;
  expect("and the workspaces still solve", scs_solve(w[0], &sol, &info, 1) == SCS_SOLVED && scs_solve(fresh, &sol, &info, 0) == SCS_SOLVED);

  for (int i = 0; i < K; ++i) {
    (void)hipFree(sd[i].x); (void)hipFree(sd[i].y); (void)hipFree(sd[i].s);
    scs_finish(w[i]); scs_finish(twin[i]); scs_finish(third[i]);
  }
  scs_finish(fresh);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
