/* Plain-C consumer of scs_hip_refine / scs_hip_refine_device (include/scs_hip.h).  One QP with an SOC (m = 6, n = 3:
 * min 1/2 x'Px + c'x, x_j <= u_j, |(x_0, x_1)| <= 2 + 0.1 x_2) is solved at eps = 1e-4 on two twin workspaces; one is polished through
 * the host entry, the other through the device entry on hipMalloc'ed vectors, and the results compared with memcmp.  The two residual
 * norms are recomputed here and compared with info and with the stop rule.  One refused call (before a solve) names its reason.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_refine.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
 * Exit code 0 on success, 2 without a device; prints one line per check. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "scs_hip.h"

enum { M = 6, N = 3, ANNZ = 6, PNNZ = 4 };

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
static double maxabs(const double *v, int k) {
  double mx = 0.;
  for (int i = 0; i < k; ++i) mx = fmax(mx, fabs(v[i]));
  return mx;
}

int main(void) {
  if (scs_hip_device_count() < 1) {
    printf("no HIP device\n");
    return 2;
  }
  scs_int Ai[ANNZ] = {0, 4, 1, 5, 2, 3}, Ap[N + 1] = {0, 2, 4, 6};
  scs_float Ax[ANNZ] = {1.0, -1.0, 1.0, -1.0, 1.0, -0.1};
  /* P = [[1, 0.2, 0], [0.2, 1, 0], [0, 0, 0.5]], upper triangle by columns */
  scs_int Pi[PNNZ] = {0, 0, 1, 2}, Pp[N + 1] = {0, 1, 3, 4};
  scs_float Px[PNNZ] = {1.0, 0.2, 1.0, 0.5};
  scs_float b[M] = {1.5, 1.5, 1.0, 2.0, 0.0, 0.0};
  scs_float c[N] = {-3.0, -2.5, -1.0};
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
  ScsData d = {M, N, &A, &P, b, c};
  ScsWork *w = scs_init(&d, &k, &st), *twin = scs_init(&d, &k, &st);
  if (!w || !twin) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }

  const double tol = 1e-10;
  ScsHipRefineOpts opts = {tol, 0, 0., 0};
  ScsHipRefineInfo ri, rd;
  scs_float x[N], y[M], s[M];
  ScsSolution sol = {x, y, s};

  /* refused before a solve */
  scs_int rc = scs_hip_refine(w, &sol, &opts, &ri);
  printf("before a solve: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("refine before a solve returns -1 and says why", rc == -1 && strstr(scs_hip_last_error(), "no solve yet") != NULL);

  ScsInfo info;
  expect("solve", scs_solve(w, &sol, &info, 0) == SCS_SOLVED);
  printf("x = %.9f %.9f %.9f after %d iterations\n", x[0], x[1], x[2], (int)info.iter);
  rc = scs_hip_refine(w, &sol, &opts, &ri);
  printf("scs_hip_refine: rc %d (%s), steps %d halvings %d lsqr_iters %d stop %d, merit %.3e -> %.3e\n", (int)rc, scs_hip_last_error(),
         (int)ri.steps, (int)ri.halvings, (int)ri.lsqr_iters, (int)ri.stop, ri.merit_before, ri.merit_after);
  expect("scs_hip_refine", rc == 0);
  expect("stop = 1 after at least one step", ri.stop == 1 && ri.steps >= 1);
  expect("the merit fell", ri.merit_after < ri.merit_before);
  printf("x = %.15f %.15f %.15f\n", x[0], x[1], x[2]);

  /* the two residuals, recomputed */
  double Pf[N][N] = {{1.0, 0.2, 0.0}, {0.2, 1.0, 0.0}, {0.0, 0.0, 0.5}};
  double ax[M] = {0}, aty[N] = {0}, px[N] = {0}, rp[M], rdl[N];
  for (int j = 0; j < N; ++j)
    for (scs_int p = Ap[j]; p < Ap[j + 1]; ++p) {
      ax[Ai[p]] += Ax[p] * x[j];
      aty[j] += Ax[p] * y[Ai[p]];
    }
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) px[i] += Pf[i][j] * x[j];
  for (int i = 0; i < M; ++i) rp[i] = ax[i] + s[i] - b[i];
  for (int i = 0; i < N; ++i) rdl[i] = px[i] + aty[i] + c[i];
  const double res_pri = maxabs(rp, M), res_dual = maxabs(rdl, N);
  const double sc_pri = fmax(maxabs(ax, M), fmax(maxabs(s, M), maxabs(b, M))), sc_dual = fmax(maxabs(px, N), fmax(maxabs(aty, N), maxabs(c, N)));
  printf("res_pri %.3e (info %.3e), res_dual %.3e (info %.3e)\n", res_pri, ri.res_pri, res_dual, ri.res_dual);
  expect("the recomputed primal residual meets the rule", res_pri <= 10 * tol * (1. + sc_pri));
  expect("the recomputed dual residual meets the rule", res_dual <= 10 * tol * (1. + sc_dual));
  expect("info.res_pri is the recomputed one", fabs(ri.res_pri - res_pri) <= 1e-12 * (1. + sc_pri) + 1e-6 * res_pri);
  expect("info.res_dual is the recomputed one", fabs(ri.res_dual - res_dual) <= 1e-12 * (1. + sc_dual) + 1e-6 * res_dual);

  /* the twin through the device entry */
  scs_float x2[N], y2[M], s2[M];
  ScsSolution sol2 = {x2, y2, s2};
  expect("twin solve", scs_solve(twin, &sol2, &info, 0) == SCS_SOLVED);
  ScsSolution sd = {dev_alloc(N), dev_alloc(M), dev_alloc(M)};
  rc = scs_hip_refine_device(twin, &sd, &opts, &rd);
  expect("scs_hip_refine_device", rc == 0);
  if (hipMemcpy(x2, sd.x, sizeof(x2), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(y2, sd.y, sizeof(y2), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(s2, sd.s, sizeof(s2), hipMemcpyDeviceToHost) != hipSuccess) {
    printf("hipMemcpy failed\n");
    return 3;
  }
  expect("device entry: x identical", memcmp(x, x2, sizeof(x)) == 0);
  expect("device entry: y identical", memcmp(y, y2, sizeof(y)) == 0);
  expect("device entry: s identical", memcmp(s, s2, sizeof(s)) == 0);
  expect("device entry: info identical", ri.steps == rd.steps && ri.halvings == rd.halvings && ri.lsqr_iters == rd.lsqr_iters && ri.stop == rd.stop &&
                                          ri.merit_before == rd.merit_before && ri.merit_after == rd.merit_after && ri.res_pri == rd.res_pri &&
                                          ri.res_dual == rd.res_dual && ri.gap == rd.gap && ri.pobj == rd.pobj && ri.dobj == rd.dobj);
  rc = scs_hip_refine_device(twin, &sol2, &opts, &rd);
  expect("host pointers are refused by the device entry", rc == -1 && strstr(scs_hip_last_error(), "not a device address") != NULL);
  expect("NULL sol, opts and info are accepted", scs_hip_refine(w, NULL, NULL, NULL) == 0);
  expect("and the workspace still solves", scs_solve(w, &sol, &info, 1) == SCS_SOLVED);

  (void)hipFree(sd.x); (void)hipFree(sd.y); (void)hipFree(sd.s);
  scs_finish(w);
  scs_finish(twin);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
