/* Plain-C consumer of scs_hip_adjoint_multi / scs_hip_derivative_multi (include/scs_hip.h).  One LP + SOC problem (m = 6, n = 3:
 * x_j <= u_j and |(x_0, x_1)| <= 2 + 0.1 x_2) is built and solved; K = 3 cotangents are differentiated by three calls of
 * scs_hip_adjoint and by ONE call of scs_hip_adjoint_multi, and the results compared with memcmp; the same for the forward derivative.
 * Then the refused calls: each returns -1 with a reason and writes nothing.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_adjoint_multi.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
 * Exit code 0 on success, 2 without a device; prints one line per check. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scs_hip.h"

enum { M = 6, N = 3, ANNZ = 6, K = 3 };

static int fails = 0;
static void expect(const char *what, int ok) {
  printf("%s -> %s\n", what, ok ? "ok" : "FAIL");
  fails += !ok;
}
static int same_info(const ScsHipDiffInfo *a, const ScsHipDiffInfo *b) {
  int same = 1;
  for (int i = 0; i < K; ++i)
    same = same && a[i].iters == b[i].iters && a[i].stop == b[i].stop && a[i].residual == b[i].residual &&
           a[i].normal_residual == b[i].normal_residual;
  return same;
}

int main(void) {
  if (scs_hip_device_count() < 1) {
    printf("no HIP device\n");
    return 2;
  }
  scs_int Ai[ANNZ] = {0, 4, 1, 5, 2, 3}, Ap[N + 1] = {0, 2, 4, 6};
  scs_float Ax[ANNZ] = {1.0, -1.0, 1.0, -1.0, 1.0, -0.1};
  scs_float b[M] = {1.5, 1.5, 1.0, 2.0, 0.0, 0.0};
  scs_float c[N] = {-1.0, -0.5, -1.0};
  scs_int q[1] = {3};
  ScsMatrix A = {Ax, Ai, Ap, M, N};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  st.eps_abs = st.eps_rel = 1e-9;
  ScsCone k;
  memset(&k, 0, sizeof(k));
  k.l = 3;
  k.q = q;
  k.qsize = 1;
  scs_float x[N], y[M], s[M];
  ScsSolution sol = {x, y, s};
  ScsInfo info;
  ScsData d = {M, N, &A, NULL, b, c};
  ScsWork *w = scs_init(&d, &k, &st);
  if (!w) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }
  expect("solve", scs_solve(w, &sol, &info, 0) == SCS_SOLVED);
  printf("x = %.6f %.6f %.6f\n", x[0], x[1], x[2]);

  scs_float gx[K][N] = {{1.0, -2.0, 0.5}, {0.0, 0.0, 0.0}, {-1.0, 1.0, 2.0}};
  scs_float gy[K][M] = {{0.3, -0.1, 0.2, 0.7, -0.4, 0.9}, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, {-0.9, 0.8, -0.7, 0.6, -0.5, 0.4}};
  scs_float gs[K][M] = {{-0.6, 0.8, 0.1, -0.2, 0.5, 0.4}, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, {0.2, 0.4, -0.6, 0.8, 1.0, -1.2}};
  ScsHipDiffOpts opts = {1e-12, 0};

  /* one by one */
  scs_float db1[K][M], dc1[K][N], dA1[K][ANNZ], dx1[K][N], dy1[K][M], ds1[K][M];
  ScsHipDiffInfo i1[K], f1[K];
  for (int i = 0; i < K; ++i) {
    expect("scs_hip_adjoint", scs_hip_adjoint(w, gx[i], gy[i], gs[i], db1[i], dc1[i], dA1[i], NULL, &opts, &i1[i]) == 0);
    expect("scs_hip_derivative", scs_hip_derivative(w, gy[i], gx[i], dx1[i], dy1[i], ds1[i], &opts, &f1[i]) == 0);
  }

  /* K directions in one call */
  scs_float db2[K][M], dc2[K][N], dA2[K][ANNZ], dx2[K][N], dy2[K][M], ds2[K][M];
  ScsHipDiffInfo i2[K], f2[K];
  scs_int rc = scs_hip_adjoint_multi(w, K, &gx[0][0], &gy[0][0], &gs[0][0], &db2[0][0], &dc2[0][0], &dA2[0][0], NULL, &opts, i2);
  printf("scs_hip_adjoint_multi: rc %d (%s), iters %d %d %d\n", (int)rc, scs_hip_last_error(), (int)i2[0].iters, (int)i2[1].iters,
         (int)i2[2].iters);
  expect("scs_hip_adjoint_multi", rc == 0);
  expect("adjoint multi: db identical", memcmp(db1, db2, sizeof(db1)) == 0);
  expect("adjoint multi: dc identical", memcmp(dc1, dc2, sizeof(dc1)) == 0);
  expect("adjoint multi: dA identical", memcmp(dA1, dA2, sizeof(dA1)) == 0);
  expect("adjoint multi: info identical", same_info(i1, i2));
  rc = scs_hip_derivative_multi(w, K, &gy[0][0], &gx[0][0], &dx2[0][0], &dy2[0][0], &ds2[0][0], &opts, f2);
  expect("scs_hip_derivative_multi", rc == 0);
  expect("derivative multi: dx identical", memcmp(dx1, dx2, sizeof(dx1)) == 0);
  expect("derivative multi: dy identical", memcmp(dy1, dy2, sizeof(dy1)) == 0);
  expect("derivative multi: ds identical", memcmp(ds1, ds2, sizeof(ds1)) == 0);
  expect("derivative multi: info identical", same_info(f1, f2));
  expect("NULL inputs, outputs and infos are accepted", scs_hip_adjoint_multi(w, K, &gx[0][0], NULL, NULL, NULL, &dc2[0][0], NULL, NULL, NULL, NULL) == 0);

  /* refused before any device work */
  memset(db2, 0, sizeof(db2));
  rc = scs_hip_adjoint_multi(w, 0, &gx[0][0], &gy[0][0], &gs[0][0], &db2[0][0], &dc2[0][0], NULL, NULL, &opts, i2);
  printf("K = 0: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("K = 0 returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "K = 0") != NULL);
  rc = scs_hip_adjoint_multi(w, 33, &gx[0][0], &gy[0][0], &gs[0][0], &db2[0][0], &dc2[0][0], NULL, NULL, &opts, i2);
  printf("K = 33: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("K = 33 returns -1 and names the limit", rc == -1 && strstr(scs_hip_last_error(), "32") != NULL);
  rc = scs_hip_adjoint_multi(w, K, &gx[0][0], &gy[0][0], &gs[0][0], &db2[0][0], &dc2[0][0], NULL, &dA2[0][0], &opts, i2);
  expect("dPx without P returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "without P") != NULL);
  int untouched = 1;
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < M; ++j) untouched = untouched && db2[i][j] == 0.0;
  expect("a refused call writes no output", untouched);
  rc = scs_hip_adjoint_multi(w, K, &gx[0][0], &gy[0][0], &gs[0][0], &db2[0][0], &dc2[0][0], &dA2[0][0], NULL, &opts, i2);
  expect("after the refusals the workspace differentiates again", rc == 0 && memcmp(db1, db2, sizeof(db1)) == 0);
  expect("and still solves", scs_solve(w, &sol, &info, 0) == SCS_SOLVED);

  scs_finish(w);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
