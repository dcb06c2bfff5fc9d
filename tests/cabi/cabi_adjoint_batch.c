/* Plain-C consumer of scs_hip_adjoint_batch / scs_hip_derivative_batch / scs_hip_diff_batch_plan / scs_hip_diff_group_launches
 * (include/scs_hip.h).  Three LP + SOC members (m = 6, n = 3: x_j <= u_j and |(x_0, x_1)| <= 2 + 0.1 x_2) that differ in b and c are
 * built and solved; their adjoints and forward derivatives are taken one by one and as one batch and compared with memcmp.  Then the
 * refused calls: each returns -1 with a reason.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_adjoint_batch.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
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

int main(void) {
  if (scs_hip_device_count() < 1) {
    printf("no HIP device\n");
    return 2;
  }
  scs_int Ai[ANNZ] = {0, 4, 1, 5, 2, 3}, Ap[N + 1] = {0, 2, 4, 6};
  scs_float Ax[ANNZ] = {1.0, -1.0, 1.0, -1.0, 1.0, -0.1};
  scs_float b[K][M] = {{1.5, 1.5, 1.0, 2.0, 0.0, 0.0}, {3.0, 3.0, 2.0, 2.0, 0.0, 0.0}, {1.0, 3.0, 0.5, 2.0, 0.0, 0.0}};
  scs_float c[K][N] = {{-1.0, -0.5, -1.0}, {-1.0, -2.0, -0.5}, {-0.25, -1.0, -2.0}};
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
  ScsWork *w[K];
  scs_float x[N], y[M], s[M];
  ScsSolution sol = {x, y, s};
  ScsInfo info;
  for (int i = 0; i < K; ++i) {
    ScsData d = {M, N, &A, NULL, b[i], c[i]};
    w[i] = scs_init(&d, &k, &st);
    if (!w[i]) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }
    expect("solve", scs_solve(w[i], &sol, &info, 0) == SCS_SOLVED);
    printf("member %d: x = %.6f %.6f %.6f\n", i, x[0], x[1], x[2]);
  }
  scs_float gx[K][N] = {{1.0, -2.0, 0.5}, {0.5, 0.25, -1.0}, {-1.0, 1.0, 2.0}};
  scs_float gy[K][M] = {{0.3, -0.1, 0.2, 0.7, -0.4, 0.9}, {0.1, 0.2, 0.3, -0.4, 0.5, -0.6}, {-0.9, 0.8, -0.7, 0.6, -0.5, 0.4}};
  scs_float gs[K][M] = {{-0.6, 0.8, 0.1, -0.2, 0.5, 0.4}, {0.6, -0.8, 0.3, 0.2, -0.5, 0.1}, {0.2, 0.4, -0.6, 0.8, 1.0, -1.2}};
  ScsHipDiffOpts opts = {1e-12, 0};

  /* one by one */
  scs_float db1[K][M], dc1[K][N], dA1[K][ANNZ], dx1[K][N], dy1[K][M], ds1[K][M];
  ScsHipDiffInfo i1[K], f1[K];
  for (int i = 0; i < K; ++i) {
    expect("scs_hip_adjoint", scs_hip_adjoint(w[i], gx[i], gy[i], gs[i], db1[i], dc1[i], dA1[i], NULL, &opts, &i1[i]) == 0);
    expect("scs_hip_derivative", scs_hip_derivative(w[i], gy[i], gx[i], dx1[i], dy1[i], ds1[i], &opts, &f1[i]) == 0);
  }

  /* as one batch */
  scs_int group_of[K] = {7, 7, 7};
  expect("scs_hip_diff_batch_plan: one group of three", scs_hip_diff_batch_plan(w, K, 1, 0, group_of) == 1 && group_of[0] == 0 &&
                                                            group_of[1] == 0 && group_of[2] == 0);
  scs_float db2[K][M], dc2[K][N], dA2[K][ANNZ], dx2[K][N], dy2[K][M], ds2[K][M];
  const scs_float *gxp[K] = {gx[0], gx[1], gx[2]}, *gyp[K] = {gy[0], gy[1], gy[2]}, *gsp[K] = {gs[0], gs[1], gs[2]};
  scs_float *dbp[K] = {db2[0], db2[1], db2[2]}, *dcp[K] = {dc2[0], dc2[1], dc2[2]}, *dAp[K] = {dA2[0], dA2[1], dA2[2]};
  scs_float *dxp[K] = {dx2[0], dx2[1], dx2[2]}, *dyp[K] = {dy2[0], dy2[1], dy2[2]}, *dsp[K] = {ds2[0], ds2[1], ds2[2]};
  ScsHipDiffInfo i2[K], f2[K], *i2p[K] = {&i2[0], &i2[1], &i2[2]}, *f2p[K] = {&f2[0], &f2[1], &f2[2]};
  const long before = scs_hip_diff_group_launches();
  scs_int rc = scs_hip_adjoint_batch(w, gxp, gyp, gsp, dbp, dcp, dAp, NULL, &opts, i2p, K);
  printf("scs_hip_adjoint_batch: rc %d (%s), iters %d %d %d, grouped launches %ld\n", (int)rc, scs_hip_last_error(), (int)i2[0].iters,
         (int)i2[1].iters, (int)i2[2].iters, scs_hip_diff_group_launches() - before);
  expect("scs_hip_adjoint_batch", rc == 0);
  expect("grouped launches were issued", scs_hip_diff_group_launches() > before);
  expect("adjoint batch: db identical", memcmp(db1, db2, sizeof(db1)) == 0);
  expect("adjoint batch: dc identical", memcmp(dc1, dc2, sizeof(dc1)) == 0);
  expect("adjoint batch: dA identical", memcmp(dA1, dA2, sizeof(dA1)) == 0);
  int same = 1;
  for (int i = 0; i < K; ++i)
    same = same && i1[i].iters == i2[i].iters && i1[i].stop == i2[i].stop && i1[i].residual == i2[i].residual &&
           i1[i].normal_residual == i2[i].normal_residual;
  expect("adjoint batch: info identical", same);
  rc = scs_hip_derivative_batch(w, gyp, gxp, dxp, dyp, dsp, &opts, f2p, K);
  expect("scs_hip_derivative_batch", rc == 0);
  expect("derivative batch: dx identical", memcmp(dx1, dx2, sizeof(dx1)) == 0);
  expect("derivative batch: dy identical", memcmp(dy1, dy2, sizeof(dy1)) == 0);
  expect("derivative batch: ds identical", memcmp(ds1, ds2, sizeof(ds1)) == 0);
  same = 1;
  for (int i = 0; i < K; ++i) same = same && f1[i].iters == f2[i].iters && f1[i].stop == f2[i].stop && f1[i].residual == f2[i].residual;
  expect("derivative batch: info identical", same);
  expect("NULL arrays and NULL entries are accepted", scs_hip_adjoint_batch(w, gxp, NULL, NULL, NULL, dcp, NULL, NULL, NULL, NULL, K) == 0);

  /* refused before any device work */
  memset(db2, 0, sizeof(db2));
  rc = scs_hip_adjoint_batch(w, gxp, gyp, gsp, dbp, dcp, NULL, NULL, &opts, i2p, 0);
  printf("count 0: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("a count of 0 returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "count") != NULL);
  ScsWork *hole[K] = {w[0], NULL, w[2]};
  rc = scs_hip_adjoint_batch(hole, gxp, gyp, gsp, dbp, dcp, NULL, NULL, &opts, i2p, K);
  printf("NULL member: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("a NULL member returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "member 1") != NULL);
  ScsWork *twice[K] = {w[0], w[1], w[0]};
  rc = scs_hip_derivative_batch(twice, gyp, gxp, dxp, dyp, dsp, &opts, f2p, K);
  expect("a workspace twice returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "twice") != NULL);
  int untouched = 1;
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < M; ++j) untouched = untouched && db2[i][j] == 0.0;
  expect("a refused call writes no output", untouched);
  rc = scs_hip_adjoint_batch(w, gxp, gyp, gsp, dbp, dcp, dAp, NULL, &opts, i2p, K);
  expect("after the refusals the batch differentiates again", rc == 0 && memcmp(db1, db2, sizeof(db1)) == 0);

  for (int i = 0; i < K; ++i) scs_finish(w[i]);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
