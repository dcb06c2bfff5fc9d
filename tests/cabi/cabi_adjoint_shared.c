/* Plain-C consumer of scs_hip_adjoint_shared (include/scs_hip.h).  One LP + SOC problem (m = 6, n = 3: x_j <= u_j and
 * |(x_0, x_1)| <= 2 + 0.1 x_2) and a clone of it with another b and c are solved; the gradient of the shared A, summed over the two, is
 * compared with two scs_hip_adjoint calls added on the host.  Both are sums of the same 2K = 4 products per entry in some order, so they
 * differ by at most (2K + 2) 2^-52 sum|products| (tests/test_grad_shared_gpu.py: that bound holds for either against the exact sum at
 * half its size).  db, dc and the LSQR figures must be the bits of the one-by-one calls.  Then the refused calls: each returns -1 with
 * a reason.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_adjoint_shared.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
 * Exit code 0 on success, 2 without a device; prints one line per check. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scs_hip.h"

enum { M = 6, N = 3, ANNZ = 6, K = 2 };

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
  scs_float b[K][M] = {{1.5, 1.5, 1.0, 2.0, 0.0, 0.0}, {3.0, 3.0, 2.0, 2.0, 0.0, 0.0}};
  scs_float c[K][N] = {{-1.0, -0.5, -1.0}, {-1.0, -2.0, -0.5}};
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
  ScsData d = {M, N, &A, NULL, b[0], c[0]};
  ScsWork *w[K];
  w[0] = scs_init(&d, &k, &st);
  if (!w[0]) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }
  w[1] = scs_hip_clone(w[0]);
  if (!w[1]) { printf("scs_hip_clone failed: %s\n", scs_hip_last_error()); return 3; }
  expect("the clone shares the matrix", scs_hip_shares_matrix(w[0], w[1]) == 1);
  expect("scs_update of the clone", scs_update(w[1], b[1], c[1]) == 0);
  scs_float x[K][N], y[K][M], s[K][M];
  ScsInfo info;
  for (int i = 0; i < K; ++i) {
    ScsSolution sol = {x[i], y[i], s[i]};
    expect("solve", scs_solve(w[i], &sol, &info, 0) == SCS_SOLVED);
    printf("member %d: x = %.6f %.6f %.6f\n", i, x[i][0], x[i][1], x[i][2]);
  }
  scs_float gx[K][N] = {{1.0, -2.0, 0.5}, {0.5, 0.25, -1.0}};
  scs_float gy[K][M] = {{0.3, -0.1, 0.2, 0.7, -0.4, 0.9}, {0.1, 0.2, 0.3, -0.4, 0.5, -0.6}};
  scs_float gs[K][M] = {{-0.6, 0.8, 0.1, -0.2, 0.5, 0.4}, {0.6, -0.8, 0.3, 0.2, -0.5, 0.1}};
  ScsHipDiffOpts opts = {1e-12, 0};

  /* one by one */
  scs_float db1[K][M], dc1[K][N], dA1[K][ANNZ];
  ScsHipDiffInfo i1[K];
  for (int i = 0; i < K; ++i)
    expect("scs_hip_adjoint", scs_hip_adjoint(w[i], gx[i], gy[i], gs[i], db1[i], dc1[i], dA1[i], NULL, &opts, &i1[i]) == 0);

  /* shared: one dA for both */
  scs_float db2[K][M], dc2[K][N], dA2[ANNZ];
  const scs_float *gxp[K] = {gx[0], gx[1]}, *gyp[K] = {gy[0], gy[1]}, *gsp[K] = {gs[0], gs[1]};
  scs_float *dbp[K] = {db2[0], db2[1]}, *dcp[K] = {dc2[0], dc2[1]};
  ScsHipDiffInfo i2[K], *i2p[K] = {&i2[0], &i2[1]};
  scs_int rc = scs_hip_adjoint_shared(w, gxp, gyp, gsp, dbp, dcp, dA2, NULL, &opts, i2p, K);
  printf("scs_hip_adjoint_shared: rc %d (%s), iters %d %d\n", (int)rc, scs_hip_last_error(), (int)i2[0].iters, (int)i2[1].iters);
  expect("scs_hip_adjoint_shared", rc == 0);
  expect("shared: db identical", memcmp(db1, db2, sizeof(db1)) == 0);
  expect("shared: dc identical", memcmp(dc1, dc2, sizeof(dc1)) == 0);
  int same = 1;
  for (int i = 0; i < K; ++i)
    same = same && i1[i].iters == i2[i].iters && i1[i].stop == i2[i].stop && i1[i].residual == i2[i].residual &&
           i1[i].normal_residual == i2[i].normal_residual;
  expect("shared: info identical", same);
  int within = 1, nonzero = 0;
  for (int j = 0; j < N; ++j)
    for (int p = Ap[j]; p < Ap[j + 1]; ++p) {
      const int i = Ai[p];
      double mag = 0.0;
      for (int m = 0; m < K; ++m) mag += fabs(y[m][i] * dc1[m][j]) + fabs(db1[m][i] * x[m][j]);
      const double host = dA1[0][p] + dA1[1][p], bound = (2 * K + 2) * ldexp(1.0, -52) * mag;
      printf("dA[%d]: shared %.17g  host sum %.17g  bound %.3g\n", p, dA2[p], host, bound);
      within = within && fabs(dA2[p] - host) <= bound;
      nonzero = nonzero || dA2[p] != 0.0;
    }
  expect("shared: dA is the sum of the two adjoints' dA within the bound", within && nonzero);
  scs_float dA3[ANNZ];
  expect("db and dc may be NULL", scs_hip_adjoint_shared(w, gxp, gyp, gsp, NULL, NULL, dA3, NULL, &opts, NULL, K) == 0);
  expect("two calls: identical dA", memcmp(dA2, dA3, sizeof(dA2)) == 0);

  /* refused before any device work */
  scs_float dP[1] = {0.0};
  memset(dA3, 0, sizeof(dA3));
  rc = scs_hip_adjoint_shared(w, gxp, gyp, gsp, dbp, dcp, NULL, NULL, &opts, i2p, K);
  printf("both NULL: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("both sums NULL returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "both NULL") != NULL);
  rc = scs_hip_adjoint_shared(w, gxp, gyp, gsp, dbp, dcp, dA3, dP, &opts, i2p, K);
  printf("dPx_sum without P: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("dPx_sum for workspaces without P returns -1 with a reason",
         rc == -1 && strstr(scs_hip_last_error(), "member 0") != NULL && strstr(scs_hip_last_error(), "without P") != NULL);
  ScsWork *apart = scs_init(&d, &k, &st);
  if (!apart) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }
  {
    scs_float xa[N], ya[M], sa[M];
    ScsSolution sol = {xa, ya, sa};
    expect("solve", scs_solve(apart, &sol, &info, 0) == SCS_SOLVED);
  }
  ScsWork *mixed[K] = {w[0], apart};
  rc = scs_hip_adjoint_shared(mixed, gxp, gyp, gsp, dbp, dcp, dA3, NULL, &opts, i2p, K);
  printf("another matrix set: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("a member of another matrix set returns -1 with a reason",
         rc == -1 && strstr(scs_hip_last_error(), "member 1") != NULL && strstr(scs_hip_last_error(), "share") != NULL);
  int untouched = 1;
  for (int p = 0; p < ANNZ; ++p) untouched = untouched && dA3[p] == 0.0;
  expect("a refused call writes no output", untouched);
  rc = scs_hip_adjoint_shared(w, gxp, gyp, gsp, dbp, dcp, dA3, NULL, &opts, i2p, K);
  expect("after the refusals the call works again", rc == 0 && memcmp(dA2, dA3, sizeof(dA2)) == 0 && memcmp(db1, db2, sizeof(db1)) == 0);

  scs_finish(apart);
  for (int i = 0; i < K; ++i) scs_finish(w[i]);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
