/* Plain-C consumer of scs_hip_adjoint / scs_hip_adjoint_device / scs_hip_derivative / scs_hip_derivative_device (include/scs_hip.h).
 * The QP of cabi_update_matrix.c (m = 6, n = 3: 0 <= x_j <= u_j with coupling entries in A and P) is solved; its adjoint and forward
 * derivative are taken through the host and the device entries and compared with memcmp; <g, derivative(d)> is compared with
 * <adjoint(g), d>.  Then the refused calls: each returns -1 with a reason and leaves the workspace usable.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_adjoint.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
 * Exit code 0 on success, 2 without a device; prints one line per check. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "scs_hip.h"

enum { M = 6, N = 3, ANNZ = 8, PNNZ = 5 };

static int fails = 0;
static void expect(const char *what, int ok) {
  printf("%s -> %s\n", what, ok ? "ok" : "FAIL");
  fails += !ok;
}
static scs_float *to_device(const scs_float *h, size_t count) {
  scs_float *d = NULL;
  if (hipMalloc((void **)&d, count * sizeof(scs_float)) != hipSuccess) { printf("hipMalloc failed\n"); exit(3); }
  if (h && hipMemcpy(d, h, count * sizeof(scs_float), hipMemcpyHostToDevice) != hipSuccess) { printf("hipMemcpy failed\n"); exit(3); }
  return d;
}
static int same_as_device(const scs_float *host, const scs_float *dev, size_t count) {
  scs_float tmp[16];
  if (hipMemcpy(tmp, dev, count * sizeof(scs_float), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return memcmp(host, tmp, count * sizeof(scs_float)) == 0;
}
static scs_float dot(const scs_float *a, const scs_float *b, int n) {
  scs_float s = 0;
  for (int i = 0; i < n; ++i) s += a[i] * b[i];
  return s;
}

int main(void) {
  if (scs_hip_device_count() < 1) {
    printf("no HIP device\n");
    return 2;
  }
  scs_int Ai[ANNZ] = {0, 1, 3, 1, 4, 0, 2, 5}, Ap[N + 1] = {0, 3, 5, 8};
  scs_float Ax[ANNZ] = {1.0, 0.25, -1.0, 1.0, -1.0, -0.5, 1.0, -1.0};
  scs_int Pi[PNNZ] = {0, 0, 1, 1, 2}, Pp[N + 1] = {0, 1, 3, 5};
  scs_float Px[PNNZ] = {2.0, 0.5, 1.0, -0.25, 3.0};
  scs_float b[M] = {1.0, 2.0, 3.0, 0.0, 0.0, 0.0}, c[N] = {-1.0, 1.0, -2.0};
  ScsMatrix A = {Ax, Ai, Ap, M, N}, P = {Px, Pi, Pp, N, N};
  ScsData d = {M, N, &A, &P, b, c}, dlp = {M, N, &A, NULL, b, c};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  st.eps_abs = st.eps_rel = 1e-9;
  ScsCone k;
  memset(&k, 0, sizeof(k));
  k.l = M;
  ScsWork *w = scs_init(&d, &k, &st), *wlp = scs_init(&dlp, &k, &st);
  if (!w || !wlp) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }

  scs_float gx[N] = {1.0, -2.0, 0.5}, gy[M] = {0.3, -0.1, 0.2, 0.7, -0.4, 0.9}, gs[M] = {-0.6, 0.8, 0.1, -0.2, 0.5, 0.4};
  scs_float db[M], dc[N], dA[ANNZ], dP[PNNZ];
  ScsHipDiffOpts opts = {1e-12, 0};
  ScsHipDiffInfo hi, di;

  /* before the first solve */
  scs_int rc = scs_hip_adjoint(w, gx, gy, gs, db, dc, NULL, NULL, &opts, &hi);
  printf("no solve yet: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("before the first solve: -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "no solve yet") != NULL);

  scs_float x[N], y[M], s[M];
  ScsSolution sol = {x, y, s};
  ScsInfo info;
  expect("solve", scs_solve(w, &sol, &info, 0) == SCS_SOLVED);

  rc = scs_hip_adjoint(w, gx, gy, gs, db, dc, dA, dP, &opts, &hi);
  printf("host adjoint: rc %d iters %d stop %d residual %.3e normal %.3e\n", (int)rc, (int)hi.iters, (int)hi.stop, hi.residual, hi.normal_residual);
  expect("scs_hip_adjoint", rc == 0 && hi.iters >= 1 && (hi.stop == 1 || hi.stop == 2));
  scs_float *gx_d = to_device(gx, N), *gy_d = to_device(gy, M), *gs_d = to_device(gs, M);
  scs_float *db_d = to_device(NULL, M), *dc_d = to_device(NULL, N), *dA_d = to_device(NULL, ANNZ), *dP_d = to_device(NULL, PNNZ);
  rc = scs_hip_adjoint_device(w, gx_d, gy_d, gs_d, db_d, dc_d, dA_d, dP_d, &opts, &di);
  expect("scs_hip_adjoint_device", rc == 0 && di.iters == hi.iters && di.stop == hi.stop);
  expect("adjoint: db identical", same_as_device(db, db_d, M));
  expect("adjoint: dc identical", same_as_device(dc, dc_d, N));
  expect("adjoint: dA identical", same_as_device(dA, dA_d, ANNZ));
  expect("adjoint: dP identical", same_as_device(dP, dP_d, PNNZ));

  scs_float vb[M] = {0.5, -1.0, 0.25, 1.0, -0.75, 0.1}, vc[N] = {-0.3, 0.6, 1.2}, dx[N], dy[M], ds[M];
  rc = scs_hip_derivative(w, vb, vc, dx, dy, ds, &opts, &hi);
  expect("scs_hip_derivative", rc == 0 && (hi.stop == 1 || hi.stop == 2));
  scs_float *vb_d = to_device(vb, M), *vc_d = to_device(vc, N), *dx_d = to_device(NULL, N), *dy_d = to_device(NULL, M), *ds_d = to_device(NULL, M);
  rc = scs_hip_derivative_device(w, vb_d, vc_d, dx_d, dy_d, ds_d, &opts, &di);
  expect("scs_hip_derivative_device", rc == 0 && di.iters == hi.iters);
  expect("derivative: dx identical", same_as_device(dx, dx_d, N));
  expect("derivative: dy identical", same_as_device(dy, dy_d, M));
  expect("derivative: ds identical", same_as_device(ds, ds_d, M));
  const scs_float lhs = dot(gx, dx, N) + dot(gy, dy, M) + dot(gs, ds, M), rhs = dot(db, vb, M) + dot(dc, vc, N);
  printf("duality: %.15e vs %.15e\n", lhs, rhs);
  expect("<g, derivative(d)> = <adjoint(g), d>", fabs(lhs - rhs) <= 1e-8 * (fabs(lhs) + fabs(rhs) + 1.0));
  scs_float dc_only[N];
  expect("NULL inputs and outputs are accepted", scs_hip_adjoint(w, gx, NULL, NULL, NULL, dc_only, NULL, NULL, NULL, NULL) == 0);

  /* refused before any device work */
  rc = scs_hip_adjoint(NULL, gx, gy, gs, db, dc, NULL, NULL, &opts, &hi);
  expect("NULL workspace returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "null workspace") != NULL);
  rc = scs_hip_adjoint_device(w, gx, gy_d, gs_d, db_d, dc_d, NULL, NULL, &opts, &di);
  printf("host address as gx_dev: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("host address as gx_dev returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "gx_dev") != NULL);
  rc = scs_hip_derivative_device(w, vb_d, vc_d, dx, dy_d, ds_d, &opts, &di);
  expect("host address as dx_dev returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "dx_dev") != NULL);
  scs_float xl[N], yl[M], sl[M];
  ScsSolution soll = {xl, yl, sl};
  expect("solve (no P)", scs_solve(wlp, &soll, &info, 0) == SCS_SOLVED);
  rc = scs_hip_adjoint(wlp, gx, gy, gs, db, dc, NULL, dP, &opts, &hi);
  printf("dPx without P: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("dPx for a workspace without P returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "without P") != NULL);
  expect("scs_update", scs_update(w, b, NULL) == 0);
  rc = scs_hip_derivative(w, vb, vc, dx, dy, ds, &opts, &hi);
  printf("after scs_update: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("a stale solution returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "stale") != NULL);
  expect("after the refusals the workspace solves", scs_solve(w, &sol, &info, 0) == SCS_SOLVED);
  scs_float db2[M], dc2[N];
  rc = scs_hip_adjoint(w, gx, gy, gs, db2, dc2, NULL, NULL, &opts, &hi);
  scs_float diff = 0;
  for (int i = 0; i < M; ++i) diff = fmax(diff, fabs(db2[i] - db[i]));
  for (int i = 0; i < N; ++i) diff = fmax(diff, fabs(dc2[i] - dc[i]));
  printf("adjoint after the new solve: max difference %.3e\n", diff);
  expect("... and differentiates again", rc == 0 && diff <= 1e-6);

  scs_finish(w); scs_finish(wlp);
  (void)hipFree(gx_d); (void)hipFree(gy_d); (void)hipFree(gs_d); (void)hipFree(db_d); (void)hipFree(dc_d); (void)hipFree(dA_d); (void)hipFree(dP_d);
  (void)hipFree(vb_d); (void)hipFree(vc_d); (void)hipFree(dx_d); (void)hipFree(dy_d); (void)hipFree(ds_d);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
