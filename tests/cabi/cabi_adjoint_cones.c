/* Plain-C consumer of scs_hip_adjoint / scs_hip_derivative and their device twins (include/scs_hip.h) on a problem with a box cone:
 * the bounded QP  min 1/2 x'P x + c'x  s.t. bl <= x <= bu  (n = 3), written as (t, x) in the box cone with t fixed to 1 by a zero row of A
 * (m = 4, b = (1, 0, 0, 0), the bound rows of A are -I).  At the solution x = (1, -0.825, -0.5): x_0 sits on its upper bound, x_2 on its
 * lower bound, x_1 is free, so dx/dc_1 = (0, -1 / P_11, 0) = (0, -1, 0) exactly.  The host and device entries are compared with memcmp,
 * <g, derivative(d)> with <adjoint(g), d>.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_adjoint_cones.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
 * Exit code 0 on success, 2 without a device; prints one line per check. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "scs_hip.h"

enum { M = 4, N = 3, ANNZ = 3, PNNZ = 5 };

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
  scs_int Ai[ANNZ] = {1, 2, 3}, Ap[N + 1] = {0, 1, 2, 3};
  scs_float Ax[ANNZ] = {-1.0, -1.0, -1.0};
  scs_int Pi[PNNZ] = {0, 0, 1, 1, 2}, Pp[N + 1] = {0, 1, 3, 5};
  scs_float Px[PNNZ] = {2.0, 0.5, 1.0, -0.25, 3.0};
  scs_float b[M] = {1.0, 0.0, 0.0, 0.0}, c[N] = {-5.0, 0.2, 4.0};
  scs_float bl[N] = {0.0, -1.0, -0.5}, bu[N] = {1.0, 1.0, 0.5};
  ScsMatrix A = {Ax, Ai, Ap, M, N}, P = {Px, Pi, Pp, N, N};
  ScsData d = {M, N, &A, &P, b, c};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  st.eps_abs = st.eps_rel = 1e-10;
  ScsCone k;
  memset(&k, 0, sizeof(k));
  k.bl = bl;
  k.bu = bu;
  k.bsize = M;
  ScsWork *w = scs_init(&d, &k, &st);
  if (!w) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }

  scs_float x[N], y[M], s[M];
  ScsSolution sol = {x, y, s};
  ScsInfo info;
  expect("solve", scs_solve(w, &sol, &info, 0) == SCS_SOLVED);
  printf("x = %.9f %.9f %.9f\n", x[0], x[1], x[2]);
  expect("the bounds are active as built", fabs(x[0] - 1.0) <= 1e-7 && fabs(x[1] + 0.825) <= 1e-7 && fabs(x[2] + 0.5) <= 1e-7);

  scs_float gx[N] = {1.0, -2.0, 0.5}, gy[M] = {0.3, -0.1, 0.2, 0.7}, gs[M] = {-0.6, 0.8, 0.1, -0.2};
  scs_float db[M], dc[N], dA[ANNZ], dP[PNNZ];
  ScsHipDiffOpts opts = {1e-12, 0};
  ScsHipDiffInfo hi, di;
  scs_int rc = scs_hip_adjoint(w, gx, gy, gs, db, dc, dA, dP, &opts, &hi);
  printf("host adjoint: rc %d (%s) iters %d stop %d residual %.3e\n", (int)rc, rc ? scs_hip_last_error() : "", (int)hi.iters, (int)hi.stop, hi.residual);
  expect("scs_hip_adjoint on a box cone", rc == 0 && hi.iters >= 1 && (hi.stop == 1 || hi.stop == 2));
  scs_float *gx_d = to_device(gx, N), *gy_d = to_device(gy, M), *gs_d = to_device(gs, M);
  scs_float *db_d = to_device(NULL, M), *dc_d = to_device(NULL, N), *dA_d = to_device(NULL, ANNZ), *dP_d = to_device(NULL, PNNZ);
  rc = scs_hip_adjoint_device(w, gx_d, gy_d, gs_d, db_d, dc_d, dA_d, dP_d, &opts, &di);
  expect("scs_hip_adjoint_device", rc == 0 && di.iters == hi.iters && di.stop == hi.stop);
  expect("adjoint: db identical", same_as_device(db, db_d, M));
  expect("adjoint: dc identical", same_as_device(dc, dc_d, N));
  expect("adjoint: dA identical", same_as_device(dA, dA_d, ANNZ));
  expect("adjoint: dP identical", same_as_device(dP, dP_d, PNNZ));

  scs_float e1[N] = {0.0, 1.0, 0.0}, dx[N], dy[M], ds[M];
  rc = scs_hip_derivative(w, NULL, e1, dx, dy, ds, &opts, &hi);
  printf("dx / dc_1 = %.12f %.12f %.12f\n", dx[0], dx[1], dx[2]);
  expect("the free variable moves by -1 / P_11, the bounded ones stay", rc == 0 && fabs(dx[0]) <= 1e-9 && fabs(dx[1] + 1.0) <= 1e-9 && fabs(dx[2]) <= 1e-9);

  scs_float vb[M] = {0.5, -1.0, 0.25, 1.0}, vc[N] = {-0.3, 0.6, 1.2};
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
  expect("after differentiating the workspace solves", scs_solve(w, &sol, &info, 1) == SCS_SOLVED);

  scs_finish(w);
  (void)hipFree(gx_d); (void)hipFree(gy_d); (void)hipFree(gs_d); (void)hipFree(db_d); (void)hipFree(dc_d); (void)hipFree(dA_d); (void)hipFree(dP_d);
  (void)hipFree(vb_d); (void)hipFree(vc_d); (void)hipFree(dx_d); (void)hipFree(dy_d); (void)hipFree(ds_d);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
