/* Plain-C consumer of the device-resident endpoints (include/scs_hip.h: scs_hip_update_device, scs_hip_solve_device): b, c, x, y, s
 * live in hipMalloc'ed memory.  min c'x  s.t. 0 <= x_j <= u_j (an LP with m = 6, n = 3); one workspace is updated and solved through
 * the device entry points, a second one through scs_update / scs_solve with the same values, and the results are compared with memcmp.
 * Then the refused calls: a warm start with a NULL vector and a host address where a device address belongs return -1 with a reason.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_device_io.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
 * Exit code 0 on success, 2 without a device; prints one line per check. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "scs_hip.h"

enum { M = 6, N = 3 };

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
static void to_host(scs_float *h, const scs_float *d, size_t count) {
  if (hipMemcpy(h, d, count * sizeof(scs_float), hipMemcpyDeviceToHost) != hipSuccess) { printf("hipMemcpy failed\n"); exit(3); }
}

int main(void) {
  if (scs_hip_device_count() < 1) {
    printf("no HIP device\n");
    return 2;
  }
  /* rows 0..2:  x_j + s = u_j  (x_j <= u_j);  rows 3..5:  -x_j + s = 0  (x_j >= 0) */
  scs_float Ax[2 * N] = {1.0, -1.0, 1.0, -1.0, 1.0, -1.0};
  scs_int Ai[2 * N] = {0, 3, 1, 4, 2, 5}, Ap[N + 1] = {0, 2, 4, 6};
  scs_float b[M] = {1.0, 2.0, 3.0, 0.0, 0.0, 0.0}, c[N] = {-1.0, 1.0, -2.0};
  scs_float b2[M] = {1.5, 2.5, 0.75, 0.0, 0.0, 0.0}, c2[N] = {-1.0, -0.5, 3.0};
  ScsMatrix A = {Ax, Ai, Ap, M, N};
  ScsData d = {M, N, &A, NULL, b, c};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  st.eps_abs = st.eps_rel = 1e-7;
  ScsCone k;
  memset(&k, 0, sizeof(k));
  k.l = M;
  ScsWork *wd = scs_init(&d, &k, &st), *wh = scs_init(&d, &k, &st);
  if (!wd || !wh) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }

  scs_float hx[N], hy[M], hs[M], gx[N], gy[M], gs[M];
  ScsSolution hsol = {hx, hy, hs};
  ScsInfo hi, di;
  scs_float *b_dev = to_device(b2, M), *c_dev = to_device(c2, N);
  scs_float *x_dev = to_device(NULL, N), *y_dev = to_device(NULL, M), *s_dev = to_device(NULL, M);

  /* cold: update(b, c) + solve on both paths */
  expect("scs_hip_update_device(b, c)", scs_hip_update_device(wd, b_dev, c_dev) == 0);
  expect("scs_update(b, c)", scs_update(wh, b2, c2) == 0);
  scs_int rd = scs_hip_solve_device(wd, x_dev, y_dev, s_dev, &di, 0), rh = scs_solve(wh, &hsol, &hi, 0);
  to_host(gx, x_dev, N); to_host(gy, y_dev, M); to_host(gs, s_dev, M);
  expect("cold solve: status", rd == SCS_SOLVED && rh == SCS_SOLVED && strcmp(di.status, hi.status) == 0);
  expect("cold solve: x, y, s identical", memcmp(gx, hx, sizeof hx) == 0 && memcmp(gy, hy, sizeof hy) == 0 && memcmp(gs, hs, sizeof hs) == 0);
  expect("cold solve: iter, pobj identical", di.iter == hi.iter && memcmp(&di.pobj, &hi.pobj, sizeof(scs_float)) == 0);
  printf("x* = %.6f %.6f %.6f after %d iterations\n", gx[0], gx[1], gx[2], (int)di.iter);
  expect("x* = (1.5, 2.5, 0)", gx[0] > 1.5 - 1e-4 && gx[0] < 1.5 + 1e-4 && gx[1] > 2.5 - 1e-4 && gx[1] < 2.5 + 1e-4 && gx[2] > -1e-4 && gx[2] < 1e-4);

  /* warm: update c only (b kept), warm start from the solution where it lies */
  scs_float *c0_dev = to_device(c, N);
  expect("scs_hip_update_device(NULL, c)", scs_hip_update_device(wd, NULL, c0_dev) == 0);
  expect("scs_update(NULL, c)", scs_update(wh, NULL, c) == 0);
  rd = scs_hip_solve_device(wd, x_dev, y_dev, s_dev, &di, 1);
  rh = scs_solve(wh, &hsol, &hi, 1);
  to_host(gx, x_dev, N); to_host(gy, y_dev, M); to_host(gs, s_dev, M);
  expect("warm solve: status", rd == SCS_SOLVED && rh == SCS_SOLVED);
  expect("warm solve: x, y, s identical", memcmp(gx, hx, sizeof hx) == 0 && memcmp(gy, hy, sizeof hy) == 0 && memcmp(gs, hs, sizeof hs) == 0);
  expect("warm solve: iter, pobj identical", di.iter == hi.iter && memcmp(&di.pobj, &hi.pobj, sizeof(scs_float)) == 0);

  /* a NULL output is skipped */
  to_host(gy, y_dev, M);
  rd = scs_hip_solve_device(wd, x_dev, NULL, s_dev, &di, 0);
  to_host(hy, y_dev, M);
  expect("NULL y_dev: solved, y_dev untouched", rd == SCS_SOLVED && memcmp(gy, hy, sizeof hy) == 0);

  /* refused, not dereferenced */
  memset(&di, 0, sizeof di);
  rd = scs_hip_solve_device(wd, x_dev, NULL, s_dev, &di, 1);
  printf("warm start with a NULL vector: %d (%s)\n", (int)rd, scs_hip_last_error());
  expect("warm start with a NULL vector returns -1 with a reason", rd == -1 && strlen(scs_hip_last_error()) > 0 && di.status[0] == 0);
  rd = scs_hip_update_device(wd, b2, NULL);
  printf("host address as b_dev: %d (%s)\n", (int)rd, scs_hip_last_error());
  expect("host address as b_dev returns -1 with a reason", rd == -1 && strlen(scs_hip_last_error()) > 0);
  rd = scs_hip_solve_device(wd, x_dev, y_dev, s_dev, &di, 0);
  expect("the workspace still solves", rd == SCS_SOLVED);

  scs_finish(wd);
  scs_finish(wh);
  (void)hipFree(b_dev); (void)hipFree(c_dev); (void)hipFree(c0_dev); (void)hipFree(x_dev); (void)hipFree(y_dev); (void)hipFree(s_dev);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
