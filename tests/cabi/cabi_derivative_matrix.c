/* Plain-C consumer of scs_hip_derivative_full[_device], scs_hip_derivative_full_batch and scs_hip_data_perturbation[_device]
 * (include/scs_hip.h).  The QP of cabi_adjoint.c (m = 6, n = 3) is solved; its forward derivative with perturbations of the values of A
 * and P is taken through the host and the device entries and compared with memcmp; <g, derivative(db, dc, dA, dP)> is compared with
 * <adjoint(g), (db, dc, dA, dP)>; the products dP x + dA' y and dA x are compared with a host loop; a batch of two workspaces returns
 * the bits of the one-workspace calls.  Then the refused calls: each returns -1 with a reason and leaves the workspace usable.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_derivative_matrix.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
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
  scs_float b[M] = {1.0, 2.0, 3.0, 0.0, 0.0, 0.0}, c[N] = {-1.0, 1.0, -2.0}, b2[M] = {1.5, 2.0, 2.5, 0.0, 0.0, 0.0};
  ScsMatrix A = {Ax, Ai, Ap, M, N}, P = {Px, Pi, Pp, N, N};
  ScsData d = {M, N, &A, &P, b, c}, d2 = {M, N, &A, &P, b2, c}, dlp = {M, N, &A, NULL, b, c};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  st.eps_abs = st.eps_rel = 1e-9;
  ScsCone k;
  memset(&k, 0, sizeof(k));
  k.l = M;
  ScsWork *w = scs_init(&d, &k, &st), *w2 = scs_init(&d2, &k, &st), *wlp = scs_init(&dlp, &k, &st);
  if (!w || !w2 || !wlp) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }

  scs_float vb[M] = {0.5, -1.0, 0.25, 1.0, -0.75, 0.1}, vc[N] = {-0.3, 0.6, 1.2};
  scs_float vA[ANNZ] = {0.4, -0.2, 0.7, 1.1, -0.5, 0.3, -0.9, 0.6}, vP[PNNZ] = {0.8, -0.35, 0.45, 0.15, -0.6};
  scs_float dx[N], dy[M], ds[M];
  ScsHipDiffOpts opts = {1e-12, 0};
  ScsHipDiffInfo hi, di;

  /* before the first solve */
  scs_int rc = scs_hip_derivative_full(w, vb, vc, vA, vP, dx, dy, ds, &opts, &hi);
  printf("no solve yet: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("before the first solve: -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "no solve yet") != NULL);

  scs_float x[N], y[M], s[M], x2[N], y2[M], s2[M], xl[N], yl[M], sl[M];
  ScsSolution sol = {x, y, s}, sol2 = {x2, y2, s2}, soll = {xl, yl, sl};
  ScsInfo info;
  expect("solve", scs_solve(w, &sol, &info, 0) == SCS_SOLVED);
  expect("solve (second member)", scs_solve(w2, &sol2, &info, 0) == SCS_SOLVED);
  expect("solve (no P)", scs_solve(wlp, &soll, &info, 0) == SCS_SOLVED);

  /* the products on their own against a host loop at the returned solution */
  scs_float oc[N], ob[M], rc_[N] = {0, 0, 0}, rb[M] = {0, 0, 0, 0, 0, 0};
  for (int j = 0; j < N; ++j)
    for (int p = Ap[j]; p < Ap[j + 1]; ++p) {
      rc_[j] += vA[p] * y[Ai[p]];
      rb[Ai[p]] += vA[p] * x[j];
    }
  for (int j = 0; j < N; ++j)
    for (int p = Pp[j]; p < Pp[j + 1]; ++p) {
      rc_[Pi[p]] += vP[p] * x[j];
      if (Pi[p] != j) rc_[j] += vP[p] * x[Pi[p]];
    }
  rc = scs_hip_data_perturbation(w, vA, vP, oc, ob);
  scs_float worst = 0;
  for (int j = 0; j < N; ++j) worst = fmax(worst, fabs(oc[j] - rc_[j]));
  for (int i = 0; i < M; ++i) worst = fmax(worst, fabs(ob[i] - rb[i]));
  printf("products: rc %d, max difference to the host loop %.3e\n", (int)rc, worst);
  expect("scs_hip_data_perturbation", rc == 0 && worst <= 1e-14);
  scs_float *vA_d = to_device(vA, ANNZ), *vP_d = to_device(vP, PNNZ), *oc_d = to_device(NULL, N), *ob_d = to_device(NULL, M);
  rc = scs_hip_data_perturbation_device(w, vA_d, vP_d, oc_d, ob_d);
  expect("scs_hip_data_perturbation_device", rc == 0);
  expect("products: out_c identical", same_as_device(oc, oc_d, N));
  expect("products: out_b identical", same_as_device(ob, ob_d, M));

  /* the full derivative through both entries */
  rc = scs_hip_derivative_full(w, vb, vc, vA, vP, dx, dy, ds, &opts, &hi);
  printf("host derivative: rc %d iters %d stop %d residual %.3e\n", (int)rc, (int)hi.iters, (int)hi.stop, hi.residual);
  expect("scs_hip_derivative_full", rc == 0 && hi.iters >= 1 && (hi.stop == 1 || hi.stop == 2));
  scs_float *vb_d = to_device(vb, M), *vc_d = to_device(vc, N), *dx_d = to_device(NULL, N), *dy_d = to_device(NULL, M), *ds_d = to_device(NULL, M);
  rc = scs_hip_derivative_full_device(w, vb_d, vc_d, vA_d, vP_d, dx_d, dy_d, ds_d, &opts, &di);
  expect("scs_hip_derivative_full_device", rc == 0 && di.iters == hi.iters && di.stop == hi.stop);
  expect("derivative: dx identical", same_as_device(dx, dx_d, N));
  expect("derivative: dy identical", same_as_device(dy, dy_d, M));
  expect("derivative: ds identical", same_as_device(ds, ds_d, M));
  scs_float gx[N] = {1.0, -2.0, 0.5}, gy[M] = {0.3, -0.1, 0.2, 0.7, -0.4, 0.9}, gs[M] = {-0.6, 0.8, 0.1, -0.2, 0.5, 0.4};
  scs_float db[M], dc[N], dA[ANNZ], dP[PNNZ];
  expect("scs_hip_adjoint", scs_hip_adjoint(w, gx, gy, gs, db, dc, dA, dP, &opts, NULL) == 0);
  const scs_float lhs = dot(gx, dx, N) + dot(gy, dy, M) + dot(gs, ds, M);
  const scs_float rhs = dot(db, vb, M) + dot(dc, vc, N) + dot(dA, vA, ANNZ) + dot(dP, vP, PNNZ);
  printf("duality: %.15e vs %.15e\n", lhs, rhs);
  expect("<g, derivative(db, dc, dA, dP)> = <adjoint(g), (db, dc, dA, dP)>", fabs(lhs - rhs) <= 1e-8 * (fabs(lhs) + fabs(rhs) + 1.0));
  /* NULL dAx and dPx: the entry without them, bit for bit */
  scs_float px[N], py[M], ps[M], qx[N], qy[M], qs[M];
  expect("scs_hip_derivative", scs_hip_derivative(w, vb, vc, px, py, ps, &opts, NULL) == 0);
  expect("scs_hip_derivative_full with NULL dAx, dPx", scs_hip_derivative_full(w, vb, vc, NULL, NULL, qx, qy, qs, &opts, NULL) == 0);
  expect("NULL dAx and dPx: dx identical", memcmp(px, qx, sizeof(px)) == 0);
  expect("NULL dAx and dPx: dy identical", memcmp(py, qy, sizeof(py)) == 0 && memcmp(ps, qs, sizeof(ps)) == 0);
  expect("dAx alone is served without P", scs_hip_derivative_full(wlp, vb, vc, vA, NULL, qx, qy, qs, &opts, NULL) == 0);

  /* a batch of two: the bits of the one-workspace calls */
  scs_float ex[N], ey[M], es[M], fx[N], fy[M], fs[M], sx[N], sy[M], ss[M];
  ScsWork *ws[2] = {w, w2};
  const scs_float *bb[2] = {vb, vb}, *bc[2] = {vc, vc}, *bA[2] = {vA, vA}, *bP[2] = {vP, vP};
  scs_float *bx[2] = {ex, fx}, *by[2] = {ey, fy}, *bs[2] = {es, fs};
  ScsHipDiffInfo i0, i1, *infos[2] = {&i0, &i1};
  rc = scs_hip_derivative_full_batch(ws, bb, bc, bA, bP, bx, by, bs, &opts, infos, 2);
  printf("batch: rc %d (%s) iters %d %d\n", (int)rc, scs_hip_last_error(), (int)i0.iters, (int)i1.iters);
  expect("scs_hip_derivative_full_batch", rc == 0);
  expect("batch member 0: identical to its own call", memcmp(ex, dx, sizeof(dx)) == 0 && memcmp(ey, dy, sizeof(dy)) == 0 && memcmp(es, ds, sizeof(ds)) == 0 &&
                                                       i0.iters == hi.iters);
  rc = scs_hip_derivative_full(w2, vb, vc, vA, vP, sx, sy, ss, &opts, &di);
  expect("batch member 1: identical to its own call", rc == 0 && memcmp(fx, sx, sizeof(sx)) == 0 && memcmp(fy, sy, sizeof(sy)) == 0 &&
                                                       memcmp(fs, ss, sizeof(ss)) == 0 && i1.iters == di.iters);

  /* refused before any device work */
  rc = scs_hip_derivative_full(NULL, vb, vc, vA, vP, dx, dy, ds, &opts, &hi);
  expect("NULL workspace returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "null workspace") != NULL);
  rc = scs_hip_derivative_full(wlp, vb, vc, vA, vP, qx, qy, qs, &opts, &hi);
  printf("dPx without P: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("dPx for a workspace without P returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "without P") != NULL);
  rc = scs_hip_data_perturbation(wlp, NULL, vP, oc, ob);
  expect("... and so does the product entry", rc == -1 && strstr(scs_hip_last_error(), "without P") != NULL);
  rc = scs_hip_derivative_full_device(w, vb_d, vc_d, vA, vP_d, dx_d, dy_d, ds_d, &opts, &di);
  printf("host address as dAx_dev: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("host address as dAx_dev returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "dAx_dev") != NULL);
  ScsWork *wl[2] = {w, wlp};
  rc = scs_hip_derivative_full_batch(wl, bb, bc, bA, bP, bx, by, bs, &opts, infos, 2);
  printf("batch with a member without P: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("a batch names the member it refuses", rc == -1 && strstr(scs_hip_last_error(), "member 1") != NULL && strstr(scs_hip_last_error(), "without P") != NULL);
  expect("scs_update", scs_update(w, b, NULL) == 0);
  rc = scs_hip_derivative_full(w, vb, vc, vA, vP, dx, dy, ds, &opts, &hi);
  printf("after scs_update: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("a stale solution returns -1 with a reason", rc == -1 && strstr(scs_hip_last_error(), "stale") != NULL);
  expect("after the refusals the workspace solves", scs_solve(w, &sol, &info, 0) == SCS_SOLVED);
  rc = scs_hip_derivative_full(w, vb, vc, vA, vP, qx, qy, qs, &opts, &hi);
  scs_float diff = 0;
  for (int i = 0; i < N; ++i) diff = fmax(diff, fabs(qx[i] - ex[i]));
  printf("derivative after the new solve: max difference %.3e\n", diff);
  expect("... and differentiates again", rc == 0 && diff <= 1e-6);

  scs_finish(w); scs_finish(w2); scs_finish(wlp);
  (void)hipFree(vA_d); (void)hipFree(vP_d); (void)hipFree(oc_d); (void)hipFree(ob_d);
  (void)hipFree(vb_d); (void)hipFree(vc_d); (void)hipFree(dx_d); (void)hipFree(dy_d); (void)hipFree(ds_d);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
