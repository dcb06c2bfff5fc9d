/* Plain-C consumer of scs_hip_update_matrix / scs_hip_update_matrix_device (include/scs_hip.h): new values of A and P on the pattern
 * scs_init was given.  A QP with m = 6, n = 3:  min 1/2 x'Px + c'x  s.t. 0 <= x_j <= u_j (with coupling entries in A and P, so the
 * equilibration and the symmetric expansion of P have something to do).  One workspace is initialised, solved, updated to new values and
 * solved again; a second workspace is initialised on the new values; the two solutions are compared with memcmp.  The same once more
 * through the device entry, with P kept.  Then the refused calls: each returns -1 with a reason and leaves the workspace usable.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_update_matrix.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
 * Exit code 0 on success, 2 without a device; prints one line per check. */
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
typedef struct { scs_float x[N], y[M], s[M]; ScsInfo info; scs_int rc; } Result;
static void solve(ScsWork *w, Result *r) {
  ScsSolution sol = {r->x, r->y, r->s};
  r->rc = scs_solve(w, &sol, &r->info, 0);
}
static int same(const Result *a, const Result *b) {
  return a->rc == b->rc && a->info.iter == b->info.iter && memcmp(a->x, b->x, sizeof a->x) == 0 && memcmp(a->y, b->y, sizeof a->y) == 0 &&
         memcmp(a->s, b->s, sizeof a->s) == 0 && memcmp(&a->info.pobj, &b->info.pobj, sizeof(scs_float)) == 0;
}

int main(void) {
  if (scs_hip_device_count() < 1) {
    printf("no HIP device\n");
    return 2;
  }
  /* rows 0..2: x_j (+ coupling) + s = u_j; rows 3..5: -x_j + s = 0.  Column 0 also touches row 1, column 2 row 0. */
  scs_int Ai[ANNZ] = {0, 1, 3, 1, 4, 0, 2, 5}, Ap[N + 1] = {0, 3, 5, 8};
  scs_float Ax[ANNZ] = {1.0, 0.25, -1.0, 1.0, -1.0, -0.5, 1.0, -1.0};
  scs_float Ax2[ANNZ] = {1.5, 0.0, -1.0, 0.75, -2.0, 0.125, 3.0, -0.5}; /* (one entry exactly 0.0: it stays a stored value) */
  scs_float Ax3[ANNZ] = {0.5, 1.0, -3.0, 1.25, -1.0, -0.25, 2.0, -1.5};
  /* upper triangle of P: (0,0) (0,1) (1,1) (1,2) (2,2) */
  scs_int Pi[PNNZ] = {0, 0, 1, 1, 2}, Pp[N + 1] = {0, 1, 3, 5};
  scs_float Px[PNNZ] = {2.0, 0.5, 1.0, -0.25, 3.0};
  scs_float Px2[PNNZ] = {1.0, -0.125, 4.0, 0.5, 0.75};
  scs_float b[M] = {1.0, 2.0, 3.0, 0.0, 0.0, 0.0}, c[N] = {-1.0, 1.0, -2.0};
  ScsMatrix A = {Ax, Ai, Ap, M, N}, P = {Px, Pi, Pp, N, N};
  ScsMatrix A2 = {Ax2, Ai, Ap, M, N}, P2 = {Px2, Pi, Pp, N, N}, A3 = {Ax3, Ai, Ap, M, N};
  ScsData d = {M, N, &A, &P, b, c}, d2 = {M, N, &A2, &P2, b, c}, d3 = {M, N, &A3, &P2, b, c}, dlp = {M, N, &A, NULL, b, c};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  st.eps_abs = st.eps_rel = 1e-7;
  ScsCone k;
  memset(&k, 0, sizeof(k));
  k.l = M;
  ScsWork *w = scs_init(&d, &k, &st), *w2 = scs_init(&d2, &k, &st), *w3 = scs_init(&d3, &k, &st), *wlp = scs_init(&dlp, &k, &st);
  if (!w || !w2 || !w3 || !wlp) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }

  Result r0, r1, ref;
  solve(w, &r0);
  expect("first solve", r0.rc == SCS_SOLVED);
  expect("scs_hip_update_matrix(Ax2, Px2)", scs_hip_update_matrix(w, Ax2, Px2) == 0);
  solve(w, &r1);
  solve(w2, &ref);
  expect("host entry: solved", r1.rc == SCS_SOLVED && ref.rc == SCS_SOLVED);
  expect("host entry: x, y, s, iter, pobj identical to scs_init on the new values", same(&r1, &ref));
  expect("host entry: the solution moved", memcmp(r1.x, r0.x, sizeof r0.x) != 0);

  scs_float *a_dev = to_device(Ax3, ANNZ);
  expect("scs_hip_update_matrix_device(Ax3, NULL)", scs_hip_update_matrix_device(w, a_dev, NULL) == 0);
  solve(w, &r1);
  solve(w3, &ref);
  expect("device entry, P kept: x, y, s, iter, pobj identical to scs_init on the new values", same(&r1, &ref));
  expect("both NULL is a no-op", scs_hip_update_matrix(w, NULL, NULL) == 0);
  solve(w, &r0);
  expect("after the no-op: identical", same(&r0, &r1));

  /* refused before any device work */
  scs_int rc = scs_hip_update_matrix(NULL, Ax2, NULL);
  expect("NULL workspace returns -1 with a reason", rc == -1 && strlen(scs_hip_last_error()) > 0);
  rc = scs_hip_update_matrix(wlp, NULL, Px2);
  printf("Px without P: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("Px for a workspace without P returns -1 with a reason", rc == -1 && strlen(scs_hip_last_error()) > 0);
  rc = scs_hip_update_matrix_device(w, Ax2, NULL);
  printf("host address as Ax_dev: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("host address as Ax_dev returns -1 with a reason", rc == -1 && strlen(scs_hip_last_error()) > 0);
  ScsWork *cl = scs_hip_clone(w);
  rc = cl ? scs_hip_update_matrix(w, Ax2, NULL) : 0;
  printf("shared matrix set: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("a set shared with a live clone returns -1 and names the count", cl && rc == -1 && strstr(scs_hip_last_error(), "2 workspaces") != NULL);
  solve(w, &r0);
  expect("after the refusals: identical", same(&r0, &r1));
  scs_finish(cl);
  expect("with the clone gone the update goes through", scs_hip_update_matrix(w, Ax2, NULL) == 0);

  /* The same P with column 1 stored as (1,1), (0,1): scs_init takes unsorted row indices, but the k-th entry of such a column is not the
   * k-th lower entry of row 1 of the full matrix, so there is no value order to update in place.  Refused before any device work — for
   * Ax alone as well (with `normalize`, new values of A re-equilibrate P from its raw values) — and the workspace solves as before. */
  scs_int Piu[PNNZ] = {0, 1, 0, 1, 2};
  scs_float Pxu[PNNZ] = {2.0, 1.0, 0.5, -0.25, 3.0}, Pxu2[PNNZ] = {1.0, 4.0, -0.125, 0.5, 0.75};
  ScsMatrix Pu = {Pxu, Piu, Pp, N, N};
  ScsData du = {M, N, &A, &Pu, b, c};
  ScsWork *wu = scs_init(&du, &k, &st), *ws = scs_init(&d, &k, &st);
  if (!wu || !ws) { printf("scs_init (unsorted P) failed: %s\n", scs_hip_last_error()); return 3; }
  Result u0, u1, s0;
  solve(wu, &u0);
  solve(ws, &s0);
  expect("unsorted column of P: scs_init solves it like the sorted P", same(&u0, &s0));
  rc = scs_hip_update_matrix(wu, NULL, Pxu2);
  printf("unsorted column of P, Px: %d (%s)\n", (int)rc, scs_hip_last_error());
  expect("Px for a P with an unsorted column returns -1 and says why", rc == -1 && strstr(scs_hip_last_error(), "ascend") != NULL);
  rc = scs_hip_update_matrix(wu, Ax2, NULL);
  expect("Ax alone for that workspace returns -1 and says why", rc == -1 && strstr(scs_hip_last_error(), "ascend") != NULL);
  solve(wu, &u1);
  expect("after the refusals: identical", same(&u1, &u0));
  scs_finish(wu); scs_finish(ws);

  scs_finish(w); scs_finish(w2); scs_finish(w3); scs_finish(wlp);
  (void)hipFree(a_dev);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
