/* Plain-C consumer of the C-ABI built WITH -DUSE_SPECTRAL_CONES: ScsCone carries the spectral fields and the plain name
 * scs_init reaches the spectral-aware entry (include/scs_hip.h).  One ell1 cone of length 2 and one log-det cone of order 1,
 * min 1/2 |z - w|^2 s.t. z in K, whose solution is the projection of w (rows: the d cone first, then ell1):
 *   d:    w = (-1, 1, 1) -> (-1, 1, 1)      (inside: 1 log(1 / 1) = 0 >= -1)
 *   ell1: w = (0, 3, -1) -> (1.5, 1.5, 0)   (soft threshold 1.5)
 * Build: gcc -O2 -DUSE_SPECTRAL_CONES -I include tests/cabi/cabi_spectral.c -L scs-python_amd/scs -lscs_hip -Wl,-rpath,... -lm
 * Exit code 0 on success, 2 without a device. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "scs_hip.h"

#ifndef USE_SPECTRAL_CONES
#error "build with -DUSE_SPECTRAL_CONES"
#endif

int main(void) {
  if (scs_hip_device_count() < 1) {
    printf("no HIP device\n");
    return 2;
  }
  enum { L = 6 };
  scs_float w[L] = {-1., 1., 1., 0., 3., -1.};
  scs_float want[L] = {-1., 1., 1., 1.5, 1.5, 0.};
  scs_float Px[L], Ax[L], b[L], c[L];
  scs_int Pi[L], Pp[L + 1], Ai[L], Ap[L + 1];
  for (int i = 0; i < L; ++i) {
    Px[i] = 1.;
    Ax[i] = -1.;
    Pi[i] = Ai[i] = i;
    Pp[i] = Ap[i] = i;
    b[i] = 0.;
    c[i] = -w[i];
  }
  Pp[L] = Ap[L] = L;
  ScsMatrix A = {Ax, Ai, Ap, L, L}, P = {Px, Pi, Pp, L, L};
  ScsData d = {L, L, &A, &P, b, c};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  st.eps_abs = st.eps_rel = 1e-9;
  st.max_iters = 100000;
  ScsCone k;
  memset(&k, 0, sizeof(k));
  scs_int dd[1] = {1}, e1[1] = {2};
  k.d = dd;
  k.dsize = 1;
  k.ell1 = e1;
  k.ell1_size = 1;
  ScsWork *wk = scs_init(&d, &k, &st);
  if (!wk) {
    printf("scs_init failed: %s\n", scs_hip_last_error());
    return 3;
  }
  scs_float x[L], y[L], s[L];
  ScsSolution sol = {x, y, s};
  ScsInfo info;
  const scs_int rc = scs_solve(wk, &sol, &info, 0);
  int fails = rc != SCS_SOLVED;
  printf("status %s iter %d pobj %.9f\n", info.status, info.iter, info.pobj);
  for (int i = 0; i < L; ++i) {
    const int ok = fabs(x[i] - want[i]) <= 1e-5;
    printf("x[%d] = %.7f want %.7f -> %s\n", i, x[i], want[i], ok ? "ok" : "FAIL");
    fails += !ok;
  }
  fails += fabs(info.pobj - (-3.75)) > 1e-5;
  scs_finish(wk);
  printf(fails ? "FAILED\n" : "ALL OK\n");
  return fails ? 1 : 0;
}
