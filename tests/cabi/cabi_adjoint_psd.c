/* Plain-C consumer of scs_hip_adjoint / scs_hip_derivative (include/scs_hip.h) on a small SDP: the LP-SDP of tests/adjoint_psd_ref.py
 * (problem_lp_sdp: n = 9, one zero row, four nonnegative rows, one PSD block of order 4 whose solution has rank 2; the numbers below
 * are that generator's output, A dense in CSC).  The problem is solved, <g, derivative(d)> is compared with <adjoint(g), d>, the host
 * and the device entry of the adjoint are compared with memcmp, and a second adjoint call must return the bits of the first.
 * Build: gcc -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tests/cabi/cabi_adjoint_psd.c -L scs-python_amd/scs -lscs_hip -L $ROCM/lib -lamdhip64 ...
 * Exit code 0 on success, 2 without a device; prints one line per check. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "scs_hip.h"

enum { M = 15, N = 9, ANNZ = 135 };

static const scs_float Ax0[135] = {
    -0.34084158471333037, 0.37393183055240997, -0.38554234892881772, 0.4156285083012885, -0.15671324000592299, 0.072442653367052537,
    -0.032816830005529464, 0.010910738797006552, 0.040592846578529386, -0.15467800570321874, -0.3154261392440923, 0.47275779999396544,
    0.08624355853056441, 0.40199043740542689, -0.26625738639801688, -0.05011421330058765, -0.39898374405023235, 0.19367310916633443,
    0.27868192946853104, -0.096235164778429749, 0.19476322432824966, -0.25673131598014043, 0.44550631783278455, -0.22440028835543091,
    -0.20522332717960776, 0.1778770680394143, 0.35865017783078335, 0.15954844496768025, -0.012634131563618665, -0.31919009909533441,
    0.013014170517563838, 0.32720860922521472, -0.525619715771801, -0.2718954740131258, -0.29660220732696757, -0.30230356132053671,
    0.13434205804806598, -0.030107531313977795, -0.19500936341059219, 0.28256338208460846, 0.10236658812806566, -0.35581750971707088,
    -0.19671118956350589, -0.37219706578071743, 0.12441599019238518, -0.31171666243674895, -0.16037480532720519, 0.45136440661949773,
    -0.36878298815944216, -0.50726211743429084, -0.43256747297054504, -0.47339192569548888, -0.080854259090462358, 0.20420088039890327,
    -0.024270501772489548, -0.2833447142434023, 0.18560206068430354, -0.036283401637201486, -0.15816374136591035, -0.23149354741059092,
    0.30546223039150611, -0.35874699565030316, -0.14996850936866152, 0.24308828485397541, -0.3874927122588554, -0.5121969784768311,
    -0.014254978264486644, -0.15859360526411745, 0.50126466555899085, 0.2014153719332146, 0.1552206025074461, 0.36716845319371733,
    -0.014249057870874925, 0.17285628946041207, 0.0412425478454174, 0.47736185540790416, -0.53605741130737783, 0.18476546033007135,
    0.12877149772333951, -0.16118580834198618, -0.42827227490905512, 0.0073421540550606722, -0.16858415985468703, -0.001720950463860313,
    -0.20088482767292029, -0.089550941755899172, 0.0035099781796448103, 0.13055345159031662, -0.2720534094123232, 0.0010706391633978033,
    -0.54881602634715398, 0.25425319338874885, -0.032704951601626862, 0.058779660329934945, -0.11031454031802725, 0.35192013817906881,
    -0.31091840855543601, -0.08037910322350364, -0.47755927574766904, -0.32067215888320405, -0.33278776447984909, 0.10134138908772027,
    0.38606267468502953, -0.77996162847576855, -0.47616861446181896, -0.091997542964004683, -0.61923080299398248, -0.17963208625302082,
    -0.014797981133410727, -0.013671883155657094, 0.36542729748261626, -0.17625603199318862, -0.061411909399204719, -0.19822833072433135,
    -0.39292237482849041, 0.091323386384926195, 0.23150738566725257, 0.19710581907350064, -0.054709784806483093, -0.35885669785690238,
    -0.10544466766521893, 0.26302292661719701, 0.06993520205926658, -0.47596608953787684, -0.40154720603815819, 0.077060575257600974,
    -0.0069400300266221808, 0.26084122736716492, 0.16262826819904708, -0.59962262718890136, -0.23124545142944755, 0.10727282708374164,
    -0.34644453349860521, -0.42466514015721274, -0.17987033791031662};
static const scs_int Ai0[135] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 0, 1, 2, 3, 4, 5, 6, 7, 8,
    9, 10, 11, 12, 13, 14, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 0, 1, 2,
    3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
    12, 13, 14, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 0, 1, 2, 3, 4, 5,
    6, 7, 8, 9, 10, 11, 12, 13, 14, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14,
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14};
static const scs_int Ap0[10] = {
    0, 15, 30, 45, 60, 75, 90, 105, 120, 135};
static const scs_float b0[15] = {
    -1.0899630396438611, 0.58857867342933123, -1.3647663262512264, 0.65708544286999471, 0.63074384199083944, 1.63406587533604,
    -0.92085616136233628, -0.3444105861468918, -0.22105469038921383, -0.37231085754083115, -0.59814048556190369, 0.7798812453332632,
    0.23211225220789533, -0.32810978117967549, 0.16352231839676479};
static const scs_float c0[9] = {
    -0.39594437834429891, 0.44286661800395632, 0.049879077898552608, -0.44191172304720405, 0.91190080517121719, 1.2160594418819617,
    -0.96355553301218155, 1.197725031912318, 0.27322356743266213};
static const scs_float gx0[9] = {
    0.4277699642047284, -0.57083755688644555, 2.6544606897300973, -1.6085449528642095, 0.66171566166416906, -0.14342594397899663,
    -0.3545063884714269, 1.0663588121198411, -1.8179220006075487};
static const scs_float gy0[15] = {
    -0.98467621008865325, -0.11416014445729655, 1.7412738366841587, 0.089046871153780835, 0.89568823700888844, -1.8633059650275363,
    -1.2388875452076324, 0.96952947342423035, -0.62817974004336674, -0.062995460248876714, 0.73086910462290366, -2.205017534697761,
    -1.2011655652359481, -0.09384084596981232, -1.5464760689954131};
static const scs_float gs0[15] = {
    -0.71059622021114821, -0.042414763677518424, -0.66512079689092563, -0.26877931950658895, 0.041064483696860034, 1.3301960591048283,
    1.5786530571202153, -0.39456915897688244, -0.8277516376614229, 0.889344350731057, 0.51055591493121621, 0.24907593742772269,
    -0.90823933158814896, 0.64495070665628162, 0.87220685320245739};
static const scs_float vb0[15] = {
    -1.7847916074881127, 1.0174393331492972, -0.072799742075061485, -0.74349520044824646, -1.5770707519558578, -0.34177930546447538,
    -0.06114594768040537, -0.37479113598302272, -1.2043813104854644, -1.1953372761986167, 0.7054006714715072, 0.047717759119236355,
    0.28460898445219074, 0.62907040427132888, 0.71762038559114949};
static const scs_float vc0[9] = {
    1.7351288255855741, -0.071322935232539283, -0.25945433004389518, -0.95824532333057499, 0.24943479118110851, 0.26447118013773641,
    -0.75974855469828284, -0.032522944875870423, -0.018055083353823248};
static const scs_float x_built[9] = {
    1.1865118634329741, -0.75103566382779041, 0.66835778829471038, 0.10338436876855045, 0.83965782282220425, -0.62675154603448413,
    0.93673121667667825, 1.161921542001894, 0.34111680827674901};

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
  scs_float tmp[ANNZ];
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
  scs_float Ax[ANNZ], b[M], c[N], gx[N], gy[M], gs[M], vb[M], vc[N];
  scs_int Ai[ANNZ], Ap[N + 1];
  memcpy(Ax, Ax0, sizeof(Ax)); memcpy(Ai, Ai0, sizeof(Ai)); memcpy(Ap, Ap0, sizeof(Ap));
  memcpy(b, b0, sizeof(b)); memcpy(c, c0, sizeof(c));
  memcpy(gx, gx0, sizeof(gx)); memcpy(gy, gy0, sizeof(gy)); memcpy(gs, gs0, sizeof(gs));
  memcpy(vb, vb0, sizeof(vb)); memcpy(vc, vc0, sizeof(vc));
  ScsMatrix A = {Ax, Ai, Ap, M, N};
  ScsData d = {M, N, &A, NULL, b, c};
  ScsSettings st;
  scs_set_default_settings(&st);
  st.verbose = 0;
  st.eps_abs = st.eps_rel = 1e-9;
  scs_int sdim[1] = {4};
  ScsCone k;
  memset(&k, 0, sizeof(k));
  k.z = 1;
  k.l = 4;
  k.s = sdim;
  k.ssize = 1;
  ScsWork *w = scs_init(&d, &k, &st);
  if (!w) { printf("scs_init failed: %s\n", scs_hip_last_error()); return 3; }

  scs_float x[N], y[M], s[M];
  ScsSolution sol = {x, y, s};
  ScsInfo info;
  expect("solve", scs_solve(w, &sol, &info, 0) == SCS_SOLVED);
  scs_float far = 0;
  for (int i = 0; i < N; ++i) far = fmax(far, fabs(x[i] - x_built[i]));
  printf("distance from the generator's x: %.3e\n", far);
  expect("the solution is the generator's", far <= 1e-5);

  scs_float db[M], dc[N], dA[ANNZ], db2[M], dc2[N], dx[N], dy[M], ds[M];
  ScsHipDiffOpts opts = {1e-12, 0};
  ScsHipDiffInfo hi, di;
  scs_int rc = scs_hip_adjoint(w, gx, gy, gs, db, dc, dA, NULL, &opts, &hi);
  printf("host adjoint: rc %d (%s) iters %d stop %d residual %.3e normal %.3e\n", (int)rc, scs_hip_last_error(), (int)hi.iters, (int)hi.stop,
         hi.residual, hi.normal_residual);
  expect("scs_hip_adjoint on an SDP", rc == 0 && hi.iters >= 1 && (hi.stop == 1 || hi.stop == 2));
  rc = scs_hip_adjoint(w, gx, gy, gs, db2, dc2, NULL, NULL, &opts, &di);
  expect("a second call returns the same bits", rc == 0 && di.iters == hi.iters && memcmp(db, db2, sizeof(db)) == 0 && memcmp(dc, dc2, sizeof(dc)) == 0);
  scs_float *gx_d = to_device(gx, N), *gy_d = to_device(gy, M), *gs_d = to_device(gs, M);
  scs_float *db_d = to_device(NULL, M), *dc_d = to_device(NULL, N), *dA_d = to_device(NULL, ANNZ);
  rc = scs_hip_adjoint_device(w, gx_d, gy_d, gs_d, db_d, dc_d, dA_d, NULL, &opts, &di);
  expect("scs_hip_adjoint_device", rc == 0 && di.iters == hi.iters && di.stop == hi.stop);
  expect("adjoint: db identical", same_as_device(db, db_d, M));
  expect("adjoint: dc identical", same_as_device(dc, dc_d, N));
  expect("adjoint: dA identical", same_as_device(dA, dA_d, ANNZ));

  rc = scs_hip_derivative(w, vb, vc, dx, dy, ds, &opts, &hi);
  printf("host derivative: rc %d iters %d stop %d residual %.3e\n", (int)rc, (int)hi.iters, (int)hi.stop, hi.residual);
  expect("scs_hip_derivative on an SDP", rc == 0 && (hi.stop == 1 || hi.stop == 2));
  const scs_float lhs = dot(gx, dx, N) + dot(gy, dy, M) + dot(gs, ds, M), rhs = dot(db, vb, M) + dot(dc, vc, N);
  printf("duality: %.15e vs %.15e\n", lhs, rhs);
  expect("<g, derivative(d)> = <adjoint(g), d>", fabs(lhs - rhs) <= 1e-8 * (fabs(lhs) + fabs(rhs) + 1.0));
  expect("after the calls the workspace solves", scs_solve(w, &sol, &info, 1) == SCS_SOLVED);

  scs_finish(w);
  (void)hipFree(gx_d); (void)hipFree(gy_d); (void)hipFree(gs_d); (void)hipFree(db_d); (void)hipFree(dc_d); (void)hipFree(dA_d);
  printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
