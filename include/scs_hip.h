/*
 * scs_hip.h — C-ABI of libscs_hip.so, the MI355X-native (gfx950) implementation
 * of SCS's ADMM hot path.  Plain pointers and sizes only; no torch types.
 *
 * PART 1 is exactly the core API the reference's CPython glue binds
 * (SURVEY.md §8 row b6); a maintainer can re-compile R:scs/scsobject.h against
 * this header + scs_types.h to obtain `scs._scs_hip`.
 * PART 2 are kernel-level entry points used by the parity tests and bench.py
 * (they have no counterpart in the reference's public API; each cites the
 * absent upstream file whose role it plays).
 */
#ifndef SCS_HIP_H_GUARD
#define SCS_HIP_H_GUARD

#include "scs_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The library is compiled with hidden default visibility: what this header declares is all it exports. */
#define SCS_HIP_API __attribute__((visibility("default")))

typedef struct ScsHipWork ScsWork;

/* ------------------------------------------------------------------ PART 1 */

/* replaces scs_init — called at R:scs/scsobject.h:903.  Copies all of d,k,stgs
 * (the glue frees its views right after, :908).  Builds CSR(A) next to the
 * caller's CSC(A), equilibrates, uploads everything to HBM, pre-solves g.
 * Returns NULL on invalid data / allocation failure / no usable GPU. */
SCS_HIP_API ScsWork *scs_init(const ScsData *d, const ScsCone *k, const ScsSettings *stgs);

/* replaces scs_solve — called at R:scs/scsobject.h:986 with the GIL released.
 * Runs the whole ADMM loop device-resident; only info scalars and the final
 * x,y,s cross PCIe.  sol holds the warm start on entry when warm_start != 0. */
SCS_HIP_API scs_int scs_solve(ScsWork *w, ScsSolution *sol, ScsInfo *info, scs_int warm_start);

/* replaces scs_update — called at R:scs/scsobject.h:1217.  b and/or c may be NULL. */
SCS_HIP_API scs_int scs_update(ScsWork *w, scs_float *b, scs_float *c);

/* replaces scs_finish — called at R:scs/scsobject.h:1240. */
SCS_HIP_API void scs_finish(ScsWork *w);

/* replaces scs_set_default_settings — called at R:scs/scsobject.h:520. */
SCS_HIP_API void scs_set_default_settings(ScsSettings *stgs);

/* replaces scs_version — called at R:scs/scsmodule.h:5. */
SCS_HIP_API const char *scs_version(void);

/* sizeof(scs_int), sizeof(scs_float): what R:scs/scsmodule.h:16-23 report. */
SCS_HIP_API size_t scs_sizeof_int(void);
SCS_HIP_API size_t scs_sizeof_float(void);

/* ------------------------------------------------------------------ PART 2 */

/* number of visible HIP devices (0 => library unusable); does not initialise a context */
SCS_HIP_API int scs_hip_device_count(void);
/* choose the device used by subsequent scs_init calls (and the kernel-level entry points below): the process-wide
 * default (0 at start), or — set_thread_device, dev < 0 clears it — a default of the calling thread only.  A workspace
 * remembers the device it was created on: scs_solve / scs_update / scs_finish select it themselves, so one process
 * may drive several GPUs. */
SCS_HIP_API int scs_hip_set_device(int dev);
SCS_HIP_API int scs_hip_set_thread_device(int dev);
/* 1 when this library is the -DSCS_HIP_LABS build (scs-python_amd/Makefile `make labs`: the experiments that lost their measurement and
 * the lab switches of the kernels compiled in and readable from the environment — csrc/options.hpp), 0 for the product. */
SCS_HIP_API int scs_hip_labs_build(void);
/* free and total HBM bytes of the device subsequent scs_init calls would use, plus the bytes this library's block pool holds for
 * reuse (they count as free for a new workspace).  What the Python layer's `LinearSolver.AUTO` asks before it picks the dense direct
 * solver (R:scs/py/__init__.py:45-54 resolves AUTO to the best DIRECT backend that is usable).  0 on success, -1 without a device. */
SCS_HIP_API int scs_hip_mem_info(size_t *free_bytes, size_t *total_bytes);

/* y (+)= A x or A' x through the hot-path SpMV kernels (row a3; plays the role
 * of scs_source/linsys/scs_matrix.c accum_by_a / accum_by_atrans, R:meson.build:199-202).
 * A is CSC with int32 indices; x,y are host pointers.  Returns 0 on success. */
SCS_HIP_API int scs_hip_spmv(const ScsMatrix *A, const scs_float *x, scs_float *y, int transpose);

/* HOST-ONLY check of the column-sorted pass layout the large-matrix SpMV kernels read (spmv_cs.hpp): builds the
 * layout of A (transpose=0) or A' (transpose=1) with the host builder (rows per lane `rpt` = 1, 2, 4, 8, 16, or 0 =
 * the geometry scs_init would pick; `split` = 1, or 2 workgroups per row chunk as scs_init uses for A') and
 * evaluates y += M x by walking it exactly as the kernel does (slot scatter, per-lane runs, pass order, partial sums).
 * No GPU needed.  Returns 0, 1 if the pattern does not fit the format, -1 on error. */
SCS_HIP_API int scs_hip_cs_layout_host_spmv(const ScsMatrix *A, const scs_float *x, scs_float *y, int transpose, int rpt, int split);
/* Same walk for the virtual-row variant of that layout (round 3): rows longer than max(piece_len, what a count field
 * holds) are cut into pieces of at most piece_len nonzeros that ride in the passes; the pieces of a row are then added
 * the way the device does it (64 lanes striding over them, shuffle tree).  Returns 1 when no row is that long. */
SCS_HIP_API int scs_hip_cs_layout_host_spmv_pieces(const ScsMatrix *A, const scs_float *x, scs_float *y, int transpose, int piece_len);

/* Time `reps` launches of the A (transpose=0) or A' (transpose=1) SpMV kernel
 * with HIP events on the launch stream; inputs already resident in HBM.
 * Returns average milliseconds per launch, <0 on error.  (bench.py roofline leg) */
SCS_HIP_API double scs_hip_spmv_bench(const ScsMatrix *A, int transpose, int reps);

/* In-place projection of x (length m, host pointer) onto K (dual=0) or K*
 * (dual=1) with the hot-path cone kernels (row a5; scs_source/src/cones.c,
 * exp_cone.c, R:meson.build:188,190). */
SCS_HIP_API int scs_hip_proj_cone(scs_float *x, const ScsCone *k, scs_int m, int dual);

/* The derivative of that projection (csrc/dproj.hpp) at v, applied to u: out_Wu = W u and out_WmIu = (W - I) u with W = D Pi_K(v)
 * (v, u, the outputs: `len` doubles, host pointers; an output may be NULL).  Zero, nonnegative, box, second-order, real PSD (s) and power (p)
 * cones; the others are refused by name.  (parity tests) */
SCS_HIP_API int scs_hip_dproj_cone(const scs_float *v, const scs_float *u, const ScsCone *cone, scs_int len, scs_float *out_Wu, scs_float *out_WmIu);

/* The pack and sum kernels of scs_hip_adjoint_shared (below; csrc/grad_shared.hpp) on host stacks and nothing else: with X, DC (K x n) and
 * Y, DB (K x m) row-major,
 *     out_dA[p] = sum_k ( Y[k,i] DC[k,j] - DB[k,i] X[k,j] )     p = stored entry (i, j) of the m x n CSC pattern (Ap, Ai)
 *     out_dP[q] = sum_k ( DC[k,c] X[k,r] + DC[k,r] X[k,c] ), c < r;  sum_k DC[k,r] X[k,r] on the diagonal     q = entry (c, r) of the
 * CSC pattern (Pp, Pi) of an upper triangle of order n (Pp may be NULL: no P; an output may be NULL; an entry below the diagonal gets 0).
 * An output without an entry launches nothing.  Two calls give the same bits.  0, or -1 with the reason in scs_hip_last_error (a pattern
 * that is no pattern, K < 1).  (parity tests) */
SCS_HIP_API int scs_hip_grad_matrix_sum(scs_int m, scs_int n, const scs_int *Ap, const scs_int *Ai, const scs_int *Pp, const scs_int *Pi, scs_int K,
                                        const scs_float *X, const scs_float *Y, const scs_float *DB, const scs_float *DC, scs_float *out_dA,
                                        scs_float *out_dP);

/* The same projection applied to `count` vectors one after the other (xs: count x m, row-major, in place) through ONE set of cone
 * workspaces, warm-started from call to call as inside the ADMM loop (K9: eigenvectors of the previous call, periodic
 * re-orthogonalisation, refinement stage; box cone: the previous t).  stats (may be NULL): scs_hip_psd_refine_stats records of the
 * first stats_cap large PSD matrices after the last call.  Returns the number of records written, -1 on error.  (parity tests) */
SCS_HIP_API int scs_hip_proj_cone_seq(scs_float *xs, const ScsCone *k, scs_int m, int dual, int count, scs_float *stats, int stats_cap);

/* One indirect KKT solve [[R_x+P, A'],[A,-R_y]] z = rhs (in place, length n+m)
 * with the device PCG (row a4; scs_source/linsys/cpu/indirect/private.c,
 * R:meson.build:261).  cg_iters may be NULL. */
SCS_HIP_API int scs_hip_kkt_solve(const ScsMatrix *A, const ScsMatrix *P, const scs_float *diag_r, scs_float *rhs,
                      scs_float tol, scs_int *cg_iters);

/* Same system solved with the DENSE DIRECT linsys (csrc/dense.hpp): G = R_x + P + A' R_y^{-1} A is formed and inverted on
 * the device (blocked Gauss-Jordan on the fp64 MFMA), x = G^{-1}(rhs_x + A' R_y^{-1} rhs_y), y = R_y^{-1}(A x - rhs_y).  n <= 8192.
 * Plays the role of the reference's direct backends (QDLDL / cuDSS / the LAPACK dense module: R:meson.build:241-262,374-391). */
SCS_HIP_API int scs_hip_kkt_solve_dense(const ScsMatrix *A, const ScsMatrix *P, const scs_float *diag_r, scs_float *rhs);

/* scs_init with an explicit choice of the linear-system solver: 1 = sparse indirect (PCG; what scs_init builds unless the
 * environment says SCS_HIP_LINSYS=dense), 2 = dense direct (n <= 8192: the explicit inverse of the reduced KKT matrix lives in
 * HBM, the linear solve of an ADMM iteration is three dependent launches and never waits for the host), 0 = the default.
 * The reference selects its linear solver by MODULE (R:scs/py/__init__.py:40-66: _scs_direct, _scs_indirect, _scs_gpu, ...);
 * scs._scs_hip binds 1, scs._scs_hip_dense binds 2.  Everything else is scs_init's contract. */
SCS_HIP_API ScsWork *scs_hip_init_linsys(const ScsData *d, const ScsCone *k, const ScsSettings *stgs, int linsys);
/* 1 / 2 as above for a live workspace (0: NULL) */
SCS_HIP_API int scs_hip_linsys_kind(const ScsWork *w);

/* Equilibrate (A,P,b,c) exactly as scs_init does (row a7; scs_source/src/normalize.c,
 * R:meson.build:192).  A->x, P->x, b, c are overwritten; D (m), E (n), sigma (1) filled. */
SCS_HIP_API int scs_hip_normalize(ScsMatrix *A, ScsMatrix *P, scs_float *b, scs_float *c, const ScsCone *k,
                      scs_float *D, scs_float *E, scs_float *sigma);

/* Measured device-copy bandwidth ceiling in GB/s (float4 copy of `bytes` bytes). */
SCS_HIP_API double scs_hip_copy_bandwidth(size_t bytes, int reps);

/* Live timing of the two dominant kernels inside scs_solve: when enabled, one CG step per
 * host sync is bracketed by HIP events on the solver's own stream.  out[12] =
 * {K1 total ms, K1 samples, K2 total ms, K2 samples, nnz(A), K1 workgroups, K2 workgroups, nnz(P full),
 *  nonlinear cone projections total ms, samples (one per queued iteration), K3 total ms, K3 samples}
 * where K1 = z <- R_y^{-1} A p,  K2 = Gp <- A' z + R_x p (+ P p)  and, for problems with P, K3 = P p (between K1 and K2). */
SCS_HIP_API void scs_hip_set_profiling(ScsWork *w, int on);
SCS_HIP_API void scs_hip_kernel_times(const ScsWork *w, double *out);
/* The final (x, y, s) of the last scs_solve, copied from the workspace's HBM buffers to caller-provided DEVICE pointers
 * (any may be NULL; n, m, m doubles) on the workspace's stream, complete on return.  Same values, bit for bit, as the
 * host copies scs_solve returned (NaN where the status leaves a vector undefined).  scs/batch.py gathers from these. */
SCS_HIP_API int scs_hip_solution_to_device(ScsWork *w, scs_float *x_dev, scs_float *y_dev, scs_float *s_dev);

/* Device-resident endpoints: scs_update / scs_solve / scs_hip_solve_batch for callers whose b, c, warm start and solution live in
 * HBM (a sweep over one matrix inside a device program).  Every *_dev pointer is a DEVICE address on the workspace's device
 * (scs_hip_work_device); anything else is refused with -1 before device work starts.  No vector of n or m doubles crosses the host:
 * an update reads back three doubles (max |b|, max |c|, sigma), a solve the flags and residual partials scs_solve reads.
 *
 * STREAM CONTRACT.  The library works on its own non-blocking stream.  The CALLER guarantees that the inputs (b_dev, c_dev and, with
 * warm_start, x_dev / y_dev / s_dev) are complete before the call — synchronise the stream that produced them.  The LIBRARY drains
 * its stream before it returns, as scs_solve does, so the outputs may be read from any stream afterwards.
 *
 *   update_device: b_dev (m) / c_dev (n), NULL = keep the current vector.  Same arithmetic as scs_update: a following solve gives the
 *                  same bits.  Host and device updates may be mixed; scs_hip_clone still starts from what scs_init was given.
 *   solve_device:  x_dev (n), y_dev (m), s_dev (m) hold the warm start on entry when warm_start != 0 (all three are required
 *                  then) and the solution on return; a NULL pointer skips that output.  info, the status, NaN for a vector the status
 *                  leaves undefined, Ctrl-C, log_csv and verbose are scs_solve's; the return value is the status, -1 for refused
 *                  arguments (scs_hip_last_error).
 *   solve_batch_device: the grouped solve over arrays of such pointers (any of the three arrays may be NULL without warm_start).  Its
 *                  groups are those of scs_hip_solve_batch: scs_hip_batch_plan is the plan. */
SCS_HIP_API scs_int scs_hip_update_device(ScsWork *w, const scs_float *b_dev, const scs_float *c_dev);
SCS_HIP_API scs_int scs_hip_solve_device(ScsWork *w, scs_float *x_dev, scs_float *y_dev, scs_float *s_dev, ScsInfo *info, scs_int warm_start);
SCS_HIP_API scs_int scs_hip_solve_batch_device(ScsWork **w, scs_float **x_dev, scs_float **y_dev, scs_float **s_dev, ScsInfo **info,
                                               scs_int count, scs_int warm_start);
/* Matrix values: new VALUES of A and / or P on the sparsity pattern scs_init was given (a re-linearised model, a time-varying cost),
 * written into every resident layout instead of a new scs_init.  Ax holds nnz(A) and Px nnz(P) doubles in the order of the CSC arrays
 * scs_init got (P: the upper triangle as passed; explicit zeros are values); NULL keeps that matrix, both NULL is a no-op returning 0.
 * scs_hip_update_matrix takes HOST pointers, scs_hip_update_matrix_device DEVICE pointers of the workspace's device (the stream contract
 * of the device endpoints above: inputs complete on entry, the library drains its stream before it returns); the host entry stages its
 * values into a device buffer and runs the same path.
 *
 * CONTRACT.  Afterwards the workspace is in the state scs_init would leave a NEW workspace in, given the new values on the old pattern,
 * the workspace's CURRENT b and c (after any scs_update / scs_hip_update_device), and the same cone, settings, linear solver and
 * environment: cold iterate, empty Anderson history, scale = settings.scale, fresh D, E, sigma, box bounds rescaled from the caller's,
 * diag(P), R and the preconditioner or G^-1, g (deferred where scs_init defers them).  A following solve returns the x, y, s, iteration
 * and CG-step counts of that new workspace bit for bit.  A warm start is what the caller passes to the solve.  What a LATER
 * scs_hip_clone starts from (the b, c scs_init was given) is unchanged; the clone shares the updated matrices.
 *
 * Returns 0, or -1 with the reason in scs_hip_last_error.  Refused before any device work, the workspace unchanged and usable: a NULL
 * workspace; Px for a workspace created without P; (device entry) a pointer that is not device memory of the workspace's device;
 * a matrix set other workspaces share (live clones — it is read-only for them; the message names the count); a workspace whose P
 * scs_init got with entries below the diagonal or with row indices that do not ascend inside a column (scs_init accepts both; the
 * value order of the triangle cannot be mapped onto the full matrix then).
 * One refusal comes AFTER device work, at the first call only: a value map that does not reproduce, bit for bit, the values a resident
 * layout holds (the map kernels, scans and a check pass have run by then; no matrix value has been written, the maps are released,
 * the workspace is unchanged and usable).  It guards layouts whose placement the map builder cannot re-derive.
 *
 * The first call builds one int32 source index per stored value slot of every resident form except CSR(A') (csrc/matrix_update.hpp;
 * 4 bytes per slot, INTEGRATION.md has the total); later calls allocate nothing new (temporaries come back from the block pool). */
SCS_HIP_API scs_int scs_hip_update_matrix(ScsWork *w, const scs_float *Ax, const scs_float *Px);
SCS_HIP_API scs_int scs_hip_update_matrix_device(ScsWork *w, const scs_float *Ax_dev, const scs_float *Px_dev);
/* Derivatives of the last solve, on the device (csrc/diff.hpp, lsqr.hpp, dproj.hpp).  At a solution with v = s - y the optimality
 * conditions F(x, v) = 0 have the Jacobian J = [[P, A'(W - I)], [A, W]], W = the derivative of the projection onto K at v.
 *   adjoint:    given gx = dL/dx (n), gy = dL/dy (m), gs = dL/ds (m) — NULL counts as 0 — solves J' lambda = (gx ; W gs + (W - I) gy) and
 *               writes dL/db (m), dL/dc (n), dL/dA (nnz(A) values in the order of the CSC arrays scs_init got) and dL/dP (nnz(P) values
 *               of the triangle as passed; an off-diagonal entry stands for both of its mirror images); a NULL output is skipped.
 *   derivative: given db (m), dc (n) — NULL counts as 0 — solves J (dx ; dv) = (-dc ; db) and writes dx (n), dy (m), ds (m).
 * Both run LSQR on the resident, equilibrated matrices; the results are in the caller's coordinates.  opts may be NULL (tol 1e-8,
 * max_iters 0 = 4 (n + m)); info may be NULL.  info->residual and info->normal_residual are LSQR's running estimates of
 * |M l - g| / |g| and |M' r| / (|M| |r|) (|M|: the Frobenius-norm estimate of the bidiagonalisation); stop = 1: the system is
 * consistent to tol, 2: the least-squares conditions hold to tol, 3: the iteration cap.  A singular J (a degenerate solution: a
 * tight row with a zero multiplier, more tight rows than columns) is NOT an error: LSQR then returns the minimum-norm least-squares
 * answer, usually with stop = 2.
 *
 * The *_device entries take DEVICE pointers of the workspace's device under the stream contract above; scs_hip_adjoint and
 * scs_hip_derivative take HOST pointers, stage them into device buffers and run the same path (same bits).  The first call of a
 * workspace takes 8 m + 6 n doubles of scratch from the block pool and keeps them until scs_finish; a request for dL/dP adds n + 1
 * ints.  A call reads the resident solution and matrices and writes nothing a later solve reads.  Two calls on the same state give
 * the same bits.  Clones and both linear solvers are served; users of a matrix set with pass layouts take turns, as for a solve.
 *
 * Returns 0, or -1 with the reason in scs_hip_last_error — refused before any device work, the workspace unchanged and usable: a NULL
 * workspace; no solve yet, or the last solve did not end SCS_SOLVED / SCS_SOLVED_INACCURATE; scs_update, scs_hip_update_device or
 * scs_hip_update_matrix[_device] ran since the last solve (the resident solution is stale); a cone other than z, l, box, q, s, p (named in the
 * message); (device entries) a pointer that is not device memory of the workspace's device; dPx for a workspace created without P, or
 * with a P whose values scs_hip_update_matrix would refuse (entries below the diagonal, unsorted rows). */
typedef struct {
  scs_float tol;      /* LSQR's atol = btol; <= 0: 1e-8 */
  scs_int max_iters;  /* <= 0: 4 (n + m) */
} ScsHipDiffOpts;
typedef struct {
  scs_int iters;
  scs_float residual, normal_residual;
  scs_int stop;
  scs_float time_ms;
} ScsHipDiffInfo;
SCS_HIP_API scs_int scs_hip_adjoint_device(ScsWork *w, const scs_float *gx_dev, const scs_float *gy_dev, const scs_float *gs_dev,
                                           scs_float *db_dev, scs_float *dc_dev, scs_float *dAx_dev, scs_float *dPx_dev,
                                           const ScsHipDiffOpts *opts, ScsHipDiffInfo *info);
SCS_HIP_API scs_int scs_hip_adjoint(ScsWork *w, const scs_float *gx, const scs_float *gy, const scs_float *gs, scs_float *db, scs_float *dc,
                                    scs_float *dAx, scs_float *dPx, const ScsHipDiffOpts *opts, ScsHipDiffInfo *info);
SCS_HIP_API scs_int scs_hip_derivative_device(ScsWork *w, const scs_float *db_dev, const scs_float *dc_dev, scs_float *dx_dev,
                                              scs_float *dy_dev, scs_float *ds_dev, const ScsHipDiffOpts *opts, ScsHipDiffInfo *info);
SCS_HIP_API scs_int scs_hip_derivative(ScsWork *w, const scs_float *db, const scs_float *dc, scs_float *dx, scs_float *dy, scs_float *ds,
                                       const ScsHipDiffOpts *opts, ScsHipDiffInfo *info);
/* The forward derivative with perturbations of the matrix VALUES as well (csrc/perturb.hpp): dAx = nnz(A) values in the order of the CSC
 * arrays scs_init got, dPx = nnz(P) values of the stored upper triangle (an off-diagonal value stands for both of its mirror images, as
 * in dL/dP: the full perturbation is T + T' - diag(T)); NULL counts as 0.  From F1 = P x + A' y + c, F2 = A x + s - b the system is
 *     J (dx ; dv) = (-(dc + dP x + dA' y) ; db - dA x)
 * with x, y the resident solution: three row products on the caller's pattern (values read through the index maps scs_hip_update_matrix
 * uses; one lane group per row, fixed summation order, no floating-point atomics) form the effective (dc ; db), and the path of
 * scs_hip_derivative runs unchanged.  scs_hip_derivative[_device] ARE these entries with NULL dAx and dPx: such a call allocates and
 * launches nothing of this and returns the bits it always did.  The first call that passes dAx or dPx takes n + m doubles of scratch
 * from the block pool (kept until scs_finish) and, when scs_hip_update_matrix has not built them, the int32 maps of CSR(A) (nnz(A), for
 * dAx) and of the full CSR(P) (its nnz, for dPx), kept with the matrix set — no layout map is built.  Two calls give the same bits, and
 * so do the host and device entries.  Clones and both linear solvers are served.
 * Refusals (as above: -1, the reason in scs_hip_last_error, before any device work, the workspace usable) in addition to those of
 * scs_hip_derivative: dPx for a workspace created without P, or with a P whose values scs_hip_update_matrix would refuse (entries below
 * the diagonal, row indices that do not ascend inside a column); (device entries) dAx / dPx that is not memory of the workspace's device. */
SCS_HIP_API scs_int scs_hip_derivative_full_device(ScsWork *w, const scs_float *db_dev, const scs_float *dc_dev, const scs_float *dAx_dev,
                                                   const scs_float *dPx_dev, scs_float *dx_dev, scs_float *dy_dev, scs_float *ds_dev,
                                                   const ScsHipDiffOpts *opts, ScsHipDiffInfo *info);
SCS_HIP_API scs_int scs_hip_derivative_full(ScsWork *w, const scs_float *db, const scs_float *dc, const scs_float *dAx, const scs_float *dPx,
                                            scs_float *dx, scs_float *dy, scs_float *ds, const ScsHipDiffOpts *opts, ScsHipDiffInfo *info);
/* The perturbation products of those entries on their own (tests, parity with a host product): out_c (n) = dP x + dA' y and
 * out_b (m) = dA x at the resident solution; a NULL input counts as 0, a NULL output is skipped.  Refusals as scs_hip_derivative_full. */
SCS_HIP_API scs_int scs_hip_data_perturbation_device(ScsWork *w, const scs_float *dAx_dev, const scs_float *dPx_dev, scs_float *out_c_dev,
                                                     scs_float *out_b_dev);
SCS_HIP_API scs_int scs_hip_data_perturbation(ScsWork *w, const scs_float *dAx, const scs_float *dPx, scs_float *out_c, scs_float *out_b);

/* The same for a batch of `count` solved workspaces (csrc/diff_batch.hpp).  Members that agree in device, n, m, has-P, normalisation,
 * the z / l / q / s cone structure and in whether dAx / dPx are requested, whose matrices use the CSR-stream layout and whose PSD blocks
 * have order <= 32, are differentiated in lock step and SHARE every launch of the LSQR iteration (blockIdx.y = member); every other
 * member is served by the one-workspace path in turn.  Each member's outputs, info->iters, stop, residual and normal_residual are
 * bit-identical to its own scs_hip_adjoint[_device] / scs_hip_derivative[_device] call (time_ms is the group's).  A call writes nothing
 * a later solve reads.
 *   Every array argument holds `count` entries and may be NULL ("no such input or output for any member"); an entry may be NULL too.
 *   opts (tol, max_iters) hold for every member; info may be NULL, and so may info[i].
 *   Refusals are those of the one-workspace entries, checked for EVERY member before any device work: the call returns -1, writes no
 *   output, scs_hip_last_error() names the member index and the reason, and every workspace stays usable.  A workspace that appears
 *   twice, a NULL member and count <= 0 are refused as well.  The workspaces must live on one device and must not be used by other
 *   threads meanwhile (as scs_hip_solve_batch).  The grouped preparation of PSD members borrows at most 256 MiB of pool scratch at once.
 * scs_hip_adjoint_batch / scs_hip_derivative_batch take HOST pointers, stage them and run the device path (same bits). */
SCS_HIP_API scs_int scs_hip_adjoint_batch_device(ScsWork **w, const scs_float **gx_dev, const scs_float **gy_dev, const scs_float **gs_dev,
                                                 scs_float **db_dev, scs_float **dc_dev, scs_float **dAx_dev, scs_float **dPx_dev,
                                                 const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count);
SCS_HIP_API scs_int scs_hip_adjoint_batch(ScsWork **w, const scs_float **gx, const scs_float **gy, const scs_float **gs, scs_float **db,
                                          scs_float **dc, scs_float **dAx, scs_float **dPx, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info,
                                          scs_int count);
/* The adjoint of `count` workspaces that SHARE one matrix set (a workspace and its scs_hip_clone's), with the gradients of the matrix
 * values SUMMED over the members: the case of one learned matrix and a batch of right-hand sides.  gx .. dc are the arrays of
 * scs_hip_adjoint_batch[_device]; the two matrix outputs are ONE vector each, dAx_sum of nnz(A) and dPx_sum of nnz(P) (triangle) values in
 * the order of scs_hip_adjoint's dAx / dPx; either may be NULL.
 *   The members are differentiated exactly as scs_hip_adjoint_batch[_device] does with dAx = dPx = NULL — the same grouping, the same
 *   launches — so every member's db, dc and info (but time_ms) are bit for bit those of that call; a member whose db / dc is not asked for
 *   keeps them in its own scratch.  Then the members' x, y, db, dc are packed, at most 256 members at a time, into panels with the member
 *   index fastest, and one kernel per matrix walks the stored pattern ONCE per chunk (csrc/grad_shared.hpp):
 *       dAx_sum[p] = sum_k ( y_k[i] dc_k[j] - db_k[i] x_k[j] ),    dPx_sum[q] = sum_k ( dc_k[c] x_k[r] + dc_k[r] x_k[c] )  (diagonal: once)
 *   over all members in index order.  Nothing of K x nnz is formed: the call borrows 2 (n + m) min(K, 256) doubles of panels from the block
 *   pool (the chunk is lowered where that would exceed 256 MiB, the cap of the grouped PSD preparation above) and returns them.  The order
 *   of every sum is fixed by count and the chunk alone; there are no floating-point atomics, and two calls on the same state give the same
 *   bits, as do the host and the device entry.
 *   Refusals (-1, the reason with the member index in scs_hip_last_error, before any device work, every workspace usable): those of
 *   scs_hip_adjoint_batch[_device]; a member that does not hold the matrix set of member 0 (scs_hip_shares_matrix); dPx_sum where
 *   scs_hip_adjoint refuses dPx (no P, or a P whose values scs_hip_update_matrix would refuse); dAx_sum and dPx_sum both NULL.
 * scs_hip_adjoint_shared takes HOST pointers, stages them and runs the device path (same bits). */
SCS_HIP_API scs_int scs_hip_adjoint_shared_device(ScsWork **w, const scs_float **gx_dev, const scs_float **gy_dev, const scs_float **gs_dev,
                                                  scs_float **db_dev, scs_float **dc_dev, scs_float *dAx_sum_dev, scs_float *dPx_sum_dev,
                                                  const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count);
SCS_HIP_API scs_int scs_hip_adjoint_shared(ScsWork **w, const scs_float **gx, const scs_float **gy, const scs_float **gs, scs_float **db,
                                           scs_float **dc, scs_float *dAx_sum, scs_float *dPx_sum, const ScsHipDiffOpts *opts,
                                           ScsHipDiffInfo **info, scs_int count);
SCS_HIP_API scs_int scs_hip_derivative_batch_device(ScsWork **w, const scs_float **db_dev, const scs_float **dc_dev, scs_float **dx_dev,
                                                    scs_float **dy_dev, scs_float **ds_dev, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info,
                                                    scs_int count);
SCS_HIP_API scs_int scs_hip_derivative_batch(ScsWork **w, const scs_float **db, const scs_float **dc, scs_float **dx, scs_float **dy,
                                             scs_float **ds, const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count);
/* scs_hip_derivative_full for a batch: dAx / dPx hold `count` entries like the other arrays (NULL array or NULL entry = no perturbation
 * of that matrix for that member).  Members are grouped as above, and by whether they pass dAx / dPx (as the adjoint groups by the
 * request for dAx / dPx); the launch count of a group does not depend on its size.  scs_hip_derivative_batch[_device] are these entries
 * with NULL dAx and dPx. */
SCS_HIP_API scs_int scs_hip_derivative_full_batch_device(ScsWork **w, const scs_float **db_dev, const scs_float **dc_dev,
                                                         const scs_float **dAx_dev, const scs_float **dPx_dev, scs_float **dx_dev,
                                                         scs_float **dy_dev, scs_float **ds_dev, const ScsHipDiffOpts *opts,
                                                         ScsHipDiffInfo **info, scs_int count);
SCS_HIP_API scs_int scs_hip_derivative_full_batch(ScsWork **w, const scs_float **db, const scs_float **dc, const scs_float **dAx,
                                                  const scs_float **dPx, scs_float **dx, scs_float **dy, scs_float **ds,
                                                  const ScsHipDiffOpts *opts, ScsHipDiffInfo **info, scs_int count);
/* The grouping those entries would use for members that all request (want_dA, want_dP), as scs_hip_batch_plan: group_of[i] = the index
 * of member i's group, -1 = served alone.  Returns the number of groups, -1 on error. */
SCS_HIP_API int scs_hip_diff_batch_plan(ScsWork **w, scs_int count, int want_dA, int want_dP, scs_int *group_of);
/* grouped launches issued by the batch derivative entries since the process started (tests, tools; as scs_hip_tiled_launches) */
SCS_HIP_API long scs_hip_diff_group_launches(void);
/* host synchronisations made by those groups (and by the groups of scs_hip_refine_batch) since the process started (tools) */
SCS_HIP_API long scs_hip_diff_group_syncs(void);
/* Several directions at ONE solution: K cotangents (adjoint) or K perturbations (derivative) of the workspace's last solve in one call.
 * The arrays are row-major, one direction per row: GX K x n, GY and GS K x m (NULL = zeros, as in scs_hip_adjoint), DB K x m, DC K x n,
 * DAx K x nnz(A), DPx K x nnz(P) (NULL = not wanted); for the derivative DB K x m and DC K x n in, DX K x n, DY and DS K x m out.
 * infos: K entries, or NULL.  The preparation (the fixed point, the cone records, the eigen-decomposition of the PSD blocks) runs once,
 * then the K directions are K LSQR lanes on the one workspace in lock step: one launch per kernel for all lanes, and the products read
 * A, A' and P once per tile of lanes.  Every direction's outputs and info (apart from time_ms, which is the call's) have the bits of
 * scs_hip_adjoint / scs_hip_derivative on that direction alone.  A workspace whose layouts the grouped derivative does not cover
 * (column-sorted or slab layouts, PSD orders above 32, a long box cone) is served one direction after the other, same bits.
 * Refusals as the single entries', and K < 1 or K > 32 (the caller chunks; the lanes beyond the first cost 8 m + 6 n doubles each and
 * are kept until scs_finish).  The host twins stage the arrays like the single entries do. */
SCS_HIP_API scs_int scs_hip_adjoint_multi_device(ScsWork *w, scs_int K, const scs_float *GX_dev, const scs_float *GY_dev,
                                                 const scs_float *GS_dev, scs_float *DB_dev, scs_float *DC_dev, scs_float *DAx_dev,
                                                 scs_float *DPx_dev, const ScsHipDiffOpts *opts, ScsHipDiffInfo *infos);
SCS_HIP_API scs_int scs_hip_adjoint_multi(ScsWork *w, scs_int K, const scs_float *GX, const scs_float *GY, const scs_float *GS, scs_float *DB,
                                          scs_float *DC, scs_float *DAx, scs_float *DPx, const ScsHipDiffOpts *opts, ScsHipDiffInfo *infos);
SCS_HIP_API scs_int scs_hip_derivative_multi_device(ScsWork *w, scs_int K, const scs_float *DB_dev, const scs_float *DC_dev,
                                                    scs_float *DX_dev, scs_float *DY_dev, scs_float *DS_dev, const ScsHipDiffOpts *opts,
                                                    ScsHipDiffInfo *infos);
SCS_HIP_API scs_int scs_hip_derivative_multi(ScsWork *w, scs_int K, const scs_float *DB, const scs_float *DC, scs_float *DX, scs_float *DY,
                                             scs_float *DS, const ScsHipDiffOpts *opts, ScsHipDiffInfo *infos);
/* lanes per workgroup of the multi entries' products: sets 4 or 8 (anything else: only reads) and returns the previous value.  For
 * tools/adjoint_multi_bench.py, which measures both; the results do not depend on it. */
SCS_HIP_API int scs_hip_diff_lane_tile(int tile);
/* Newton polish of the resident solution (csrc/refine.hpp).  The solve is a first-order method: it reaches 1e-4 quickly and 1e-9 slowly,
 * and the derivative entries above are only meaningful at an accurate fixed point.  A Newton step on F(x, v) = 0 is one forward-mode
 * solve J d = -F on the machinery of scs_hip_derivative; Pi_K(v) = W(v) v (Pi_K is positively homogeneous) gives s = Pi(v) and
 * y = Pi(v) - v from one apply of W, so no projection of the solve is called and none of its state is touched.
 *   Start: the resident (x, v = s - y) of the last solve.  Step: LSQR on J d = -F (lsqr_tol, lsqr_max_iters), then t = 1, 1/2, ... (at
 *   most 10 halvings) until |F(z + t d)|_2 < (1 - 1e-4 t) |F(z)|_2; every trial re-derives W at its own v.  Stop rule: the solver's
 *   three criteria with eps_abs = eps_rel = tol in the caller's units,
 *       |Ax + s - b|_inf <= tol (1 + max(|Ax|_inf, |s|_inf, |b|_inf)),  |Px + A'y + c|_inf <= tol (1 + max(|Px|_inf, |A'y|_inf, |c|_inf)),
 *       |x'Px + c'x + b'y| <= tol (1 + max(|x'Px|, |c'x|, |b'y|)).
 *   info->stop = 1: the criteria hold; 2: max_steps reached; 3: no t gave a decrease.  On 2 and 3 the best accepted point is kept.
 *   steps = accepted steps, halvings and lsqr_iters are totals; merit = |F|_2 in the solver's scaled coordinates; res_pri, res_dual,
 *   gap, pobj, dobj are those of the final point (the *_before ones: of the starting point), in the caller's units.
 * A start that already meets the criteria returns steps = 0, stop = 1 and leaves the resident solution bit for bit as it was, and so
 * does a call in which no step is accepted.  Otherwise the accepted point REPLACES the resident solution: every later derivative
 * entry, scs_hip_solution_to_device and a device warm start read it.  sol (host pointers for scs_hip_refine, device pointers of the
 * workspace's device for scs_hip_refine_device; sol or any member may be NULL) receives the resident x, y, s after the call.  opts and
 * info may be NULL.  Two calls on the same state give the same bits, and so do the host and the device entry.  The first call takes
 * 2 (n + m) doubles (plus the partials of one reduction pass) from the block pool beside the derivative's scratch, kept until
 * scs_finish; a workspace that never refines takes nothing.  Every loop is bounded on the host.
 * Returns 0, or -1 with the reason in scs_hip_last_error — before any device work, the workspace unchanged and usable: a NULL workspace;
 * the refusals of scs_hip_derivative (no solve yet, not solved, stale, a cone without a derivative, by name); a NaN tol; (device
 * entry) a pointer that is not device memory of the workspace's device. */
typedef struct {
  scs_float tol;          /* stop rule; <= 0: 1e-9 */
  scs_int max_steps;      /* <= 0: 10 */
  scs_float lsqr_tol;     /* inner atol = btol; <= 0: 1e-8 */
  scs_int lsqr_max_iters; /* <= 0: 4 (n + m) */
} ScsHipRefineOpts;
typedef struct {
  scs_int steps, halvings, lsqr_iters, stop;
  scs_float merit_before, merit_after;
  scs_float res_pri_before, res_dual_before, gap_before, res_pri, res_dual, gap, pobj, dobj, time_ms;
} ScsHipRefineInfo;
SCS_HIP_API scs_int scs_hip_refine(ScsWork *w, ScsSolution *sol, const ScsHipRefineOpts *opts, ScsHipRefineInfo *info);
SCS_HIP_API scs_int scs_hip_refine_device(ScsWork *w, ScsSolution *sol_dev, const ScsHipRefineOpts *opts, ScsHipRefineInfo *info);
/* scs_hip_refine for `count` solved workspaces at once (csrc/refine_batch.hpp).  Members are grouped as scs_hip_adjoint_batch groups them
 * with no matrix gradient requested (scs_hip_diff_batch_plan(w, count, 0, 0, ..) describes it): equally shaped members whose layouts the
 * grouped derivative covers are refined in LOCK STEP, one launch per kernel for the group (scs_hip_diff_group_launches counts them; the
 * count does not depend on the group's size) and one host synchronisation per evaluation of the residual for the group; a member
 * without a group goes through the path of scs_hip_refine.  The control flow is per member, on the host, over lists: members of one
 * group may take different numbers of steps and halvings and stop for different reasons.  Every member's x, y, s and info have the bits
 * of scs_hip_refine on that member alone, except time_ms, which is its group's; the host and the device entry give the same bits.
 *   sol and info hold `count` entries; either array and any entry may be NULL.  opts (may be NULL) hold for every member.  Afterwards
 *   every member's polished point is its resident solution, as after scs_hip_refine.
 *   Returns 0, or -1 with the reason and the member's index ("member i") in scs_hip_last_error, checked for EVERY member before any
 *   device work, all workspaces unchanged and usable: the refusals of scs_hip_refine; a NULL member; a workspace that appears twice;
 *   count <= 0; members on different devices; (device entry) a pointer that is not device memory of the members' device. */
SCS_HIP_API scs_int scs_hip_refine_batch(ScsWork **w, ScsSolution **sol, const ScsHipRefineOpts *opts, ScsHipRefineInfo **info, scs_int count);
SCS_HIP_API scs_int scs_hip_refine_batch_device(ScsWork **w, ScsSolution **sol_dev, const ScsHipRefineOpts *opts, ScsHipRefineInfo **info,
                                                scs_int count);
/* the HIP device a workspace lives on (-1: NULL) */
SCS_HIP_API int scs_hip_work_device(const ScsWork *w);

/* Grouped solve of `count` independent, already initialised workspaces (BASELINE.json configs[4]: a batch of small cone
 * programs; the reference's notion is "independent instances run concurrently", R:test/test_thread_safety.py:78-93 —
 * one scs_solve per thread).  Members of equal shape (n, m, cone structure, Anderson schedule) whose matrices use the
 * CSR-stream layout advance through the ADMM loop in lock step and SHARE every kernel launch (blockIdx.y = problem,
 * arguments from a per-problem record in HBM; csrc/batch.hpp); whatever cannot be grouped is solved by scs_solve's own
 * loop, one after the other.  sol[i] / info[i] are filled exactly as scs_solve(w[i], sol[i], info[i], warm_start) fills
 * them — the grouped kernels run the same device code over the same block decomposition, so iterates, iteration and
 * CG-step counts are bit-identical to separate solves (timing fields are those of the group).  Returns 0, -1 on error
 * (scs_hip_last_error).  The workspaces must live on one device and must not be used by other threads meanwhile. */
SCS_HIP_API scs_int scs_hip_solve_batch(ScsWork **w, ScsSolution **sol, ScsInfo **info, scs_int count, scs_int warm_start);
/* The grouping scs_hip_solve_batch(w, .., count, ..) would use, without solving: group_of[i] = the index of the group member i
 * would join, -1 for a member it would solve alone by scs_solve.  Returns the number of groups, -1 on error (null arguments,
 * a workspace twice; scs_hip_last_error).  scs_hip_solve_batch forms its groups with the same code. */
SCS_HIP_API int scs_hip_batch_plan(ScsWork **w, scs_int count, scs_int *group_of);

/* One matrix, many (b, c): a workspace in the state scs_init left `w` in — w's ORIGINAL b, c and settings (not what scs_update or a
 * solve made of them since), cold start, empty Anderson history — that SHARES w's resident matrix data (every layout of A', A and P,
 * the diagonal of P, the equilibration vectors) and allocates only per-solve state.  The shared set is read-only after scs_init and
 * reference-counted: it is released by whichever of its users is finished last, so w may be finished before its clones.  A clone is a
 * workspace like any other (scs_update, scs_solve, scs_finish, scs_hip_solution_to_device, scs_hip_solve_batch, scs_hip_clone);
 * w and its clones may be solved from different threads at the same time (users of a set with column-sorted layouts take turns).
 * Inside a scs_hip_solve_batch group, members that share a set read one copy of the matrix, with iterates bit-identical to
 * separate solves (the labs build can launch their products per tile of four members: csrc/batch.hpp, SCS_HIP_SHARED_TILE=1).  The file names of
 * write_data_filename / log_csv_filename are not inherited.  Returns NULL on error (scs_hip_last_error). */
SCS_HIP_API ScsWork *scs_hip_clone(ScsWork *w);
/* 1 when a and b hold the same matrix set (a workspace and its clones, clones of clones), else 0. */
SCS_HIP_API int scs_hip_shares_matrix(const ScsWork *a, const ScsWork *b);

/* bench.py: a timestamp inside the next scs_solve calls.  When ADMM iteration `iter` is about to start, the stream is
 * drained and out[4] = {ms since the start of the solve, CG steps so far, Anderson calls so far, accepted so far} is
 * recorded (out[0] < 0: the solve ended before that iteration); iter < 0 switches it off. */
SCS_HIP_API void scs_hip_set_mark(ScsWork *w, int iter);
SCS_HIP_API void scs_hip_get_mark(const ScsWork *w, double *out);
/* `reps` back-to-back launches of K1, then of K2 and — problems with P — of K3 on the solver's own stream and HBM-resident
 * data, one HIP event pair per batch (the ~10-20 us per-event overhead is amortised).
 * out[4] = {K1 avg ms, K2 avg ms, K3 avg ms as the CG step runs it — between K1 and K2: (K1, K3, K2) x reps minus (K1, K2) x reps —, K3 avg ms
 * back to back (its matrix may then stay in the Infinity Cache)}; K3: 0 without P.  Returns 0 on success. */
SCS_HIP_API int scs_hip_time_matvec(ScsWork *w, int reps, double *out);

/* Anderson acceleration as a standalone object on host vectors (row a6): the interface of scs_source/src/aa.c
 * (aa_init / aa_apply / aa_safeguard / aa_reset / aa_finish; named at R:meson.build:187, knobs R:README.md:98-104,
 * statistics R:scs/scsobject.h:1096-1107).  mem <= 32.  scs_solve runs the same device object on the resident iterate.
 *   apply:     f = F(x) on entry; on return f may hold the extrapolated iterate.  Returns aa_norm (0: history
 *              still filling, < 0: step rejected and history reset, NaN: error).
 *   safeguard: f_new = F(x_new) of the step after an accepted extrapolation; returns -1 and restores the
 *              pre-extrapolation pair when the fixed-point residual grew, else 0.
 *   last_gamma: weights of the most recent solve (returns their count; gamma may be NULL). */
typedef struct ScsHipAa ScsHipAa;
SCS_HIP_API ScsHipAa *scs_hip_aa_init(scs_int dim, scs_int mem, scs_int type1, scs_float regularization, scs_float relaxation,
                          scs_float safeguard_factor, scs_float max_weight_norm);
SCS_HIP_API scs_float scs_hip_aa_apply(ScsHipAa *a, scs_float *f, const scs_float *x);
SCS_HIP_API scs_int scs_hip_aa_safeguard(ScsHipAa *a, scs_float *f_new, scs_float *x_new);
SCS_HIP_API void scs_hip_aa_reset(ScsHipAa *a);
SCS_HIP_API void scs_hip_aa_get_stats(const ScsHipAa *a, ScsAaStats *st);
SCS_HIP_API scs_int scs_hip_aa_last_gamma(const ScsHipAa *a, scs_float *gamma);
SCS_HIP_API void scs_hip_aa_finish(ScsHipAa *a);

/* bench.py --workload config4_psd: average duration of one batched PSD projection (all `s` cones, warm-started as inside
 * the ADMM loop) on the solver's stream; out[4] = {ms per projection, matrices, largest order, reference flop count
 * ((16/3 + 2) n^3 per matrix)}.  0 on success, 1 when the problem has no PSD cone. */
SCS_HIP_API int scs_hip_time_psd(ScsWork *w, int reps, double *out);

/* tools/adjoint_bench.py --cones: after a solve, the kernels of the box and power derivative (csrc/dproj_box_pow.hpp) at the solution's
 * fixed point, timed with events on the workspace's stream, `reps` launches each.  out[8] = {ms per box W apply in the one-workgroup
 * form, ms in the two-launch form (both at this cone's size, whatever form a call would pick), ms per projection of the same cone in
 * the form a solve uses (on scratch: the solve's warm start is not touched), bsize, ms per W apply of the power cones, ms per
 * preparation of their W, ms per projection of them, their count}; the entries of a cone the problem does not have are 0.
 * 0 on success, -1 with a reason where scs_hip_adjoint would refuse the workspace. */
SCS_HIP_API int scs_hip_time_dproj(ScsWork *w, int reps, double *out);

/* Hands the device blocks this library caches for reuse (dead workspaces' buffers, at most SCS_HIP_POOL_MB = 1024 MiB by default) back
 * to the driver: for a process that shares its GPUs with allocators this library does not see (torch, RCCL, other processes). */
SCS_HIP_API void scs_hip_trim_pool(void);

/* The block pool's account, read under the pool's lock (host counters only: no device work).  held_* = what the pool caches now;
 * live_bytes = device bytes this library obtained from hipMalloc and has not handed back with hipFree yet (held blocks included: with no
 * workspace alive live_bytes == held_bytes, and both are 0 after scs_hip_trim_pool); hits / misses = allocations since the process
 * started that the pool served / that went to hipMalloc. */
typedef struct {
  size_t held_bytes, held_blocks, live_bytes, hits, misses;
} ScsHipPoolStats;
SCS_HIP_API void scs_hip_pool_stats(ScsHipPoolStats *out);

/* How many solves of this process were restarted because a spinning multi-workgroup kernel (multi-CU PSD sweeps, persistent CG)
 * timed out at a barrier — another process held part of the GPU — and were then finished without such kernels (tests). */
SCS_HIP_API long scs_hip_spin_fallbacks(void);
/* How many tiled CSR-stream launches (one read of a shared matrix per tile of members, csrc/batch.hpp) grouped solves of this
 * process have issued (tests, tools/shared_batch_bench.py). */
SCS_HIP_API long scs_hip_tiled_launches(void);

/* K9's refinement stage (csrc/psd.hpp psd_stop_test), diagnostics for tests and bench: for each of the first `cap` PSD matrices of
 * order > 32 of the workspace EIGHT doubles {calls that took the refinement stage so far, refinements whose a-posteriori test sent the
 * matrix back to the sweeps, |K1|_F^2 at the last gate, mixed-sign off-norm^2 / |A|_F^2 after the last refinement, stage flag of the
 * last call (0 none, 1 refined, 2 refined + sweeps), and the gate's view of the last call's matrix as it arrived: |K1|_F^2,
 * |off|_F^2 / |A|_F^2, omega}.  Returns the number of matrices written, -1 on error. */
SCS_HIP_API int scs_hip_psd_refine_stats(ScsWork *w, double *out, int cap);

/* last error message of the calling thread ("" if none) */
SCS_HIP_API const char *scs_hip_last_error(void);

/* ------------------------------------------------------- spectral cones
 * The same entry points for a cone that carries the spectral fields of ScsCone (scs_types.h, USE_SPECTRAL_CONES): they
 * read the whole struct, the plain names above read it only up to psize.  A consumer compiled with -DUSE_SPECTRAL_CONES
 * reaches them through the plain names (the remapping below); one compiled without the flag keeps the short struct and
 * the plain entries.  INTEGRATION.md §B. */
#if defined(USE_SPECTRAL_CONES)
SCS_HIP_API ScsWork *scs_init_spectral(const ScsData *d, const ScsCone *k, const ScsSettings *stgs);
SCS_HIP_API ScsWork *scs_hip_init_linsys_spectral(const ScsData *d, const ScsCone *k, const ScsSettings *stgs, int linsys);
SCS_HIP_API int scs_hip_proj_cone_spectral(scs_float *x, const ScsCone *k, scs_int m, int dual);
/* scs_hip_normalize for a cone with spectral rows: each log-det, nuclear, ell1 and sum-of-largest cone is one block with one
 * row scale (tests).  Not remapped below: the plain name stays the short-struct entry. */
SCS_HIP_API int scs_hip_normalize_spectral(ScsMatrix *A, ScsMatrix *P, scs_float *b, scs_float *c, const ScsCone *k,
                      scs_float *D, scs_float *E, scs_float *sigma);
#if !defined(SCS_HIP_BUILDING_LIBRARY)
#define scs_init scs_init_spectral
#define scs_hip_init_linsys scs_hip_init_linsys_spectral
#define scs_hip_proj_cone scs_hip_proj_cone_spectral
#endif
#endif

#ifdef __cplusplus
}
#endif
#endif
