// device_io.hpp — the device-resident endpoints of a workspace (include/scs_hip.h: scs_hip_update_device, scs_hip_solve_device,
// scs_hip_solve_batch_device): b / c arrive as device vectors, the warm start is built from device x, y, s, and the solution is
// handed over device to device.  The host twins (scs_update: csrc/scs_hip.hip, begin_solve's host loop: work_solve_ends.inl,
// normalize_b_c: host_setup.hpp) do the same arithmetic on the host; every expression here keeps their operands and their
// order, products and quotients only (nothing a compiler may contract), so both paths leave the same bits.
#pragma once
#include "common.hpp"
#include "vec.hpp"

namespace scship {

static_assert(S_NM_C == S_NM_B + 1 && S_SIGMA == S_NM_B + 2 && S_SIGMA < S_COUNT, "the three slots k_bc_load leaves are read back in one copy");

// ---- update: h = [c E ; b D] (raw when D == nullptr), raw copies, the four max-norms and sigma --------------------------------
// b_src / c_src: the caller's vectors, or b_raw / c_raw themselves ("keep": nothing is stored back then).
// part: [max |b| | max |c| | max |b D| | max |c E|], gridDim.x entries each.  The LAST workgroup to arrive (agent-scope ticket, as
// k_cg_update_dir: nothing waits) folds them in index order — maxima are exact, so the fold order does not show — and leaves
// sc[S_NM_B], sc[S_NM_C] and sc[S_SIGMA], sigma by the rule of normalize_b_c / device_normalize_b_c.
__global__ __launch_bounds__(kVecThreads) void k_bc_load(const double *b_src, const double *c_src, double *b_raw, double *c_raw,
                                                         const double *__restrict__ D, const double *__restrict__ E, int n, int m,
                                                         double *h, double *part, double *sc, unsigned *ticket) {
  __shared__ double sm[kVecThreads / 64];
  __shared__ unsigned tk;
  const int nb = (int)gridDim.x;
  const bool store_b = b_src != b_raw, store_c = c_src != c_raw;
  double mb = 0., mc = 0., mbd = 0., mce = 0.;
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)nb * kVecThreads) {
    if (i < n) {
      const double ci = c_src[i];
      if (store_c) c_raw[i] = ci;
      mc = fmax(mc, fabs(ci));
      const double ce = E ? ci * E[i] : ci;
      h[i] = ce;
      mce = fmax(mce, fabs(ce));
    } else {
      const long k = i - n;
      const double bi = b_src[k];
      if (store_b) b_raw[k] = bi;
      mb = fmax(mb, fabs(bi));
      const double bd = D ? bi * D[k] : bi;
      h[i] = bd;
      mbd = fmax(mbd, fabs(bd));
    }
  }
  mb = block_max<kVecThreads>(mb, sm);
  mc = block_max<kVecThreads>(mc, sm);
  mbd = block_max<kVecThreads>(mbd, sm);
  mce = block_max<kVecThreads>(mce, sm);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = mb;
    part[nb + blockIdx.x] = mc;
    part[2 * nb + blockIdx.x] = mbd;
    part[3 * nb + blockIdx.x] = mce;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (threadIdx.x == 0) tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (tk != (unsigned)nb - 1) return;
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const double nm_b = part_max(part, nb, sm);
  const double nm_c = part_max(part + nb, nb, sm);
  const double nm_bd = part_max(part + 2 * nb, nb, sm);
  const double nm_ce = part_max(part + 3 * nb, nb, sm);
  if (threadIdx.x == 0) {
    double sigma = fmax(nm_ce, nm_bd);
    sigma = sigma < 1e-4 ? 1.0 : sigma;
    sigma = sigma > 1e4 ? 1e4 : sigma;
    sigma = sigma < 1e-18 ? 1.0 / 1e-18 : 1.0 / sigma;  // safediv_pos(1, sigma)
    sc[S_NM_B] = nm_b;
    sc[S_NM_C] = nm_c;
    sc[S_SIGMA] = sigma;
  }
}

// h *= sigma; Dinv = 1 / (D sigma); Einv = 1 / (E sigma) — sigma from the slot k_bc_load left (normalised workspaces only)
__global__ __launch_bounds__(kVecThreads) void k_bc_finish(double *h, const double *__restrict__ D, const double *__restrict__ E,
                                                           double *Dinv, double *Einv, int n, int m, const double *sc) {
  const double sigma = sc[S_SIGMA];
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < (long)n + m; i += (long)gridDim.x * kVecThreads) {
    h[i] *= sigma;
    if (i < n) Einv[i] = 1.0 / (E[i] * sigma);
    else Dinv[i - n] = 1.0 / (D[i - n] * sigma);
  }
}

// ---- warm start: v = [x / (E / sg) ; y / (D / sg) + (s (D sg)) / r_y ; 1], non-finite entries 0 (begin_solve's host loop) ----
// r_y = ry_z on the first nz rows (zero cone), ry_o elsewhere; D == nullptr: an un-normalised workspace (x, y, s as they are)
__global__ __launch_bounds__(kVecThreads) void k_warm_v(const double *__restrict__ x, const double *__restrict__ y,
                                                        const double *__restrict__ s, const double *__restrict__ D,
                                                        const double *__restrict__ E, double sg, double ry_z, double ry_o, int nz, int n,
                                                        int m, double *v) {
  const long l = (long)n + m + 1;
  for (long i = (long)blockIdx.x * kVecThreads + threadIdx.x; i < l; i += (long)gridDim.x * kVecThreads) {
    double val;
    if (i < n) {
      val = E ? x[i] / (E[i] / sg) : x[i];
    } else if (i < l - 1) {
      const long k = i - n;
      const double ry = k < nz ? ry_z : ry_o;
      const double yh = D ? y[k] / (D[k] / sg) : y[k];
      const double sh = D ? s[k] * (D[k] * sg) : s[k];
      val = yh + sh / ry;
    } else {
      val = 1.0;
    }
    v[i] = isfinite(val) ? val : 0.;
  }
}

}  // namespace scship
