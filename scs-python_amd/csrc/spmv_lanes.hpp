// spmv_lanes.hpp — the CSR-stream product of ONE matrix with the vectors of K lanes (diff_batch.hpp: the K directions of a multi call on
// one solved workspace): the matrix is read once per lane tile, not once per lane.
//
// Grid (row blocks, lane tiles); tile y holds entries y * TILE .. of the launch's lane list, TILE in {4, 8}.  A workgroup loads its row
// block's blk, its lanes' row extents and its val / col into registers ONCE — at most kNnzPerWg / kSpmvThreads = 8 nonzeros per lane
// of the wavefront, as d_spmv_stream_tiled (batch.hpp) — and then, for each live lane of the tile in turn, gathers that lane's x,
// stages v[k] * x[c[k]] in one of TWO 16 KiB product buffers, sums the rows with the shared stream_rows (spmv.hpp) and calls that
// lane's epilogue.  The buffers alternate, so a lane costs one barrier: lane t + 1 stages into the other buffer while slower wavefronts
// still sum lane t, and the barrier of lane t + 1 is what frees lane t's buffer for lane t + 2.  LDS is 32 KiB + the reduction scratch
// whatever the tile width (batch.hpp's prod[T][kNnzPerWg] grows with it), so the occupancy does not fall with the tile.
// A row block with more than kNnzPerWg nonzeros (one long row): each nonzero is read once and feeds every live lane's running sum in
// that lane's own order (k = tid, tid + 256, ..), then one group_sum per lane.
// Per lane the floating-point sequence is that of spmv_stream_block: a lane's product has the bits of a launch of its own.  A lane
// whose done flag is up is skipped, a tile with none alive returns at once.  No atomics: every sum keeps its fixed order.
#pragma once

namespace scship {

constexpr int kLaneTileMax = 8;

template <class Epi, int TILE>
__device__ __forceinline__ void d_spmv_stream_lanes(const SpmvRec<Epi> *__restrict__ tab, const int *__restrict__ list, int cnt) {
  static_assert(TILE >= 1 && TILE <= kLaneTileMax, "lane tile");
  const int tid = (int)threadIdx.x;
  // the tile's lanes (uniform: scalar loads).  -1 = past the end of the list, or a lane that has converged
  int mem[TILE], first = -1;
#pragma unroll
  for (int t = 0; t < TILE; ++t) {
    const int at = (int)blockIdx.y * TILE + t;
    int g = at < cnt ? list[at] : -1;
    if (g >= 0) {
      const int *done = tab[g].tail.tail.tail.head;
      if (done && *done) g = -1;
    }
    mem[t] = g;
    if (g >= 0 && first < 0) first = g;
  }
  if (first < 0) return;
  const CsrView A = tab[first].head;  // the one matrix: every lane's record holds this view
  if ((int)blockIdx.x >= A.nblk) return;
  __shared__ double prod[2][kNnzPerWg];
  __shared__ double red[kSpmvThreads / 64];
  const int b = A.pbase + (int)blockIdx.x, nb = A.pstride > 0 ? A.pstride : (int)gridDim.x;
  const int4 bi = A.blk[blockIdx.x];
  const int r0 = bi.x, r1 = bi.y, p0 = bi.z, p1 = bi.w;
  const int nnz = p1 - p0;
  constexpr int NS = Epi::kSums > 0 ? Epi::kSums : 1, NM = Epi::kMaxs > 0 ? Epi::kMaxs : 1;
  const BlockSync sync{};
  if (nnz <= kNnzPerWg) {
    constexpr int NK = kNnzPerWg / kSpmvThreads;
    const double *__restrict__ v = A.val + p0;
    const int *__restrict__ c = A.col + p0;
    int ra[kRowsPerLane], re[kRowsPerLane];
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
      const int r = r0 + tid + j * kSpmvThreads;
      ra[j] = r < r1 ? A.rowptr[r] - p0 : 0;
      re[j] = r < r1 ? A.rowptr[r + 1] - p0 : 0;
    }
    double vv[NK];
    int cc[NK];
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int k = tid + i * kSpmvThreads;
      vv[i] = k < nnz ? v[k] : 0.;
      cc[i] = k < nnz ? c[k] : 0;
    }
    int buf = 0;
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
      if (mem[t] < 0) continue;
      const double *__restrict__ x = tab[mem[t]].tail.head;
      double *pb = prod[buf];
#pragma unroll
      for (int i = 0; i < NK; ++i) {
        const int k = tid + i * kSpmvThreads;  // (k < nnz <= kNnzPerWg: inside the buffer)
        if (k < nnz) pb[k] = vv[i] * x[cc[i]];
      }
      sync();
      const Epi epi = tab[mem[t]].tail.tail.head;
      double sums[NS], maxs[NM];
#pragma unroll
      for (int i = 0; i < NS; ++i) sums[i] = 0.;
#pragma unroll
      for (int i = 0; i < NM; ++i) maxs[i] = 0.;
      stream_rows(epi, pb, ra, re, r0, r1, tid, sums, maxs);
      stream_partials(epi, sums, maxs, b, nb, red, tid, sync);
      buf ^= 1;
    }
  } else {
    const double *xs[TILE];
    double acc[TILE];
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
      xs[t] = mem[t] >= 0 ? tab[mem[t]].tail.head : nullptr;
      acc[t] = 0.;
    }
    for (int k = p0 + tid; k < p1; k += kSpmvThreads) {
      const double a = A.val[k];
      const int col = A.col[k];
#pragma unroll
      for (int t = 0; t < TILE; ++t)
        if (xs[t]) acc[t] += a * xs[t][col];
    }
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
      if (mem[t] < 0) continue;
      const Epi epi = tab[mem[t]].tail.tail.head;
      double sums[NS], maxs[NM];
#pragma unroll
      for (int i = 0; i < NS; ++i) sums[i] = 0.;
#pragma unroll
      for (int i = 0; i < NM; ++i) maxs[i] = 0.;
      const double s = group_sum<kSpmvThreads>(acc[t], red, tid, sync);
      if (tid == 0) epi(r0, s, sums, maxs);
      stream_partials(epi, sums, maxs, b, nb, red, tid, sync);
    }
  }
}
template <class Epi, int TILE>
__global__ __launch_bounds__(kSpmvThreads) void k_spmv_stream_lanes(const SpmvRec<Epi> *tab, const int *list, int cnt) {
  d_spmv_stream_lanes<Epi, TILE>(tab, list, cnt);
}
// the lanes launch of a d_spmv_stream<Epi> table: gridDim.y = lane tiles over the first cnt entries of list
template <auto Fn, int Threads, class Epi>
inline void launch_lanes(const GTable<Fn, Threads, CsrView, const double *, Epi, const int *, int *> &t, const int *list, int cnt, int tile,
                         hipStream_t s) {
  static_assert(Threads == kSpmvThreads, "CSR-stream tables only");
  if (!t.used || cnt <= 0 || t.gx <= 0) return;
  const dim3 g((unsigned)t.gx, (unsigned)ceil_div(cnt, tile)), b(kSpmvThreads);
  if (tile == 8) hipLaunchKernelGGL((k_spmv_stream_lanes<Epi, 8>), g, b, 0, s, (const SpmvRec<Epi> *)t.dev.p, list, cnt);
  else hipLaunchKernelGGL((k_spmv_stream_lanes<Epi, 4>), g, b, 0, s, (const SpmvRec<Epi> *)t.dev.p, list, cnt);
}

}  // namespace scship
