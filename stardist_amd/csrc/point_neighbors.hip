// point_neighbors.hip -- the nearest points of every query, and the points within a radius, on the device
// (stardist_amd.utils.point_neighbors and the nearest= / within= columns of measure_labels).
//
//   sd_point_neighbors_device   mode 0: the k nearest points of every query; mode 1: the number of points within the radius;
//                               mode 2: their CSR lists, ascending by index within a row
//
// The per-query rules -- the cell of a coordinate, d2, the order (d2, index), the walk over rings of cells and the bound that ends it
// -- are csrc/point_neighbors.h's, shared with the host harness of the tests.  The phases of a call:
//   k_box        per-axis min / max of the points, one partial per workgroup, finished on the host: the call's one read-back besides
//                mode 2's total.  It sizes the grid (about two points per cell, or the caller's cell edge).
//   k_cells      the linear cell of every point (and, with a second point set, of every query, clamped into the grid)
//   radix sort   of (cell, index) over the bits the cell count needs: stable, so a cell's points ascend by index
//   k_gather     the points in sorted order, side by side
//   k_starts     the first slot of every cell, by a binary search in the sorted cells
//   k_search<M>  one lane per query, the queries taken in cell order so that the lanes of a wave read the same cells.  Mode 0 keeps a
//                lane's k best as (d2, index) in local memory, entry j of lane l at [j][l] (12 bytes x k x 64 lanes); mode 1 counts;
//                mode 2 runs after mode 1 and the 64-bit exclusive scan of its counts, writes a query's indices into its own slice,
//                sorts that slice in place (a heap sort by the lane) and then computes the d2 of each entry.  No atomics anywhere:
//                the same bits from call to call.
// Untuned: one lane walks its cells alone (a wave's lanes diverge where their cells hold different numbers of points), mode 2 walks
// the rings twice and sorts with uncoalesced accesses, the starts come from a search instead of a histogram.
#include "common.h"
#include "point_neighbors.h"
#include "stardist_hip.h"
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <algorithm>

using namespace point_neighbors;

namespace {

enum { BOX_THREADS = 256, BOX_BLOCKS = 128, MAX_CELLS = 1 << 27 };

// partial[b * 6 + a] = min of axis a over the block's points, partial[b * 6 + 3 + a] = max; NaN if any coordinate is NaN
__global__ void __launch_bounds__(BOX_THREADS) k_box(const double* __restrict__ pts, long long n, int nd, double* __restrict__ partial) {
  __shared__ double part[BOX_THREADS / 64][6];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool bad = false;
  for (long long i = (long long)blockIdx.x * BOX_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * BOX_THREADS)
    for (int a = 0; a < nd; ++a) {
      const double v = pts[i * nd + a];
      bad = bad || v != v;
      lo[a] = fmin(lo[a], v);
      hi[a] = fmax(hi[a], v);
    }
  for (int a = 0; a < 3; ++a) {
    if (bad) lo[a] = hi[a] = NAN;
    for (int s = 32; s > 0; s >>= 1) {
      const double l = __shfl_xor(lo[a], s), h = __shfl_xor(hi[a], s);
      lo[a] = (l != l || lo[a] != lo[a]) ? NAN : fmin(lo[a], l);
      hi[a] = (h != h || hi[a] != hi[a]) ? NAN : fmax(hi[a], h);
    }
  }
  const int wave = (int)threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; ++a) { part[wave][a] = lo[a]; part[wave][3 + a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = (int)threadIdx.x;
    double v = part[0][a];
    for (int w = 1; w < BOX_THREADS / 64; ++w) {
      const double o = part[w][a];
      v = (o != o || v != v) ? NAN : (a < 3 ? fmin(v, o) : fmax(v, o));
    }
    partial[blockIdx.x * 6 + a] = v;
  }
}

__global__ void k_cells(const double* __restrict__ pts, int n, Grid g, unsigned* __restrict__ keys, int* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int c[3];
  cell_of(g, pts + i * g.nd, c);
  keys[i] = (unsigned)linear_cell(g, c);
  vals[i] = (int)i;
}

__global__ void k_gather(const double* __restrict__ pts, const int* __restrict__ order, int n, int nd, double* __restrict__ sorted) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const long long i = order[s];
  for (int a = 0; a < nd; ++a) sorted[s * nd + a] = pts[i * nd + a];
}

// starts[c] = the first slot whose cell is >= c, for c = 0 .. cells (starts[cells] = n)
__global__ void k_starts(const unsigned* __restrict__ sorted_keys, int n, long long cells, int* __restrict__ starts) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > cells) return;
  int lo = 0, hi = n;                                                  // at most 32 halvings
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if ((long long)sorted_keys[mid] < c) lo = mid + 1; else hi = mid;
  }
  starts[c] = lo;
}

__global__ void k_fill_empty(long long items, int64_t* __restrict__ idx, double* __restrict__ d2) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= items) return;
  idx[i] = -1;
  d2[i] = INFINITY;
}

// a lane's list in local memory: entry j of lane l at d[j * PN_LANES + l], i[j * PN_LANES + l]
struct LaneStore {
  double* dd;
  int* ii;
  __device__ __forceinline__ double d(int j) const { return dd[j * PN_LANES]; }
  __device__ __forceinline__ int i(int j) const { return ii[j * PN_LANES]; }
  __device__ __forceinline__ void set(int j, double d_, int i_) { dd[j * PN_LANES] = d_; ii[j * PN_LANES] = i_; }
};

struct Search {
  Grid g;
  const int* starts;
  const double* sorted;        // the points in slot order
  const int* order;            // the index of the point in a slot
  const double* points;        // the points as given
  const double* queries;       // nullptr: the points are their own queries, and a query skips itself
  const int* qorder;           // the queries in cell order
  int m, k, use_radius;
  double r2;
};

enum { MODE_NEAREST = 0, MODE_COUNT = 1, MODE_LISTS = 2 };

template <int MODE>
__global__ void __launch_bounds__(PN_LANES) k_search(Search S, int64_t* __restrict__ out_idx, double* __restrict__ out_d2,
                                                    long long* __restrict__ counts, const int64_t* __restrict__ offsets) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const long long t = (long long)blockIdx.x * PN_LANES + threadIdx.x;
  if (t >= S.m) return;                                                // no barrier in this kernel
  const int qi = S.qorder[t];
  const int nd = S.g.nd;
  const double* q = (S.queries ? S.queries : S.points) + (long long)qi * nd;
  const int self = S.queries ? -1 : qi;
  if (MODE == MODE_NEAREST) {
    LaneStore st;
    st.dd = (double*)lds + threadIdx.x;
    st.ii = (int*)(lds + (size_t)S.k * PN_LANES * sizeof(double)) + threadIdx.x;
    Nearest<LaneStore> acc(st, S.k);
    search(S.g, S.starts, S.sorted, S.order, q, self, S.use_radius != 0, S.r2, acc);
    for (int j = 0; j < S.k; ++j) {
      const bool have = j < acc.count;
      out_idx[(long long)qi * S.k + j] = have ? st.i(j) : -1;
      out_d2[(long long)qi * S.k + j] = have ? st.d(j) : INFINITY;
    }
  } else if (MODE == MODE_COUNT) {
    Counter acc;
    search(S.g, S.starts, S.sorted, S.order, q, self, true, S.r2, acc);
    counts[qi] = acc.count;
  } else {
    const long long at = offsets[qi], len = offsets[qi + 1] - at;
    Appender acc(out_idx + at, len);
    search(S.g, S.starts, S.sorted, S.order, q, self, true, S.r2, acc);
    const long long have = acc.count < len ? acc.count : len;          // the count pass found the same number
    sort_ascending(out_idx + at, have);
    for (long long j = 0; j < have; ++j) out_d2[at + j] = squared_distance(q, S.points + out_idx[at + j] * nd, nd);
  }
}

int bits_for(long long cells) {
  int b = 1;
  while (b < 32 && (1ll << b) < cells) ++b;
  return b;
}

}  // namespace

extern "C" int sd_point_neighbors_device(const double* d_points, long long n, const double* d_queries, long long m, int nd, int mode, int k,
                                         int use_radius, double r2, double cell_size, long long cap, int64_t* d_indices, double* d_d2,
                                         int64_t* d_offsets, long long* h_total, double* h_cell, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_point_neighbors";
  if (h_total) *h_total = 0;
  if (h_cell) *h_cell = 0;
  if (nd != 2 && nd != 3) { sd::set_error("%s: points have 2 or 3 coordinates, got %d", who, nd); return -1; }
  if (mode < MODE_NEAREST || mode > MODE_LISTS) { sd::set_error("%s: mode outside 0 .. 2", who); return -1; }
  if (n < 0 || m < 0 || n > INT_MAX - 1 || m > INT_MAX - 1) { sd::set_error("%s: n and m must be in 0 .. 2^31 - 2", who); return -1; }
  if (!d_queries && m != n) { sd::set_error("%s: without queries m must be n", who); return -1; }
  if (mode == MODE_NEAREST && (k < 1 || k > PN_MAX_K)) { sd::set_error("%s: k outside 1 .. %d", who, (int)PN_MAX_K); return -1; }
  if (mode != MODE_NEAREST && !use_radius) { sd::set_error("%s: modes 1 and 2 need a radius", who); return -1; }
  if (use_radius && !(r2 >= 0)) { sd::set_error("%s: the squared radius must be >= 0", who); return -1; }
  if (!(cell_size == 0 || (cell_size >= PN_MIN_CELL && cell_size <= PN_MAX_CELL))) {
    sd::set_error("%s: the cell size must be 0 (automatic) or in [2^-500, 2^500]", who);
    return -1;
  }
  if (cap < 0) { sd::set_error("%s: negative capacity", who); return -1; }
  if (mode == MODE_NEAREST && m > 0 && (!d_indices || !d_d2)) { sd::set_error("%s: null output", who); return -1; }
  if (mode == MODE_COUNT && m > 0 && !d_offsets) { sd::set_error("%s: null output", who); return -1; }
  if (mode == MODE_LISTS && (!d_offsets || !h_total || (cap > 0 && (!d_indices || !d_d2)))) { sd::set_error("%s: null output", who); return -1; }
  if ((n > 0 && !d_points)) { sd::set_error("%s: null points", who); return -1; }
  if (m == 0 || n == 0) {                                              // nothing to find
    if (mode == MODE_NEAREST && m > 0) {
      const long long items = m * k;
      hipLaunchKernelGGL(k_fill_empty, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, items, d_indices, d_d2);
      SD_LAUNCH_CHECK();
    } else if (mode == MODE_COUNT && m > 0) {
      SD_CHECK(hipMemsetAsync(d_offsets, 0, (size_t)m * sizeof(int64_t), s));
    } else if (mode == MODE_LISTS) {
      SD_CHECK(hipMemsetAsync(d_offsets, 0, (size_t)(m + 1) * sizeof(int64_t), s));
    }
    return 0;
  }
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;

  // the box
  const int box_blocks = (int)std::min<long long>(BOX_BLOCKS, (n + BOX_THREADS - 1) / BOX_THREADS);
  double* d_partial = A.take_n<double>((size_t)BOX_BLOCKS * 6);
  if (!d_partial) return -1;
  hipLaunchKernelGGL(k_box, dim3(box_blocks), dim3(BOX_THREADS), 0, s, d_points, n, nd, d_partial);
  SD_LAUNCH_CHECK();
  double partial[BOX_BLOCKS * 6];
  SD_CHECK(hipMemcpyAsync(partial, d_partial, (size_t)box_blocks * 6 * sizeof(double), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  Grid g;
  g.nd = nd;
  const int shift = 3 - nd;
  double extent[3] = {0, 0, 0};
  g.lo[0] = 0;
  g.dim[0] = 1;
  for (int a = 0; a < nd; ++a) {
    double lo = partial[a], hi = partial[3 + a];
    for (int b = 1; b < box_blocks; ++b) {
      const double l = partial[b * 6 + a], h = partial[b * 6 + 3 + a];
      lo = (l != l || lo != lo) ? NAN : std::min(lo, l);
      hi = (h != h || hi != hi) ? NAN : std::max(hi, h);
    }
    if (!(lo > -PN_MAX_COORD && hi < PN_MAX_COORD)) {                  // NaN fails both
      sd::set_error("%s: a coordinate of the points is not finite or not below 2^500 in magnitude", who);
      return -1;
    }
    g.lo[a + shift] = lo;
    extent[a + shift] = hi - lo;
  }
  g.h = cell_size > 0 ? cell_size : automatic_cell(extent, n);
  g.inv_h = 1.0 / g.h;
  long long cells = 1;
  for (int a = 0; a < 3; ++a) {
    g.dim[a] = cells_along(extent[a], g.h);
    if (g.dim[a] > PN_MAX_DIM) { sd::set_error("%s: more than 2^21 cells along an axis (cell size %g)", who, g.h); return -1; }
    cells *= g.dim[a];
    if (cells > MAX_CELLS) { sd::set_error("%s: more than 2^27 cells (cell size %g)", who, g.h); return -1; }
  }
  if (h_cell) *h_cell = g.h;

  // the points by cell
  const int N = (int)n, M = (int)m;
  const int end_bit = bits_for(cells);
  unsigned* k0 = A.take_n<unsigned>(std::max(N, M));
  unsigned* k1 = A.take_n<unsigned>(std::max(N, M));
  int* v0 = A.take_n<int>(std::max(N, M));
  int* order = A.take_n<int>(N);
  int* qorder = d_queries ? A.take_n<int>(M) : order;
  double* sorted = A.take_n<double>((size_t)N * nd);
  int* starts = A.take_n<int>((size_t)cells + 1);
  long long* counts = mode == MODE_LISTS ? A.take_n<long long>((size_t)M + 1) : nullptr;
  size_t sort_bytes = 0, sort_bytes_q = 0, scan_bytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, k0, k1, v0, order, N, 0, end_bit, s);
  if (d_queries) (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes_q, k0, k1, v0, qorder, M, 0, end_bit, s);
  if (mode == MODE_LISTS) (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, counts, (long long*)d_offsets, M + 1, s);
  void* tmp = A.take(std::max(std::max(sort_bytes, sort_bytes_q), scan_bytes) + 256);
  if (!k0 || !k1 || !v0 || !order || !qorder || !sorted || !starts || !tmp || (mode == MODE_LISTS && !counts)) return -1;
  hipLaunchKernelGGL(k_cells, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, d_points, N, g, k0, v0);
  SD_LAUNCH_CHECK();
  SD_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, k0, k1, v0, order, N, 0, end_bit, s));
  hipLaunchKernelGGL(k_gather, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, d_points, (const int*)order, N, nd, sorted);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_starts, dim3((unsigned)((cells + 1 + 255) / 256)), dim3(256), 0, s, (const unsigned*)k1, N, cells, starts);
  SD_LAUNCH_CHECK();
  if (d_queries) {                                                     // the queries in cell order (k1 is free again: the starts are queued)
    hipLaunchKernelGGL(k_cells, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, d_queries, M, g, k0, v0);
    SD_LAUNCH_CHECK();
    SD_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes_q, k0, k1, v0, qorder, M, 0, end_bit, s));
  }

  Search S;
  S.g = g; S.starts = starts; S.sorted = sorted; S.order = order; S.points = d_points; S.queries = d_queries; S.qorder = qorder;
  S.m = M; S.k = k; S.use_radius = use_radius ? 1 : 0; S.r2 = r2;
  const dim3 grid((unsigned)((M + PN_LANES - 1) / PN_LANES)), block(PN_LANES);
  if (mode == MODE_NEAREST) {
    const size_t lds = (size_t)k * PN_LANES * (sizeof(double) + sizeof(int));       // <= 48 KiB
    hipLaunchKernelGGL(k_search<MODE_NEAREST>, grid, block, lds, s, S, d_indices, d_d2, (long long*)nullptr, (const int64_t*)nullptr);
    SD_LAUNCH_CHECK();
    return 0;
  }
  if (mode == MODE_COUNT) {
    hipLaunchKernelGGL(k_search<MODE_COUNT>, grid, block, 0, s, S, (int64_t*)nullptr, (double*)nullptr, (long long*)d_offsets, (const int64_t*)nullptr);
    SD_LAUNCH_CHECK();
    return 0;
  }
  SD_CHECK(hipMemsetAsync(counts + M, 0, sizeof(long long), s));
  hipLaunchKernelGGL(k_search<MODE_COUNT>, grid, block, 0, s, S, (int64_t*)nullptr, (double*)nullptr, counts, (const int64_t*)nullptr);
  SD_LAUNCH_CHECK();
  SD_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, scan_bytes, counts, (long long*)d_offsets, M + 1, s));
  long long total = 0;
  SD_CHECK(hipMemcpyAsync(&total, d_offsets + M, sizeof(total), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  *h_total = total;
  if (total == 0 || total > cap) return 0;                             // the caller comes again with room for all
  hipLaunchKernelGGL(k_search<MODE_LISTS>, grid, block, 0, s, S, d_indices, d_d2, (long long*)nullptr, (const int64_t*)d_offsets);
  SD_LAUNCH_CHECK();
  return 0;
}
