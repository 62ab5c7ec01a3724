// measure_hull.hip -- the integer table behind the hull columns of stardist_amd.utils.measure_labels(hull=True): convex_area, solidity
// and feret_diameter_max are fixed functions of it and of the pixel count (label_ops.py).
//
//   sd_label_hull_device   hull[l] = {convex_area, F2} of every label 0 .. max_label of a 2D image
//
// What is computed per object is csrc/measure_hull.h's (shared with the host harness of the tests); this file is how the work is spread.
//   k_heights        a thread per label: the height of its box, and what an object too tall for LDS needs in global memory; two exclusive
//                    scans (hipcub) give every object its slice of the row table and of that workspace.  The two totals come to the host
//                    (one synchronisation) to size both.
//   k_row_extremes   a thread per pixel over the flat image: a pixel whose left neighbour in its row is not its label sends an integer
//                    atomicMin to the `first` of its (object, row) slot, one whose right neighbour is not its label an atomicMax to the
//                    `last`: coalesced label reads (the neighbours from cache), about two atomics per run of an object in a row, spread
//                    over as many addresses as there are object rows.  No workgroup walks a box, so an object as large as the image
//                    costs what a small one costs here.
//   k_object_hulls   a wave (a workgroup of 64) per object over its slice: lanes 0 and 1 build the left and the right chain of the hull,
//                    all lanes take rows for the convex image's intervals and add their lengths, lanes 0 and 1 build the chains of the
//                    intervals' hull, all lanes take vertices for the largest squared distance.  Up to MH_LDS_ROWS rows the row table,
//                    the intervals and the chains live in LDS (3.1 KB per wave), beyond that in the object's slice of the workspace,
//                    through the same code (generic pointers).
// Integer arithmetic only, integer min / max atomics: the table depends on the input alone.  Untuned: the chains are built by one lane
// each, one level after the other (an object of h rows: 2 h + 1 dependent steps, from global memory beyond the LDS tier); the pair loop
// is all pairs, not rotating calipers; k_row_extremes reads its two neighbours with loads of their own instead of shuffles.
#include "common.h"
#include "measure_hull.h"
#include "stardist_hip.h"
#include <hipcub/hipcub.hpp>

using namespace measure_hull;

namespace {

enum { BLOCK = 256, WAVE = 64, MAX_BLOCKS = 1 << 16, MAX_OBJECT_BLOCKS = 1 << 20 };

__device__ __forceinline__ int clamp_to(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sizes[l] = rows of the box of label l (0 for label 0, absent labels and the extra last entry), big[l] = its workspace beyond LDS
__global__ void __launch_bounds__(BLOCK) k_heights(const int* __restrict__ boxes, int Y, int max_label, long long* __restrict__ sizes,
                                                   long long* __restrict__ big) {
  const long long l = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (l > (long long)max_label + 1) return;
  int h = 0;
  if (l >= 1 && l <= max_label) {
    const int y0 = clamp_to(boxes[6 * l + 1], 0, Y), y1 = clamp_to(boxes[6 * l + 4], 0, Y);
    h = y1 > y0 ? y1 - y0 : 0;
  }
  sizes[l] = h;
  big[l] = h > MH_LDS_ROWS ? workspace_ints(h) : 0;
}

__global__ void __launch_bounds__(BLOCK) k_empty_rows(int* __restrict__ rows, long long n_rows) {
  const long long stride = (long long)gridDim.x * BLOCK;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n_rows; i += stride) {
    rows[2 * i] = INT_MAX;
    rows[2 * i + 1] = INT_MIN;
  }
}

__global__ void __launch_bounds__(BLOCK) k_row_extremes(const int* __restrict__ lbl, long long n, int Y, int X, int max_label,
                                                        const int* __restrict__ boxes, const long long* __restrict__ row_at,
                                                        int* __restrict__ rows) {
  const long long stride = (long long)gridDim.x * BLOCK;
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
    const int v = lbl[i];
    if (v < 1 || v > max_label) continue;
    const long long y = i / X;
    const int x = (int)(i - y * X);
    const bool starts = run_edge(v, x > 0, x > 0 ? lbl[i - 1] : 0), ends = run_edge(v, x + 1 < X, x + 1 < X ? lbl[i + 1] : 0);
    if (!starts && !ends) continue;
    const long long at = row_at[v], r = y - clamp_to(boxes[6ll * v + 1], 0, Y);
    if (r < 0 || r >= row_at[v + 1] - at) continue;                       // a box table that is not this image's: nothing is written
    if (starts) atomicMin(rows + 2 * (at + r), x);
    if (ends) atomicMax(rows + 2 * (at + r) + 1, x);
  }
}

__global__ void __launch_bounds__(WAVE) k_object_hulls(const int* __restrict__ boxes, int Y, int max_label, const long long* __restrict__ row_at,
                                                       const long long* __restrict__ big_at, const int* rows, int* work, long long* __restrict__ out) {
  __shared__ int s_rows[2 * MH_LDS_ROWS];
  __shared__ int s_iv[2 * MH_LDS_ROWS];
  __shared__ Pt s_chain[2][MH_LDS_CHAIN];
  const int lane = threadIdx.x;
  // l, h and every branch on them are the same for the 64 lanes, which are the whole workgroup: the barriers are uniform
  for (long long l = blockIdx.x; l <= max_label; l += gridDim.x) {
    const long long at = row_at[l];
    const int h = (int)(row_at[l + 1] - at);
    if (h <= 0) {
      if (lane < 2) out[2 * l + lane] = 0;
      continue;
    }
    const int y0 = clamp_to(boxes[6 * l + 1], 0, Y);
    const int* ext = rows + 2 * at;
    int* iv;
    Pt *left, *right;
    if (h <= MH_LDS_ROWS) {
      for (int k = lane; k < 2 * h; k += WAVE) s_rows[k] = ext[k];
      ext = s_rows;
      iv = s_iv;
      left = s_chain[0];
      right = s_chain[1];
    } else {
      int* w = work + big_at[l];
      iv = w;
      left = (Pt*)(w + 2ll * h);
      right = left + (2ll * h + 2);
    }
    __syncthreads();
    int n = 0;
    if (lane < 2) n = build_chain(ext, h, y0, lane ? 1 : -1, lane ? right : left);
    int nl = __shfl(n, 0), nr = __shfl(n, 1);
    __syncthreads();
    long long area = intervals_of(left, nl, right, nr, h, y0, iv, lane, WAVE);
    for (int o = WAVE / 2; o > 0; o >>= 1) area += __shfl_xor(area, o);
    __syncthreads();                                                     // the chains are read, the intervals written
    n = 0;
    if (lane < 2) n = build_chain(iv, h, y0, lane ? 1 : -1, lane ? right : left);
    nl = __shfl(n, 0);
    nr = __shfl(n, 1);
    __syncthreads();
    long long far = far_pairs(left, nl, right, nr, lane, WAVE);
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      const long long other = __shfl_xor(far, o);
      far = other > far ? other : far;
    }
    if (lane == 0) {
      out[2 * l] = area;
      out[2 * l + 1] = far;
    }
    __syncthreads();                                                     // the next object rewrites the LDS arrays
  }
}

int blocks_for(long long total, long long most) {
  const long long b = (total + BLOCK - 1) / BLOCK;
  return (int)(b < most ? (b > 0 ? b : 1) : most);
}

}  // namespace

extern "C" int sd_label_hull_device(const int32_t* d_lbl, int Y, int X, int max_label, const int32_t* d_boxes, int64_t* d_hull, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_label_hull";
  if (!d_lbl || !d_boxes || !d_hull || Y <= 0 || X <= 0 || max_label < 0) {
    sd::set_error("%s: null pointer, non-positive size or negative max_label", who);
    return -1;
  }
  if (Y >= MH_MAX_EXTENT || X >= MH_MAX_EXTENT || max_label > INT_MAX - 2) {
    sd::set_error("%s: an extent of 2^30 or more, or max_label beyond 2^31 - 3", who);
    return -1;
  }
  const long long n = (long long)Y * X;
  if (n > (1ll << 40)) { sd::set_error("%s: image too large", who); return -1; }
  if (max_label == 0) {
    SD_CHECK(hipMemsetAsync(d_hull, 0, 2 * sizeof(int64_t), s));
    return 0;
  }
  const int items = max_label + 2;                                       // one more than the labels: its offset is the total
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  long long* sizes = A.take_n<long long>(items);
  long long* big = A.take_n<long long>(items);
  long long* row_at = A.take_n<long long>(items);
  long long* big_at = A.take_n<long long>(items);
  size_t scan_bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, sizes, row_at, items, s);
  void* tmp = A.take(scan_bytes + 256);
  if (!sizes || !big || !row_at || !big_at || !tmp) return -1;
  hipLaunchKernelGGL(k_heights, dim3((unsigned)sd::div_up(items, BLOCK)), dim3(BLOCK), 0, s, (const int*)d_boxes, Y, max_label, sizes, big);
  SD_LAUNCH_CHECK();
  SD_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, scan_bytes, sizes, row_at, items, s));
  SD_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, scan_bytes, big, big_at, items, s));
  long long n_rows = 0, n_work = 0;
  SD_CHECK(hipMemcpyAsync(&n_rows, row_at + items - 1, sizeof(long long), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipMemcpyAsync(&n_work, big_at + items - 1, sizeof(long long), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  if (n_rows < 0 || n_work < 0 || n_rows > (1ll << 36) || n_work > (1ll << 38)) { sd::set_error("%s: the objects' boxes hold too many rows", who); return -1; }
  int* rows = A.take_n<int>(2 * (size_t)n_rows);
  int* work = A.take_n<int>((size_t)n_work);
  if (!rows || !work) return -1;
  if (n_rows > 0) {
    hipLaunchKernelGGL(k_empty_rows, dim3(blocks_for(n_rows, MAX_BLOCKS)), dim3(BLOCK), 0, s, rows, n_rows);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_row_extremes, dim3(blocks_for(n, MAX_BLOCKS)), dim3(BLOCK), 0, s, (const int*)d_lbl, n, Y, X, max_label, (const int*)d_boxes,
                       (const long long*)row_at, rows);
    SD_LAUNCH_CHECK();
  }
  const long long objects = (long long)max_label + 1;
  hipLaunchKernelGGL(k_object_hulls, dim3((unsigned)(objects < MAX_OBJECT_BLOCKS ? objects : MAX_OBJECT_BLOCKS)), dim3(WAVE), 0, s, (const int*)d_boxes, Y,
                     max_label, (const long long*)row_at, (const long long*)big_at, (const int*)rows, work, (long long*)d_hull);
  SD_LAUNCH_CHECK();
  return 0;
}
