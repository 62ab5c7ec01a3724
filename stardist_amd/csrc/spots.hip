// spots.hip -- spot detection on the device (stardist_amd.spots).
//
//   sd_gaussian_filter_device   scipy.ndimage.gaussian_filter(mode="reflect") bit for bit: one pass per axis that is not skipped
//   sd_peak_local_max_device    the local peaks of an image as sorted 64-bit keys (-value, raster index), cut per label and in all
//   sd_peaks_emit_device        coordinates, values and labels of those keys
//
// The per-element rules -- the reflected index, one output element of a line, the window test of a peak, the key -- are csrc/spots.h's,
// shared with the host harness of the tests.
//
// Gaussian: a pass sees the image as (outer, n, inner), n the axis it runs along.  A workgroup takes a tile of 1024 x 1 (the last axis,
// inner = 1) or 32 x 64 (any other axis: 64 contiguous elements wide), so a wave reads and writes 64 neighbouring elements in every
// pass.  The tile with its halo of r lines goes to LDS as float (uint8 and uint16 convert exactly) where it takes at most 48 KiB --
// always along the last axis, up to r = 80 along another -- and is read from global memory by the same code beyond.  Accumulation is
// in double, the weights come from a table the caller computed.  Passes alternate between `out` and `work`, ending in `out`.
//
// Peaks: k_minmax reduces the non-NaN pixels to their least and greatest order-preserving key with integer atomics, k_threshold turns
// that into the threshold in device memory (no read-back).  k_peaks takes one tile per workgroup (1 x 16 x 64, 3D 4 x 4 x 64), its halo
// of d in LDS where that fits in 48 KiB, else the window is read from global memory by the same code; a pixel tests threshold, border
// and label, then its 3^nd neighbourhood, then its window.  Peaks are appended with one atomic per wave; the total comes to the host
// (the call's one synchronisation without a per-label cap), a radix sort of the keys makes the append order irrelevant.  The per-label
// cap is a stable sort of the peaks' labels, the rank inside a label from the segment's start, and a select; it reads its count back.
// Untuned: the halo of a 3D tile is large next to the tile, the label sort always runs over 31 bits, every tile is launched even
// where the threshold leaves nothing.
#include "common.h"
#include "spots.h"
#include "stardist_hip.h"
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <math.h>

using namespace spots;

namespace {

// ------------------------------------------------------------------------------------------------------------------ Gaussian
struct GaussPass {
  long long outer, n, inner, tiles_a, tiles_i;
  int tile_a, tile_i, r;
  const double* w;
};

template <typename T>
struct GlobalLine {
  const T* base;
  long long a, n, inner, i;
  __device__ __forceinline__ double operator()(int j) const { return (double)(float)base[reflect_index(a + j, n) * inner + i]; }
};
struct TileLine {
  const float* centre;
  int stride;
  __device__ __forceinline__ double operator()(int j) const { return (double)centre[j * stride]; }
};

template <typename T, bool LDS>
__global__ void __launch_bounds__(THREADS) k_gauss(const T* __restrict__ in, float* __restrict__ out, GaussPass P) {
  extern __shared__ float tile[];
  long long b = blockIdx.x;
  const long long ti = b % P.tiles_i;
  b /= P.tiles_i;
  const long long ta = b % P.tiles_a, o = b / P.tiles_a;
  const long long a0 = ta * P.tile_a, i0 = ti * P.tile_i;
  const int rows = (int)(P.n - a0 < P.tile_a ? P.n - a0 : P.tile_a);
  const T* base = in + o * P.n * P.inner;
  if (LDS) {
    const int cells = (rows + 2 * P.r) * P.tile_i;
    for (int e = (int)threadIdx.x; e < cells; e += THREADS) {
      const int ra = e / P.tile_i, li = e % P.tile_i;
      if (i0 + li < P.inner) tile[e] = (float)base[reflect_index(a0 - P.r + ra, P.n) * P.inner + i0 + li];
    }
    __syncthreads();
  }
  const int cells = rows * P.tile_i;
  for (int e = (int)threadIdx.x; e < cells; e += THREADS) {
    const int la = e / P.tile_i, li = e % P.tile_i;
    const long long a = a0 + la, i = i0 + li;
    if (i >= P.inner) continue;
    float res;
    if (LDS) {
      const TileLine at = {tile + (la + P.r) * P.tile_i + li, P.tile_i};
      res = gauss_point(at, P.r, P.w);
    } else {
      const GlobalLine<T> at = {base, a, P.n, P.inner, i};
      res = gauss_point(at, P.r, P.w);
    }
    out[(o * P.n + a) * P.inner + i] = res;
  }
}

template <typename T>
__global__ void k_cast(const T* __restrict__ in, float* __restrict__ out, long long count) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = (float)in[i];
}

template <typename T>
int gauss_pass(const T* in, float* out, GaussPass P, hipStream_t s) {
  const bool last = P.inner == 1;
  P.tile_a = last ? G_LAST_A : G_INNER_A;
  P.tile_i = last ? 1 : G_INNER_I;
  P.tiles_a = (P.n + P.tile_a - 1) / P.tile_a;
  P.tiles_i = (P.inner + P.tile_i - 1) / P.tile_i;
  const double blocks = (double)P.outer * (double)P.tiles_a * (double)P.tiles_i;
  if (blocks > 2147483647.0) { sd::set_error("sd_gaussian_filter: more than 2^31 - 1 tiles in a pass"); return -1; }
  const dim3 grid((unsigned)(P.outer * P.tiles_a * P.tiles_i)), block(THREADS);
  if (gauss_tile_fits(P.tile_a, P.tile_i, P.r)) {
    const size_t lds = (size_t)(P.tile_a + 2 * P.r) * P.tile_i * sizeof(float);
    hipLaunchKernelGGL((k_gauss<T, true>), grid, block, lds, s, in, out, P);
  } else {
    hipLaunchKernelGGL((k_gauss<T, false>), grid, block, 0, s, in, out, P);
  }
  SD_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int gaussian(const T* in, const long long n[3], const int r[3], const double* d_w, float* out, float* work, hipStream_t s) {
  int passes = 0, done = 0;
  for (int a = 0; a < 3; ++a) passes += r[a] >= 0;
  const long long count = n[0] * n[1] * n[2];
  if (passes == 0) {
    hipLaunchKernelGGL(k_cast<T>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, in, out, count);
    SD_LAUNCH_CHECK();
    return 0;
  }
  const float* src = nullptr;
  const double* w = d_w;
  for (int a = 0; a < 3; ++a) {
    if (r[a] < 0) continue;
    GaussPass P;
    P.outer = a == 0 ? 1 : a == 1 ? n[0] : n[0] * n[1];
    P.n = n[a];
    P.inner = a == 0 ? n[1] * n[2] : a == 1 ? n[2] : 1;
    P.r = r[a];
    P.w = w;
    float* dst = ((passes - done) & 1) ? out : work;                     // the last pass writes `out`
    if (done == 0 ? gauss_pass<T>(in, dst, P, s) : gauss_pass<float>(src, dst, P, s)) return -1;
    src = dst;
    w += 2 * r[a] + 1;
    ++done;
  }
  return 0;
}

// --------------------------------------------------------------------------------------------------------------------- peaks
struct PeakArgs {
  long long n[3], tiles[3], b[3];
  int d[3], t[3];
  const int* labels;
  const double* thr;
  unsigned long long cap;
};

// an integer that orders like the value, -0.0 on +0.0: the least and greatest over the non-NaN pixels; lohi = {0xffffffff, 0} before
template <typename T>
__global__ void __launch_bounds__(THREADS) k_minmax(const T* __restrict__ in, long long count, unsigned* __restrict__ lohi) {
  __shared__ unsigned part[2];
  if (threadIdx.x == 0) { part[0] = 0xffffffffu; part[1] = 0u; }
  __syncthreads();
  unsigned lo = 0xffffffffu, hi = 0u;
  for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < count; i += (long long)gridDim.x * THREADS) {
    const T v = in[i];
    if (is_nan(v)) continue;
    const unsigned k = value_key(v);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
  if (lo <= hi) { atomicMin(&part[0], lo); atomicMax(&part[1], hi); }
  __syncthreads();
  if (threadIdx.x == 0 && part[0] <= part[1]) { atomicMin(&lohi[0], part[0]); atomicMax(&lohi[1], part[1]); }
}

__device__ double value_of_key(unsigned k, int dtype) {
  if (dtype != DT_F32) return (double)k;
  const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float v;
  memcpy(&v, &u, 4);
  return (double)v;
}

// thr = threshold_abs, else the least value; with threshold_rel the larger of that and fl64(threshold_rel * greatest value); +inf
// (no pixel passes) where every pixel is NaN
__global__ void k_threshold(const unsigned* __restrict__ lohi, int dtype, int has_abs, double t_abs, int has_rel, double t_rel,
                            double* __restrict__ thr) {
  if (lohi[0] > lohi[1]) { *thr = INFINITY; return; }
  double t = has_abs ? t_abs : value_of_key(lohi[0], dtype);
  if (has_rel) {
    const double rel = t_rel * value_of_key(lohi[1], dtype);
    t = rel > t ? rel : t;
  }
  *thr = t;
}

template <typename T>
struct GlobalImg {
  const T* in;
  const int* labels;
  long long n1, n2;
  __device__ __forceinline__ float value(long long z, long long y, long long x) const { return (float)in[(z * n1 + y) * n2 + x]; }
  __device__ __forceinline__ int label(long long z, long long y, long long x) const { return labels[(z * n1 + y) * n2 + x]; }
};
struct TileImg {
  const float* tile;
  const int* labels;
  long long n1, n2, z0, y0, x0;      // the image position of tile[0]
  int e1, e2;
  __device__ __forceinline__ float value(long long z, long long y, long long x) const {
    return tile[((int)(z - z0) * e1 + (int)(y - y0)) * e2 + (int)(x - x0)];
  }
  __device__ __forceinline__ int label(long long z, long long y, long long x) const { return labels[(z * n1 + y) * n2 + x]; }
};

template <typename T, bool LDS>
__global__ void __launch_bounds__(THREADS) k_peaks(const T* __restrict__ in, PeakArgs A, unsigned long long* __restrict__ counter,
                                                   uint64_t* __restrict__ keys) {
  extern __shared__ float tile[];
  long long b = blockIdx.x;
  const long long tx = b % A.tiles[2];
  b /= A.tiles[2];
  const long long ty = b % A.tiles[1], tz = b / A.tiles[1];
  const long long o[3] = {tz * A.t[0], ty * A.t[1], tx * A.t[2]};
  const int e[3] = {A.t[0] + 2 * A.d[0], A.t[1] + 2 * A.d[1], A.t[2] + 2 * A.d[2]};
  if (LDS) {
    const int cells = e[0] * e[1] * e[2];
    for (int s = (int)threadIdx.x; s < cells; s += THREADS) {
      const long long z = o[0] - A.d[0] + s / (e[1] * e[2]), y = o[1] - A.d[1] + s / e[2] % e[1], x = o[2] - A.d[2] + s % e[2];
      if (z >= 0 && z < A.n[0] && y >= 0 && y < A.n[1] && x >= 0 && x < A.n[2]) tile[s] = (float)in[(z * A.n[1] + y) * A.n[2] + x];
    }
    __syncthreads();
  }
  const double thr = *A.thr;
  const bool use_labels = A.labels != nullptr;
  const int cells = A.t[0] * A.t[1] * A.t[2];                            // a multiple of THREADS: every lane makes every trip
  for (int s = (int)threadIdx.x; s < cells; s += THREADS) {
    const long long z = o[0] + s / (A.t[1] * A.t[2]), y = o[1] + s / A.t[2] % A.t[1], x = o[2] + s % A.t[2];
    bool peak = false;
    uint64_t key = 0;
    if (z < A.n[0] && y < A.n[1] && x < A.n[2]) {
      const long long idx = (z * A.n[1] + y) * A.n[2] + x;
      const T v = in[idx];
      const int lab = use_labels ? A.labels[idx] : 1;
      peak = !is_nan(v) && (double)v > thr && lab != 0 && z >= A.b[0] && z < A.n[0] - A.b[0] && y >= A.b[1] && y < A.n[1] - A.b[1] &&
             x >= A.b[2] && x < A.n[2] - A.b[2];
      if (peak) {
        if (LDS) {
          const TileImg img = {tile, A.labels, A.n[1], A.n[2], o[0] - A.d[0], o[1] - A.d[1], o[2] - A.d[2], e[1], e[2]};
          peak = !is_beaten(img, A.n, A.d, z, y, x, (float)v, use_labels, lab);
        } else {
          const GlobalImg<T> img = {in, A.labels, A.n[1], A.n[2]};
          peak = !is_beaten(img, A.n, A.d, z, y, x, (float)v, use_labels, lab);
        }
        key = peak_key(v, (uint32_t)idx);
      }
    }
    // one atomic per wave: the first lane with a peak reserves the wave's slots
    const unsigned long long mask = __ballot(peak);
    if (mask) {
      const int lane = (int)(threadIdx.x & 63), leader = __ffsll((long long)mask) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
      base = __shfl(base, leader);
      const unsigned long long at = base + __popcll(mask & ((1ull << lane) - 1ull));
      if (peak && at < A.cap) keys[at] = key;
    }
  }
}

__global__ void k_key_labels(const uint64_t* __restrict__ keys, int count, const int* __restrict__ labels, unsigned* __restrict__ lab,
                             int* __restrict__ pos) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= count) return;
  lab[i] = (unsigned)labels[keys[i] & 0xffffffffull];
  pos[i] = i;
}

// keep[pos[j]] = whether slot j is among the first `per_label` of its label: its rank is j - the first slot of the label
__global__ void k_label_rank(const unsigned* __restrict__ lab, const int* __restrict__ pos, int count, long long per_label,
                             unsigned char* __restrict__ keep) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= count) return;
  const unsigned mine = lab[j];
  int lo = 0, hi = j;                                                     // at most 31 halvings
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (lab[mid] < mine) lo = mid + 1; else hi = mid;
  }
  keep[pos[j]] = (long long)(j - lo) < per_label ? 1 : 0;
}

template <typename T>
__global__ void k_emit(const T* __restrict__ in, const int* __restrict__ labels, const uint64_t* __restrict__ keys, long long count,
                       int nd, long long n1, long long n2, int64_t* __restrict__ coords, T* __restrict__ values, int* __restrict__ out_labels) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const long long idx = (long long)(keys[i] & 0xffffffffull);
  const long long x = idx % n2, y = idx / n2 % n1, z = idx / n2 / n1;
  int64_t* c = coords + i * nd;
  if (nd == 3) c[0] = z;
  c[nd - 2] = y;
  c[nd - 1] = x;
  values[i] = in[idx];
  out_labels[i] = labels ? labels[idx] : 0;
}

template <typename T>
int find_peaks(const T* in, int dtype, PeakArgs A, int has_abs, double t_abs, int has_rel, double t_rel, long long per_label,
               long long num_peaks, uint64_t* d_keys, long long* h_count, hipStream_t s) {
  sd::Arena& R = sd::arena();
  if (R.begin(s)) return -1;
  const long long count = A.n[0] * A.n[1] * A.n[2];
  unsigned* lohi = R.take_n<unsigned>(2);
  double* thr = R.take_n<double>(1);
  unsigned long long* counter = R.take_n<unsigned long long>(1);
  if (!lohi || !thr || !counter) return -1;
  const unsigned init[2] = {0xffffffffu, 0u};
  SD_CHECK(hipMemcpyAsync(lohi, init, sizeof(init), hipMemcpyHostToDevice, s));
  SD_CHECK(hipMemsetAsync(counter, 0, sizeof(*counter), s));
  if (!has_abs || has_rel) {
    const long long blocks = (count + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(k_minmax<T>, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(THREADS), 0, s, in, count, lohi);
    SD_LAUNCH_CHECK();
  } else {                                                               // the threshold is the caller's: nothing to reduce
    SD_CHECK(hipMemsetAsync(lohi, 0, 2 * sizeof(unsigned), s));
  }
  hipLaunchKernelGGL(k_threshold, dim3(1), dim3(1), 0, s, (const unsigned*)lohi, dtype, has_abs, t_abs, has_rel, t_rel, thr);
  SD_LAUNCH_CHECK();
  A.thr = thr;
  const bool is3d = A.n[0] > 1;
  peak_tile(is3d, A.t);
  double blocks = 1;
  for (int a = 0; a < 3; ++a) {
    A.tiles[a] = (A.n[a] + A.t[a] - 1) / A.t[a];
    blocks *= (double)A.tiles[a];
  }
  if (blocks > 2147483647.0) { sd::set_error("sd_peak_local_max: more than 2^31 - 1 tiles"); return -1; }
  const dim3 grid((unsigned)(A.tiles[0] * A.tiles[1] * A.tiles[2])), block(THREADS);
  if (peak_tile_fits(is3d, A.d)) {
    const size_t lds = (size_t)(A.t[0] + 2 * A.d[0]) * (A.t[1] + 2 * A.d[1]) * (A.t[2] + 2 * A.d[2]) * sizeof(float);
    hipLaunchKernelGGL((k_peaks<T, true>), grid, block, lds, s, in, A, counter, d_keys);
  } else {
    hipLaunchKernelGGL((k_peaks<T, false>), grid, block, 0, s, in, A, counter, d_keys);
  }
  SD_LAUNCH_CHECK();
  unsigned long long total = 0;
  SD_CHECK(hipMemcpyAsync(&total, counter, sizeof(total), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  h_count[0] = (long long)total;
  h_count[1] = -1;
  if (total > A.cap) return 0;                                           // the caller comes again with room for all
  if (total > (unsigned long long)INT_MAX - 1) { sd::set_error("sd_peak_local_max: more than 2^31 - 2 peaks"); return -1; }
  if (total == 0 || num_peaks == 0) { h_count[1] = 0; return 0; }
  const int M = (int)total;
  uint64_t* sorted = R.take_n<uint64_t>(M);
  size_t sort_bytes = 0, pair_bytes = 0, select_bytes = 0;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, d_keys, sorted, M, 0, 64, s);
  unsigned *lab = nullptr, *lab_sorted = nullptr;
  int *pos = nullptr, *pos_sorted = nullptr, *selected = nullptr;
  unsigned char* keep = nullptr;
  const bool cut = per_label >= 0 && A.labels != nullptr;
  if (cut) {
    lab = R.take_n<unsigned>(M); lab_sorted = R.take_n<unsigned>(M);
    pos = R.take_n<int>(M); pos_sorted = R.take_n<int>(M);
    keep = R.take_n<unsigned char>(M); selected = R.take_n<int>(1);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, pair_bytes, lab, lab_sorted, pos, pos_sorted, M, 0, 31, s);
    (void)hipcub::DeviceSelect::Flagged(nullptr, select_bytes, sorted, keep, d_keys, selected, M, s);
    if (!lab || !lab_sorted || !pos || !pos_sorted || !keep || !selected) return -1;
  }
  size_t tmp_bytes = sort_bytes > pair_bytes ? sort_bytes : pair_bytes;
  tmp_bytes = tmp_bytes > select_bytes ? tmp_bytes : select_bytes;
  void* tmp = R.take(tmp_bytes + 256);
  if (!sorted || !tmp) return -1;
  SD_CHECK(hipcub::DeviceRadixSort::SortKeys(tmp, sort_bytes, d_keys, sorted, M, 0, 64, s));
  long long kept = M;
  if (cut) {
    const dim3 g((unsigned)((M + 255) / 256)), t(256);
    hipLaunchKernelGGL(k_key_labels, g, t, 0, s, (const uint64_t*)sorted, M, A.labels, lab, pos);
    SD_LAUNCH_CHECK();
    SD_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, pair_bytes, lab, lab_sorted, pos, pos_sorted, M, 0, 31, s));
    hipLaunchKernelGGL(k_label_rank, g, t, 0, s, (const unsigned*)lab_sorted, (const int*)pos_sorted, M, per_label, keep);
    SD_LAUNCH_CHECK();
    SD_CHECK(hipcub::DeviceSelect::Flagged(tmp, select_bytes, sorted, keep, d_keys, selected, M, s));
    int n_selected = 0;
    SD_CHECK(hipMemcpyAsync(&n_selected, selected, sizeof(int), hipMemcpyDeviceToHost, s));
    SD_CHECK(hipStreamSynchronize(s));
    kept = n_selected;
  } else {
    SD_CHECK(hipMemcpyAsync(d_keys, sorted, (size_t)M * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  }
  h_count[1] = num_peaks >= 0 && num_peaks < kept ? num_peaks : kept;
  return 0;
}

bool bad_image(const char* who, const void* in, int dtype, int nd, long long n0, long long n1, long long n2) {
  if (!in) { sd::set_error("%s: null image", who); return true; }
  if (nd != 2 && nd != 3) { sd::set_error("%s: images are 2D or 3D, got %d axes", who, nd); return true; }
  if (dtype < DT_U8 || dtype > DT_F32) { sd::set_error("%s: dtype code outside 0 .. 2", who); return true; }
  if (n0 < 1 || n1 < 1 || n2 < 1 || (nd == 2 && n0 != 1)) { sd::set_error("%s: an extent below 1 (a 2D image has n0 = 1)", who); return true; }
  if ((double)n0 * (double)n1 * (double)n2 > 4294967295.0) { sd::set_error("%s: more than 2^32 - 1 pixels", who); return true; }
  return false;
}

}  // namespace

extern "C" int sd_gaussian_filter_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2,
                                         const int* h_radius, const double* d_weights, float* d_out, float* d_work, void* stream) {
  const char* who = "sd_gaussian_filter";
  if (bad_image(who, d_in, dtype, nd, n0, n1, n2)) return -1;
  if (!h_radius || !d_out) { sd::set_error("%s: null pointer", who); return -1; }
  int passes = 0;
  for (int a = 0; a < 3; ++a) {
    if (h_radius[a] > MAX_RADIUS) { sd::set_error("%s: a radius beyond %d", who, (int)MAX_RADIUS); return -1; }
    passes += h_radius[a] >= 0;
  }
  if (passes > 0 && !d_weights) { sd::set_error("%s: null weights", who); return -1; }
  if (passes > 1 && !d_work) { sd::set_error("%s: more than one pass needs the work buffer", who); return -1; }
  const long long n[3] = {n0, n1, n2};
  const int r[3] = {h_radius[0], h_radius[1], h_radius[2]};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == DT_U8) return gaussian((const uint8_t*)d_in, n, r, d_weights, d_out, d_work, s);
  if (dtype == DT_U16) return gaussian((const uint16_t*)d_in, n, r, d_weights, d_out, d_work, s);
  return gaussian((const float*)d_in, n, r, d_weights, d_out, d_work, s);
}

extern "C" int sd_peak_local_max_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2, const int32_t* d_labels,
                                        const int* h_distance, const long long* h_border, int has_abs, double threshold_abs, int has_rel,
                                        double threshold_rel, long long per_label, long long num_peaks, long long cap, uint64_t* d_keys,
                                        long long* h_count, void* stream) {
  const char* who = "sd_peak_local_max";
  if (bad_image(who, d_in, dtype, nd, n0, n1, n2)) return -1;
  if (!h_distance || !h_border || !h_count || cap < 0 || (cap > 0 && !d_keys)) { sd::set_error("%s: null pointer or negative capacity", who); return -1; }
  PeakArgs A;
  A.n[0] = n0; A.n[1] = n1; A.n[2] = n2;
  for (int a = 0; a < 3; ++a) {
    if (h_distance[a] < 0 || h_distance[a] > PEAK_MAX_DISTANCE) { sd::set_error("%s: a distance outside 0 .. 2^20", who); return -1; }
    if (h_border[a] < 0) { sd::set_error("%s: a negative border", who); return -1; }
    A.d[a] = h_distance[a];
    A.b[a] = h_border[a] < A.n[a] ? h_border[a] : A.n[a];                 // a border of the whole axis and more leaves nothing either way
  }
  if (has_abs && threshold_abs != threshold_abs) { sd::set_error("%s: the threshold is NaN", who); return -1; }
  if (has_rel && threshold_rel != threshold_rel) { sd::set_error("%s: the relative threshold is NaN", who); return -1; }
  A.labels = d_labels;
  A.thr = nullptr;
  A.cap = (unsigned long long)cap;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == DT_U8) return find_peaks((const uint8_t*)d_in, dtype, A, has_abs, threshold_abs, has_rel, threshold_rel, per_label, num_peaks, d_keys, h_count, s);
  if (dtype == DT_U16) return find_peaks((const uint16_t*)d_in, dtype, A, has_abs, threshold_abs, has_rel, threshold_rel, per_label, num_peaks, d_keys, h_count, s);
  return find_peaks((const float*)d_in, dtype, A, has_abs, threshold_abs, has_rel, threshold_rel, per_label, num_peaks, d_keys, h_count, s);
}

extern "C" int sd_peaks_emit_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2, const int32_t* d_labels,
                                    const uint64_t* d_keys, long long count, int64_t* d_coords, void* d_values, int32_t* d_out_labels,
                                    void* stream) {
  const char* who = "sd_peaks_emit";
  if (bad_image(who, d_in, dtype, nd, n0, n1, n2)) return -1;
  if (count < 0 || count > 4294967295ll) { sd::set_error("%s: count outside 0 .. 2^32 - 1", who); return -1; }
  if (count == 0) return 0;
  if (!d_keys || !d_coords || !d_values || !d_out_labels) { sd::set_error("%s: null pointer", who); return -1; }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((count + 255) / 256)), block(256);
  if (dtype == DT_U8) hipLaunchKernelGGL(k_emit<uint8_t>, grid, block, 0, s, (const uint8_t*)d_in, d_labels, d_keys, count, nd, n1, n2, d_coords, (uint8_t*)d_values, d_out_labels);
  else if (dtype == DT_U16) hipLaunchKernelGGL(k_emit<uint16_t>, grid, block, 0, s, (const uint16_t*)d_in, d_labels, d_keys, count, nd, n1, n2, d_coords, (uint16_t*)d_values, d_out_labels);
  else hipLaunchKernelGGL(k_emit<float>, grid, block, 0, s, (const float*)d_in, d_labels, d_keys, count, nd, n1, n2, d_coords, (float*)d_values, d_out_labels);
  SD_LAUNCH_CHECK();
  return 0;
}
