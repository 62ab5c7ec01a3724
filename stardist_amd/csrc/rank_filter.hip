// rank_filter.hip -- rank filters and grey morphology on the device (stardist_amd.rank_filters).
//
//   sd_minmax_box_device    scipy.ndimage.minimum_filter / maximum_filter with `size`: one separable pass per axis whose size is not 1,
//                           the last pass optionally fused with the top-hat's subtraction (or xor) against a second image
//   sd_rank_filter_device   the rank-th smallest element under any footprint: minimum, maximum, median, rank and percentile filters
//
// The per-element rules -- scipy's boundary index maps, the keys, the line's minimum / maximum, the selection by bisection, the fused
// operation, the tiers -- are csrc/rank_filter.h's, shared with the host harness of the tests.  Both kernels work on keys: unsigned
// integers of the element's width that sort like the values, every NaN on the greatest key, so that "a window that covers a NaN gives
// NaN" costs no branch.  The boundary rule is applied once, while a tile is staged, so that the walks over a window are plain reads.
//
// Box: a pass sees the image as (outer, n, inner), n the axis it runs along.  A workgroup takes a tile of 1024 x 1 (the last axis,
// inner = 1) or 32 x 64 (any other axis: 64 contiguous elements wide), so a wave reads and writes 64 neighbouring elements in every
// pass.  The tile with its size - 1 halo lines goes to LDS as keys -- bytes, halves or words -- where it takes at most 48 KiB: always
// along the last axis, along another up to size 737 (uint8), 353 (uint16) or 161 (float32), from global memory by the same code
// beyond.  An output is a walk over its `size` keys (no running-extremum scheme: untuned for long windows).  Passes alternate between
// `out` and `work`, ending in `out`; the input is never written.
//
// Footprint: one tile of 1 x 16 x 64 pixels (3D 4 x 4 x 64) per workgroup, the tile with the footprint's halo in LDS as keys where
// that fits in 48 KiB, else the same code maps and reads global memory per element.  The footprint arrives as a table of (dz, dy, dx),
// read through the scalar cache (the index is wave-uniform).  The rank-th key is found by bisection over the key's bits from the top,
// 8, 16 or 32 walks that count the keys below a candidate; rank 0 and rank n - 1 are one walk.  No atomics, no per-pixel storage, no
// read-back: stream-ordered on the caller's stream.  Untuned: no register path for 3 x 3 / 5 x 5 windows, LDS reads are one key wide.
#include "common.h"
#include "rank_filter.h"
#include "stardist_hip.h"
#include <math.h>

using namespace rankf;

namespace {

__device__ __forceinline__ uint8_t fuse_any(uint8_t x, uint8_t ref, int op) { return fuse_u8(x, ref, op); }
__device__ __forceinline__ uint16_t fuse_any(uint16_t x, uint16_t ref, int op) { return fuse<uint16_t>(x, ref, op); }
__device__ __forceinline__ float fuse_any(float x, float ref, int op) { return fuse<float>(x, ref, op); }

// ----------------------------------------------------------------------------------------------------------------------- box
struct BoxPass {
  long long outer, n, inner, tiles_a, tiles_i;
  int tile_a, tile_i, size, left, mode, is_max, op;
};

template <typename T, typename K>
struct GlobalLine {
  const T* base;            // the line's element 0 (at this outer and inner position)
  long long first, n, inner;
  int mode;
  K cval;
  __device__ __forceinline__ K operator()(int j) const {
    const long long m = map_index(first + j, n, mode);
    return m < 0 ? cval : to_key(base[m * inner]);
  }
};
template <typename K>
struct TileLine {
  const K* first;
  int stride;
  __device__ __forceinline__ K operator()(int j) const { return first[j * stride]; }
};

template <typename T, bool LDS>
__global__ void __launch_bounds__(THREADS) k_box(const T* __restrict__ in, const T* __restrict__ ref, T* __restrict__ out, BoxPass P,
                                                 typename KeyOf<T>::type cval) {
  typedef typename KeyOf<T>::type K;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  K* tile = (K*)smem;
  long long b = blockIdx.x;
  const long long ti = b % P.tiles_i;
  b /= P.tiles_i;
  const long long ta = b % P.tiles_a, o = b / P.tiles_a;
  const long long a0 = ta * P.tile_a, i0 = ti * P.tile_i;
  const int rows = (int)(P.n - a0 < P.tile_a ? P.n - a0 : P.tile_a);
  const T* base = in + o * P.n * P.inner;
  if (LDS) {
    const int cells = (rows + P.size - 1) * P.tile_i;
    for (int e = (int)threadIdx.x; e < cells; e += THREADS) {
      const int ra = e / P.tile_i, li = e % P.tile_i;
      if (i0 + li < P.inner) {
        const long long m = map_index(a0 - P.left + ra, P.n, P.mode);
        tile[e] = m < 0 ? cval : to_key(base[m * P.inner + i0 + li]);
      }
    }
    __syncthreads();
  }
  const int cells = rows * P.tile_i;
  for (int e = (int)threadIdx.x; e < cells; e += THREADS) {
    const int la = e / P.tile_i, li = e % P.tile_i;
    const long long a = a0 + la, i = i0 + li;
    if (i >= P.inner) continue;
    K res;
    if (LDS) {
      const TileLine<K> at = {tile + la * P.tile_i + li, P.tile_i};
      res = minmax_line<K>(at, P.size, P.is_max != 0);
    } else {
      const GlobalLine<T, K> at = {base + i, a - P.left, P.n, P.inner, P.mode, cval};
      res = minmax_line<K>(at, P.size, P.is_max != 0);
    }
    const long long idx = (o * P.n + a) * P.inner + i;
    T v = from_key(res, T());
    if (P.op != FUSE_NONE) v = fuse_any(v, ref[idx], P.op);
    out[idx] = v;
  }
}

template <typename T>
__global__ void k_copy_fuse(const T* __restrict__ in, const T* __restrict__ ref, T* __restrict__ out, long long count, int op) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  T v = from_key(to_key(in[i]), T());
  if (op != FUSE_NONE) v = fuse_any(v, ref[i], op);
  out[i] = v;
}

template <typename T>
int box_pass(const T* in, const T* ref, T* out, BoxPass P, typename KeyOf<T>::type cval, hipStream_t s) {
  const bool last = P.inner == 1;
  P.tile_a = last ? B_LAST_A : B_INNER_A;
  P.tile_i = last ? 1 : B_INNER_I;
  P.tiles_a = (P.n + P.tile_a - 1) / P.tile_a;
  P.tiles_i = (P.inner + P.tile_i - 1) / P.tile_i;
  const double blocks = (double)P.outer * (double)P.tiles_a * (double)P.tiles_i;
  if (blocks > 2147483647.0) { sd::set_error("sd_minmax_box: more than 2^31 - 1 tiles in a pass"); return -1; }
  const dim3 grid((unsigned)(P.outer * P.tiles_a * P.tiles_i)), block(THREADS);
  const int bytes = (int)sizeof(typename KeyOf<T>::type);
  if (box_tile_fits(P.tile_a, P.tile_i, P.size, bytes)) {
    const size_t lds = (size_t)(P.tile_a + P.size - 1) * P.tile_i * bytes;
    hipLaunchKernelGGL((k_box<T, true>), grid, block, lds, s, in, ref, out, P, cval);
  } else {
    hipLaunchKernelGGL((k_box<T, false>), grid, block, 0, s, in, ref, out, P, cval);
  }
  SD_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int minmax_box(const T* in, const long long n[3], const int size[3], const int origin[3], int is_max, int mode, T cval, int op,
               const T* ref, T* out, T* work, hipStream_t s) {
  int passes = 0, done = 0;
  for (int a = 0; a < 3; ++a) passes += size[a] > 1;
  const long long count = n[0] * n[1] * n[2];
  if (passes == 0) {                                                      // a window of one element: the image itself
    hipLaunchKernelGGL(k_copy_fuse<T>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, in, ref, out, count, op);
    SD_LAUNCH_CHECK();
    return 0;
  }
  const T* src = in;
  for (int a = 0; a < 3; ++a) {
    if (size[a] <= 1) continue;
    BoxPass P;
    P.outer = a == 0 ? 1 : a == 1 ? n[0] : n[0] * n[1];
    P.n = n[a];
    P.inner = a == 0 ? n[1] * n[2] : a == 1 ? n[2] : 1;
    P.size = size[a];
    P.left = window_left(size[a], origin[a]);
    P.mode = mode;
    P.is_max = is_max;
    const bool final_pass = done == passes - 1;
    P.op = final_pass ? op : FUSE_NONE;
    T* dst = ((passes - done) & 1) ? out : work;                          // the last pass writes `out`
    if (box_pass<T>(src, ref, dst, P, to_key(cval), s)) return -1;
    src = dst;
    ++done;
  }
  return 0;
}

// ----------------------------------------------------------------------------------------------------------------- footprint
struct RankArgs {
  long long n[3], tiles[3];
  int t[3], fs[3], left[3];
  int mode, count, rank;
};

template <typename K>
struct TileWindow {
  const K* corner;          // the key of the window's element (0, 0, 0)
  const int* tab;
  int e1, e2;
  __device__ __forceinline__ K operator()(int k) const { return corner[(tab[3 * k] * e1 + tab[3 * k + 1]) * e2 + tab[3 * k + 2]]; }
};
template <typename T, typename K>
struct GlobalWindow {
  const T* in;
  const int* tab;
  long long z, y, x, n0, n1, n2;                                           // the image position of the window's element (0, 0, 0)
  int mode;
  K cval;
  __device__ __forceinline__ K operator()(int k) const {
    const long long mz = map_index(z + tab[3 * k], n0, mode), my = map_index(y + tab[3 * k + 1], n1, mode),
                    mx = map_index(x + tab[3 * k + 2], n2, mode);
    return (mz | my | mx) < 0 ? cval : to_key(in[(mz * n1 + my) * n2 + mx]);
  }
};

template <typename T, bool LDS>
__global__ void __launch_bounds__(THREADS) k_rank(const T* __restrict__ in, T* __restrict__ out, const int* __restrict__ tab, RankArgs A,
                                                  typename KeyOf<T>::type cval) {
  typedef typename KeyOf<T>::type K;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  K* tile = (K*)smem;
  long long b = blockIdx.x;
  const long long tx = b % A.tiles[2];
  b /= A.tiles[2];
  const long long ty = b % A.tiles[1], tz = b / A.tiles[1];
  const long long o[3] = {tz * A.t[0], ty * A.t[1], tx * A.t[2]};
  const int e[3] = {A.t[0] + A.fs[0] - 1, A.t[1] + A.fs[1] - 1, A.t[2] + A.fs[2] - 1};
  if (LDS) {
    const int cells = e[0] * e[1] * e[2];
    for (int s = (int)threadIdx.x; s < cells; s += THREADS) {
      const long long mz = map_index(o[0] - A.left[0] + s / (e[1] * e[2]), A.n[0], A.mode),
                      my = map_index(o[1] - A.left[1] + s / e[2] % e[1], A.n[1], A.mode),
                      mx = map_index(o[2] - A.left[2] + s % e[2], A.n[2], A.mode);
      tile[s] = (mz | my | mx) < 0 ? cval : to_key(in[(mz * A.n[1] + my) * A.n[2] + mx]);
    }
    __syncthreads();
  }
  const int cells = A.t[0] * A.t[1] * A.t[2];
  for (int s = (int)threadIdx.x; s < cells; s += THREADS) {
    const int lz = s / (A.t[1] * A.t[2]), ly = s / A.t[2] % A.t[1], lx = s % A.t[2];
    const long long z = o[0] + lz, y = o[1] + ly, x = o[2] + lx;
    if (z >= A.n[0] || y >= A.n[1] || x >= A.n[2]) continue;
    K res;
    if (LDS) {
      const TileWindow<K> at = {tile + (lz * e[1] + ly) * e[2] + lx, tab, e[1], e[2]};
      res = select_rank<K>(at, A.count, A.rank, (int)KeyOf<T>::BITS);
    } else {
      const GlobalWindow<T, K> at = {in, tab, z - A.left[0], y - A.left[1], x - A.left[2], A.n[0], A.n[1], A.n[2], A.mode, cval};
      res = select_rank<K>(at, A.count, A.rank, (int)KeyOf<T>::BITS);
    }
    out[(z * A.n[1] + y) * A.n[2] + x] = from_key(res, T());
  }
}

template <typename T>
int rank_filter(const T* in, const int* tab, RankArgs A, T cval, T* out, hipStream_t s) {   // tab: count x (dz, dy, dx) on the device
  const bool is3d = A.n[0] > 1;
  footprint_tile(is3d, A.t);
  double blocks = 1;
  for (int a = 0; a < 3; ++a) {
    A.tiles[a] = (A.n[a] + A.t[a] - 1) / A.t[a];
    blocks *= (double)A.tiles[a];
  }
  if (blocks > 2147483647.0) { sd::set_error("sd_rank_filter: more than 2^31 - 1 tiles"); return -1; }
  const dim3 grid((unsigned)(A.tiles[0] * A.tiles[1] * A.tiles[2])), block(THREADS);
  const int bytes = (int)sizeof(typename KeyOf<T>::type);
  if (footprint_tile_fits(is3d, A.fs, bytes)) {
    const size_t lds = (size_t)(A.t[0] + A.fs[0] - 1) * (A.t[1] + A.fs[1] - 1) * (A.t[2] + A.fs[2] - 1) * bytes;
    hipLaunchKernelGGL((k_rank<T, true>), grid, block, lds, s, in, out, tab, A, to_key(cval));
  } else {
    hipLaunchKernelGGL((k_rank<T, false>), grid, block, 0, s, in, out, tab, A, to_key(cval));
  }
  SD_LAUNCH_CHECK();
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

// mode inside its range; cval not NaN and a value of the dtype
bool bad_boundary(const char* who, int dtype, int mode, double cval) {
  if (mode < MODE_REFLECT || mode > MODE_CONSTANT) { sd::set_error("%s: mode code outside 0 .. 3", who); return true; }
  bool ok = cval == cval;
  if (ok && dtype != DT_F32) ok = cval >= 0 && cval <= (dtype == DT_U8 ? 255.0 : 65535.0) && cval == floor(cval);
  if (ok && dtype == DT_F32) ok = (double)(float)cval == cval;
  if (!ok) { sd::set_error("%s: cval is NaN or no value of the image's dtype", who); return true; }
  return false;
}

// 1 <= size <= MAX_WINDOW and 0 <= size / 2 + origin < size on every axis; a 2D image has size 1 on axis 0
bool bad_window(const char* who, int nd, const int* size, const int* origin) {
  for (int a = 0; a < 3; ++a) {
    if (size[a] < 1 || size[a] > MAX_WINDOW) { sd::set_error("%s: a window length outside 1 .. %d", who, (int)MAX_WINDOW); return true; }
    const long long left = (long long)size[a] / 2 + origin[a];
    if (left < 0 || left >= size[a]) { sd::set_error("%s: an origin outside its window", who); return true; }
  }
  if (nd == 2 && size[0] != 1) { sd::set_error("%s: a 2D image has window length 1 on axis 0", who); return true; }
  return false;
}

}  // namespace

extern "C" int sd_minmax_box_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2, const int* h_size,
                                    const int* h_origin, int is_max, int mode, double cval, int fuse_op, const void* d_ref, void* d_out,
                                    void* d_work, void* stream) {
  const char* who = "sd_minmax_box";
  if (bad_image(who, d_in, dtype, nd, n0, n1, n2)) return -1;
  if (!h_size || !h_origin || !d_out) { sd::set_error("%s: null pointer", who); return -1; }
  if (bad_boundary(who, dtype, mode, cval) || bad_window(who, nd, h_size, h_origin)) return -1;
  if (fuse_op < FUSE_NONE || fuse_op > FUSE_XOR || (fuse_op == FUSE_XOR && dtype != DT_U8)) { sd::set_error("%s: fuse code outside 0 .. 3 (3: uint8 only)", who); return -1; }
  if (fuse_op != FUSE_NONE && !d_ref) { sd::set_error("%s: a fused operation needs the second image", who); return -1; }
  int passes = 0;
  for (int a = 0; a < 3; ++a) passes += h_size[a] > 1;
  if (passes > 1 && !d_work) { sd::set_error("%s: more than one pass needs the work buffer", who); return -1; }
  if (d_out == d_in || d_work == d_in || d_out == d_ref || (d_work && d_work == d_ref) || d_out == d_work) { sd::set_error("%s: the buffers must be distinct", who); return -1; }
  const long long n[3] = {n0, n1, n2};
  const int size[3] = {h_size[0], h_size[1], h_size[2]}, origin[3] = {h_origin[0], h_origin[1], h_origin[2]};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == DT_U8) return minmax_box<uint8_t>((const uint8_t*)d_in, n, size, origin, is_max != 0, mode, (uint8_t)cval, fuse_op, (const uint8_t*)d_ref, (uint8_t*)d_out, (uint8_t*)d_work, s);
  if (dtype == DT_U16) return minmax_box<uint16_t>((const uint16_t*)d_in, n, size, origin, is_max != 0, mode, (uint16_t)cval, fuse_op, (const uint16_t*)d_ref, (uint16_t*)d_out, (uint16_t*)d_work, s);
  return minmax_box<float>((const float*)d_in, n, size, origin, is_max != 0, mode, (float)cval, fuse_op, (const float*)d_ref, (float*)d_out, (float*)d_work, s);
}

extern "C" int sd_rank_filter_device(const void* d_in, int dtype, int nd, long long n0, long long n1, long long n2, const int* h_extent,
                                     const int* h_origin, const int* h_offsets, int count, int rank, int mode, double cval, void* d_out,
                                     void* stream) {
  const char* who = "sd_rank_filter";
  if (bad_image(who, d_in, dtype, nd, n0, n1, n2)) return -1;
  if (!h_extent || !h_origin || !h_offsets || !d_out) { sd::set_error("%s: null pointer", who); return -1; }
  if (bad_boundary(who, dtype, mode, cval) || bad_window(who, nd, h_extent, h_origin)) return -1;
  if (count < 1 || count > MAX_FOOTPRINT) { sd::set_error("%s: a footprint of 1 .. %d elements", who, (int)MAX_FOOTPRINT); return -1; }
  if (rank < 0 || rank >= count) { sd::set_error("%s: rank outside 0 .. count - 1", who); return -1; }
  if (d_out == d_in) { sd::set_error("%s: the output must not be the input", who); return -1; }
  for (int k = 0; k < count; ++k)
    for (int a = 0; a < 3; ++a)
      if (h_offsets[3 * k + a] < 0 || h_offsets[3 * k + a] >= h_extent[a]) { sd::set_error("%s: a footprint offset outside its extent", who); return -1; }
  hipStream_t s = (hipStream_t)stream;
  sd::Arena& R = sd::arena();
  if (R.begin(s)) return -1;
  int* tab = R.take_n<int>((size_t)count * 3);
  if (!tab) return -1;
  SD_CHECK(hipMemcpyAsync(tab, h_offsets, (size_t)count * 3 * sizeof(int), hipMemcpyHostToDevice, s));
  RankArgs A;
  A.n[0] = n0; A.n[1] = n1; A.n[2] = n2;
  for (int a = 0; a < 3; ++a) {
    A.fs[a] = h_extent[a];
    A.left[a] = window_left(h_extent[a], h_origin[a]);
  }
  A.mode = mode;
  A.count = count;
  A.rank = rank;
  if (dtype == DT_U8) return rank_filter<uint8_t>((const uint8_t*)d_in, tab, A, (uint8_t)cval, (uint8_t*)d_out, s);
  if (dtype == DT_U16) return rank_filter<uint16_t>((const uint16_t*)d_in, tab, A, (uint16_t)cval, (uint16_t*)d_out, s);
  return rank_filter<float>((const float*)d_in, tab, A, (float)cval, (float*)d_out, s);
}
