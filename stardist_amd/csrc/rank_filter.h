// rank_filter.h -- the per-element rules of csrc/rank_filter.hip (stardist_amd.rank_filters: minimum / maximum / median / rank /
// percentile filters and grey morphology): scipy.ndimage's boundary index rules, the order-preserving keys
// with one key for every NaN, the minimum / maximum of a line, the selection of a window's rank-th key by bisection over the key's
// bits, the top-hat's last operation and the caps and LDS tier boundaries.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: tests/host/rank_filter_check.cpp
// runs the same rules with plain loops and compares them with the host route of stardist_amd/rank_filters.py.
#pragma once
#include <stdint.h>
#include <string.h>

#include "select_rank.h"

#if defined(__HIPCC__)
#define RF_HD __host__ __device__ __forceinline__
#else
#define RF_HD inline
#endif

namespace rankf {

enum Dtype { DT_U8 = 0, DT_U16 = 1, DT_F32 = 2 };
enum Mode { MODE_REFLECT = 0, MODE_NEAREST = 1, MODE_MIRROR = 2, MODE_CONSTANT = 3 };
enum Fuse { FUSE_NONE = 0, FUSE_REF_MINUS = 1, FUSE_MINUS_REF = 2, FUSE_XOR = 3 };   // the last pass's operation against a second image

enum {
  MAX_WINDOW = 1025,             // a window's length along an axis (box and footprint): longer windows take the host route
  MAX_FOOTPRINT = 4096,          // true elements of a footprint: larger footprints take the host route
  THREADS = 256,
  // box tiles, (along the axis) x (along the contiguous axis): a pass along the last axis takes 1024 x 1, any other 32 x 64
  B_LAST_A = 1024, B_INNER_A = 32, B_INNER_I = 64,
  LDS_BYTES = 48 * 1024,         // what a tile with its halo may take (spots.h's budget); beyond it the same code reads global memory
  // footprint tiles z, y, x: 1 x 16 x 64 for a 2D image, 4 x 4 x 64 for a 3D one
  F_X = 64, F_Y2 = 16, F_Y3 = 4, F_Z3 = 4
};

// ---- scipy.ndimage's index rules (ni_support.c, NI_InitFilterOffsets / NI_ExtendLine), for windows longer than the axis as well.
// Returns the index inside 0 .. n - 1 that position i reads, or -1 where mode 'constant' reads cval.
//   reflect   d c b a | a b c d | d c b a     period 2 n
//   mirror    d c b | a b c d | c b a         period 2 n - 2 (n = 1: always 0)
//   nearest   a a a a | a b c d | d d d d
RF_HD long long map_index(long long i, long long n, int mode) {
  if (i >= 0 && i < n) return i;
  if (mode == MODE_CONSTANT) return -1;
  if (mode == MODE_NEAREST) return i < 0 ? 0 : n - 1;
  if (n == 1) return 0;
  if (mode == MODE_REFLECT) {
    const long long p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
  }
  const long long p = 2 * n - 2;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// the window of output position i along an axis: size elements starting at i - left, left = size / 2 + origin (0 <= left < size)
RF_HD int window_left(int size, int origin) { return size / 2 + origin; }

// ---- keys: select_rank.h's unsigned integers that sort like the values (-0.0 below +0.0), and one key for every NaN, the greatest.
typedef uint32_t key32;
template <typename T> struct KeyOf;
template <> struct KeyOf<uint8_t> { typedef uint8_t type; enum { BITS = 8 }; };
template <> struct KeyOf<uint16_t> { typedef uint16_t type; enum { BITS = 16 }; };
template <> struct KeyOf<float> { typedef uint32_t type; enum { BITS = 32 }; };

const uint32_t NAN_KEY = 0xffffffffu;                                     // decodes to a quiet NaN (0x7fffffff)

RF_HD uint8_t to_key(uint8_t v) { return v; }
RF_HD uint16_t to_key(uint16_t v) { return v; }
RF_HD uint32_t to_key(float v) { return v != v ? NAN_KEY : selrank::key_of(v); }
RF_HD uint8_t from_key(uint8_t k, uint8_t) { return k; }
RF_HD uint16_t from_key(uint16_t k, uint16_t) { return k; }
RF_HD float from_key(uint32_t k, float) { return selrank::f32_of_key(k); }
RF_HD bool is_nan_key(uint8_t) { return false; }
RF_HD bool is_nan_key(uint16_t) { return false; }
RF_HD bool is_nan_key(uint32_t k) { return k == NAN_KEY; }

// ---- minimum / maximum of a line: at(j), j = 0 .. len - 1, are the window's keys.  A NaN anywhere gives NaN.
template <typename K, class At>
RF_HD K minmax_line(const At& at, int len, bool is_max) {
  K lo = at(0), hi = lo;
  for (int j = 1; j < len; ++j) {
    const K k = at(j);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
  return (is_max || is_nan_key(hi)) ? hi : lo;
}

// ---- the rank-th smallest (0-based) of the n keys at(0 .. n - 1): the greatest value v with #{keys < v} <= rank, built bit by bit
// from the top -- `bits` rounds, every one a walk over the window that counts, no storage per pixel, the same path for every pixel.
// Rank 0 and rank n - 1 are one walk.  A NaN anywhere gives NaN (found in the first walk: the NaN key is the greatest).
template <typename K, class At>
RF_HD K select_rank(const At& at, int n, int rank, int bits) {
  if (rank == 0 || rank == n - 1) return minmax_line<K>(at, n, rank != 0);
  K res = 0;
  bool nan = false;
  for (int b = bits - 1; b >= 0; --b) {
    const K cand = (K)(res | (K)((K)1 << b));
    int below = 0;
    if (b == bits - 1) {
      for (int j = 0; j < n; ++j) {
        const K k = at(j);
        below += k < cand;
        nan = nan || is_nan_key(k);
      }
      if (nan) return (K)NAN_KEY;
    } else {
      for (int j = 0; j < n; ++j) below += at(j) < cand;
    }
    if (below <= rank) res = cand;
  }
  return res;
}

// ---- the top-hat's last operation, in the image's dtype (unsigned types wrap as numpy's do; bool images, which travel as uint8, xor)
template <typename T>
RF_HD T fuse(T x, T ref, int op) {
  if (op == FUSE_REF_MINUS) return (T)(ref - x);
  if (op == FUSE_MINUS_REF) return (T)(x - ref);
  return x;
}
RF_HD uint8_t fuse_u8(uint8_t x, uint8_t ref, int op) { return op == FUSE_XOR ? (uint8_t)(x ^ ref) : fuse<uint8_t>(x, ref, op); }

// ---- tiers: whether a tile with its halo fits in LDS, in elements of `bytes` bytes (1 uint8 / bool, 2 uint16, 4 float32)
RF_HD bool box_tile_fits(int tile_a, int tile_i, int size, int bytes) { return (long long)(tile_a + size - 1) * tile_i * bytes <= LDS_BYTES; }
RF_HD void footprint_tile(bool is3d, int t[3]) {
  t[0] = is3d ? F_Z3 : 1;
  t[1] = is3d ? F_Y3 : F_Y2;
  t[2] = F_X;
}
// fs: the footprint's extents z y x
RF_HD bool footprint_tile_fits(bool is3d, const int fs[3], int bytes) {
  int t[3];
  footprint_tile(is3d, t);
  return (long long)(t[0] + fs[0] - 1) * (t[1] + fs[1] - 1) * (t[2] + fs[2] - 1) * bytes <= LDS_BYTES;
}

}  // namespace rankf
