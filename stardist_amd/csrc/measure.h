// measure.h -- the intensity statistics of one labelled object (stardist_amd.utils.measure_labels): which pixels a lane reads, in which
// order the values are added and how the partial results are combined.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/measure.hip runs it with one
// thread per lane, tests/host/measure_check.cpp with plain loops over the lanes, and tests/test_cpu_measure.py compares the latter
// with the host function.
//
// Per object L (box from sd_label_boxes_device) and channel c, over the pixels p of the box with lbl[p] == L, v = img[p * C + c]:
//   integer images (uint8, uint16)  S = sum v, S2 = sum v * v in int64 (exact, also beyond 2^53); min, max in int32
//   float32 images                  S = sum double(v), S2 = sum double(v) * double(v) in float64 (every square is exact: a 24-bit
//                                   mantissa squares into 48 bits); min, max in float32
//   a NaN pixel makes S, S2, min and max NaN (min / max take a NaN and keep it, as numpy's do); +-inf follow IEEE.
// The derived columns (mean = double(S) / count, var = max(0, S2 / count - mean^2), std = sqrt(var)) are computed by the caller.
//
// Order of the float64 additions -- a function of the box alone, hence of (shape, lbl), never of the grid, the device or the call:
//   chunks   the rows of the box (z-major: row r is z = r / by, y = r % by) are cut into chunks of chunk_rows = max(1, MS_CHUNK_PIXELS
//            / bx) whole rows; a box of at most MS_CHUNK_PIXELS pixels is one chunk.
//   lanes    a chunk is read by `lanes` lanes: 64 for a box of at most MS_WAVE_PIXELS pixels, else 256.  Lane t adds the pixels with
//            flattened index i = t, t + lanes, t + 2 lanes, ... of the chunk (i = row * bx + x) in ascending order, starting from 0.
//   tree     the lanes of every group of 64 are folded with the offsets 32, 16, 8, 4, 2, 1 (lane t takes lane t + offset); with 256
//            lanes the four group results are then added in ascending order.
//   chunks   the chunk results are added in ascending chunk order (the convention of sd_conv3_wgrad_ndhwc_device's partial sums).
// There is no floating-point atomic anywhere.  Integer sums are exact in any order and take the same path.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MS_HD __host__ __device__ __forceinline__
#else
#define MS_HD inline
#endif

namespace measure {

enum { MS_GROUP = 64, MS_WAVE_LANES = 64, MS_BLOCK_LANES = 256, MS_WAVE_PIXELS = 4096, MS_CHUNK_PIXELS = 65536 };

struct Box {
  int z0, y0, x0;      // first pixel of the box in the image
  int bz, by, bx;      // box extents (0 where the label is absent)
  int rows;            // bz * by
  int chunk_rows;      // whole rows per chunk
  int chunks;          // ceil(rows / chunk_rows); 0 where the label is absent
  long long pixels;    // rows * bx
};

MS_HD int clamp_to(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// box = {z0, y0, x0, z1, y1, x1}, stops exclusive; clamped to the image, so that no table can make a reader leave it.  Z * Y fits int.
MS_HD Box box_of(const int32_t* t, int Z, int Y, int X) {
  Box b;
  b.z0 = clamp_to(t[0], 0, Z); b.y0 = clamp_to(t[1], 0, Y); b.x0 = clamp_to(t[2], 0, X);
  b.bz = clamp_to(t[3], b.z0, Z) - b.z0; b.by = clamp_to(t[4], b.y0, Y) - b.y0; b.bx = clamp_to(t[5], b.x0, X) - b.x0;
  b.rows = b.bz * b.by;
  b.pixels = (long long)b.rows * b.bx;
  if (b.pixels <= 0) { b.rows = 0; b.pixels = 0; b.chunk_rows = 1; b.chunks = 0; return b; }
  b.chunk_rows = MS_CHUNK_PIXELS / b.bx > 1 ? MS_CHUNK_PIXELS / b.bx : 1;
  b.chunks = (int)(((long long)b.rows + b.chunk_rows - 1) / b.chunk_rows);
  return b;
}

MS_HD int lanes_of(const Box& b) { return b.pixels <= (long long)MS_WAVE_PIXELS ? (int)MS_WAVE_LANES : (int)MS_BLOCK_LANES; }

// the values min / max start from, and what the tables hold for an absent label
template <typename M> struct Lim;
template <> struct Lim<float> {
  static MS_HD float hi() { return __builtin_inff(); }
  static MS_HD float lo() { return -__builtin_inff(); }
};
template <> struct Lim<int32_t> {
  static MS_HD int32_t hi() { return INT32_MAX; }
  static MS_HD int32_t lo() { return INT32_MIN; }
};

// A: int64_t or double (sums), M: int32_t or float (min / max)
template <typename A, typename M>
struct Stat {
  A s, s2;
  M mn, mx;
};

template <typename M> MS_HD M keep_min(M a, M v) { return (v < a || v != v) ? v : a; }   // a NaN is taken and then kept
template <typename M> MS_HD M keep_max(M a, M v) { return (v > a || v != v) ? v : a; }

template <typename A, typename M>
MS_HD void stat_init(Stat<A, M>& s) {
  s.s = 0; s.s2 = 0; s.mn = Lim<M>::hi(); s.mx = Lim<M>::lo();
}

template <typename A, typename M>
MS_HD void stat_add(Stat<A, M>& s, M v) {
  const A a = (A)v;
  s.s += a;
  s.s2 += a * a;
  s.mn = keep_min(s.mn, v);
  s.mx = keep_max(s.mx, v);
}

// a = a + b: a is the lower lane, the lower group or the earlier chunk
template <typename A, typename M>
MS_HD void stat_merge(Stat<A, M>& a, const Stat<A, M>& b) {
  a.s += b.s;
  a.s2 += b.s2;
  a.mn = keep_min(a.mn, b.mn);
  a.mx = keep_max(a.mx, b.mx);
}

// tables: sums[(l * C + c) * 2] = {S, S2}, minmax[(l * C + c) * 2] = {min, max}
template <typename A, typename M>
MS_HD void stat_store(const Stat<A, M>& s, A* sums, M* minmax, long long l, int C, int c) {
  const long long at = 2 * (l * C + c);
  sums[at] = s.s; sums[at + 1] = s.s2;
  minmax[at] = s.mn; minmax[at + 1] = s.mx;
}

// 64-bit offset of pixel (row, x) of the box in the image
MS_HD long long pixel_offset(const Box& b, int Y, int X, int row, int x) {
  int z = 0, y = row;
  if (b.bz > 1) { z = row / b.by; y = row - z * b.by; }
  return ((long long)(b.z0 + z) * Y + (b.y0 + y)) * X + b.x0 + x;
}

// pixels of chunk `chunk`: at most max(MS_CHUNK_PIXELS, bx), so the flattened index fits 32 bits
MS_HD unsigned chunk_pixels(const Box& b, int chunk) {
  const int row0 = chunk * b.chunk_rows;
  const int n = b.rows - row0 < b.chunk_rows ? b.rows - row0 : b.chunk_rows;
  return (unsigned)n * (unsigned)b.bx;
}

// what lane `lane` of `lanes` adds to s for channel c of chunk `chunk`; T: the image's element type
template <typename T, typename A, typename M>
MS_HD void lane_accumulate(Stat<A, M>& s, const int32_t* __restrict__ lbl, const T* __restrict__ img, int C, int c, int Y, int X, const Box& b,
                           int chunk, int L, int lane, int lanes) {
  const int row0 = chunk * b.chunk_rows;
  const unsigned n = chunk_pixels(b, chunk), bx = (unsigned)b.bx;
  for (unsigned i = (unsigned)lane; i < n; i += (unsigned)lanes) {
    const unsigned r = i / bx, x = i - r * bx;
    const long long p = pixel_offset(b, Y, X, row0 + (int)r, (int)x);
    if (lbl[p] == L) stat_add(s, (M)img[p * C + c]);
  }
}

// the tree and the group order, over an array of per-lane results; the result is a[0]
template <typename A, typename M>
MS_HD void reduce_lanes(Stat<A, M>* a, int lanes) {
  for (int g = 0; g < lanes; g += MS_GROUP)
    for (int o = MS_GROUP / 2; o > 0; o >>= 1)
      for (int t = 0; t < o; ++t) stat_merge(a[g + t], a[g + t + o]);
  for (int g = MS_GROUP; g < lanes; g += MS_GROUP) stat_merge(a[0], a[g]);
}

}  // namespace measure
