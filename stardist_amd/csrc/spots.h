// spots.h -- the per-element rules of csrc/spots.hip (stardist_amd.spots: gaussian_filter, difference_of_gaussians, peak_local_max;
// DESIGN.md section 3w): the reflected index, one output element of a Gaussian line, "is this pixel beaten inside its window", the
// 64-bit sort key of a peak and the LDS tier boundaries.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: tests/host/spots_check.cpp runs
// the same rules with plain loops and compares them with the host route of stardist_amd/spots.py.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SP_HD __host__ __device__ __forceinline__
#else
#define SP_HD inline
#endif

namespace spots {

enum Dtype { DT_U8 = 0, DT_U16 = 1, DT_F32 = 2 };

enum {
  MAX_RADIUS = 512,              // the Gaussian's radius cap: longer windows take the host route
  PEAK_MAX_DISTANCE = 1 << 20,   // min_distance per axis (the callers clamp it to the extent - 1 first)
  THREADS = 256,
  // Gaussian tiles, (along the axis) x (along the contiguous axis): a pass along the last axis takes 1024 x 1, any other 32 x 64
  G_LAST_A = 1024, G_INNER_A = 32, G_INNER_I = 64,
  LDS_BYTES = 48 * 1024,         // what a tile with its halo may take; beyond it the same code reads global memory
  // peak tiles z, y, x: 1 x 16 x 64 for a 2D image, 4 x 4 x 64 for a 3D one
  P_X = 64, P_Y2 = 16, P_Y3 = 4, P_Z3 = 4
};

// scipy's 'reflect' (d c b a | a b c d | d c b a) with period 2n, for windows longer than the line as well
SP_HD long long reflect_index(long long i, long long n) {
  const long long p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}

// One output element: at(j) is the line's value j places from the element, as a double.  Farthest taps first, every operation rounded
// (the library and the harness are built with -ffp-contract=off).
template <class At>
SP_HD float gauss_point(const At& at, int r, const double* w) {
  double tmp = at(0) * w[r];
  for (int j = r; j >= 1; --j) tmp += (at(-j) + at(j)) * w[r - j];
  return (float)tmp;
}

// the floats of a Gaussian tile with its halo: whether it fits in LDS
SP_HD bool gauss_tile_fits(int tile_a, int tile_i, int r) { return (long long)(tile_a + 2 * r) * tile_i * 4 <= LDS_BYTES; }
// the largest radius of a pass along an axis that is not the last whose tile fits
SP_HD int gauss_lds_radius() { return (LDS_BYTES / 4 / G_INNER_I - G_INNER_A) / 2; }

SP_HD void peak_tile(bool is3d, int t[3]) {
  t[0] = is3d ? P_Z3 : 1;
  t[1] = is3d ? P_Y3 : P_Y2;
  t[2] = P_X;
}
SP_HD bool peak_tile_fits(bool is3d, const int d[3]) {
  int t[3];
  peak_tile(is3d, t);
  return (long long)(t[0] + 2 * d[0]) * (t[1] + 2 * d[1]) * (t[2] + 2 * d[2]) * 4 <= LDS_BYTES;
}

// Rule 4 of peak_local_max: does a pixel q inside the image with |q[a] - p[a]| <= d[a] beat p?  q beats p when v(q) > v(p), or
// v(q) == v(p) and idx(q) < idx(p); with labels only where labels(q) == labels(p).  Values compare as numbers (-0.0 == +0.0, a NaN
// never beats).  img.value(z, y, x) is the pixel as a float (uint8 / uint16 convert exactly), img.label(z, y, x) its label.
// The 3^nd neighbourhood first, then the whole window: most pixels that pass the threshold lose to a direct neighbour.
template <class Img>
SP_HD bool is_beaten(const Img& img, const long long n[3], const int d[3], long long z, long long y, long long x, float v, bool use_labels,
                     int lab) {
  const long long idx = (z * n[1] + y) * n[2] + x;
  for (int phase = 0; phase < 2; ++phase) {
    long long lo[3], hi[3];
    const long long p[3] = {z, y, x};
    bool wider = false;
    for (int a = 0; a < 3; ++a) {
      const long long e = phase == 0 ? (d[a] < 1 ? d[a] : 1) : d[a];
      wider = wider || d[a] > 1;
      lo[a] = p[a] - e < 0 ? 0 : p[a] - e;
      hi[a] = p[a] + e > n[a] - 1 ? n[a] - 1 : p[a] + e;
    }
    if (phase == 1 && !wider) break;
    for (long long qz = lo[0]; qz <= hi[0]; ++qz)
      for (long long qy = lo[1]; qy <= hi[1]; ++qy)
        for (long long qx = lo[2]; qx <= hi[2]; ++qx) {
          const float u = img.value(qz, qy, qx);
          if (u > v || (u == v && (qz * n[1] + qy) * n[2] + qx < idx))
            if (!use_labels || img.label(qz, qy, qx) == lab) return true;
        }
  }
  return false;
}

// ---- the sort key of a peak: ascending keys are (-v, idx) ascending.  The high word is the complement of an unsigned integer that
// sorts like the value (csrc/select_rank.h's key, with -0.0 folded onto +0.0), the low word the raster index.
SP_HD uint32_t value_key(float v) {
  if (v == 0.0f) v = 0.0f;                                                // -0.0 -> +0.0
  uint32_t u;
  memcpy(&u, &v, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SP_HD uint32_t value_key(uint8_t v) { return v; }
SP_HD uint32_t value_key(uint16_t v) { return v; }
template <typename T>
SP_HD uint64_t peak_key(T v, uint32_t idx) { return ((uint64_t)(~value_key(v)) << 32) | idx; }

SP_HD bool is_nan(float v) { return v != v; }
SP_HD bool is_nan(uint8_t) { return false; }
SP_HD bool is_nan(uint16_t) { return false; }

}  // namespace spots
