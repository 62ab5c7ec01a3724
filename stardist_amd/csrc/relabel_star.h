// relabel_star.h -- what csrc/relabel_star.hip shares between its kernels and its host entry points: the march of one star-convex ray
// from one pixel (c_star_dist, stardist/lib/stardist2d.cpp:55-124; c_star_dist3d, stardist/lib/stardist3d.cpp:245-346), written once
// for both sides, and the 2D direction table.
//
// Statement.  A ray starts at the pixel (bi, bj[, bk]) and adds its float direction to a float offset step by step; after every step
// the pixel under it is lrint(start + offset) per axis (round half to even).  The ray stops at the first step whose pixel lies outside
// the image or holds another id.  2D: the offset is then moved by (t_corr - 1) * direction, t_corr = .5 / max(|dx|, |dy|), and the
// distance is sqrtf(x * x + y * y).  3D: the distance is the double sqrt of the INTEGER sum of the squared rounded offsets, stored as
// float.  A background start gives 0.  Ids are compared as the reference reads them, as unsigned short: the low 16 bits of the int32
// label, so ids that agree modulo 65536 are one object to a ray and a multiple of 65536 is background.
//
// Every float operation is rounded on its own (the library and the tests' host build compile with -ffp-contract=off) and in the order
// of csrc/star_dist.hip, whose dense kernels these rows equal bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

namespace relabelstar {

enum { RS_MAX_RAYS = 4096 };   // the ray table of one launch lives in LDS: 3 floats per ray, 48 KiB at most

RS_HD inline int round_to_int(float r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float2int_rn(r);
#else
  return (int)lrintf(r);   // the default rounding mode: half to even
#endif
}

RS_HD inline unsigned short low16(int v) { return (unsigned short)(unsigned)v; }

// dx = sin(phi), dy = cos(phi) as in stardist2d.cpp:93-95: x runs along the rows' index i, y along j
RS_HD inline float march2d(const int32_t* lbl, int H, int W, int bi, int bj, float dx, float dy) {
  const unsigned short value = low16(lbl[(size_t)bi * W + bj]);
  if (value == 0) return 0.f;
  float x = 0.f, y = 0.f;
  while (1) {
    x += dx; y += dy;
    const int ii = round_to_int((float)bi + x), jj = round_to_int((float)bj + y);   // :101
    if (ii < 0 || ii >= H || jj < 0 || jj >= W || value != low16(lbl[(size_t)ii * W + jj])) {
      const float t_corr = .5f / fmaxf(fabsf(dx), fabsf(dy));                        // :108
      x += (t_corr - 1.f) * dx;
      y += (t_corr - 1.f) * dy;
      return sqrtf(x * x + y * y);
    }
  }
}

RS_HD inline float march3d(const int32_t* lbl, int Z, int Y, int X, int bi, int bj, int bk, float dz, float dy, float dx) {
  const unsigned short value = low16(lbl[((size_t)bi * Y + bj) * X + bk]);
  if (value == 0) return 0.f;
  float x = 0.f, y = 0.f, z = 0.f;
  while (1) {
    x += dx; y += dy; z += dz;
    const int ii = round_to_int((float)bi + z), jj = round_to_int((float)bj + y), kk = round_to_int((float)bk + x);   // :307
    if (ii < 0 || ii >= Z || jj < 0 || jj >= Y || kk < 0 || kk >= X || value != low16(lbl[((size_t)ii * Y + jj) * X + kk])) {
      const int x2 = round_to_int(x), y2 = round_to_int(y), z2 = round_to_int(z);
      return (float)sqrt((double)(x2 * x2 + y2 * y2 + z2 * z2));                    // :317-320 (sqrt(int) -> double)
    }
  }
}

// the 2D direction table, by the host's libm: phi = k * (float)(2 pi / n_rays), table[2k] = sinf(phi), table[2k + 1] = cosf(phi)   :91-95
inline void dirs2d(int n_rays, float* table) {
  const float st_rays = (2 * M_PI) / n_rays;
  for (int k = 0; k < n_rays; ++k) {
    const float phi = k * st_rays;
    table[2 * k] = sinf(phi);
    table[2 * k + 1] = cosf(phi);
  }
}

// a 3D ray that is zero (or NaN) in every component never leaves its voxel: the march would not end
RS_HD inline bool has_direction(float dz, float dy, float dx) { return fabsf(dz) + fabsf(dy) + fabsf(dx) > 0.f; }

// is the int64 coordinate an index of an axis of extent n?
RS_HD inline bool within(long long c, int n) { return c >= 0 && c < (long long)n; }

}  // namespace relabelstar
