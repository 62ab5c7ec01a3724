// edt_feature.h -- the nearest-feature transform of a 2D / 3D image (stardist_amd.utils.expand_labels, distance_transform): for every
// pixel the nearest feature pixel under a per-axis spacing, its exact Euclidean distance, and scipy's choice among equally near ones.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/edt_feature.hip runs it with
// one thread per pixel, tests/host/edt_feature_check.cpp with plain loops, and tests/test_cpu_expand_labels.py compares the latter
// with a brute-force statement of the definition.
//
// DEFINITION.  Pixels are p = (p0, p1, p2) = (z, y, x), linear index (z * Y + y) * X + x (int32: at most 2^31 - 1 pixels); a 2D image
// is Z = 1 and its axes are 1 and 2.  For a pixel p and a feature q, in float64, every operation rounded on its own (no fused
// multiply-add: the library and the harness are built with -ffp-contract=off):
//     D(p, q) = ((s0 d0)^2 + (s1 d1)^2) + (s2 d2)^2,   each term  t = s * (double)d;  t * t,   d = |q - p| along the axis
// -- the floats of scipy's `dt *= sampling; dt *= dt; add.reduce(axis=0)`; with Z = 1 the first term is 0 and 0 + a == a.
// nearest(p) is the feature of smallest D; among equal D the smallest x wins, then the smallest y, then the smallest z (the smallest
// Fortran-order index).  dist(p) = sqrt(D(p, nearest(p))).  Under a bound B a pixel has a nearest feature only if dist(p) <= B;
// otherwise, and in an image without features, nearest = -1 and dist = +inf.
//
// PASSES, in scipy's axis order, one pixel one scan (scan_axis) per pass:
//   first   (axis 0 of a volume, axis 1 of an image) the candidates are the pixels of p's line themselves: value 0 for a feature, inf
//           otherwise.  p carries (value, linear index) of the best one.
//   middle  (axis 1 of a volume) the candidate at position k' of p's line is what the pixel there carries: value' + (s (k' - pos))^2.
//   last    (axis 2) the same, and the epilogue: dist = sqrt(value), nearest, the gathered label, under the bound.
// A scan starts from the pixel's own carried value and walks outwards, step k = 1, 2, ... on both sides.  A candidate on the lower
// side replaces the best one when its value is <= (it has the lower coordinate along this axis: it wins the tie), one on the upper
// side only when < .  Both sides of a step have the same axis term c = (s k)^2 and every candidate of that step is >= c, c grows with
// k, so the scan ends when c > best -- strictly: at c == best a lower-side candidate of carried value 0 still wins the tie.
// Why this is the definition's nearest(p): the float sum a + c is monotone in a, so among the features of one line of an earlier axis
// the carried one minimises every later sum it enters, and among equals the lower coordinate was kept; the last axis decides first,
// as the rule says.  (Monotone, not strictly: spacings so unequal that a whole axis term is absorbed by rounding, about 2^26 : 1 at
// one pixel apart, could tie two features of a line in D that the line's pass told apart.  Images are not sampled like that.)
// No parabola intersections, no divisions: nothing here rounds differently from the definition.
//
// BOUND.  A side of a scan also ends when t = s k > B.  That drops only what cannot pass dist <= B: t * t is one term of D, sums and
// the correctly rounded sqrt are monotone and sqrt(t * t) == t, so dist >= t > B for every feature reached through that step; and
// a pixel's true nearest feature q, if dist <= B, has s |d| <= B along every axis, so no pass drops it.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EDTF_HD __host__ __device__ __forceinline__
#else
#define EDTF_HD inline
#endif

namespace edt_feature {

enum { EDTF_THREADS = 256 };

// dtype codes of sd_nearest_feature_device: those of sd_label_components_device
enum { EDTF_U8 = 0, EDTF_U16 = 1, EDTF_I32 = 3 };

EDTF_HD double inf() { return (double)INFINITY; }

// candidate values of the first pass: the image itself
template <typename T>
struct ImageSource {
  const T* img;
  int feature_is_zero;
  EDTF_HD double operator()(long long q) const { return ((img[q] != 0) != (feature_is_zero != 0)) ? 0.0 : inf(); }
};

// candidate values of the later passes: what the pixels carry
struct CarriedSource {
  const double* val;
  EDTF_HD double operator()(long long q) const { return val[q]; }
};

struct Best {
  double value;      // inf: no feature reached
  long long at;      // the pixel of p's line whose candidate won
};

// The scan of pixel p along the axis of element stride `stride` and extent `len`, p at position `pos` of its line.
template <typename Source>
EDTF_HD Best scan_axis(const Source& src, long long p, long long stride, int len, int pos, double s, double bound) {
  Best b = {src(p), p};
  bool down = pos > 0, up = pos + 1 < len;
  for (int k = 1; down || up; ++k) {
    const double t = s * (double)k, c = t * t;
    if (c > b.value || t > bound) break;
    if (down) {
      const long long q = p - (long long)k * stride;
      const double v = src(q) + c;
      if (v <= b.value && v < inf()) { b.value = v; b.at = q; }
      down = pos - k > 0;
    }
    if (up) {
      const long long q = p + (long long)k * stride;
      const double v = src(q) + c;
      if (v < b.value) { b.value = v; b.at = q; }
      up = pos + k + 1 < len;
    }
  }
  return b;
}

// first pass: the winner is a pixel of the image
template <typename T>
EDTF_HD void first_pass_pixel(const ImageSource<T>& src, long long p, long long stride, int len, double s, double bound, double* val, int* idx) {
  const Best b = scan_axis(src, p, stride, len, (int)((p / stride) % len), s, bound);
  val[p] = b.value;
  idx[p] = b.value < inf() ? (int)b.at : -1;
}

// middle pass: the winner is what the pixel b.at carries
EDTF_HD void middle_pass_pixel(const double* val_in, const int* idx_in, long long p, long long stride, int len, double s, double bound, double* val,
                               int* idx) {
  const CarriedSource src = {val_in};
  const Best b = scan_axis(src, p, stride, len, (int)((p / stride) % len), s, bound);
  val[p] = b.value;
  idx[p] = b.value < inf() ? idx_in[b.at] : -1;
}

// last pass and epilogue; lbl / out_lbl, out_idx, out_dist may each be null
EDTF_HD void last_pass_pixel(const double* val_in, const int* idx_in, long long p, int len, double s, double bound, const int* lbl, int* out_lbl,
                             int* out_idx, double* out_dist) {
  const CarriedSource src = {val_in};
  const Best b = scan_axis(src, p, 1, len, (int)(p % len), s, bound);
  const double d = sqrt(b.value);
  const bool found = b.value < inf() && d <= bound;
  const int q = found ? idx_in[b.at] : -1;
  if (out_lbl) out_lbl[p] = found ? lbl[q] : 0;
  if (out_idx) out_idx[p] = q;
  if (out_dist) out_dist[p] = found ? d : inf();
}

// the bound of an entry point: max_distance < 0 or inf means none
EDTF_HD double bound_of(double max_distance) { return max_distance < 0.0 ? inf() : max_distance; }

}  // namespace edt_feature
