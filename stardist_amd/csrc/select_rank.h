// select_rank.h -- the host-checkable pieces of the exact percentile (csrc/normalize.hip): order-preserving keys, the digit plan of the
// radix selection, "which bin holds rank r", and numpy's linear interpolation between two order statistics.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: tests/host/select_rank_check.cpp runs
// the same digit-by-digit selection on host arrays and compares it with np.partition / np.percentile.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SR_HD __host__ __device__ __forceinline__
#else
#define SR_HD inline
#endif

namespace selrank {

enum Dtype { DT_U8 = 0, DT_U16 = 1, DT_F32 = 2 };

// ---- keys: an unsigned integer that sorts like the value.  float32: flip the sign bit of non-negatives, all bits of negatives, so
// -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN (negative NaNs sort first; a segment with any NaN reports NaN and never reads its ranks).
SR_HD uint32_t key_of(uint8_t v) { return v; }
SR_HD uint32_t key_of(uint16_t v) { return v; }
SR_HD uint32_t key_of(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SR_HD float f32_of_key(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float v;
  memcpy(&v, &u, 4);
  return v;
}

// ---- digit plan: the key's bits from the top, one histogram pass per digit.  uint8: 8; uint16: 16; float32: 11 + 11 + 10.
SR_HD int n_passes(int dtype) { return dtype == DT_F32 ? 3 : 1; }
SR_HD int digit_bits(int dtype, int pass) { return dtype == DT_U8 ? 8 : dtype == DT_U16 ? 16 : (pass < 2 ? 11 : 10); }
// number of key bits below the digit of `pass`
SR_HD int digit_shift(int dtype, int pass) { return dtype == DT_F32 ? (pass == 0 ? 21 : pass == 1 ? 10 : 0) : 0; }
SR_HD uint32_t digit_of(uint32_t key, int dtype, int pass) { return (key >> digit_shift(dtype, pass)) & ((1u << digit_bits(dtype, pass)) - 1u); }
// the digits above `pass`, right-aligned (0 for pass 0): an element takes part in `pass` for a rank whose prefix equals this
SR_HD uint32_t prefix_of(uint32_t key, int dtype, int pass) {
  const int s = digit_shift(dtype, pass) + digit_bits(dtype, pass);
  return s >= 32 ? 0u : key >> s;
}

// ---- which bin holds rank r: the first bin whose running count exceeds *r; *r becomes the rank inside that bin.  Returns nb - 1 with
// *r reduced by everything before it if the counts do not reach r (the caller's ranks are < the total, so this is not reached).
SR_HD int find_bin(const unsigned long long* hist, int nb, unsigned long long* r) {
  unsigned long long rest = *r;
  int b = 0;
  for (; b < nb - 1; ++b) {
    if (rest < hist[b]) break;
    rest -= hist[b];
  }
  *r = rest;
  return b;
}

// ---- numpy's `linear` percentile of n sorted values: the two order statistics to fetch and the weight between them, the way
// numpy.lib._function_base_impl._quantile computes them.  numpy (>= 2.0) divides q by 100 in the data's dtype when q is a Python scalar,
// so for float32 data the virtual index q/100 * (n - 1), the weight and the interpolation are float32; integer data (and q given as a
// float64 array) take float64 throughout.  `f32` selects the former.  The weight comes back as a double holding the float32 value.
struct Lerp { long long lo, hi; double t; };
SR_HD Lerp lerp_plan(long long n, double q, bool f32) {
  Lerp L;
  double vi, top;
  if (f32) {
    const float qf = (float)q / 100.0f;
    const float v = (float)(n - 1) * qf;
    vi = v; top = (float)(n - 1);
  } else {
    vi = (double)(n - 1) * (q / 100.0);
    top = (double)(n - 1);
  }
  double lo = floor(vi), hi = lo + 1.0;
  if (vi >= top) lo = hi = -1.0;     // _get_indexes: above the last index -> index -1, and the weight is taken against -1
  if (vi < 0.0) lo = hi = 0.0;
  L.t = f32 ? (double)((float)vi - (float)lo) : vi - lo;
  L.lo = lo < 0 ? n - 1 : (long long)lo;
  L.hi = hi < 0 ? n - 1 : (long long)hi;
  if (L.lo > n - 1) L.lo = n - 1;
  if (L.hi > n - 1) L.hi = n - 1;
  return L;
}

// numpy's _lerp(a, b, t): a + (b - a) * t, replaced by b - (b - a) * (1 - t) where t >= 0.5; every operation rounded on its own
// (the library is built with -ffp-contract=off; the host harness likewise)
SR_HD float lerp_f32(float a, float b, float t) {
  const float d = b - a;
  const float lo = a + d * t;
  const float hi = b - d * (1.0f - t);
  return t >= 0.5f ? hi : lo;
}
// integer data: b - a is taken in the integer type (b >= a: no wrap), the rest in float64; the caller casts the result to float32
SR_HD double lerp_f64(double a, double b, double t) {
  const double d = b - a;
  const double lo = a + d * t;
  const double hi = b - d * (1.0 - t);
  return t >= 0.5 ? hi : lo;
}

}  // namespace selrank
