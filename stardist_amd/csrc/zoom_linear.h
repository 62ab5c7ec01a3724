// zoom_linear.h -- the arithmetic of scipy.ndimage.zoom(x, zoom, order=1) (mode 'constant', cval 0, grid_mode False) for one output
// element, bit for bit (scipy 1.15: ni_interpolation.c NI_ZoomShift, ni_splines.c).
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/zoom.hip runs zoom_element once
// per thread, tests/host/zoom_check.cpp once per loop iteration, and tests/test_cpu_zoom.py compares the latter with scipy.
//
// The per-axis tables come from the host (stardist_amd.utils._zoom_axis_table), one entry per OUTPUT index k of the axis, with
// cc = float64(k) * ((n - 1) / (m - 1)) the source coordinate:
//   i0[k]  floor(cc), or -1 where cc > n - 1.  The product can round past the last index for the last k; scipy then treats the
//          coordinate as outside the array and writes the constant 0 for every output element with this k.
//   w0[k]  1 - (cc - floor(cc))
//   w1[k]  1 - w0[k]   (scipy takes the last weight as one minus the others: not always the bits of cc - floor(cc))
// The second sample of an axis is i0 + 1; where that is n, scipy reads the mirrored index n - 2 (0 for n = 1) instead.  Its weight is
// then 0, so the value read matters only when it is not finite (0 * inf = NaN, as in scipy).
//
// Sum: float64, t = 0; the 2^rank corners with the last axis fastest and sample 0 before sample 1; per corner the value as float64,
// multiplied by the axis weights from axis 0 on, then added.  Every product and sum rounds on its own (built with -ffp-contract=off).
// Store: float32(t); uint8 / uint16: 0 for t <= 0, else t + 0.5 limited to the type's maximum and truncated.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZL_HD __host__ __device__ __forceinline__
#else
#define ZL_HD inline
#endif

namespace zoomlin {

enum { MAX_RANK = 4 };

struct Plan {
  int rank;
  int n[MAX_RANK];               // source extents
  int m[MAX_RANK];               // output extents
  long long stride[MAX_RANK];    // source strides in elements (contiguous)
  long long table[MAX_RANK];     // first entry of the axis in i0 / w0 / w1
};

ZL_HD float store_as(double t, float) { return (float)t; }
ZL_HD uint8_t store_as(double t, uint8_t) {
  t = t > 0.0 ? t + 0.5 : 0.0;
  return (uint8_t)(t > 255.0 ? 255.0 : t);
}
ZL_HD uint16_t store_as(double t, uint16_t) {
  t = t > 0.0 ? t + 0.5 : 0.0;
  return (uint16_t)(t > 65535.0 ? 65535.0 : t);
}

// output element `o` (row-major index into the output) of the zoom of src; P.rank == RANK.  IDX: unsigned where the output has fewer
// than 2^32 elements (the index arithmetic is 32-bit divisions then), unsigned long long otherwise
template <typename T, int RANK, typename IDX>
ZL_HD T zoom_element(const T* __restrict__ src, IDX o, const Plan& P, const int32_t* __restrict__ i0, const double* __restrict__ w0,
                     const double* __restrict__ w1) {
  long long off[RANK][2];
  double w[RANK][2];
  bool outside = false;
#pragma unroll
  for (int d = RANK - 1; d >= 0; --d) {
    const IDX q = o / (IDX)(unsigned)P.m[d];
    const long long k = P.table[d] + (long long)(o - q * (IDX)(unsigned)P.m[d]);
    o = q;
    const int n = P.n[d];
    int a = i0[k];
    if (a < 0) { outside = true; a = 0; }
    if (a > n - 1) a = n - 1;                       // never taken with the tables of the host; keeps every read inside src
    const int b = a + 1 < n ? a + 1 : (n > 1 ? n - 2 : 0);
    off[d][0] = a * P.stride[d];
    off[d][1] = b * P.stride[d];
    w[d][0] = w0[k];
    w[d][1] = w1[k];
  }
  if (outside) return store_as(0.0, T());
  double t = 0.0;
#pragma unroll
  for (int c = 0; c < (1 << RANK); ++c) {
    long long at = 0;
#pragma unroll
    for (int d = 0; d < RANK; ++d) at += off[d][(c >> (RANK - 1 - d)) & 1];
    double coeff = (double)src[at];
#pragma unroll
    for (int d = 0; d < RANK; ++d) coeff *= w[d][(c >> (RANK - 1 - d)) & 1];
    t += coeff;
  }
  return store_as(t, T());
}

}  // namespace zoomlin
