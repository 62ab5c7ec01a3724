// augment.h -- one output pixel of a training augmentation chain (stardist_amd.augment.Compose), bit for bit what the host route
// (numpy / scipy.ndimage.map_coordinates, scipy 1.15: ni_interpolation.c NI_GeometricTransform, ni_support.c map_coordinate) gives.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/augment.hip runs augment_pixel
// once per thread, tests/host/augment_check.cpp once per loop iteration, and tests/test_cpu_augment.py compares the latter with the
// host route.
//
// The chain of one sample, in this order whatever was asked for:
//   FlipRot90   F(j) = src[base + sum_d j[d] * step[d]]: a permutation of axes of equal extent and per-axis flips are signed element
//               steps and a start offset (Sample::base, Sample::step, from the host).  Image and labels.
//   Warp        one resampling of F.  Coordinate of output pixel i along axis d, float64, every operation rounding on its own (built
//               with -ffp-contract=off):  c = ((o[d] + M[d][0] i[0]) + M[d][1] i[1] (+ M[d][2] i[2])) + float64(disp[comp[d]][i])
//               (the last term only where comp[d] >= 0).  Then per axis of extent n:
//                 constant  c < 0 or c > n - 1 on any axis: the pixel is 0, image and label.
//                 reflect   c is mapped first (reflect_coord: scipy's 'reflect', half-sample symmetric).
//               Image, order 1: s = floor(c), w0 = 1 - (c - s), w1 = 1 - w0; the second sample s + 1 is reflected (reflect_index) in
//               reflect mode, and in constant mode, where it is n, reads n - 2 (0 for n = 1) with weight 0 -- so 0 * inf = NaN as in
//               scipy.  Sum: float64, t = 0; the 2^nd corners with the last axis fastest, sample 0 before sample 1; per corner the value
//               as float64 times the axis weights from axis 0 on, then added.  Stored as float32(t).
//               Labels, order 0: index floor(c + 0.5), reflected in reflect mode.
//               Without a Warp the pixel is F(i) itself, bits and all.
//   IntensityScaleShift   v * scale + shift in float32, two roundings.
//   AdditiveNoise         v + sigma * n in float32, two roundings; n = float32(g), g = (S - (6 * 2^32 - 6)) * 2^-32 in float64 (exact),
//               S the sum of the twelve 32-bit words of the three Philox4x32-10 blocks with counter (pixel index low, pixel index
//               high, Sample::sample, 0 / 1 / 2) and the sample's key: an Irwin-Hall variate, variance 1, |g| < 6, no
//               transcendental function anywhere.
// Every index that reaches memory is limited to the sample's extent, whatever the parameters.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AUG_HD __host__ __device__ __forceinline__
#else
#define AUG_HD inline
#endif

namespace augment {

enum { AUG_THREADS = 256 };

// Plan::flags
enum { AUG_WARP = 1, AUG_REFLECT = 2, AUG_INTENSITY = 4, AUG_NOISE = 8 };

// one sample's parameters: a row of the packed table (stardist_amd.augment._SAMPLE_DTYPE has the same layout, 168 bytes)
struct Sample {
  double M[3][3];      // Warp: the matrix (rows beyond nd unused)
  double o[3];         //       the offset
  long long base;      // FlipRot90: element offset of F(0) in the sample
  long long step[3];   //            signed element step of F per output axis
  float scale, shift;  // IntensityScaleShift
  float sigma;         // AdditiveNoise
  uint32_t key[2];
  uint32_t sample;     //                the third counter word: the sample's index, as the host route was given it
  int32_t comp[3];     // Warp: the displacement component added to axis d, -1 for none
  int32_t pad_;
};

// what every sample of a call shares
struct Plan {
  int nd;              // 2 or 3
  int B;
  int flags;
  int na;              // displacement components per sample (0: no displacement field)
  int n[3];            // the patch extents, nd of them
  long long npix;
};

AUG_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t a = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, b = (uint32_t)p1, e = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, f = (uint32_t)p0;
    c[0] = a; c[1] = b; c[2] = e; c[3] = f;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the noise variate of pixel `pix` of the sample with third counter word `sample`
AUG_HD float noise_value(unsigned long long pix, uint32_t sample, uint32_t k0, uint32_t k1) {
  uint64_t S = 0;
  for (uint32_t blk = 0; blk < 3; ++blk) {
    uint32_t c[4] = {(uint32_t)pix, (uint32_t)(pix >> 32), sample, blk};
    philox4x32_10(c, k0, k1);
    S += (uint64_t)c[0] + c[1] + c[2] + c[3];
  }
  const double g = (double)((long long)S - 25769803770LL) * (1.0 / 4294967296.0);
  return (float)g;
}

// scipy's map_coordinate for NI_EXTEND_REFLECT
AUG_HD double reflect_coord(double c, int n) {
  if (c < 0) {
    if (n <= 1) return 0.0;
    const int sz2 = 2 * n;
    if (c < -sz2) c = (double)sz2 * trunc(-c / sz2) + c;
    c = c < -n ? c + sz2 : -c - 1;
  } else if (c > n - 1) {
    if (n <= 1) return 0.0;
    const int sz2 = 2 * n;
    c -= (double)sz2 * trunc(c / sz2);
    if (c >= n) c = sz2 - c - 1;
  }
  return c;
}

// the same rule on a sample index
AUG_HD long long reflect_index(long long k, int n) {
  if (k < 0) {
    if (n <= 1) return 0;
    const long long sz2 = 2LL * n;
    if (k < -sz2) k = sz2 * (-k / sz2) + k;
    k = k < -n ? k + sz2 : -k - 1;
  } else if (k > n - 1) {
    if (n <= 1) return 0;
    const long long sz2 = 2LL * n;
    k -= sz2 * (k / sz2);
    if (k >= n) k = sz2 - k - 1;
  }
  return k;
}

AUG_HD long long inside(long long k, int n) { return k < 0 ? 0 : (k > n - 1 ? n - 1 : k); }

// output pixel `pix` of a sample: x, y, ox, oy point at the sample's first element, disp at its first displacement component (or null)
template <int ND>
AUG_HD void augment_pixel(const Plan& P, const Sample& S, const float* __restrict__ x, const int32_t* __restrict__ y,
                          const float* __restrict__ disp, long long pix, float* __restrict__ ox, int32_t* __restrict__ oy) {
  int i[ND];
  {
    long long r = pix;
#pragma unroll
    for (int d = ND - 1; d >= 0; --d) {
      const long long q = r / P.n[d];
      i[d] = (int)(r - q * P.n[d]);
      r = q;
    }
  }
  float v;
  int32_t l;
  if (!(P.flags & AUG_WARP)) {
    long long at = S.base;
#pragma unroll
    for (int d = 0; d < ND; ++d) at += i[d] * S.step[d];
    v = x[at];
    l = y[at];
  } else {
    const bool reflect = (P.flags & AUG_REFLECT) != 0;
    bool outside = false;
    long long off[ND][2], off0 = S.base;
    double w[ND][2];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const int n = P.n[d];
      double c = S.o[d] + S.M[d][0] * (double)i[0];
      c = c + S.M[d][1] * (double)i[1];
      if (ND == 3) c = c + S.M[d][2] * (double)i[ND - 1];
      if (S.comp[d] >= 0) c = c + (double)disp[(long long)S.comp[d] * P.npix + pix];
      if (reflect) {
        c = reflect_coord(c, n);
        if (!(c >= -1.0 && c <= (double)n)) c = 0.0;          // never taken for finite parameters
      } else if (!(c >= 0.0 && c <= (double)(n - 1))) {
        outside = true;
        c = 0.0;
      }
      long long k0 = (long long)floor(c + 0.5);
      const double s = floor(c);
      w[d][0] = 1.0 - (c - s);
      w[d][1] = 1.0 - w[d][0];
      long long a = (long long)s, e = a + 1;
      if (reflect) {
        k0 = reflect_index(k0, n);
        a = reflect_index(a, n);
        e = reflect_index(e, n);
      } else if (e >= n) {
        e = n > 1 ? n - 2 : 0;
      }
      off0 += inside(k0, n) * S.step[d];
      off[d][0] = inside(a, n) * S.step[d];
      off[d][1] = inside(e, n) * S.step[d];
    }
    if (outside) {
      v = 0.0f;
      l = 0;
    } else {
      double t = 0.0;
#pragma unroll
      for (int corner = 0; corner < (1 << ND); ++corner) {
        long long at = S.base;
#pragma unroll
        for (int d = 0; d < ND; ++d) at += off[d][(corner >> (ND - 1 - d)) & 1];
        double coeff = (double)x[at];
#pragma unroll
        for (int d = 0; d < ND; ++d) coeff *= w[d][(corner >> (ND - 1 - d)) & 1];
        t += coeff;
      }
      v = (float)t;
      l = y[off0];
    }
  }
  if (P.flags & AUG_INTENSITY) {
    v = v * S.scale;
    v = v + S.shift;
  }
  if (P.flags & AUG_NOISE) {
    const float sn = S.sigma * noise_value((unsigned long long)pix, S.sample, S.key[0], S.key[1]);
    v = v + sn;
  }
  ox[pix] = v;
  oy[pix] = l;
}

// 0 if the FlipRot90 map of every sample stays inside a sample of P.npix elements (host side; both entry points call it)
inline int check_table(const Plan& P, const Sample* tab) {
  for (int b = 0; b < P.B; ++b) {
    long long lo = tab[b].base, hi = tab[b].base;
    for (int d = 0; d < P.nd; ++d) {
      const long long span = (long long)(P.n[d] - 1) * tab[b].step[d];
      if (span < 0) lo += span; else hi += span;
      if (tab[b].comp[d] < -1 || tab[b].comp[d] >= P.na) return -1;
    }
    if (lo < 0 || hi >= P.npix) return -1;
  }
  return 0;
}

}  // namespace augment
