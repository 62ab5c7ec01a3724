// edt_feature.hip -- the nearest-feature transform on the device: an exact Euclidean distance transform with indices, and on top of
// it skimage.segmentation.expand_labels (stardist_amd.utils.distance_transform, expand_labels).
//
//   sd_nearest_feature_device   d_index = linear index of the nearest feature (-1: none), d_dist = its distance (float64, inf: none)
//   sd_expand_labels_device     d_out = the label of the nearest labelled pixel within `distance`, 0 elsewhere
//
// The definition (the float64 expression of the squared distance, the tie rule, the bound), the scan of one pixel and the reasons it
// is exact are csrc/edt_feature.h's, shared with the host harness of the tests.  Separable, in scipy's axis order, one thread per
// pixel and pass; every pixel carries (value, index): the squared distance over the axes done so far and the feature it belongs to.
// Launches of one call, all on the caller's stream, nothing read back to the host:
//   k_first    along z (volume) or y (image): reads the image, 1 - 4 B per step; writes 12 B per pixel.
//   k_middle   along y of a volume: reads the carried values of the line, 8 B per step, one index for the winner; writes 12 B.
//   k_last     along x: the same over contiguous memory, then sqrt, the bound test, the gathered label; writes what was asked for.
// Neighbouring lanes are neighbouring x in every pass, so each step of a wave is one coalesced row segment whatever the axis.  A scan
// ends after about the distance to the nearest feature (or the bound), so the cost follows the largest distance in the result.
// No atomics; the result depends on the input alone.  Workspace: (double, int) per pixel, twice for a volume.
// Untuned: the last pass reads its row through the caches, not from an LDS tile; lanes of a wave scan to different lengths.
#include "common.h"
#include "edt_feature.h"
#include "stardist_hip.h"
#include <limits.h>

using namespace edt_feature;

namespace {

template <typename T>
__global__ void __launch_bounds__(EDTF_THREADS) k_first(ImageSource<T> src, long long n, long long stride, int len, double s, double bound,
                                                        double* __restrict__ val, int* __restrict__ idx) {
  const long long p = (long long)blockIdx.x * EDTF_THREADS + threadIdx.x;
  if (p < n) first_pass_pixel(src, p, stride, len, s, bound, val, idx);
}

__global__ void __launch_bounds__(EDTF_THREADS) k_middle(const double* __restrict__ val_in, const int* __restrict__ idx_in, long long n,
                                                         long long stride, int len, double s, double bound, double* __restrict__ val,
                                                         int* __restrict__ idx) {
  const long long p = (long long)blockIdx.x * EDTF_THREADS + threadIdx.x;
  if (p < n) middle_pass_pixel(val_in, idx_in, p, stride, len, s, bound, val, idx);
}

__global__ void __launch_bounds__(EDTF_THREADS) k_last(const double* __restrict__ val_in, const int* __restrict__ idx_in, long long n, int len,
                                                       double s, double bound, const int* __restrict__ lbl, int* __restrict__ out_lbl,
                                                       int* __restrict__ out_idx, double* __restrict__ out_dist) {
  const long long p = (long long)blockIdx.x * EDTF_THREADS + threadIdx.x;
  if (p < n) last_pass_pixel(val_in, idx_in, p, len, s, bound, lbl, out_lbl, out_idx, out_dist);
}

template <typename T>
int run(const T* d_img, int Z, int Y, int X, int feature_is_zero, double sz, double sy, double sx, double bound, const int* d_lbl, int* d_out_lbl,
        int* d_index, double* d_dist, hipStream_t s) {
  const long long n = (long long)Z * Y * X;
  sd::Arena& ar = sd::arena();
  if (ar.begin(s)) return -1;
  double* val = ar.take_n<double>((size_t)n);
  int* idx = ar.take_n<int>((size_t)n);
  double* val2 = Z > 1 ? ar.take_n<double>((size_t)n) : val;
  int* idx2 = Z > 1 ? ar.take_n<int>((size_t)n) : idx;
  if (!val || !idx || !val2 || !idx2) return -1;
  const dim3 grid((unsigned)((n + EDTF_THREADS - 1) / EDTF_THREADS)), block(EDTF_THREADS);
  const ImageSource<T> src = {d_img, feature_is_zero};
  if (Z > 1) {
    hipLaunchKernelGGL(k_first<T>, grid, block, 0, s, src, n, (long long)Y * X, Z, sz, bound, val, idx);
    hipLaunchKernelGGL(k_middle, grid, block, 0, s, (const double*)val, (const int*)idx, n, (long long)X, Y, sy, bound, val2, idx2);
  } else {
    hipLaunchKernelGGL(k_first<T>, grid, block, 0, s, src, n, (long long)X, Y, sy, bound, val, idx);
  }
  hipLaunchKernelGGL(k_last, grid, block, 0, s, (const double*)val2, (const int*)idx2, n, X, sx, bound, d_lbl, d_out_lbl, d_index, d_dist);
  SD_LAUNCH_CHECK();
  return 0;
}

// the checks both entry points share; 0 if the sizes and spacings are usable
int check_geometry(const char* who, int Z, int Y, int X, double sz, double sy, double sx) {
  if (Z <= 0 || Y <= 0 || X <= 0) { sd::set_error("%s: non-positive size", who); return -1; }
  if ((long long)Z * Y > INT_MAX || (long long)Z * Y * X > INT_MAX) { sd::set_error("%s: more than 2^31 - 1 pixels", who); return -1; }
  if (!(sz > 0) || !(sy > 0) || !(sx > 0) || isinf(sz) || isinf(sy) || isinf(sx)) {
    sd::set_error("%s: the spacing must be positive and finite", who);
    return -1;
  }
  return 0;
}

}  // namespace

extern "C" int sd_nearest_feature_device(const void* d_img, int dtype, int Z, int Y, int X, int feature_is_zero, double sz, double sy, double sx,
                                         double max_distance, int32_t* d_index, double* d_dist, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_nearest_feature";
  if (!d_img) { sd::set_error("%s: null image", who); return -1; }
  if (check_geometry(who, Z, Y, X, sz, sy, sx)) return -1;
  if (max_distance != max_distance) { sd::set_error("%s: max_distance is not a number", who); return -1; }
  if (feature_is_zero != 0 && feature_is_zero != 1) { sd::set_error("%s: feature_is_zero must be 0 or 1", who); return -1; }
  const double bound = bound_of(max_distance);
  if (dtype == EDTF_U8) return run<uint8_t>((const uint8_t*)d_img, Z, Y, X, feature_is_zero, sz, sy, sx, bound, nullptr, nullptr, d_index, d_dist, s);
  if (dtype == EDTF_U16) return run<uint16_t>((const uint16_t*)d_img, Z, Y, X, feature_is_zero, sz, sy, sx, bound, nullptr, nullptr, d_index, d_dist, s);
  if (dtype == EDTF_I32) return run<int32_t>((const int32_t*)d_img, Z, Y, X, feature_is_zero, sz, sy, sx, bound, nullptr, nullptr, d_index, d_dist, s);
  sd::set_error("%s: dtype must be 0 (uint8), 1 (uint16) or 3 (int32)", who);
  return -1;
}

extern "C" int sd_expand_labels_device(const int32_t* d_lbl, int Z, int Y, int X, double sz, double sy, double sx, double distance, int32_t* d_out,
                                       void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_expand_labels";
  if (!d_lbl || !d_out || d_lbl == d_out) { sd::set_error("%s: null pointer, or the output is the input", who); return -1; }
  if (check_geometry(who, Z, Y, X, sz, sy, sx)) return -1;
  if (!(distance >= 0)) { sd::set_error("%s: the distance must be >= 0", who); return -1; }
  return run<int32_t>(d_lbl, Z, Y, X, 0, sz, sy, sx, distance, d_lbl, d_out, nullptr, nullptr, s);
}
