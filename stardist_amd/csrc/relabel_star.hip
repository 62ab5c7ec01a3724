// relabel_star.hip -- what `relabel_image_stardist` / `relabel_image_stardist3D` (stardist/geometry/geom2d.py:200-211, geom3d.py:201-217)
// need of a label image besides the rasterisers: the centroid of every object and the star distances AT those centroids only.
//
//   sd_label_centroid_sums_device    sums[l] = {pixel count, sum z, sum y, sum x} of every label 1 .. max_label, one pass over the image
//   sd_star_dist2d_points_device     row p = the row of sd_star_dist2d_device at pixel points[p]
//   sd_star_dist3d_points_device     row p = the row of sd_star_dist3d_device at voxel points[p], clamped below at `floor`
//   sd_star_dist{2d,3d}_points_host  the same rows over host arrays, computed by the host (no device is touched)
//
// k_centroid_sums: one thread per pixel, a wave takes 64 consecutive pixels of the flat image.  The lanes that start a run of equal
// labels are found by comparing with the lane before (ballot); (z, y, x) are summed towards the run's first lane by a segmented
// shuffle reduction, the count is the run's length; the first lane of every object run sends one 64-bit atomic per non-zero term.  A
// nucleus costs a few atomics per row it covers and an object that fills the image three or four per wave, not four per pixel.
// Integer sums: the table does not depend on the order in which the atomics land.
// k_points2d / k_points3d: one thread per (point, ray), the ray fastest; the ray table in LDS as in csrc/star_dist.hip; the march is
// relabelstar::march2d / march3d of csrc/relabel_star.h.  A point outside the image gets a row of zeros and raises a flag that the
// entry point reads back (its only copy to the host) and turns into the error.
// Bound: the sums pass reads the image once; the point kernels read a few pixels along every ray and write n * n_rays floats.  At
// the sizes relabel sees (thousands of objects) both are launch-latency bound.
#include "common.h"
#include "relabel_star.h"
#include "stardist_hip.h"
#include "wave_runs.h"
#include <vector>

using namespace relabelstar;

namespace {

enum { BLOCK = 256, MAX_BLOCKS = 1 << 16 };
using wave_runs::WAVE;
using wave_runs::add64;

__global__ void __launch_bounds__(BLOCK) k_centroid_sums(const int* __restrict__ lbl, long long n, int Y, int X, int max_label, bool volume,
                                                         long long* sums) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long stride = (long long)gridDim.x * BLOCK;
  // the loop bound is the same for the 64 lanes of a wave: all of them take part in every shuffle
  for (long long base = (long long)blockIdx.x * BLOCK + (threadIdx.x - lane); base < n; base += stride) {
    const long long i = base + lane;
    int L = 0;
    if (i < n) {
      const int v = lbl[i];
      L = (v >= 1 && v <= max_label) ? v : 0;
    }
    const wave_runs::Runs r = wave_runs::runs_of(L, lane);
    if (wave_runs::all_background(r, L)) continue;                        // (uniform: every lane sees the same heads)
    const long long row = i / X;
    long long sx = i - row * X, sy = volume ? row % Y : row, sz = volume ? row / Y : 0;
    for (int o = 1; o < WAVE; o <<= 1) {
      wave_runs::run_add(sx, o, lane, r);
      wave_runs::run_add(sy, o, lane, r);
      if (volume) wave_runs::run_add(sz, o, lane, r);
    }
    if (r.head && L) {
      long long* s = sums + 4ll * L;
      add64(s, r.end - lane);
      if (sz) add64(s + 1, sz);
      if (sy) add64(s + 2, sy);
      if (sx) add64(s + 3, sx);
    }
  }
}

__global__ void __launch_bounds__(BLOCK) k_points2d(const int* __restrict__ lbl, int H, int W, const long long* __restrict__ pts, int n,
                                                    int R, const float2* __restrict__ dirs, float* __restrict__ dst, int* bad) {
  extern __shared__ float2 sdir[];
  for (int k = threadIdx.x; k < R; k += blockDim.x) sdir[k] = dirs[k];
  __syncthreads();
  const long long total = (long long)n * R;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(t % R);
    const long long p = t / R;
    const long long i = pts[2 * p], j = pts[2 * p + 1];
    float out = 0.f;
    if (within(i, H) && within(j, W)) out = march2d(lbl, H, W, (int)i, (int)j, sdir[k].x, sdir[k].y);
    else if (k == 0) atomicOr(bad, 1);
    dst[t] = out;
  }
}

__global__ void __launch_bounds__(BLOCK) k_points3d(const int* __restrict__ lbl, int Z, int Y, int X, const long long* __restrict__ pts, int n,
                                                    int R, const float* __restrict__ pdz, const float* __restrict__ pdy,
                                                    const float* __restrict__ pdx, float floor_, float* __restrict__ dst, int* bad) {
  extern __shared__ float sray[];   // 3 * R : dz | dy | dx
  for (int k = threadIdx.x; k < R; k += blockDim.x) { sray[k] = pdz[k]; sray[R + k] = pdy[k]; sray[2 * R + k] = pdx[k]; }
  __syncthreads();
  const long long total = (long long)n * R;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(t % R);
    const long long p = t / R;
    const long long a = pts[3 * p], b = pts[3 * p + 1], c = pts[3 * p + 2];
    const float dz = sray[k], dy = sray[R + k], dx = sray[2 * R + k];
    float out = 0.f;
    if (!has_direction(dz, dy, dx)) { if (p == 0) atomicOr(bad, 2); }   // such a ray never leaves its voxel: not marched
    else if (within(a, Z) && within(b, Y) && within(c, X)) out = fmaxf(march3d(lbl, Z, Y, X, (int)a, (int)b, (int)c, dz, dy, dx), floor_);
    else if (k == 0) atomicOr(bad, 1);
    dst[t] = out;
  }
}

int blocks_for(long long total) {
  const long long b = (total + BLOCK - 1) / BLOCK;
  return (int)(b < MAX_BLOCKS ? (b > 0 ? b : 1) : MAX_BLOCKS);
}

// what the point entries refuse; 1 = nothing to do
int check_points(const char* who, const void* lbl, int Z, int Y, int X, const void* pts, int n, int n_rays, const void* dist) {
  if (Z <= 0 || Y <= 0 || X <= 0 || n < 0 || n_rays <= 0) { sd::set_error("%s: non-positive size or negative n", who); return -1; }
  if (n_rays > RS_MAX_RAYS) { sd::set_error("%s: n_rays %d exceeds %d", who, n_rays, (int)RS_MAX_RAYS); return -1; }
  if ((long long)Z * Y * X > (1ll << 40)) { sd::set_error("%s: image too large", who); return -1; }
  if (n == 0) return 1;
  if (!lbl || !pts || !dist) { sd::set_error("%s: null pointer", who); return -1; }
  return 0;
}

int read_flag(const char* who, const int* d_bad, hipStream_t s) {
  int bad = 0;
  SD_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  if (bad) { sd::set_error(bad & 2 ? "%s: a ray without a direction (zero or NaN)" : "%s: a point lies outside the image", who); return -1; }
  return 0;
}

}  // namespace

extern "C" int sd_label_centroid_sums_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, int64_t* d_sums, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!d_lbl || !d_sums || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0) {
    sd::set_error("sd_label_centroid_sums: null pointer, non-positive size or negative max_label");
    return -1;
  }
  const long long n = (long long)Z * Y * X;
  if (n > (1ll << 40)) { sd::set_error("sd_label_centroid_sums: image too large"); return -1; }
  SD_CHECK(hipMemsetAsync(d_sums, 0, 4 * ((size_t)max_label + 1) * sizeof(int64_t), s));
  if (max_label == 0) return 0;
  hipLaunchKernelGGL(k_centroid_sums, dim3(blocks_for(n)), dim3(BLOCK), 0, s, (const int*)d_lbl, n, Y, X, max_label, Z > 1, (long long*)d_sums);
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" int sd_star_dist2d_points_device(const int32_t* d_lbl, int H, int W, const int64_t* d_points, int n, int n_rays, float* d_dist,
                                            void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_star_dist2d_points";
  const int rc = check_points(who, d_lbl, 1, H, W, d_points, n, n_rays, d_dist);
  if (rc) return rc < 0 ? -1 : 0;
  std::vector<float> dirs(2 * (size_t)n_rays);
  dirs2d(n_rays, dirs.data());
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  float2* d_dirs = A.take_n<float2>(n_rays);
  int* d_bad = A.take_n<int>(1);
  if (!d_dirs || !d_bad) return -1;
  SD_CHECK(hipMemcpyAsync(d_dirs, dirs.data(), n_rays * sizeof(float2), hipMemcpyHostToDevice, s));
  SD_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_points2d, dim3(blocks_for((long long)n * n_rays)), dim3(BLOCK), n_rays * sizeof(float2), s, (const int*)d_lbl, H, W,
                     (const long long*)d_points, n, n_rays, d_dirs, d_dist, d_bad);
  SD_LAUNCH_CHECK();
  return read_flag(who, d_bad, s);   // the synchronisation also keeps `dirs` alive for the copy
}

extern "C" int sd_star_dist3d_points_device(const int32_t* d_lbl, int Z, int Y, int X, const int64_t* d_points, int n, const float* d_dz,
                                            const float* d_dy, const float* d_dx, int n_rays, float floor, float* d_dist, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_star_dist3d_points";
  const int rc = check_points(who, d_lbl, Z, Y, X, d_points, n, n_rays, d_dist);
  if (rc) return rc < 0 ? -1 : 0;
  if (!d_dz || !d_dy || !d_dx) { sd::set_error("%s: null pointer", who); return -1; }
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  int* d_bad = A.take_n<int>(1);
  if (!d_bad) return -1;
  SD_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_points3d, dim3(blocks_for((long long)n * n_rays)), dim3(BLOCK), 3 * n_rays * sizeof(float), s, (const int*)d_lbl, Z, Y, X,
                     (const long long*)d_points, n, n_rays, d_dz, d_dy, d_dx, floor, d_dist, d_bad);
  SD_LAUNCH_CHECK();
  return read_flag(who, d_bad, s);
}

extern "C" int sd_star_dist2d_points_host(const int32_t* lbl, int H, int W, const int64_t* points, int n, int n_rays, float* dist) {
  const char* who = "sd_star_dist2d_points";
  const int rc = check_points(who, lbl, 1, H, W, points, n, n_rays, dist);
  if (rc) return rc < 0 ? -1 : 0;
  for (int p = 0; p < n; ++p)
    if (!within(points[2 * p], H) || !within(points[2 * p + 1], W)) { sd::set_error("%s: a point lies outside the image", who); return -1; }
  std::vector<float> dirs(2 * (size_t)n_rays);
  dirs2d(n_rays, dirs.data());
  for (int p = 0; p < n; ++p)
    for (int k = 0; k < n_rays; ++k)
      dist[(size_t)p * n_rays + k] = march2d(lbl, H, W, (int)points[2 * p], (int)points[2 * p + 1], dirs[2 * k], dirs[2 * k + 1]);
  return 0;
}

extern "C" int sd_star_dist3d_points_host(const int32_t* lbl, int Z, int Y, int X, const int64_t* points, int n, const float* dz,
                                          const float* dy, const float* dx, int n_rays, float floor, float* dist) {
  const char* who = "sd_star_dist3d_points";
  const int rc = check_points(who, lbl, Z, Y, X, points, n, n_rays, dist);
  if (rc) return rc < 0 ? -1 : 0;
  if (!dz || !dy || !dx) { sd::set_error("%s: null pointer", who); return -1; }
  for (int k = 0; k < n_rays; ++k)
    if (!has_direction(dz[k], dy[k], dx[k])) { sd::set_error("%s: a ray without a direction (zero or NaN)", who); return -1; }
  for (int p = 0; p < n; ++p)
    if (!within(points[3 * p], Z) || !within(points[3 * p + 1], Y) || !within(points[3 * p + 2], X)) {
      sd::set_error("%s: a point lies outside the image", who);
      return -1;
    }
  for (int p = 0; p < n; ++p)
    for (int k = 0; k < n_rays; ++k)
      dist[(size_t)p * n_rays + k] =
          fmaxf(march3d(lbl, Z, Y, X, (int)points[3 * p], (int)points[3 * p + 1], (int)points[3 * p + 2], dz[k], dy[k], dx[k]), floor);
  return 0;
}
