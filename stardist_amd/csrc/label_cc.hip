// label_cc.hip -- connected components of a 2D / 3D image on the device (stardist_amd.utils.label_components): what
// skimage.measure.label / scipy.ndimage.label compute, ids in raster order of each component's first pixel.
//
//   sd_label_components_device   d_out = the label image (int32), d_count = the number of components
//
// A tiled parallel union-find over linear pixel indices; the algorithm, its two invariants (par[p] <= p at every instant; the root of
// a finished component is its smallest index) and what a pixel does in each phase are csrc/label_cc.h's, shared with the host harness
// of the tests.  d_out is the parent array first and becomes the result.  Launches of one call, all on the caller's stream, nothing
// read back to the host:
//   k_tile      one workgroup of LCC_THREADS per tile: values and parents of the tile in LDS (16 KiB), the tile's inner edges united
//               there with LDS atomicMin, then par[p] = global index of the tile-local root (-1: background).  One read of the image.
//   k_border    the same grid: the face pixels of every tile unite with their backward neighbours in other tiles, in global memory
//               (atomicMin; finds read with relaxed agent-scope loads, so that a walk sees what other CUs wrote).
//   k_flatten   one thread per pixel: walk to the root, store it.
//   scan        hipcub::DeviceScan::ExclusiveSum over the flags par[p] == p (read through an iterator, never stored) -> rank[]
//   k_number    one thread per pixel: d_out[p] = rank[root] + 1, 0 for background; the thread of the last pixel writes d_count.
// No loop has an iteration cap and none needs one (invariant A).  Workspace: rank[], one int per pixel, and hipcub's.
// Untuned: no path compression in the border phase, one generic tile shape per rank, every tile pixel tests whether it is a face pixel.
#include "common.h"
#include "label_cc.h"
#include "stardist_hip.h"
#include <hipcub/hipcub.hpp>
#include <limits.h>

using namespace label_cc;

namespace {

enum { PER_THREAD = LCC_TILE_PIXELS / LCC_THREADS };

struct LdsMem {
  __device__ __forceinline__ int load(const int* p) const { return *(const volatile int*)p; }
  __device__ __forceinline__ int min(int* p, int v) const { return atomicMin(p, v); }
};

struct GlobalMem {
  __device__ __forceinline__ int load(const int* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int min(int* p, int v) const { return atomicMin(p, v); }
};

template <typename T>
__global__ void __launch_bounds__(LCC_THREADS) k_tile(const T* __restrict__ img, Geometry g, int n_offsets, long long background,
                                                      int* __restrict__ out) {
  __shared__ int val[LCC_TILE_PIXELS];
  __shared__ int par[LCC_TILE_PIXELS];
  const Origin o = tile_origin(g, blockIdx.x);
  LdsMem mem;
  for (int k = 0; k < PER_THREAD; ++k) tile_load<T>(g, o, k * LCC_THREADS + (int)threadIdx.x, img, background, val, par);
  __syncthreads();
  for (int k = 0; k < PER_THREAD; ++k) tile_link(g, k * LCC_THREADS + (int)threadIdx.x, n_offsets, val, par, mem);
  __syncthreads();
  for (int k = 0; k < PER_THREAD; ++k) tile_store(g, o, k * LCC_THREADS + (int)threadIdx.x, par, out, mem);
}

template <typename T>
__global__ void __launch_bounds__(LCC_THREADS) k_border(const T* __restrict__ img, Geometry g, int n_offsets, long long background, int* par) {
  const Origin o = tile_origin(g, blockIdx.x);
  GlobalMem mem;
  for (int k = 0; k < PER_THREAD; ++k) border_link<T>(g, o, k * LCC_THREADS + (int)threadIdx.x, img, background, n_offsets, par, mem);
}

__global__ void __launch_bounds__(LCC_THREADS) k_flatten(int* par, int n) {
  const long long p = (long long)blockIdx.x * LCC_THREADS + threadIdx.x;
  GlobalMem mem;
  if (p < n) flatten_pixel(par, (int)p, mem);
}

__global__ void __launch_bounds__(LCC_THREADS) k_number(int* __restrict__ par, const int* __restrict__ rank, int n, int* __restrict__ count) {
  const long long p = (long long)blockIdx.x * LCC_THREADS + threadIdx.x;
  if (p >= n) return;
  if (p == n - 1) *count = rank[p] + is_root(par, (int)p);
  number_pixel(par, rank, (int)p);
}

struct RootFlag {
  const int* par;
  __host__ __device__ __forceinline__ int operator()(int p) const { return is_root(par, p); }
};
typedef hipcub::TransformInputIterator<int, RootFlag, hipcub::CountingInputIterator<int>> FlagIterator;

template <typename T>
int run(const T* d_img, int Z, int Y, int X, int connectivity, long long background, int* d_out, int* d_count, hipStream_t s) {
  const Geometry g = geometry_of(Z, Y, X);
  const int n = (int)((long long)Z * Y * X), n_offsets = offset_count(connectivity);
  const long long tiles = tile_count(g);
  if (tiles > INT_MAX) { sd::set_error("sd_label_components: more tiles than a grid holds"); return -1; }
  sd::Arena& ar = sd::arena();
  if (ar.begin(s)) return -1;
  int* rank = ar.take_n<int>((size_t)n);
  RootFlag flag = {d_out};
  FlagIterator flags(hipcub::CountingInputIterator<int>(0), flag);
  size_t tmp_bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, flags, rank, n, s);
  void* tmp = ar.take(tmp_bytes + 256);
  if (!rank || !tmp) return -1;
  const unsigned pixel_blocks = (unsigned)(((long long)n + LCC_THREADS - 1) / LCC_THREADS);
  hipLaunchKernelGGL(k_tile<T>, dim3((unsigned)tiles), dim3(LCC_THREADS), 0, s, d_img, g, n_offsets, background, d_out);
  hipLaunchKernelGGL(k_border<T>, dim3((unsigned)tiles), dim3(LCC_THREADS), 0, s, d_img, g, n_offsets, background, d_out);
  hipLaunchKernelGGL(k_flatten, dim3(pixel_blocks), dim3(LCC_THREADS), 0, s, d_out, n);
  SD_LAUNCH_CHECK();
  SD_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, flags, rank, n, s));
  hipLaunchKernelGGL(k_number, dim3(pixel_blocks), dim3(LCC_THREADS), 0, s, d_out, (const int*)rank, n, d_count);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int sd_label_components_device(const void* d_img, int dtype, int Z, int Y, int X, int connectivity, long long background, int* d_out,
                                          int* d_count, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_label_components";
  if (!d_img || !d_out || !d_count || Z <= 0 || Y <= 0 || X <= 0) { sd::set_error("%s: null pointer or non-positive size", who); return -1; }
  if (connectivity < 1 || connectivity > 3) { sd::set_error("%s: connectivity outside 1 .. 3", who); return -1; }
  if ((long long)Z * Y > INT_MAX || (long long)Z * Y * X > INT_MAX) { sd::set_error("%s: more than 2^31 - 1 pixels", who); return -1; }
  if (dtype == LCC_U8) return run<uint8_t>((const uint8_t*)d_img, Z, Y, X, connectivity, background, d_out, d_count, s);
  if (dtype == LCC_U16) return run<uint16_t>((const uint16_t*)d_img, Z, Y, X, connectivity, background, d_out, d_count, s);
  if (dtype == LCC_I32) return run<int32_t>((const int32_t*)d_img, Z, Y, X, connectivity, background, d_out, d_count, s);
  sd::set_error("%s: dtype must be 0 (uint8), 1 (uint16) or 3 (int32)", who);
  return -1;
}
