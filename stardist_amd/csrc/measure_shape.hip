// measure_shape.hip -- the integer tables behind the shape columns of stardist_amd.utils.measure_labels(shape=True): inertia tensor,
// axis lengths, eccentricity, orientation, perimeter, Crofton perimeter and Euler number are fixed functions of them (label_ops.py).
//
//   sd_label_moment_sums_device      m2[l] = the six second-order sums of the box-local coordinates of every label 0 .. max_label
//   sd_label_contour_counts_device   counts[l] = {n_1, n_r2, n_h, h_1 .. h_15} of every label 0 .. max_label of a 2D image
//
// What a pixel adds is csrc/measure_shape.h's (shared with the host harness of the tests); this file is how the pixels are spread
// over threads and how equal labels are combined before the atomics.  Integer arithmetic only, 64-bit integer atomics: the tables
// depend on the input alone.  Nothing is copied to the host, the stream is not synchronised.
// k_moment_sums     one thread per pixel over the flat image, as k_centroid_sums (csrc/relabel_star.hip): the six (2D: three) products
//                   are summed over the runs of equal labels of a wave (csrc/wave_runs.h) and the run's first lane sends one atomic per
//                   non-zero term.  The box start of a pixel's label is a gather from the box table, L2-resident.
// k_contour_counts  one workgroup per tile of MSH_TILE_Y x MSH_TILE_X pixels: the labels with a halo of 2 go to LDS (5.4 KB, row
//                   stride 68 words: a wave reads 64 consecutive words, no bank conflict), the border bits with a halo of 1 are
//                   computed from them (1.2 KB), then every wave takes rows of 64 pixels; a pixel's 18 counters travel as three
//                   packed words through the same segmented reduction, and the run's first lane unpacks them into atomics.  An
//                   interior pixel adds one count (h_15), so a nucleus costs about one atomic per row it covers plus its contour.
// Bound: both read the image once (the halo adds 33 % to the tile's reads, from L2); with thousands of objects the atomics spread
// over as many table rows, with one object that fills the image they queue on one row: 3 .. 6 per wave, as k_centroid_sums.
#include "common.h"
#include "measure_shape.h"
#include "stardist_hip.h"
#include "wave_runs.h"

using namespace measure_shape;
using namespace wave_runs;

namespace {

enum { BLOCK = 256, MAX_BLOCKS = 1 << 16, MAX_TILE_BLOCKS = 1 << 22 };

__global__ void __launch_bounds__(BLOCK) k_moment_sums(const int* __restrict__ lbl, long long n, int Z, int Y, int X, int max_label, bool volume,
                                                       const int* __restrict__ tab, long long* m2) {
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
    const Runs r = runs_of(L, lane);
    if (all_background(r, L)) continue;
    long long t[6] = {0, 0, 0, 0, 0, 0};
    if (L) {
      int z0, y0, x0;
      box_start(tab + 6ll * L, Z, Y, X, &z0, &y0, &x0);
      const long long row = i / X;
      const long long x = i - row * X, y = volume ? row % Y : row, z = volume ? row / Y : 0;
      moment_terms(volume ? z - z0 : 0, y - y0, x - x0, t);
    }
    for (int o = 1; o < WAVE; o <<= 1) {
#pragma unroll
      for (int k = 3; k < 6; ++k) run_add(t[k], o, lane, r);
      if (volume) {                                                       // (uniform: a kernel argument)
#pragma unroll
        for (int k = 0; k < 3; ++k) run_add(t[k], o, lane, r);
      }
    }
    if (r.head && L) {
      long long* s = m2 + 6ll * L;
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (t[k]) add64(s + k, t[k]);
    }
  }
}

__global__ void __launch_bounds__(BLOCK) k_contour_counts(const int* __restrict__ lbl, int Y, int X, int max_label, int tiles_x, long long tiles,
                                                          long long* counts) {
  __shared__ int32_t tile[MSH_LY * MSH_LX];
  __shared__ uint8_t border[MSH_BY * MSH_BX];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long y0 = (t / tiles_x) * MSH_TILE_Y, x0 = (t % tiles_x) * MSH_TILE_X;
    for (int k = threadIdx.x; k < MSH_LY * MSH_LX; k += BLOCK) {
      const int ly = k / MSH_LX, lx = k - ly * MSH_LX;
      tile[k] = tile_label(lbl, Y, X, max_label, 0, y0 + ly - MSH_HALO, x0 + lx - MSH_HALO);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < MSH_BY * MSH_BX; k += BLOCK) {
      const int by = k / MSH_BX, bx = k - by * MSH_BX;
      border[k] = (uint8_t)border_bit(tile, by + 1, bx + 1);
    }
    __syncthreads();
    // the row loop's bounds are the same for the 64 lanes of a wave: all of them take part in every shuffle
    for (int ty = wave; ty < MSH_TILE_Y && y0 + ty < Y; ty += BLOCK / WAVE) {
      unsigned long long w[MSH_WORDS];
      const int L = pixel_counts(tile, border, ty, lane, w);
      const Runs r = runs_of(L, lane);
      if (all_background(r, L)) continue;                                 // a row of background
      for (int o = 1; o < WAVE; o <<= 1) {
#pragma unroll
        for (int k = 0; k < MSH_WORDS; ++k) run_add(w[k], o, lane, r);
      }
      if (r.head && L) {
        long long* c = counts + (long long)MSH_COUNTS * L;
        for (int f = 0; f < MSH_COUNTS; ++f) {
          const int v = get_field(w, f);
          if (v) add64(c + f, v);
        }
      }
    }
    __syncthreads();                                                      // the next tile rewrites the LDS arrays
  }
}

int blocks_for(long long total, long long most) {
  const long long b = (total + BLOCK - 1) / BLOCK;
  return (int)(b < most ? (b > 0 ? b : 1) : most);
}

}  // namespace

extern "C" int sd_label_moment_sums_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, const int32_t* d_boxes, int64_t* d_m2,
                                           void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!d_lbl || !d_boxes || !d_m2 || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0) {
    sd::set_error("sd_label_moment_sums: null pointer, non-positive size or negative max_label");
    return -1;
  }
  const long long n = (long long)Z * Y * X;
  if (n > (1ll << 40)) { sd::set_error("sd_label_moment_sums: image too large"); return -1; }
  SD_CHECK(hipMemsetAsync(d_m2, 0, 6 * ((size_t)max_label + 1) * sizeof(int64_t), s));
  if (max_label == 0) return 0;
  hipLaunchKernelGGL(k_moment_sums, dim3(blocks_for(n, MAX_BLOCKS)), dim3(BLOCK), 0, s, (const int*)d_lbl, n, Z, Y, X, max_label, Z > 1,
                     (const int*)d_boxes, (long long*)d_m2);
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" int sd_label_contour_counts_device(const int32_t* d_lbl, int Y, int X, int max_label, int64_t* d_counts, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!d_lbl || !d_counts || Y <= 0 || X <= 0 || max_label < 0) {
    sd::set_error("sd_label_contour_counts: null pointer, non-positive size or negative max_label");
    return -1;
  }
  if ((long long)Y * X > (1ll << 40)) { sd::set_error("sd_label_contour_counts: image too large"); return -1; }
  SD_CHECK(hipMemsetAsync(d_counts, 0, (size_t)MSH_COUNTS * ((size_t)max_label + 1) * sizeof(int64_t), s));
  if (max_label == 0) return 0;
  const int tiles_x = sd::div_up(X, MSH_TILE_X);
  const long long tiles = (long long)tiles_x * sd::div_up(Y, MSH_TILE_Y);
  const int blocks = (int)(tiles < MAX_TILE_BLOCKS ? tiles : MAX_TILE_BLOCKS);
  hipLaunchKernelGGL(k_contour_counts, dim3(blocks), dim3(BLOCK), 0, s, (const int*)d_lbl, Y, X, max_label, tiles_x, tiles, (long long*)d_counts);
  SD_LAUNCH_CHECK();
  return 0;
}
