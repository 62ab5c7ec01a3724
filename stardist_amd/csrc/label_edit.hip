// label_edit.hip -- label clean-up on the device (stardist_amd.utils.find_boundaries, clear_border, remove_small_objects): what
// skimage.segmentation.find_boundaries / clear_border and skimage.morphology.remove_small_objects compute.
//
//   sd_find_boundaries_device        d_out = 1 where a pixel is a boundary pixel (modes thick, inner, outer), else 0
//   sd_label_border_flags_device     d_flags[k] = 1 for every key k that has a pixel in the border band / where the mask is 0
//   sd_label_clear_flagged_device    d_out[p] = d_flags[d_key[p]] ? bgval : d_val[p]
//
// The per-pixel rules are csrc/label_edit.h's, shared with the host harness of the tests.
//   k_boundaries  one workgroup of LE_THREADS per tile (beyond 2^20 tiles a workgroup strides over them): the tile's labels with a halo of 1 in LDS (at most 15.5 KiB; a cell outside the
//                 image holds the clamped pixel, see the header), then every pixel reads its 3^nd window from LDS -- only the offsets
//                 its connectivity allows, the whole window in mode outer, where the two extrema are taken in the same pass -- and
//                 stores one byte.  One read of the labels (the halo cells again, from cache), one byte written per pixel, no atomics.
//   k_flag_band   one thread per pixel of the border band only; k_flag_mask: one thread per pixel, a pass over the mask.  Every writer
//                 stores the constant 1 with a plain vector store.
//   k_clear       four pixels per thread with 16-byte loads and stores where the pointers allow it.
// Nothing is read back and the stream is not synchronised.  Untuned: one byte per lane in k_boundaries' store, a generic tile shape
// per rank, the window loop is not specialised per connectivity.
#include "common.h"
#include "label_edit.h"
#include "stardist_hip.h"
#include <limits.h>
#include <algorithm>

using namespace label_edit;

namespace {

// MAX_TILE_BLOCKS: beyond 2^20 tiles (2^31 pixels of whole tiles) only degenerate extents go, whose blocks then take several tiles
enum { PER_THREAD = LE_TILE_PIXELS / LE_THREADS, MAX_BLOCKS = 8192, MAX_TILE_BLOCKS = 1 << 20 };

__global__ void __launch_bounds__(LE_THREADS) k_boundaries(const int* __restrict__ lbl, Tile g, long long tiles, int connectivity, int mode, long long background,
                                                           long long sentinel, unsigned char* __restrict__ out) {
  __shared__ int cells[LE_LDS_CELLS];
  const int n_cells = cell_count(g);
  // a block takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the same tiles for all its threads, so the barriers are uniform
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const Origin o = tile_origin(g, t);
    for (int c = (int)threadIdx.x; c < n_cells; c += LE_THREADS) cells[c] = lbl[cell_source(g, o, c)];
    __syncthreads();
    for (int k = 0; k < PER_THREAD; ++k) {
      int lz, ly, lx;
      local_coords(g, k * LE_THREADS + (int)threadIdx.x, lz, ly, lx);
      if (in_image(g, o, lz, ly, lx))
        out[global_index(g, o, lz, ly, lx)] = boundary_at(cells, g, lz, ly, lx, connectivity, mode, background, sentinel);
    }
    __syncthreads();                                                        // the next tile overwrites the cells
  }
}

__global__ void __launch_bounds__(LE_THREADS) k_flag_band(const int* __restrict__ key, Band b, long long count, unsigned char* flags,
                                                          long long n_flags) {
  for (long long t = (long long)blockIdx.x * LE_THREADS + threadIdx.x; t < count; t += (long long)gridDim.x * LE_THREADS)
    flag_pixel(key, band_pixel(b, t), flags, n_flags);
}

__global__ void __launch_bounds__(LE_THREADS) k_flag_mask(const int* __restrict__ key, const unsigned char* __restrict__ mask, long long n,
                                                          unsigned char* flags, long long n_flags) {
  for (long long p = (long long)blockIdx.x * LE_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * LE_THREADS)
    if (!mask[p]) flag_pixel(key, p, flags, n_flags);
}

__global__ void __launch_bounds__(LE_THREADS) k_clear(const int* __restrict__ val, const int* __restrict__ key, const unsigned char* __restrict__ flags,
                                                      long long n_flags, long long n, bool vec, int bgval, int* __restrict__ out) {
  const long long n_quads = (n + 3) / 4;
  for (long long q = (long long)blockIdx.x * LE_THREADS + threadIdx.x; q < n_quads; q += (long long)gridDim.x * LE_THREADS) {
    const long long i0 = q * 4;
    if (vec) {
      const int4 v = *reinterpret_cast<const int4*>(val + i0);
      const int4 k = *reinterpret_cast<const int4*>(key + i0);
      int4 r;
      r.x = cleared_value(v.x, k.x, flags, n_flags, bgval);
      r.y = cleared_value(v.y, k.y, flags, n_flags, bgval);
      r.z = cleared_value(v.z, k.z, flags, n_flags, bgval);
      r.w = cleared_value(v.w, k.w, flags, n_flags, bgval);
      *reinterpret_cast<int4*>(out + i0) = r;
    } else {
      const int m = (int)std::min(4ll, n - i0);
      for (int j = 0; j < m; ++j) out[i0 + j] = cleared_value(val[i0 + j], key[i0 + j], flags, n_flags, bgval);
    }
  }
}

unsigned grid_for(long long work_items) { return (unsigned)std::max(1ll, std::min<long long>((work_items + LE_THREADS - 1) / LE_THREADS, MAX_BLOCKS)); }

bool too_many_pixels(int Z, int Y, int X) { return (long long)Z * Y > INT_MAX || (long long)Z * Y * X > INT_MAX; }

}  // namespace

extern "C" int sd_find_boundaries_device(const int32_t* d_lbl, int Z, int Y, int X, int connectivity, int mode, long long background,
                                         long long sentinel, uint8_t* d_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_find_boundaries";
  if (!d_lbl || !d_out || Z <= 0 || Y <= 0 || X <= 0) { sd::set_error("%s: null pointer or non-positive size", who); return -1; }
  if ((const void*)d_lbl == (const void*)d_out) { sd::set_error("%s: the output is the input", who); return -1; }
  if (connectivity < 1 || connectivity > 3) { sd::set_error("%s: connectivity outside 1 .. 3", who); return -1; }
  if (mode != LE_THICK && mode != LE_INNER && mode != LE_OUTER) { sd::set_error("%s: mode must be 0 (thick), 1 (inner) or 2 (outer)", who); return -1; }
  if (too_many_pixels(Z, Y, X)) { sd::set_error("%s: more than 2^31 - 1 pixels", who); return -1; }
  const Tile g = tile_of(Z, Y, X);
  const long long tiles = tile_count(g);
  const unsigned blocks = (unsigned)std::min<long long>(tiles, MAX_TILE_BLOCKS);
  hipLaunchKernelGGL(k_boundaries, dim3(blocks), dim3(LE_THREADS), 0, s, (const int*)d_lbl, g, tiles, connectivity, mode, background, sentinel,
                     (unsigned char*)d_out);
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" int sd_label_border_flags_device(const int32_t* d_key, int Z, int Y, int X, int ndim, int buffer_size, const uint8_t* d_mask,
                                            long long n_flags, uint8_t* d_flags, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_label_border_flags";
  if (!d_key || !d_flags || Z <= 0 || Y <= 0 || X <= 0 || n_flags <= 0) { sd::set_error("%s: null pointer or non-positive size", who); return -1; }
  if ((const void*)d_key == (const void*)d_flags || (d_mask && (const void*)d_mask == (const void*)d_flags)) {
    sd::set_error("%s: the output is an input", who);
    return -1;
  }
  if ((ndim != 2 && ndim != 3) || (ndim == 2 && Z != 1)) { sd::set_error("%s: ndim must be 2 (with Z = 1) or 3", who); return -1; }
  if (!d_mask && (buffer_size < 0 || buffer_size >= INT_MAX / 2)) { sd::set_error("%s: negative buffer size", who); return -1; }
  if (too_many_pixels(Z, Y, X)) { sd::set_error("%s: more than 2^31 - 1 pixels", who); return -1; }
  const long long n = (long long)Z * Y * X;
  SD_CHECK(hipMemsetAsync(d_flags, 0, (size_t)n_flags, s));
  if (d_mask) {
    hipLaunchKernelGGL(k_flag_mask, dim3(grid_for(n)), dim3(LE_THREADS), 0, s, (const int*)d_key, (const unsigned char*)d_mask, n,
                       (unsigned char*)d_flags, n_flags);
  } else {
    const Band b = band_of(Z, Y, X, ndim == 3, buffer_size + 1);
    const long long count = band_count(b);
    hipLaunchKernelGGL(k_flag_band, dim3(grid_for(count)), dim3(LE_THREADS), 0, s, (const int*)d_key, b, count, (unsigned char*)d_flags, n_flags);
  }
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" int sd_label_clear_flagged_device(const int32_t* d_val, const int32_t* d_key, const uint8_t* d_flags, long long n_flags, long long n,
                                             int bgval, int32_t* d_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_label_clear_flagged";
  if (!d_val || !d_key || !d_flags || !d_out || n <= 0 || n_flags <= 0) { sd::set_error("%s: null pointer or non-positive size", who); return -1; }
  if (d_out == d_val || d_out == d_key || (const void*)d_out == (const void*)d_flags) { sd::set_error("%s: the output is an input", who); return -1; }
  if (n > INT_MAX) { sd::set_error("%s: more than 2^31 - 1 pixels", who); return -1; }
  const bool vec = (uintptr_t)d_val % 16 == 0 && (uintptr_t)d_key % 16 == 0 && (uintptr_t)d_out % 16 == 0 && n % 4 == 0;
  hipLaunchKernelGGL(k_clear, dim3(grid_for((n + 3) / 4)), dim3(LE_THREADS), 0, s, (const int*)d_val, (const int*)d_key,
                     (const unsigned char*)d_flags, n_flags, n, vec, bgval, (int*)d_out);
  SD_LAUNCH_CHECK();
  return 0;
}
