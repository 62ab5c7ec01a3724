// fill_holes.hip -- fill the holes of every labelled object (stardist/utils.py:137-153 `fill_label_holes`) and the per-label bounding
// boxes behind it and behind `calculate_extents` (scipy.ndimage.find_objects).
//
//   sd_label_boxes_device        boxes[l] = {z0, y0, x0, z1, y1, x1} of every label 1 .. max_label, one pass over the image
//   sd_fill_label_holes_device   out = max(lbl, 0), then every hole pixel of label L gets max(out, L)
//
// The reference fills object by object on the grown bounding box; csrc/fill_holes.h states the same thing without the grown box and
// holds the bit-plane passes (shared with the host harness of the tests).  Launches of one call, all on the caller's stream, nothing
// read back to the host:
//   k_boxes_init      the table gets the sentinel (starts INT_MAX, stops 0)
//   k_label_boxes     one thread per pixel; the first pixel of a run of equal labels in x (runs are cut into pieces every 64 columns)
//                     walks to the piece's end and sends at most one min / max per axis.  An extreme is not sent where a neighbour
//                     proves that another piece holds a better one: the same label right above (below) for the y start (stop), in
//                     the neighbouring plane for z, diagonally before the first pixel or above / below the pixel past the last one
//                     for x.  Every such witness is strictly better, so the chain ends at a piece that does send; a disc costs
//                     a handful of atomics, not six per row.  Writes out = max(lbl, 0).
//   k_compact         the labels present, into three device lists with device-side counts: objects whose two planes fit
//                     FH_WAVE_WORDS, those that fit FH_LDS_WORDS, and the others
//   k_fill_holes      one launch per list, each a persistent grid: workgroup w takes list entries w, w + gridDim.x, ...; planes in
//                     LDS (first list: single-wave workgroups, many per CU -- nuclei are of this kind; second list: 256 threads, two
//                     workgroups per CU) or in a per-workgroup slice of a global workspace (third list, FH_BIG_GROUPS workgroups);
//                     the passes of fill_holes.h to the fixpoint; atomicMax(out[p], L) for every bit of free & ~reach (holes of
//                     nested rings overlap).
// Bound: the box pass is one read and one write of the image; the fill pass re-reads the pixels of every box once (L2-resident for
// nuclei-sized objects) and is latency-bound on the LDS sweeps of small objects.
#include "common.h"
#include "fill_holes.h"
#include "stardist_hip.h"
#include <limits.h>
#include <algorithm>

using namespace fillholes;

namespace {

enum { BLOCK = 256, RUN_CUT = 64, FH_BIG_GROUPS = 16, FH_GROUPS_PER_CU = 2, FH_WAVE_GROUPS_PER_CU = 16 };
enum Tier { TIER_WAVE = 0, TIER_LDS = 1, TIER_GLOBAL = 2 };

__global__ void __launch_bounds__(BLOCK) k_boxes_init(int* __restrict__ tab, long long n6) {
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i < n6) tab[i] = (i % 6) < 3 ? INT_MAX : 0;
}

__global__ void __launch_bounds__(BLOCK) k_label_boxes(const int* __restrict__ lbl, long long n, int Y, int X, int max_label, int* tab,
                                                       int* __restrict__ out) {
  const long long p = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n) return;
  const int l = lbl[p];
  const bool object = l > 0 && l <= max_label;
  if (out) out[p] = object ? l : 0;
  if (!object) return;
  const long long row = p / X;
  const int x = (int)(p - row * X);
  const bool cut = x != 0 && lbl[p - 1] == l;                          // the run goes on to the left
  if (cut && (x % RUN_CUT) != 0) return;                               // not the first pixel of its piece
  int e = x + 1;
  while (e < X && (e % RUN_CUT) != 0 && lbl[p + (e - x)] == l) ++e;
  const int y = (int)(row % Y), z = (int)(row / Y);
  const long long plane = (long long)Y * X, q = p + (e - x);           // q: the pixel past the piece, where e < X
  const bool up = y > 0, dn = y < Y - 1;
  int* t = tab + 6ll * l;
  if (!(p >= plane && lbl[p - plane] == l)) atomicMin(t + 0, z);
  if (!(up && lbl[p - X] == l)) atomicMin(t + 1, y);
  if (!(cut || (x > 0 && ((up && lbl[p - X - 1] == l) || (dn && lbl[p + X - 1] == l))))) atomicMin(t + 2, x);
  if (!(p + plane < n && lbl[p + plane] == l)) atomicMax(t + 3, z + 1);
  if (!(dn && lbl[p + X] == l)) atomicMax(t + 4, y + 1);
  if (!(e < X && (lbl[q] == l || (up && lbl[q - X] == l) || (dn && lbl[q + X] == l)))) atomicMax(t + 5, e);
}

// counts[tier]: entries of that tier's list
__global__ void __launch_bounds__(BLOCK) k_compact(const int* __restrict__ tab, int max_label, int* __restrict__ tiny, int* __restrict__ small,
                                                   int* __restrict__ big, int* __restrict__ counts) {
  const long long l = (long long)blockIdx.x * BLOCK + threadIdx.x + 1;
  if (l > max_label) return;
  const int* t = tab + 6 * l;
  if (t[2] >= t[5]) return;                                            // absent
  const Geo g = geo_of(t);
  if (g.bx < 3 || g.by < 3) return;                                    // every pixel of such a box is on its outer layer
  if (fits_wave(g)) tiny[atomicAdd(&counts[TIER_WAVE], 1)] = (int)l;
  else if (fits_lds(g)) small[atomicAdd(&counts[TIER_LDS], 1)] = (int)l;
  else big[atomicAdd(&counts[TIER_GLOBAL], 1)] = (int)l;
}

// one object by the whole workgroup of NT threads; fr / rc: its planes (LDS or global), flag: one LDS word
template <int NT, typename P>
__device__ __forceinline__ void fill_object(const int* __restrict__ lbl, int volume, int Y, int X, const Geo& g, int L, P fr, P rc,
                                            volatile uint32_t* flag, int* __restrict__ out) {
  const int tid = threadIdx.x;
  for (long long i = tid; i < g.words; i += NT) {
    const int w = (int)(i % g.wx), row = (int)(i / g.wx);
    const int y = row % g.by, z = row / g.by;
    const uint32_t f = free_word(lbl, Y, X, g, z, y, w, L);
    fr[i] = f;
    rc[i] = f & outer_word(g, volume, z, y, w);
  }
  __syncthreads();
  const int ny = g.bz * g.wx, nz = g.by * g.wx;
  for (;;) {
    if (tid == 0) *flag = 0;
    __syncthreads();
    bool ch = false;
    for (int r = tid; r < g.rows; r += NT) ch |= pass_rows(rc, fr, g, r);
    __syncthreads();
    for (int c = tid; c < ny; c += NT) ch |= pass_y(rc, fr, g, c);
    __syncthreads();
    if (g.bz > 1) {
      for (int c = tid; c < nz; c += NT) ch |= pass_z(rc, fr, g, c);
    }
    if (ch) *flag = 1;
    __syncthreads();
    const uint32_t any = *flag;
    __syncthreads();
    if (!any) break;
  }
  for (long long i = tid; i < g.words; i += NT) {
    uint32_t h = fr[i] & ~rc[i];
    if (!h) continue;
    const int w = (int)(i % g.wx), row = (int)(i / g.wx);
    const int y = row % g.by, z = row / g.by;
    int* o = out + ((long long)(g.z0 + z) * Y + (g.y0 + y)) * X + g.x0 + 32 * w;
    while (h) {
      const int k = __ffs((int)h) - 1;
      h &= h - 1;
      atomicMax(o + k, L);
    }
  }
  __syncthreads();                                                     // the planes are rewritten by the next object
}

template <int TIER>
__global__ void __launch_bounds__(TIER == TIER_WAVE ? 64 : BLOCK) k_fill_holes(const int* __restrict__ lbl, int volume, int Y, int X,
                                                                                const int* __restrict__ tab, const int* __restrict__ list,
                                                                                const int* __restrict__ count, uint32_t* ws,
                                                                                long long ws_words, int* __restrict__ out) {
  extern __shared__ uint32_t lds[];
  const int n = *count;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int L = list[i];
    const Geo g = geo_of(tab + 6ll * L);
    if (TIER == TIER_GLOBAL) {
      if (2 * g.words > ws_words) continue;                            // cannot happen: a box is no larger than the image
      uint32_t* fr = ws + (long long)blockIdx.x * ws_words;
      fill_object<BLOCK>(lbl, volume, Y, X, g, L, fr, fr + g.words, lds, out);
    } else if (TIER == TIER_LDS) {
      fill_object<BLOCK>(lbl, volume, Y, X, g, L, lds, lds + g.words, lds + FH_LDS_WORDS, out);
    } else {
      fill_object<64>(lbl, volume, Y, X, g, L, lds, lds + g.words, lds + FH_WAVE_WORDS, out);
    }
  }
}

bool bad_image(const void* a, const void* b, int Z, int Y, int X, int max_label) {
  return !a || !b || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0;
}

int launch_boxes(const int32_t* d_lbl, int Z, int Y, int X, int max_label, int* tab, int* out, hipStream_t s) {
  const long long n = (long long)Z * Y * X, n6 = 6ll * ((long long)max_label + 1);
  hipLaunchKernelGGL(k_boxes_init, dim3((unsigned)((n6 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, tab, n6);
  hipLaunchKernelGGL(k_label_boxes, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, (const int*)d_lbl, n, Y, X, max_label,
                     tab, out);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int sd_label_boxes_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, int32_t* d_boxes, void* stream) {
  if (bad_image(d_lbl, d_boxes, Z, Y, X, max_label)) {
    sd::set_error("sd_label_boxes: null pointer, non-positive size or negative max_label");
    return -1;
  }
  if ((long long)Z * Y * X > (1ll << 40)) { sd::set_error("sd_label_boxes: image too large"); return -1; }
  return launch_boxes(d_lbl, Z, Y, X, max_label, d_boxes, nullptr, (hipStream_t)stream);
}

extern "C" int sd_fill_label_holes_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, int32_t* d_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (bad_image(d_lbl, d_out, Z, Y, X, max_label) || d_lbl == d_out) {
    sd::set_error("sd_fill_label_holes: null pointer, non-positive size, negative max_label or out == lbl");
    return -1;
  }
  if ((long long)Z * Y * X > (1ll << 40)) { sd::set_error("sd_fill_label_holes: image too large"); return -1; }
  static bool lds_allowed[sd::kMaxDevices] = {};
  const void* kernels[1] = {(const void*)k_fill_holes<TIER_LDS>};
  const int lds_bytes = (FH_LDS_WORDS + 4) * (int)sizeof(uint32_t);
  if (sd::allow_dynamic_lds(kernels, 1, lds_bytes, lds_allowed)) return -1;
  const int cus = sd::cu_count();
  if (cus < 0) return -1;
  // the planes of the largest box this image can hold; only where they exceed the LDS budget can the second list get entries
  const long long image_words = 2ll * Z * Y * ((X + 31) / 32);
  const bool may_be_big = image_words > (long long)FH_LDS_WORDS;
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  const size_t nl = (size_t)max_label + 1;
  int* tab = A.take_n<int>(6 * nl);
  int* tiny = A.take_n<int>(nl);
  int* small = A.take_n<int>(nl);
  int* big = A.take_n<int>(nl);
  int* counts = A.take_n<int>(4);
  uint32_t* ws = may_be_big ? A.take_n<uint32_t>((size_t)image_words * FH_BIG_GROUPS) : nullptr;
  if (!tab || !tiny || !small || !big || !counts || (may_be_big && !ws)) return -1;
  SD_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(int), s));
  if (launch_boxes(d_lbl, Z, Y, X, max_label, tab, d_out, s)) return -1;
  if (max_label == 0) return 0;
  hipLaunchKernelGGL(k_compact, dim3((unsigned)((max_label + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, (const int*)tab, max_label, tiny, small,
                     big, counts);
  const int volume = Z > 1 ? 1 : 0;
  const int wave_groups = (int)std::min<long long>((long long)cus * FH_WAVE_GROUPS_PER_CU, max_label);
  hipLaunchKernelGGL(k_fill_holes<TIER_WAVE>, dim3(wave_groups), dim3(64), (FH_WAVE_WORDS + 4) * sizeof(uint32_t), s, (const int*)d_lbl,
                     volume, Y, X, (const int*)tab, (const int*)tiny, (const int*)(counts + TIER_WAVE), (uint32_t*)nullptr, 0ll, d_out);
  if (image_words > (long long)FH_WAVE_WORDS) {
    const int groups = (int)std::min<long long>((long long)cus * FH_GROUPS_PER_CU, max_label);
    hipLaunchKernelGGL(k_fill_holes<TIER_LDS>, dim3(groups), dim3(BLOCK), lds_bytes, s, (const int*)d_lbl, volume, Y, X, (const int*)tab,
                       (const int*)small, (const int*)(counts + TIER_LDS), (uint32_t*)nullptr, 0ll, d_out);
  }
  if (may_be_big)
    hipLaunchKernelGGL(k_fill_holes<TIER_GLOBAL>, dim3(std::min<int>(FH_BIG_GROUPS, max_label)), dim3(BLOCK), 4 * sizeof(uint32_t), s,
                       (const int*)d_lbl, volume, Y, X, (const int*)tab, (const int*)big, (const int*)(counts + TIER_GLOBAL), ws, image_words,
                       d_out);
  SD_LAUNCH_CHECK();
  return 0;
}
