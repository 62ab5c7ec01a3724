// measure.hip -- the intensity statistics of every labelled object (stardist_amd.utils.measure_labels): sum, sum of squares, minimum
// and maximum of the image's values over the pixels of every label, per channel.
//
//   sd_label_intensity_stats_device   sums[l][c] = {S, S2}, minmax[l][c] = {min, max} of every label 0 .. max_label
//
// The boxes come from sd_label_boxes_device, the pixel counts and coordinate sums from sd_label_centroid_sums_device; this file adds
// the pass that needs the image.  It is a per-object pass over the boxes, as csrc/fill_holes.hip's: which pixels a lane reads and
// the order of every addition are csrc/measure.h's (shared with the host harness of the tests), so the float64 sums depend on
// (shape, lbl, img) alone.  Launches of one call, all on the caller's stream, nothing read back to the host:
//   k_compact   one thread per table row: an absent label gets the sentinel; a label present goes into one of three device lists
//               with device-side counts (one atomic per wave and list): boxes of at most MS_WAVE_PIXELS pixels, other boxes of one chunk, boxes of several chunks.
//               The last kind reserves a range of the chunk workspace; one that finds no room left joins the second list.
//   k_stats     one launch per list, each a persistent grid (work item i goes to workgroup i % gridDim.x):
//                 wave   single-wave workgroups, many per CU -- nuclei are of this kind; the 64 lanes run over the flattened
//                        (row, x) index of the box, per-lane accumulators, the shuffle tree of measure.h, lane 0 writes the row
//                 block  256 threads per object; chunk after chunk, the chunk results added in chunk order; thread 0 writes the row
//                 chunk  256 threads per (object, chunk): the chunks of a large box spread over the grid; each leaves its partial
//                        result in the workspace
//   k_combine   one thread per (object of the third list, channel): its partial results added in chunk order, the row written
// The second and third kind run the same code per chunk and add the chunk results in the same order, so where an object is worked
// off does not show in the result.  Channels are passes of their own over the box (C = 1 reads every box pixel's label once).
// Bound: one read of the label and of the value per box pixel, L2-resident for nuclei-sized boxes; the wave tier is latency-bound
// on the dependent label -> value loads of a few pixels per lane.
#include "common.h"
#include "measure.h"
#include "stardist_hip.h"
#include <limits.h>
#include <algorithm>

using namespace measure;

namespace {

enum { BLOCK = 256, MS_WAVE_GROUPS_PER_CU = 32, MS_BLOCK_GROUPS_PER_CU = 8, MS_MAX_CHANNELS = 64 };
enum Tier { TIER_WAVE = 0, TIER_BLOCK = 1, TIER_CHUNK = 2 };
enum Count { N_WAVE = 0, N_BLOCK = 1, N_CHUNKED = 2, N_CHUNKS = 3 };

// M: the table's min / max type; the sums of an absent label are zero bits in either type
template <typename M>
__global__ void __launch_bounds__(BLOCK) k_compact(const int* __restrict__ tab, int max_label, int Z, int Y, int X, int C, int* __restrict__ tiny,
                                                   int* __restrict__ whole, int* __restrict__ cut, int* counts, int* __restrict__ chunk_base,
                                                   int* __restrict__ owner, int cap, long long* __restrict__ sums, M* __restrict__ minmax) {
  const long long l = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int kind = -1;                                                       // the list this label joins; -1: none
  if (l <= max_label) {
    const Box b = box_of(tab + 6 * l, Z, Y, X);
    if (l == 0 || b.chunks == 0) {
      for (int c = 0; c < C; ++c) {
        const long long at = 2 * (l * C + c);
        sums[at] = 0; sums[at + 1] = 0;
        minmax[at] = Lim<M>::hi(); minmax[at + 1] = Lim<M>::lo();
      }
    } else if (b.chunks == 1) {
      kind = lanes_of(b) == MS_WAVE_LANES ? N_WAVE : N_BLOCK;
    } else {
      int base = counts[N_CHUNKS];
      for (;;) {
        if (base + b.chunks > cap) { base = -1; break; }
        const int seen = atomicCAS(&counts[N_CHUNKS], base, base + b.chunks);
        if (seen == base) break;
        base = seen;
      }
      if (base < 0) {
        kind = N_BLOCK;
      } else {
        cut[atomicAdd(&counts[N_CHUNKED], 1)] = (int)l;
        chunk_base[l] = base;
        for (int k = 0; k < b.chunks; ++k) owner[base + k] = (int)l;
      }
    }
  }
  // one atomic per wave and list, not one per label: a million nuclei on one counter would queue up behind each other
  for (int which = N_WAVE; which <= N_BLOCK; ++which) {
    const unsigned long long mask = __ballot(kind == which);
    if (!mask) continue;
    const int leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&counts[which], __popcll(mask));
    base = __shfl(base, leader);
    if (kind == which) (which == N_WAVE ? tiny : whole)[base + __popcll(mask & ((1ull << lane) - 1ull))] = (int)l;
  }
}

// one chunk of one channel by the NT threads of the workgroup, measure.h's order; the result is thread 0's
template <typename T, typename A, typename M, int NT>
__device__ __forceinline__ Stat<A, M> chunk_stat(const int* __restrict__ lbl, const T* __restrict__ img, int C, int c, int Y, int X, const Box& b,
                                                 int chunk, int L) {
  Stat<A, M> s;
  stat_init(s);
  lane_accumulate<T, A, M>(s, lbl, img, C, c, Y, X, b, chunk, L, (int)threadIdx.x, NT);
  for (int o = MS_GROUP / 2; o > 0; o >>= 1) {
    Stat<A, M> other;
    other.s = __shfl_down(s.s, o);
    other.s2 = __shfl_down(s.s2, o);
    other.mn = __shfl_down(s.mn, o);
    other.mx = __shfl_down(s.mx, o);
    stat_merge(s, other);
  }
  if (NT > MS_GROUP) {
    __shared__ Stat<A, M> part[NT / MS_GROUP];
    if ((threadIdx.x & (MS_GROUP - 1)) == 0) part[threadIdx.x / MS_GROUP] = s;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int g = 1; g < NT / MS_GROUP; ++g) stat_merge(s, part[g]);
    __syncthreads();                                                   // the next chunk rewrites part[]
  }
  return s;
}

template <typename T, typename A, typename M, int TIER>
__global__ void __launch_bounds__(TIER == TIER_WAVE ? 64 : BLOCK) k_stats(const int* __restrict__ lbl, const T* __restrict__ img, int Z, int Y, int X,
                                                                           int C, const int* __restrict__ tab, const int* __restrict__ list,
                                                                           const int* __restrict__ count, const int* __restrict__ chunk_base,
                                                                           Stat<A, M>* __restrict__ partial, A* __restrict__ sums,
                                                                           M* __restrict__ minmax) {
  const int n = *count;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const int L = list[i];
    const Box b = box_of(tab + 6ll * L, Z, Y, X);
    if (TIER == TIER_CHUNK) {
      const int chunk = i - chunk_base[L];
      for (int c = 0; c < C; ++c) {
        const Stat<A, M> s = chunk_stat<T, A, M, BLOCK>(lbl, img, C, c, Y, X, b, chunk, L);
        if (threadIdx.x == 0) partial[(long long)i * C + c] = s;
      }
    } else if (TIER == TIER_BLOCK) {
      for (int c = 0; c < C; ++c) {
        Stat<A, M> total = chunk_stat<T, A, M, BLOCK>(lbl, img, C, c, Y, X, b, 0, L);
        for (int k = 1; k < b.chunks; ++k) {
          const Stat<A, M> s = chunk_stat<T, A, M, BLOCK>(lbl, img, C, c, Y, X, b, k, L);
          stat_merge(total, s);
        }
        if (threadIdx.x == 0) stat_store(total, sums, minmax, L, C, c);
      }
    } else {
      for (int c = 0; c < C; ++c) {
        const Stat<A, M> s = chunk_stat<T, A, M, 64>(lbl, img, C, c, Y, X, b, 0, L);
        if (threadIdx.x == 0) stat_store(s, sums, minmax, L, C, c);
      }
    }
  }
}

template <typename A, typename M>
__global__ void __launch_bounds__(BLOCK) k_combine(const int* __restrict__ tab, int Z, int Y, int X, int C, const int* __restrict__ cut,
                                                   const int* __restrict__ count, const int* __restrict__ chunk_base,
                                                   const Stat<A, M>* __restrict__ partial, A* __restrict__ sums, M* __restrict__ minmax) {
  const long long total = (long long)*count * C;
  for (long long t = (long long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * BLOCK) {
    const int c = (int)(t % C), L = cut[t / C];
    const Box b = box_of(tab + 6ll * L, Z, Y, X);
    const Stat<A, M>* p = partial + (long long)chunk_base[L] * C + c;
    Stat<A, M> s = p[0];
    for (int k = 1; k < b.chunks; ++k) stat_merge(s, p[(long long)k * C]);
    stat_store(s, sums, minmax, L, C, c);
  }
}

template <typename T, typename A, typename M>
int run(const int32_t* d_lbl, int Z, int Y, int X, int max_label, const int32_t* d_boxes, const T* d_img, int C, A* d_sums, M* d_minmax,
        hipStream_t s) {
  const int cus = sd::cu_count();
  if (cus < 0) return -1;
  const long long n = (long long)Z * Y * X;
  // room for the chunks of the boxes of several chunks: a box has at most pixels / (MS_CHUNK_PIXELS / 2) + 1 of them
  const int cap = (int)std::min<long long>(n / (MS_CHUNK_PIXELS / 4) + 1024, INT_MAX / 2);
  const bool may_block = n > (long long)MS_WAVE_PIXELS, may_chunk = n > (long long)MS_CHUNK_PIXELS;
  sd::Arena& ar = sd::arena();
  if (ar.begin(s)) return -1;
  const size_t nl = (size_t)max_label + 1;
  int* tiny = ar.take_n<int>(nl);
  int* whole = ar.take_n<int>(nl);
  int* cut = ar.take_n<int>(nl);
  int* chunk_base = ar.take_n<int>(nl);
  int* counts = ar.take_n<int>(4);
  int* owner = ar.take_n<int>(may_chunk ? cap : 1);
  Stat<A, M>* partial = ar.take_n<Stat<A, M>>(may_chunk ? (size_t)cap * C : 1);
  if (!tiny || !whole || !cut || !chunk_base || !counts || !owner || !partial) return -1;
  SD_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(int), s));
  static_assert(sizeof(A) == sizeof(long long), "the sums of an absent label are written as zero bits");
  hipLaunchKernelGGL(k_compact<M>, dim3((unsigned)((nl + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, (const int*)d_boxes, max_label, Z, Y, X, C, tiny,
                     whole, cut, counts, chunk_base, owner, may_chunk ? cap : 0, (long long*)d_sums, d_minmax);
  if (max_label > 0) {
    const int* lbl = (const int*)d_lbl;
    const int* tab = (const int*)d_boxes;
    const int wave_groups = (int)std::min<long long>((long long)cus * MS_WAVE_GROUPS_PER_CU, max_label);
    const int block_groups = (int)std::min<long long>((long long)cus * MS_BLOCK_GROUPS_PER_CU, max_label);
    hipLaunchKernelGGL((k_stats<T, A, M, TIER_WAVE>), dim3(wave_groups), dim3(64), 0, s, lbl, d_img, Z, Y, X, C, tab, (const int*)tiny,
                       (const int*)(counts + N_WAVE), (const int*)chunk_base, partial, d_sums, d_minmax);
    if (may_block)
      hipLaunchKernelGGL((k_stats<T, A, M, TIER_BLOCK>), dim3(block_groups), dim3(BLOCK), 0, s, lbl, d_img, Z, Y, X, C, tab, (const int*)whole,
                         (const int*)(counts + N_BLOCK), (const int*)chunk_base, partial, d_sums, d_minmax);
    if (may_chunk) {
      const int chunk_groups = std::min<int>(cus * MS_BLOCK_GROUPS_PER_CU, cap);
      hipLaunchKernelGGL((k_stats<T, A, M, TIER_CHUNK>), dim3(chunk_groups), dim3(BLOCK), 0, s, lbl, d_img, Z, Y, X, C, tab, (const int*)owner,
                         (const int*)(counts + N_CHUNKS), (const int*)chunk_base, partial, d_sums, d_minmax);
      hipLaunchKernelGGL((k_combine<A, M>), dim3(std::min<int>(cus, sd::div_up((long long)max_label * C, BLOCK))), dim3(BLOCK), 0, s, tab, Z, Y, X,
                         C, (const int*)cut, (const int*)(counts + N_CHUNKED), (const int*)chunk_base, (const Stat<A, M>*)partial, d_sums,
                         d_minmax);
    }
  }
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int sd_label_intensity_stats_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, const int32_t* d_boxes, const void* d_img,
                                               int dtype, int C, int64_t* d_isum2, double* d_fsum2, void* d_minmax, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_label_intensity_stats";
  if (!d_lbl || !d_boxes || !d_img || !d_minmax || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0) {
    sd::set_error("%s: null pointer, non-positive size or negative max_label", who);
    return -1;
  }
  if (dtype < 0 || dtype > 2 || C < 1 || C > MS_MAX_CHANNELS) { sd::set_error("%s: dtype outside 0 .. 2 or C outside 1 .. %d", who, (int)MS_MAX_CHANNELS); return -1; }
  if (dtype == 2 ? !d_fsum2 : !d_isum2) { sd::set_error("%s: no table for the sums of this dtype", who); return -1; }
  if ((long long)Z * Y * X > (1ll << 40) || (long long)Z * Y > INT_MAX) { sd::set_error("%s: image too large", who); return -1; }
  if (dtype == 0)
    return run<uint8_t, long long, int32_t>(d_lbl, Z, Y, X, max_label, d_boxes, (const uint8_t*)d_img, C, (long long*)d_isum2, (int32_t*)d_minmax, s);
  if (dtype == 1)
    return run<uint16_t, long long, int32_t>(d_lbl, Z, Y, X, max_label, d_boxes, (const uint16_t*)d_img, C, (long long*)d_isum2, (int32_t*)d_minmax, s);
  return run<float, double, float>(d_lbl, Z, Y, X, max_label, d_boxes, (const float*)d_img, C, d_fsum2, (float*)d_minmax, s);
}
