// measure_rank.hip -- exact intensity percentiles of every labelled object (stardist_amd.utils.measure_labels(percentiles=)):
//
//   sd_label_percentiles_device   out[l][c][j] = np.percentile(values of label l in channel c, q[j]) (method 'linear') for l = 0 .. max_label
//
// A segmented selection over the box table of sd_label_boxes_device, one per (object, channel); what decides a result -- members, keys,
// digit plan, descent, ranks, interpolation, the NaN rule, the tier limits -- is csrc/measure_rank.h's, shared with the host harness of
// the tests.  Launches of one call, all on the caller's stream, nothing read back to the host:
//   k_plan      one thread per table row: an absent label gets NaN; a label present joins one of three device lists with device-side
//               counts (one atomic per wave and list, as csrc/measure.hip's k_compact).  A box of several chunks reserves C slots of the
//               chunk workspace and a range of the chunk list; one that finds no room joins the block list.
//   k_sort      single-wave workgroups, many per CU -- nuclei are of this kind: the members' keys are compacted into LDS by wave
//               ballots (one read of the box per channel), sorted there as measure_rank.h states (up to 64 keys by counting, beyond
//               by its bitonic network), and lane j reads the two order statistics of q[j] from LDS.  4 KiB of LDS per workgroup.
//               Latency-bound, as measure.hip's wave tier: a few dependent label -> value loads per lane, then LDS steps between
//               barriers of one wave.
//   k_block     256 threads per (object, channel): per digit one pass over the box into at most 16 LDS histograms of 64-bit counters
//               (32 KiB), then thread r descends rank r
//   k_chunk_hist / k_chunk_descend   per digit: one workgroup per (chunk, channel) counts into 32-bit LDS histograms (a chunk has fewer
//               than 2^31 pixels) and adds the non-zero counters to the slot's 64-bit histograms with integer atomics; then one small
//               workgroup per slot descends its ranks, clears the histograms for the next digit and, after the last, writes the row
// Counting is in integers only; no floating-point atomic; 64-bit offsets.
#include "common.h"
#include "measure_rank.h"
#include "stardist_hip.h"
#include <limits.h>
#include <math.h>
#include <algorithm>

using namespace mrank;
using measure::Box;
using measure::box_of;

namespace {

typedef unsigned long long u64;
enum { BLOCK = MR_BLOCK_LANES, SORT_BATCH = 4, MR_SORT_GROUPS_PER_CU = 32, MR_BLOCK_GROUPS_PER_CU = 4, MR_MAX_CHANNELS = 64 };
enum Count { N_SORT = 0, N_BLOCK = 1, N_CHUNKED = 2, N_CHUNKS = 3, N_SLOTS = 4, N_COUNTS = 5 };

struct Params {
  double q[MR_MAX_Q];
  int n_q, f32, dtype;
};

// reserve `want` of a counter that may not pass `cap`: the base, or -1
__device__ __forceinline__ int reserve(int* counter, int want, int cap) {
  int base = *counter;
  for (;;) {
    if (base + want > cap) return -1;
    const int seen = atomicCAS(counter, base, base + want);
    if (seen == base) return base;
    base = seen;
  }
}

__global__ void __launch_bounds__(BLOCK) k_plan(const int* __restrict__ tab, int max_label, int Z, int Y, int X, int C, int n_q, int* __restrict__ sortl,
                                                int* __restrict__ blockl, int* __restrict__ cut, int* counts, int* __restrict__ chunk_base,
                                                int* __restrict__ slot_base, int* __restrict__ owner, int cap, int slots, double* __restrict__ out) {
  const long long l = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int kind = -1;
  if (l <= max_label) {
    const Box b = box_of(tab + 6 * l, Z, Y, X);
    const int tier = l == 0 ? (int)TIER_NONE : tier_of(b);
    if (tier == TIER_NONE) {
      const long long at = l * C * n_q;
      for (int k = 0; k < C * n_q; ++k) out[at + k] = nan_result();
    } else if (tier == TIER_SORT) {
      kind = N_SORT;
    } else if (tier == TIER_BLOCK) {
      kind = N_BLOCK;
    } else {
      // the slots first: slots left over by a label that then finds no room for its chunks are never visited
      const int sb = reserve(&counts[N_SLOTS], C, slots);
      const int base = sb < 0 ? -1 : reserve(&counts[N_CHUNKS], b.chunks, cap);
      if (base < 0) {
        kind = N_BLOCK;
      } else {
        cut[atomicAdd(&counts[N_CHUNKED], 1)] = (int)l;
        chunk_base[l] = base;
        slot_base[l] = sb;
        for (int k = 0; k < b.chunks; ++k) owner[base + k] = (int)l;
      }
    }
  }
  for (int which = N_SORT; which <= N_BLOCK; ++which) {
    const u64 mask = __ballot(kind == which);
    if (!mask) continue;
    const int leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&counts[which], __popcll(mask));
    base = __shfl(base, leader);
    if (kind == which) (which == N_SORT ? sortl : blockl)[base + __popcll(mask & ((1ull << lane) - 1ull))] = (int)l;
  }
}

// ------------------------------------------------------------------------------------------------------------------ sort tier
template <typename T>
__global__ void __launch_bounds__(MR_SORT_LANES) k_sort(const int* __restrict__ lbl, const T* __restrict__ img, int Z, int Y, int X, int C,
                                                        const int* __restrict__ tab, const int* __restrict__ list, const int* __restrict__ count,
                                                        Params P, double* __restrict__ out) {
  __shared__ uint32_t keys[MR_SORT_KEYS];
  const int lane = threadIdx.x;
  const int total = *count;
  for (int it = blockIdx.x; it < total; it += gridDim.x) {
    const int L = list[it];
    const Box b = box_of(tab + 6ll * L, Z, Y, X);
    // tier_of(b) == TIER_SORT for every entry of the list; a table that changed since k_plan must not make the staging leave keys[]
    const unsigned npix = b.pixels <= (long long)MR_SORT_KEYS ? (unsigned)b.pixels : 0u;
    const unsigned bx = (unsigned)(b.bx > 0 ? b.bx : 1);
    for (int c = 0; c < C; ++c) {
      unsigned n = 0;
      int nan = 0;
      // SORT_BATCH steps of 64 pixels at a time: their labels and values are all loaded before the first vote, and a value is loaded
      // whatever its label (a pixel of the clamped box), so that an object costs one round of loads in flight, not two per step
      for (unsigned base = 0; base < npix; base += SORT_BATCH * MR_SORT_LANES) {
        bool in[SORT_BATCH];
        T v[SORT_BATCH];
#pragma unroll
        for (int k = 0; k < SORT_BATCH; ++k) {
          const unsigned i = base + (unsigned)k * MR_SORT_LANES + (unsigned)lane;
          in[k] = false;
          v[k] = T(0);
          if (i < npix) {
            const unsigned r = i / bx, x = i - r * bx;
            const long long p = measure::pixel_offset(b, Y, X, (int)r, (int)x);
            in[k] = member(lbl, p, L);
            v[k] = img[p * C + c];
          }
        }
#pragma unroll
        for (int k = 0; k < SORT_BATCH; ++k) {
          if (in[k] && is_nan(v[k])) nan = 1;
          const u64 mask = __ballot(in[k]);
          if (in[k]) keys[n + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = selrank::key_of(v[k]);
          n += (unsigned)__popcll(mask);
        }
      }
      nan = __any(nan);
      const unsigned m = sort_size(n);
      for (unsigned i = n + (unsigned)lane; i < m; i += MR_SORT_LANES) keys[i] = 0xffffffffu;
      __syncthreads();
      if (n > 1 && !nan) {
        if (n <= (unsigned)MR_RANK_KEYS) {
          const bool mine = (unsigned)lane < n;
          const uint32_t key = mine ? keys[lane] : 0u;
          const unsigned pos = mine ? rank_position(keys, n, (unsigned)lane) : 0u;
          __syncthreads();
          if (mine) keys[pos] = key;
          __syncthreads();
        } else {
          for (unsigned k = 2; k <= m; k <<= 1)
            for (unsigned j = k >> 1; j > 0; j >>= 1) {
              for (unsigned t = (unsigned)lane; t < m / 2; t += MR_SORT_LANES) bitonic_exchange(keys, k, j, t);
              __syncthreads();
            }
        }
      }
      if (lane < P.n_q) {
        double res = nan_result();
        if (n > 0 && !nan) {
          const selrank::Lerp pl = selrank::lerp_plan((long long)n, P.q[lane], P.f32 != 0);
          res = result_of(keys[pl.lo], keys[pl.hi], pl.t, P.dtype, P.f32 != 0);
        }
        out[((long long)L * C + c) * P.n_q + lane] = res;
      }
      __syncthreads();                                                     // the next channel rewrites keys[]
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ block tier
struct AddLds64 {
  u64* h;
  __device__ __forceinline__ void operator()(int at) { atomicAdd(&h[at], 1ull); }
};
struct AddLds32 {
  unsigned* h;
  __device__ __forceinline__ void operator()(int at) { atomicAdd(&h[at], 1u); }
};

template <typename T>
__global__ void __launch_bounds__(BLOCK) k_block(const int* __restrict__ lbl, const T* __restrict__ img, int Z, int Y, int X, int C,
                                                 const int* __restrict__ tab, const int* __restrict__ list, const int* __restrict__ count, Params P,
                                                 double* __restrict__ out) {
  __shared__ u64 hist[MR_MAX_RANKS * MR_BINS];
  __shared__ Sel sel;
  __shared__ int hist_of[MR_MAX_RANKS];
  __shared__ uint32_t lead[MR_MAX_RANKS];
  __shared__ int s_nh, s_nan;
  const int tid = threadIdx.x, n_ranks = 2 * P.n_q, passes = n_passes(P.dtype);
  const long long total = (long long)*count * C;
  for (long long it = blockIdx.x; it < total; it += gridDim.x) {
    const int L = list[it / C], c = (int)(it % C);
    const Box b = box_of(tab + 6ll * L, Z, Y, X);
    if (tid == 0) s_nan = 0;
    for (int pass = 0; pass < passes; ++pass) {
      if (tid == 0) {
        if (pass == 0) { lead[0] = 0; s_nh = 1; }
        else s_nh = sel_groups(sel, n_ranks, hist_of, lead);
      }
      __syncthreads();
      const int nh = s_nh;
      for (int i = tid; i < nh * MR_BINS; i += BLOCK) hist[i] = 0;
      __syncthreads();
      AddLds64 add = {hist};
      int nan = 0;
      for (int k = 0; k < b.chunks; ++k) lane_histogram<T>(lbl, img, C, c, Y, X, b, k, L, tid, BLOCK, P.dtype, pass, lead, nh, add, &nan);
      if (nan) s_nan = 1;
      __syncthreads();
      if (pass == 0) {
        if (tid == 0) {
          u64 n = 0;
          for (int i = 0; i < MR_BINS; ++i) n += hist[i];
          sel_begin(sel, n, P.q, P.n_q, P.f32 != 0);
          for (int r = 0; r < n_ranks; ++r) hist_of[r] = 0;
        }
        __syncthreads();
      }
      if (tid < n_ranks && sel.n > 0) sel_descend(sel, tid, hist, hist_of);
      __syncthreads();
    }
    if (tid < P.n_q) {
      double res = nan_result();
      if (sel.n > 0 && !s_nan) res = sel_result(sel, tid, P.q[tid], P.dtype, P.f32 != 0);
      out[((long long)L * C + c) * P.n_q + tid] = res;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------ chunked tier
template <typename T>
__global__ void __launch_bounds__(BLOCK) k_chunk_hist(const int* __restrict__ lbl, const T* __restrict__ img, int Z, int Y, int X, int C,
                                                      const int* __restrict__ tab, const int* __restrict__ owner, const int* __restrict__ count,
                                                      const int* __restrict__ chunk_base, const int* __restrict__ slot_base, Params P, int pass,
                                                      const Sel* __restrict__ sels, u64* __restrict__ ghist, int* __restrict__ gnan) {
  __shared__ unsigned hist[MR_MAX_RANKS * MR_BINS];
  __shared__ int hist_of[MR_MAX_RANKS];
  __shared__ uint32_t lead[MR_MAX_RANKS];
  __shared__ int s_nh, s_nan;
  const int tid = threadIdx.x, n_ranks = 2 * P.n_q;
  const long long total = (long long)*count * C;
  for (long long it = blockIdx.x; it < total; it += gridDim.x) {
    const int e = (int)(it / C), c = (int)(it % C);
    const int L = owner[e];
    const Box b = box_of(tab + 6ll * L, Z, Y, X);
    const int chunk = e - chunk_base[L], slot = slot_base[L] + c;
    if (tid == 0) {
      s_nan = 0;
      if (pass == 0) { lead[0] = 0; s_nh = 1; }
      else s_nh = sel_groups(sels[slot], n_ranks, hist_of, lead);
    }
    __syncthreads();
    const int nh = s_nh;
    for (int i = tid; i < nh * MR_BINS; i += BLOCK) hist[i] = 0;
    __syncthreads();
    AddLds32 add = {hist};
    int nan = 0;
    if (chunk >= 0 && chunk < b.chunks && (pass == 0 || sels[slot].n > 0))
      lane_histogram<T>(lbl, img, C, c, Y, X, b, chunk, L, tid, BLOCK, P.dtype, pass, lead, nh, add, &nan);
    if (nan) s_nan = 1;
    __syncthreads();
    u64* g = ghist + (long long)slot * n_ranks * MR_BINS;
    for (int i = tid; i < nh * MR_BINS; i += BLOCK) {
      const unsigned cnt = hist[i];
      if (cnt) atomicAdd(&g[i], (u64)cnt);
    }
    if (tid == 0 && s_nan) atomicOr(&gnan[slot], 1);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64) k_chunk_descend(int C, const int* __restrict__ cut, const int* __restrict__ count,
                                                      const int* __restrict__ slot_base, Params P, int pass, int last, Sel* __restrict__ sels,
                                                      u64* __restrict__ ghist, const int* __restrict__ gnan, double* __restrict__ out) {
  __shared__ Sel sel;
  __shared__ int hist_of[MR_MAX_RANKS];
  __shared__ uint32_t lead[MR_MAX_RANKS];
  __shared__ int s_nh;
  const int tid = threadIdx.x, n_ranks = 2 * P.n_q;
  const long long total = (long long)*count * C;
  for (long long it = blockIdx.x; it < total; it += gridDim.x) {
    const int L = cut[it / C], c = (int)(it % C);
    const int slot = slot_base[L] + c;
    u64* g = ghist + (long long)slot * n_ranks * MR_BINS;
    if (tid == 0) {
      if (pass == 0) {
        u64 n = 0;
        for (int i = 0; i < MR_BINS; ++i) n += g[i];
        sel_begin(sel, n, P.q, P.n_q, P.f32 != 0);
        for (int r = 0; r < n_ranks; ++r) hist_of[r] = 0;
        s_nh = 1;
      } else {
        sel = sels[slot];
        s_nh = sel_groups(sel, n_ranks, hist_of, lead);
      }
    }
    __syncthreads();
    if (tid < n_ranks && sel.n > 0) sel_descend(sel, tid, g, hist_of);
    __syncthreads();
    if (last) {
      if (tid < P.n_q) {
        double res = nan_result();
        if (sel.n > 0 && !gnan[slot]) res = sel_result(sel, tid, P.q[tid], P.dtype, P.f32 != 0);
        out[((long long)L * C + c) * P.n_q + tid] = res;
      }
    } else {
      if (tid == 0) sels[slot] = sel;
      for (int i = tid; i < s_nh * MR_BINS; i += 64) g[i] = 0;
    }
    __syncthreads();
  }
}

template <typename T>
int run(const int32_t* d_lbl, int Z, int Y, int X, int max_label, const int32_t* d_boxes, const T* d_img, int C, const Params& P, double* d_out,
        hipStream_t s) {
  const int cus = sd::cu_count();
  if (cus < 0) return -1;
  const long long n = (long long)Z * Y * X;
  // room for the chunks of the boxes of several chunks, as csrc/measure.hip: a box has at most pixels / (MS_CHUNK_PIXELS / 2) + 1 of them
  const int cap = (int)std::min<long long>(n / (measure::MS_CHUNK_PIXELS / 4) + 1024, INT_MAX / 2);
  const bool may_block = n > (long long)MR_SORT_KEYS, may_chunk = n > (long long)measure::MS_CHUNK_PIXELS;
  const int n_ranks = 2 * P.n_q;
  sd::Arena& ar = sd::arena();
  if (ar.begin(s)) return -1;
  const size_t nl = (size_t)max_label + 1;
  int* sortl = ar.take_n<int>(nl);
  int* blockl = ar.take_n<int>(nl);
  int* cut = ar.take_n<int>(nl);
  int* chunk_base = ar.take_n<int>(nl);
  int* slot_base = ar.take_n<int>(nl);
  int* counts = ar.take_n<int>(N_COUNTS);
  int* owner = ar.take_n<int>(may_chunk ? cap : 1);
  Sel* sels = ar.take_n<Sel>(may_chunk ? MR_CHUNK_SLOTS : 1);
  const size_t hist_words = may_chunk ? (size_t)MR_CHUNK_SLOTS * n_ranks * MR_BINS : 1;
  u64* ghist = ar.take_n<u64>(hist_words);
  int* gnan = ar.take_n<int>(MR_CHUNK_SLOTS);
  if (!sortl || !blockl || !cut || !chunk_base || !slot_base || !counts || !owner || !sels || !ghist || !gnan) return -1;
  SD_CHECK(hipMemsetAsync(counts, 0, N_COUNTS * sizeof(int), s));
  if (may_chunk) {
    SD_CHECK(hipMemsetAsync(ghist, 0, hist_words * sizeof(u64), s));
    SD_CHECK(hipMemsetAsync(gnan, 0, MR_CHUNK_SLOTS * sizeof(int), s));
  }
  const int* lbl = (const int*)d_lbl;
  const int* tab = (const int*)d_boxes;
  hipLaunchKernelGGL(k_plan, dim3((unsigned)((nl + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, tab, max_label, Z, Y, X, C, P.n_q, sortl, blockl, cut, counts,
                     chunk_base, slot_base, owner, may_chunk ? cap : 0, may_chunk ? (int)MR_CHUNK_SLOTS : 0, d_out);
  if (max_label > 0) {
    const int sort_groups = (int)std::min<long long>((long long)cus * MR_SORT_GROUPS_PER_CU, max_label);
    const int block_groups = (int)std::min<long long>((long long)cus * MR_BLOCK_GROUPS_PER_CU, (long long)max_label * C);
    hipLaunchKernelGGL((k_sort<T>), dim3(sort_groups), dim3(MR_SORT_LANES), 0, s, lbl, d_img, Z, Y, X, C, tab, (const int*)sortl,
                       (const int*)(counts + N_SORT), P, d_out);
    if (may_block)
      hipLaunchKernelGGL((k_block<T>), dim3(block_groups), dim3(BLOCK), 0, s, lbl, d_img, Z, Y, X, C, tab, (const int*)blockl,
                         (const int*)(counts + N_BLOCK), P, d_out);
    if (may_chunk) {
      const int hist_groups = (int)std::min<long long>((long long)cus * MR_BLOCK_GROUPS_PER_CU * 2, (long long)cap * C);
      const int passes = n_passes(P.dtype);
      for (int pass = 0; pass < passes; ++pass) {
        hipLaunchKernelGGL((k_chunk_hist<T>), dim3(hist_groups), dim3(BLOCK), 0, s, lbl, d_img, Z, Y, X, C, tab, (const int*)owner,
                           (const int*)(counts + N_CHUNKS), (const int*)chunk_base, (const int*)slot_base, P, pass, (const Sel*)sels, ghist, gnan);
        hipLaunchKernelGGL(k_chunk_descend, dim3(MR_CHUNK_SLOTS), dim3(64), 0, s, C, (const int*)cut, (const int*)(counts + N_CHUNKED),
                           (const int*)slot_base, P, pass, pass == passes - 1 ? 1 : 0, sels, ghist, (const int*)gnan, d_out);
      }
    }
  }
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int sd_label_percentiles_device(const int32_t* d_lbl, int Z, int Y, int X, int max_label, const int32_t* d_boxes, const void* d_img,
                                           int dtype, int C, const double* h_q, int n_q, int interp_f32, double* d_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_label_percentiles";
  if (!d_lbl || !d_boxes || !d_img || !h_q || !d_out || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0) {
    sd::set_error("%s: null pointer, non-positive size or negative max_label", who);
    return -1;
  }
  if (dtype < 0 || dtype > 2 || C < 1 || C > MR_MAX_CHANNELS) { sd::set_error("%s: dtype outside 0 .. 2 or C outside 1 .. %d", who, (int)MR_MAX_CHANNELS); return -1; }
  if (n_q < 1 || n_q > MR_MAX_Q) { sd::set_error("%s: n_q outside 1 .. %d", who, (int)MR_MAX_Q); return -1; }
  Params P;
  for (int j = 0; j < MR_MAX_Q; ++j) P.q[j] = 0.0;
  for (int j = 0; j < n_q; ++j) {
    if (!(h_q[j] >= 0.0 && h_q[j] <= 100.0)) { sd::set_error("%s: percentiles must be finite and in the range [0, 100]", who); return -1; }
    P.q[j] = h_q[j];
  }
  if ((long long)Z * Y * X > (1ll << 40) || (long long)Z * Y > INT_MAX) { sd::set_error("%s: image too large", who); return -1; }
  P.n_q = n_q;
  P.dtype = dtype;
  P.f32 = (dtype == selrank::DT_F32 && interp_f32) ? 1 : 0;
  if (dtype == 0) return run<uint8_t>(d_lbl, Z, Y, X, max_label, d_boxes, (const uint8_t*)d_img, C, P, d_out, s);
  if (dtype == 1) return run<uint16_t>(d_lbl, Z, Y, X, max_label, d_boxes, (const uint16_t*)d_img, C, P, d_out, s);
  return run<float>(d_lbl, Z, Y, X, max_label, d_boxes, (const float*)d_img, C, P, d_out, s);
}
