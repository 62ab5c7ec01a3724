// measure_rank.h -- the exact intensity percentiles of one labelled object (stardist_amd.utils.measure_labels(percentiles=)): which
// pixels belong to it, the key of a value, the digit plan of every tier, how a rank descends through the histograms, the two ranks and
// the weight of a percentile, the interpolation and the NaN rule.
//
// Everything here is __host__ __device__ and free of HIP headers when compiled by a host compiler: csrc/measure_rank.hip runs it with
// one thread per lane, tests/host/measure_rank_check.cpp with plain loops over the lanes, and tests/test_cpu_measure_percentiles.py
// compares the latter with the host function.
//
// Per object L (box from sd_label_boxes_device, clamped to the image by measure::box_of) and channel c:
//   members  the pixels p of the box with lbl[p] == L; n = their number, counted while the box is read (no table supplies it)
//   keys     selrank::key_of(img[p * C + c]): an unsigned integer that sorts like the value
//   ranks    for every q, selrank::lerp_plan(n, q, f32) gives the order statistics lo, hi and the weight t: numpy's `linear` method
//   result   integer images: lerp_f64(double(a), double(b), t); float32 images: lerp_f32(a, b, float(t)) (f32) or float(lerp_f64(a, b,
//            t)), widened to double; a = value of rank lo, b = value of rank hi
//   NaN      a NaN among the members makes every result of (L, c) NaN; so does n = 0 (a box without a pixel of L: no table of
//            sd_label_boxes_device has one)
// The order statistics are exact and every count is an integer, so the result is a function of (extents, lbl, img, q) alone: the tier
// an object is worked off in, the lane that reads a pixel and the order of the atomics do not show in it.
//
// Tiers, by the box (none of the limits is tuned: they follow from the LDS budget and from measure.h's chunk size):
//   sort     at most MR_SORT_KEYS pixels: the members' keys are compacted into LDS once (MR_SORT_KEYS * 4 bytes = 4 KiB per
//            workgroup of one wave, so that LDS admits the 32 waves a CU holds, as in measure.hip's wave tier) and sorted there; every rank is then one LDS read.  A sort rather than a radix
//            selection: all 2 n_q ranks come out of one staging with no histogram per rank, and uint16 and float32 need no digit
//            passes.  Up to MR_RANK_KEYS = 64 members (one per lane) every lane counts the keys that sort before its own and stores
//            its key there: two barriers.  Beyond, a bitonic network: log2(m) (log2(m) + 1) / 2 steps with a barrier each.
//   block    a box of one chunk (measure.h: at most MS_CHUNK_PIXELS pixels) beyond that, and any box the chunk workspace has no room
//            for: one workgroup of MR_BLOCK_LANES threads per (object, channel), one histogram pass over the box per digit,
//            histograms in LDS
//   chunked  a box of several chunks: the chunks are spread over the grid one digit pass at a time, their counts merged into the
//            histograms of the object's slot in a global workspace (MR_CHUNK_SLOTS slots, one per (object, channel)) by integer atomics
// Digit plan of the block and chunked tiers: MR_DIGIT_BITS = 8 bits per pass from the top of the key -- uint8 one pass, uint16 two,
// float32 four; MR_BINS = 256 counters per histogram.  Pass 0 counts every member (its total is n); in a later pass a member counts
// for the ranks whose digits so far equal its own, and ranks that still agree share one histogram: at most MR_MAX_RANKS = 2 * MR_MAX_Q
// histograms of 256 64-bit counters, 32 KiB.
#pragma once
#include <stdint.h>
#include "measure.h"
#include "select_rank.h"

#if defined(__HIPCC__)
#define MR_HD __host__ __device__ __forceinline__
#else
#define MR_HD inline
#endif

namespace mrank {

enum { MR_SORT_KEYS = 1024, MR_RANK_KEYS = 64, MR_SORT_LANES = 64, MR_BLOCK_LANES = 256, MR_DIGIT_BITS = 8, MR_BINS = 256, MR_MAX_Q = 8, MR_MAX_RANKS = 16,
       MR_CHUNK_SLOTS = 128 };
enum Tier { TIER_NONE = -1, TIER_SORT = 0, TIER_BLOCK = 1, TIER_CHUNKED = 2 };

// the tier of a box with room in the chunk workspace (without room a TIER_CHUNKED box is worked off as TIER_BLOCK)
MR_HD int tier_of(const measure::Box& b) {
  if (b.chunks == 0) return TIER_NONE;
  if (b.pixels <= (long long)MR_SORT_KEYS) return TIER_SORT;
  return b.chunks == 1 ? TIER_BLOCK : TIER_CHUNKED;
}

// ---- members and their keys
MR_HD bool member(const int32_t* __restrict__ lbl, long long p, int L) { return lbl[p] == L; }
MR_HD bool is_nan(uint8_t) { return false; }
MR_HD bool is_nan(uint16_t) { return false; }
MR_HD bool is_nan(float v) { return v != v; }

// ---- digit plan of the block and chunked tiers
MR_HD int n_passes(int dtype) { return dtype == selrank::DT_U8 ? 1 : dtype == selrank::DT_U16 ? 2 : 4; }
MR_HD int digit_shift(int dtype, int pass) { return MR_DIGIT_BITS * (n_passes(dtype) - 1 - pass); }
MR_HD uint32_t digit_of(uint32_t key, int dtype, int pass) { return (key >> digit_shift(dtype, pass)) & (uint32_t)(MR_BINS - 1); }
// the digits above `pass`, right-aligned (0 for pass 0)
MR_HD uint32_t prefix_of(uint32_t key, int dtype, int pass) { return pass == 0 ? 0u : key >> (digit_shift(dtype, pass) + MR_DIGIT_BITS); }

// ---- the selection state of one (object, channel): rank r = 2 j is the lower, 2 j + 1 the upper order statistic of q[j]
struct Sel {
  unsigned long long n;                    // members
  unsigned long long rank[MR_MAX_RANKS];   // rank among the members that share the prefix
  uint32_t prefix[MR_MAX_RANKS];           // digits found so far, right-aligned; after the last pass the key
};

MR_HD void sel_begin(Sel& s, unsigned long long n, const double* q, int n_q, bool f32) {
  s.n = n;
  for (int j = 0; j < n_q; ++j) {
    selrank::Lerp L;
    L.lo = L.hi = 0;
    if (n > 0) L = selrank::lerp_plan((long long)n, q[j], f32);
    s.rank[2 * j] = (unsigned long long)L.lo; s.rank[2 * j + 1] = (unsigned long long)L.hi;
    s.prefix[2 * j] = s.prefix[2 * j + 1] = 0;
  }
}

// histogram g belongs to the g-th distinct prefix in rank order: hist_of[r] = the histogram of rank r, lead[g] = its prefix; returns
// the number of histograms
MR_HD int sel_groups(const Sel& s, int n_ranks, int* hist_of, uint32_t* lead) {
  int nh = 0;
  for (int r = 0; r < n_ranks; ++r) {
    int g = 0;
    for (; g < nh; ++g)
      if (lead[g] == s.prefix[r]) break;
    if (g == nh) lead[nh++] = s.prefix[r];
    hist_of[r] = g;
  }
  return nh;
}
// the histogram a member with this prefix counts into, or -1
MR_HD int group_for(const uint32_t* lead, int nh, uint32_t prefix) {
  for (int g = 0; g < nh; ++g)
    if (lead[g] == prefix) return g;
  return -1;
}

// rank r descends one digit: hist = the histograms of this pass, [nh][MR_BINS]
MR_HD void sel_descend(Sel& s, int r, const unsigned long long* hist, const int* hist_of) {
  unsigned long long rest = s.rank[r];
  const int bin = selrank::find_bin(hist + (long long)hist_of[r] * MR_BINS, MR_BINS, &rest);
  s.rank[r] = rest;
  s.prefix[r] = (s.prefix[r] << MR_DIGIT_BITS) | (uint32_t)bin;
}

// ---- the result of one q from the keys of its two order statistics and the weight between them (no NaN among the members)
MR_HD double result_of(uint32_t ka, uint32_t kb, double t, int dtype, bool f32) {
  if (dtype == selrank::DT_F32) {
    const float a = selrank::f32_of_key(ka), b = selrank::f32_of_key(kb);
    const float res = f32 ? selrank::lerp_f32(a, b, (float)t) : (float)selrank::lerp_f64((double)a, (double)b, t);
    return (double)res;
  }
  return selrank::lerp_f64((double)ka, (double)kb, t);
}
// ... after the last digit pass of the block and chunked tiers (s.n > 0)
MR_HD double sel_result(const Sel& s, int j, double q, int dtype, bool f32) {
  const selrank::Lerp L = selrank::lerp_plan((long long)s.n, q, f32);
  return result_of(s.prefix[2 * j], s.prefix[2 * j + 1], L.t, dtype, f32);
}
MR_HD double nan_result() { return (double)__builtin_nanf(""); }

// ---- sort tier: a bitonic network over m = sort_size(n) keys, the tail padded with 0xffffffff (no rank reads it).  Step (k, j), k =
// 2, 4 .. m, j = k / 2 .. 1, has m / 2 independent exchanges t; the lanes share them out as t = lane, lane + lanes, ...
MR_HD unsigned sort_size(unsigned n) {
  unsigned m = 2;
  while (m < n) m <<= 1;
  return m;
}
MR_HD void bitonic_exchange(uint32_t* keys, unsigned k, unsigned j, unsigned t) {
  const unsigned i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), p = i | j;
  const bool up = (i & k) == 0;
  const uint32_t a = keys[i], b = keys[p];
  if ((a > b) == up) { keys[i] = b; keys[p] = a; }
}
// at most MR_RANK_KEYS = one key per lane: no network, lane t counts the keys that sort before its own (equal keys in staging order)
// and, once every lane has counted, stores its key at that position -- n reads of one LDS word by all lanes at once, two barriers
MR_HD unsigned rank_position(const uint32_t* keys, unsigned n, unsigned t) {
  const uint32_t k = keys[t];
  unsigned pos = 0;
  for (unsigned j = 0; j < n; ++j) pos += (unsigned)((keys[j] < k) | ((keys[j] == k) & (j < t)));
  return pos;
}

// ---- block and chunked tiers: what lane `lane` of `lanes` counts for channel c of chunk `chunk` in pass `pass`: add(g * MR_BINS + digit)
// for every member whose prefix has a histogram g; *nan is set if a member is a NaN.  T: the image's element type
template <typename T, typename Add>
MR_HD void lane_histogram(const int32_t* __restrict__ lbl, const T* __restrict__ img, int C, int c, int Y, int X, const measure::Box& b, int chunk,
                          int L, int lane, int lanes, int dtype, int pass, const uint32_t* lead, int nh, Add& add, int* nan) {
  const int row0 = chunk * b.chunk_rows;
  const unsigned n = measure::chunk_pixels(b, chunk), bx = (unsigned)b.bx;
  for (unsigned i = (unsigned)lane; i < n; i += (unsigned)lanes) {
    const unsigned r = i / bx, x = i - r * bx;
    const long long p = measure::pixel_offset(b, Y, X, row0 + (int)r, (int)x);
    if (!member(lbl, p, L)) continue;
    const T v = img[p * C + c];
    if (is_nan(v)) *nan = 1;
    const uint32_t key = selrank::key_of(v);
    const int g = pass == 0 ? 0 : group_for(lead, nh, prefix_of(key, dtype, pass));
    if (g >= 0) add(g * MR_BINS + (int)digit_of(key, dtype, pass));
  }
}

}  // namespace mrank
