// Host harness of stardist_amd/csrc/measure_rank.h: what csrc/measure_rank.hip does -- boxes, tiers, the staging and the bitonic network
// of the sort tier, the digit passes of the block tier, the per-chunk histograms of the chunked tier merged into a slot, the descent of
// the ranks, the interpolation, the NaN rule -- with plain loops in place of threads.  Built by tests/test_cpu_measure_percentiles.py
// (g++ -ffp-contract=off) as a shared library; with -DMEASURE_RANK_CHECK_MAIN it is a stand-alone program (for a sanitizer build) that
// runs a small scene of every image type through every tier and compares with a sort written out here.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../stardist_amd/csrc/measure_rank.h"

using namespace mrank;
using measure::Box;
using measure::box_of;

namespace {

typedef unsigned long long u64;

void boxes_of(const int32_t* lbl, int Z, int Y, int X, int max_label, int32_t* boxes) {
  for (long long i = 0; i < 6ll * (max_label + 1ll); ++i) boxes[i] = (i % 6) < 3 ? INT_MAX : 0;
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x) {
        const int l = lbl[((long long)z * Y + y) * X + x];
        if (l <= 0 || l > max_label) continue;
        int32_t* t = boxes + 6ll * l;
        if (z < t[0]) t[0] = z;
        if (y < t[1]) t[1] = y;
        if (x < t[2]) t[2] = x;
        if (z + 1 > t[3]) t[3] = z + 1;
        if (y + 1 > t[4]) t[4] = y + 1;
        if (x + 1 > t[5]) t[5] = x + 1;
      }
}

struct Add64 {
  u64* h;
  void operator()(int at) { ++h[at]; }
};
struct Add32 {
  unsigned* h;
  void operator()(int at) { ++h[at]; }
};

struct Job {
  const int32_t* lbl;
  int Z, Y, X, C, dtype, n_q, f32;
  const double* q;
};

void store(const Job& J, const Sel& sel, int nan, long long l, int c, double* out) {
  for (int j = 0; j < J.n_q; ++j) {
    double res = nan_result();
    if (sel.n > 0 && !nan) res = sel_result(sel, j, J.q[j], J.dtype, J.f32 != 0);
    out[(l * J.C + c) * J.n_q + j] = res;
  }
}

// k_sort: 64 lanes stage the box in steps of 64 pixels (the ballot puts lane t's key behind those of the lanes below it), then share out
// the exchanges of every step of the network
template <typename T>
void sort_tier(const Job& J, const T* img, const Box& b, int L, int c, double* out) {
  std::vector<uint32_t> keys(MR_SORT_KEYS);
  const unsigned npix = (unsigned)b.pixels, bx = (unsigned)b.bx;
  unsigned n = 0;
  int nan = 0;
  for (unsigned base = 0; base < npix; base += MR_SORT_LANES)
    for (unsigned lane = 0; lane < MR_SORT_LANES; ++lane) {
      const unsigned i = base + lane;
      if (i >= npix) continue;
      const unsigned r = i / bx, x = i - r * bx;
      const long long p = measure::pixel_offset(b, J.Y, J.X, (int)r, (int)x);
      if (!member(J.lbl, p, L)) continue;
      const T v = img[p * J.C + c];
      if (is_nan(v)) nan = 1;
      keys[n++] = selrank::key_of(v);
    }
  const unsigned m = sort_size(n);
  for (unsigned i = n; i < m; ++i) keys[i] = 0xffffffffu;
  if (n > 1 && !nan) {
    if (n <= (unsigned)MR_RANK_KEYS) {
      uint32_t key[MR_RANK_KEYS];
      unsigned pos[MR_RANK_KEYS];
      for (unsigned lane = 0; lane < n; ++lane) { key[lane] = keys[lane]; pos[lane] = rank_position(keys.data(), n, lane); }
      for (unsigned lane = 0; lane < n; ++lane) keys[pos[lane]] = key[lane];
    } else {
      for (unsigned k = 2; k <= m; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1)
          for (unsigned lane = 0; lane < MR_SORT_LANES; ++lane)
            for (unsigned t = lane; t < m / 2; t += MR_SORT_LANES) bitonic_exchange(keys.data(), k, j, t);
    }
  }
  for (int j = 0; j < J.n_q; ++j) {
    double res = nan_result();
    if (n > 0 && !nan) {
      const selrank::Lerp pl = selrank::lerp_plan((long long)n, J.q[j], J.f32 != 0);
      res = result_of(keys[pl.lo], keys[pl.hi], pl.t, J.dtype, J.f32 != 0);
    }
    out[((long long)L * J.C + c) * J.n_q + j] = res;
  }
}

// k_block (chunked = false): 256 lanes over chunk after chunk into 64-bit histograms; k_chunk_hist / k_chunk_descend (chunked = true):
// the chunks in descending order, each into 32-bit histograms of its own that are then added to the slot's
template <typename T>
void radix_tiers(const Job& J, const T* img, const Box& b, int L, int c, bool chunked, double* out) {
  std::vector<u64> hist((size_t)MR_MAX_RANKS * MR_BINS);
  std::vector<unsigned> part((size_t)MR_MAX_RANKS * MR_BINS);
  Sel sel;
  memset(&sel, 0, sizeof sel);
  int hist_of[MR_MAX_RANKS] = {0};
  uint32_t lead[MR_MAX_RANKS] = {0};
  const int n_ranks = 2 * J.n_q;
  int nan = 0;
  for (int pass = 0; pass < n_passes(J.dtype); ++pass) {
    int nh = 1;
    lead[0] = 0;
    if (pass > 0) nh = sel_groups(sel, n_ranks, hist_of, lead);
    for (int i = 0; i < nh * MR_BINS; ++i) hist[i] = 0;
    if (!chunked) {
      Add64 add = {hist.data()};
      for (int k = 0; k < b.chunks; ++k)
        for (int t = 0; t < MR_BLOCK_LANES; ++t)
          lane_histogram<T>(J.lbl, img, J.C, c, J.Y, J.X, b, k, L, t, MR_BLOCK_LANES, J.dtype, pass, lead, nh, add, &nan);
    } else {
      for (int k = b.chunks - 1; k >= 0; --k) {
        for (int i = 0; i < nh * MR_BINS; ++i) part[i] = 0;
        Add32 add = {part.data()};
        for (int t = MR_BLOCK_LANES - 1; t >= 0; --t)
          lane_histogram<T>(J.lbl, img, J.C, c, J.Y, J.X, b, k, L, t, MR_BLOCK_LANES, J.dtype, pass, lead, nh, add, &nan);
        for (int i = 0; i < nh * MR_BINS; ++i) hist[i] += part[i];
      }
    }
    if (pass == 0) {
      u64 n = 0;
      for (int i = 0; i < MR_BINS; ++i) n += hist[i];
      sel_begin(sel, n, J.q, J.n_q, J.f32 != 0);
      for (int r = 0; r < n_ranks; ++r) hist_of[r] = 0;
    }
    for (int r = 0; r < n_ranks && sel.n > 0; ++r) sel_descend(sel, r, hist.data(), hist_of);
  }
  store(J, sel, nan, L, c, out);
}

template <typename T>
void percentiles(const Job& J, int max_label, const T* img, int force, int slots, double* out, int* tiers) {
  std::vector<int32_t> boxes(6 * ((size_t)max_label + 1));
  boxes_of(J.lbl, J.Z, J.Y, J.X, max_label, boxes.data());
  int used = 0;
  for (long long l = 0; l <= max_label; ++l) {
    const Box b = box_of(boxes.data() + 6 * l, J.Z, J.Y, J.X);
    int tier = l == 0 ? (int)TIER_NONE : tier_of(b);
    if (tier == TIER_NONE) {
      for (int k = 0; k < J.C * J.n_q; ++k) out[l * J.C * J.n_q + k] = nan_result();
      continue;
    }
    if (force == TIER_BLOCK || force == TIER_CHUNKED) tier = force;
    if (tier == TIER_CHUNKED) {
      if (used + J.C > slots) tier = TIER_BLOCK;
      else used += J.C;
    }
    if (tiers) ++tiers[tier];
    for (int c = 0; c < J.C; ++c) {
      if (tier == TIER_SORT) sort_tier<T>(J, img, b, (int)l, c, out);
      else radix_tiers<T>(J, img, b, (int)l, c, tier == TIER_CHUNKED, out);
    }
  }
}

}  // namespace

extern "C" {

int mr_sort_keys() { return MR_SORT_KEYS; }
int mr_chunk_slots() { return MR_CHUNK_SLOTS; }
int mr_chunk_pixels() { return measure::MS_CHUNK_PIXELS; }
int mr_max_q() { return MR_MAX_Q; }
int mr_rank_keys() { return MR_RANK_KEYS; }

// the table of sd_label_percentiles_device, NaN rows included.  force: -1 = every object in the tier of its box, 1 = every object in the
// block tier, 2 = every object in the chunked tier (while slots last); slots: the capacity of the chunk workspace, < 0 = the header's;
// tiers (optional, [3]): how many objects each tier worked off
int mr_percentiles(const int32_t* lbl, int Z, int Y, int X, int max_label, const void* img, int dtype, int C, const double* q, int n_q, int f32,
                   int force, int slots, double* out, int* tiers) {
  if (!lbl || !img || !q || !out || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0 || dtype < 0 || dtype > 2 || C < 1 || n_q < 1 || n_q > MR_MAX_Q)
    return -1;
  for (int j = 0; j < n_q; ++j)
    if (!(q[j] >= 0.0 && q[j] <= 100.0)) return -1;
  if (tiers) tiers[0] = tiers[1] = tiers[2] = 0;
  const Job J = {lbl, Z, Y, X, C, dtype, n_q, (dtype == selrank::DT_F32 && f32) ? 1 : 0, q};
  if (slots < 0) slots = MR_CHUNK_SLOTS;
  if (dtype == 0) percentiles<uint8_t>(J, max_label, (const uint8_t*)img, force, slots, out, tiers);
  else if (dtype == 1) percentiles<uint16_t>(J, max_label, (const uint16_t*)img, force, slots, out, tiers);
  else percentiles<float>(J, max_label, (const float*)img, force, slots, out, tiers);
  return 0;
}

}  // extern "C"

#ifdef MEASURE_RANK_CHECK_MAIN
#include <math.h>
#include <stdio.h>
#include <algorithm>
// 70 x 1100: a frame around the whole image (several chunks, few pixels), a solid block of one chunk, small squares, a one-pixel object,
// and for float32 a NaN in one square and +inf twice in another; every image type, every tier, against std::sort and the interpolation
// written out
template <typename T>
double brute(std::vector<T> v, double q, int dtype, bool f32) {
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i] != v[i]) return nan_result();
  std::sort(v.begin(), v.end());
  const selrank::Lerp L = selrank::lerp_plan((long long)v.size(), q, f32);
  const T a = v[L.lo], b = v[L.hi];
  if (dtype == 2) return (double)(f32 ? selrank::lerp_f32((float)a, (float)b, (float)L.t) : (float)selrank::lerp_f64((double)a, (double)b, L.t));
  return selrank::lerp_f64((double)a, (double)b, L.t);
}

template <typename T>
int check(const std::vector<int32_t>& lbl, int Y, int X, int top, const std::vector<T>& img, int dtype, int C) {
  const double q[5] = {0.0, 25.0, 50.0, 99.8, 100.0};
  int bad = 0;
  for (int force = -1; force <= 2; ++force) {
    if (force == 0) continue;
    for (int f32 = 0; f32 < 2; ++f32) {
      std::vector<double> out((size_t)(top + 1) * C * 5, -7.0);
      int tiers[3];
      if (mr_percentiles(lbl.data(), 1, Y, X, top, img.data(), dtype, C, q, 5, f32, force, force == 2 ? 3 * C : -1, out.data(), tiers)) ++bad;
      if (force == -1 && !(tiers[0] && tiers[1] && tiers[2])) ++bad;
      for (int l = 0; l <= top; ++l)
        for (int c = 0; c < C; ++c) {
          std::vector<T> v;
          for (size_t p = 0; p < lbl.size(); ++p)
            if (lbl[p] == l) v.push_back(img[p * C + c]);
          for (int j = 0; j < 5; ++j) {
            const double got = out[((size_t)l * C + c) * 5 + j];
            const double want = (l == 0 || v.empty()) ? nan_result() : brute<T>(v, q[j], dtype, dtype == 2 && f32);
            if (!(got == want || (got != got && want != want))) {
              if (++bad < 5) printf("dtype %d force %d label %d channel %d q %g: %.17g, not %.17g\n", dtype, force, l, c, q[j], got, want);
            }
          }
        }
    }
  }
  printf("dtype %d: %s\n", dtype, bad ? "WRONG" : "ok");
  return bad;
}

int main() {
  const int Y = 70, X = 1100, top = 30;
  std::vector<int32_t> lbl((size_t)Y * X, 0);
  for (int y = 0; y < Y; ++y)
    for (int x = 0; x < X; ++x) {
      int32_t& l = lbl[(size_t)y * X + x];
      if (y < 1 || x < 1 || y >= Y - 1 || x >= X - 1) l = 1;
      else if (y >= 4 && y < 64 && x >= 900 && x < 1000) l = 2;
      else if (y % 20 < 7 && y % 20 > 1 && x % 60 < 11 && x < 880 && x > 1) l = 3 + ((y / 20) * 15 + x / 60) % (top - 5);
    }
  lbl[(size_t)66 * X + 1050] = top;                                       // one pixel
  int bad = 0;
  for (int dtype = 0; dtype < 3; ++dtype) {
    const int C = dtype == 0 ? 3 : 1;
    const size_t n = (size_t)Y * X * C;
    if (dtype == 0) {
      std::vector<uint8_t> a(n);
      for (size_t i = 0; i < n; ++i) a[i] = (uint8_t)((i * 7) ^ (i >> 5));
      bad += check<uint8_t>(lbl, Y, X, top, a, 0, C);
    } else if (dtype == 1) {
      std::vector<uint16_t> a(n);
      for (size_t i = 0; i < n; ++i) a[i] = (uint16_t)(i * 977 + (i >> 3));
      bad += check<uint16_t>(lbl, Y, X, top, a, 1, C);
    } else {
      std::vector<float> a(n);
      for (size_t i = 0; i < n; ++i) a[i] = (float)((int)((i * 2654435761u) % 2001u) - 1000) / 64.f * (i % 17 == 0 ? 1e20f : 1.f);
      int seen3 = 0, seen4 = 0;
      for (size_t p = 0; p < (size_t)Y * X; ++p) {
        if (lbl[p] == 3 && seen3++ == 5) a[p] = NAN;
        if (lbl[p] == 4 && (seen4++ % 9) == 2 && seen4 < 20) a[p] = INFINITY;
        if (lbl[p] == 1 && p == 17) a[p] = -INFINITY;
      }
      bad += check<float>(lbl, Y, X, top, a, 2, C);
    }
  }
  return bad ? 1 : 0;
}
#endif
