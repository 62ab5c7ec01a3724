// Host harness of stardist_amd/csrc/measure.h: what csrc/measure.hip does -- boxes, chunks, per-lane sums over the flattened index,
// the cross-lane tree, the chunk order -- with plain loops in place of threads.  Built by tests/test_cpu_measure.py (g++) as a shared
// library; with -DMEASURE_CHECK_MAIN it is a stand-alone program (for a sanitizer build) that runs a small scene of every image type.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../stardist_amd/csrc/measure.h"

using namespace measure;

namespace {

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

template <typename T, typename A, typename M>
void stats(const int32_t* lbl, int Z, int Y, int X, int max_label, const T* img, int C, A* sums, M* minmax, int* chunks_max) {
  std::vector<int32_t> boxes(6 * ((size_t)max_label + 1));
  boxes_of(lbl, Z, Y, X, max_label, boxes.data());
  std::vector<Stat<A, M>> lane(MS_BLOCK_LANES);
  int most = 0;
  for (long long l = 0; l <= max_label; ++l) {
    const Box b = box_of(boxes.data() + 6 * l, Z, Y, X);
    if (b.chunks > most) most = b.chunks;
    for (int c = 0; c < C; ++c) {
      Stat<A, M> total;
      stat_init(total);
      const int lanes = lanes_of(b);
      for (int k = 0; l > 0 && k < b.chunks; ++k) {
        for (int t = 0; t < lanes; ++t) {
          stat_init(lane[t]);
          lane_accumulate<T, A, M>(lane[t], lbl, img, C, c, Y, X, b, k, (int)l, t, lanes);
        }
        reduce_lanes(lane.data(), lanes);
        if (k == 0) total = lane[0];
        else stat_merge(total, lane[0]);
      }
      stat_store(total, sums, minmax, l, C, c);
    }
  }
  if (chunks_max) *chunks_max = most;
}

}  // namespace

extern "C" {

int ms_chunk_pixels() { return MS_CHUNK_PIXELS; }
int ms_wave_pixels() { return MS_WAVE_PIXELS; }

// the tables of sd_label_intensity_stats_device, sentinel rows included; chunks_max (optional) = the most chunks a box was cut into
int ms_stats(const int32_t* lbl, int Z, int Y, int X, int max_label, const void* img, int dtype, int C, int64_t* isum2, double* fsum2,
             void* minmax, int* chunks_max) {
  if (!lbl || !img || !minmax || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0 || dtype < 0 || dtype > 2 || C < 1) return -1;
  if (dtype == 2 ? !fsum2 : !isum2) return -1;
  if (dtype == 0) stats<uint8_t, int64_t, int32_t>(lbl, Z, Y, X, max_label, (const uint8_t*)img, C, isum2, (int32_t*)minmax, chunks_max);
  else if (dtype == 1) stats<uint16_t, int64_t, int32_t>(lbl, Z, Y, X, max_label, (const uint16_t*)img, C, isum2, (int32_t*)minmax, chunks_max);
  else stats<float, double, float>(lbl, Z, Y, X, max_label, (const float*)img, C, fsum2, (float*)minmax, chunks_max);
  return 0;
}

}  // extern "C"

#ifdef MEASURE_CHECK_MAIN
#include <stdio.h>
// a frame around the whole image (several chunks, a partial last one), small squares inside it, three image types
int main() {
  const int Y = 300, X = 523, top = 40;
  std::vector<int32_t> lbl((size_t)Y * X, 0);
  for (int y = 0; y < Y; ++y)
    for (int x = 0; x < X; ++x) {
      if (y < 2 || x < 2 || y >= Y - 2 || x >= X - 2) lbl[(size_t)y * X + x] = 1;
      else if (y % 40 < 9 && x % 70 < 13) lbl[(size_t)y * X + x] = 2 + ((y / 40) * 8 + x / 70) % (top - 2);
    }
  int bad = 0;
  for (int dtype = 0; dtype < 3; ++dtype) {
    const int C = dtype == 0 ? 3 : 1;
    const size_t n = (size_t)Y * X * C;
    std::vector<uint8_t> a(n);
    std::vector<uint16_t> b(n);
    std::vector<float> f(n);
    for (size_t i = 0; i < n; ++i) { a[i] = (uint8_t)(i * 7); b[i] = (uint16_t)(i * 977); f[i] = (float)((int)(i % 2001) - 1000) / 64.f; }
    std::vector<int64_t> is(2 * (size_t)(top + 1) * C);
    std::vector<double> fs(2 * (size_t)(top + 1) * C);
    std::vector<int32_t> mm(2 * (size_t)(top + 1) * C);
    int chunks = 0;
    const void* img = dtype == 0 ? (const void*)a.data() : dtype == 1 ? (const void*)b.data() : (const void*)f.data();
    if (ms_stats(lbl.data(), 1, Y, X, top, img, dtype, C, is.data(), fs.data(), mm.data(), &chunks)) ++bad;
    // plain sums of the frame: every partial sum of these values is exact, so any order gives the same bits
    double want_f = 0; long long want_i = 0;
    for (size_t p = 0; p < (size_t)Y * X; ++p)
      if (lbl[p] == 1) { want_f += f[p * C]; want_i += dtype == 0 ? a[p * C] : b[p * C]; }
    if (dtype == 2 ? fs[2 * C] != want_f : is[2 * C] != want_i) ++bad;
    if (chunks < 3) ++bad;
    printf("dtype %d: %d chunks, frame sum %s\n", dtype, chunks, bad ? "WRONG" : "ok");
  }
  return bad ? 1 : 0;
}
#endif
