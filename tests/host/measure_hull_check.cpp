// Host harness of stardist_amd/csrc/measure_hull.h: what csrc/measure_hull.hip does -- a row table of (first, last) columns per object
// row from one pass over the pixels, then per object the two chains of the hull, the convex image's intervals with the rows dealt to 64
// lanes, the chains of the intervals' hull and the largest squared distance with the vertices dealt to the lanes -- with plain loops in
// place of threads.  The pixels, the objects and the lanes are visited forwards or backwards: the table is made of integer minima,
// maxima and sums and must not depend on it.  Every per-object array is allocated at exactly the size the header promises to stay
// within.  Built by tests/test_cpu_measure_hull.py (g++) as a shared library; with -DMEASURE_HULL_CHECK_MAIN it is a stand-alone
// program (for a sanitizer build) that runs a small scene both ways.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../stardist_amd/csrc/measure_hull.h"

using namespace measure_hull;

namespace {

enum { LANES = 64 };

void boxes_of(const int32_t* lbl, int Y, int X, int max_label, int32_t* boxes) {
  for (long long i = 0; i < 6ll * (max_label + 1ll); ++i) boxes[i] = (i % 6) < 3 ? INT_MAX : 0;
  for (int y = 0; y < Y; ++y)
    for (int x = 0; x < X; ++x) {
      const int l = lbl[(long long)y * X + x];
      if (l <= 0 || l > max_label) continue;
      int32_t* t = boxes + 6ll * l;
      t[0] = 0;
      t[3] = 1;
      if (y < t[1]) t[1] = y;
      if (x < t[2]) t[2] = x;
      if (y + 1 > t[4]) t[4] = y + 1;
      if (x + 1 > t[5]) t[5] = x + 1;
    }
}

}  // namespace

extern "C" {

int mh_lds_rows() { return MH_LDS_ROWS; }
int mh_max_extent() { return MH_MAX_EXTENT; }

// the table of sd_label_hull_device: hull[l] = {convex_area, F2}; backwards: pixels, objects and lanes are visited from the last to the first
int mh_label_hull(const int32_t* lbl, int Y, int X, int max_label, int64_t* hull, int backwards) {
  if (!lbl || !hull || Y <= 0 || X <= 0 || max_label < 0 || Y >= MH_MAX_EXTENT || X >= MH_MAX_EXTENT) return -1;
  std::vector<int32_t> boxes(6 * ((size_t)max_label + 1));
  boxes_of(lbl, Y, X, max_label, boxes.data());
  std::vector<long long> row_at((size_t)max_label + 2, 0);
  for (int l = 1; l <= max_label; ++l) {
    const int h = boxes[6ll * l + 4] > boxes[6ll * l + 1] ? boxes[6ll * l + 4] - boxes[6ll * l + 1] : 0;
    row_at[l + 1] = row_at[l] + h;
  }
  row_at[1] = 0;
  std::vector<int> rows(2 * (size_t)row_at[(size_t)max_label + 1] + 2);
  for (size_t i = 0; i + 1 < rows.size(); i += 2) { rows[i] = INT_MAX; rows[i + 1] = INT_MIN; }
  const long long n = (long long)Y * X;
  for (long long k = 0; k < n; ++k) {
    const long long i = backwards ? n - 1 - k : k;
    const int v = lbl[i];
    if (v < 1 || v > max_label) continue;
    const long long y = i / X;
    const int x = (int)(i - y * X);
    const bool starts = run_edge(v, x > 0, x > 0 ? lbl[i - 1] : 0), ends = run_edge(v, x + 1 < X, x + 1 < X ? lbl[i + 1] : 0);
    int* slot = rows.data() + 2 * (row_at[v] + (y - boxes[6ll * v + 1]));
    if (starts && x < slot[0]) slot[0] = x;
    if (ends && x > slot[1]) slot[1] = x;
  }
  memset(hull, 0, 2 * ((size_t)max_label + 1) * sizeof(int64_t));
  for (int k = 1; k <= max_label; ++k) {
    const int l = backwards ? max_label + 1 - k : k;
    const int h = (int)(row_at[l + 1] - row_at[l]);
    if (h <= 0) continue;
    const int y0 = boxes[6ll * l + 1];
    const std::vector<int> ext(rows.begin() + 2 * row_at[l], rows.begin() + 2 * row_at[l + 1]);
    std::vector<int> iv(2 * (size_t)h);
    std::vector<Pt> left((size_t)level_count(h)), right((size_t)level_count(h));
    int nl = build_chain(ext.data(), h, y0, -1, left.data()), nr = build_chain(ext.data(), h, y0, 1, right.data());
    long long area = 0, far = 0;
    for (int t = 0; t < LANES; ++t) area += intervals_of(left.data(), nl, right.data(), nr, h, y0, iv.data(), backwards ? LANES - 1 - t : t, LANES);
    nl = build_chain(iv.data(), h, y0, -1, left.data());
    nr = build_chain(iv.data(), h, y0, 1, right.data());
    for (int t = 0; t < LANES; ++t) {
      const long long d = far_pairs(left.data(), nl, right.data(), nr, backwards ? LANES - 1 - t : t, LANES);
      if (d > far) far = d;
    }
    hull[2ll * l] = area;
    hull[2ll * l + 1] = far;
  }
  return 0;
}

}  // extern "C"

#ifdef MEASURE_HULL_CHECK_MAIN
#include <stdio.h>
// a rectangle and a column as tall as the image (closed forms: convex_area = h w, F2 = the larger of (2 h)^2 + (2 w - 2)^2 and
// (2 h - 2)^2 + (2 w)^2), a one-pixel diagonal of n (convex_area = n, F2 = (2 n)^2 + (2 n - 2)^2), single pixels in the corners, a
// label in two parts taller than the LDS tier, ids beyond max_label and negative ones; both visiting orders must give the same table
int main() {
  int bad = 0;
  const int Y = 2 * MH_LDS_ROWS + 13, X = 97, top = 40;
  std::vector<int32_t> lbl((size_t)Y * X, 0);
  auto at = [&](int y, int x) -> int32_t& { return lbl[(size_t)y * X + x]; };
  for (int y = 3; y < 10; ++y)
    for (int x = 5; x < 16; ++x) at(y, x) = 1;                                  // 7 x 11
  for (int k = 0; k < 30; ++k) at(20 + k, 40 + k) = 2;                          // a diagonal of 30
  at(0, 0) = 3; at(0, X - 1) = 4; at(Y - 1, 0) = 5; at(Y - 1, X - 1) = 6;       // corners
  at(1, 60) = 7; at(Y - 2, 70) = 7;                                             // two pixels, Y - 2 rows: beyond the LDS tier
  for (int y = 0; y < Y; ++y) at(y, 90) = 8;                                    // a column as tall as the image
  for (int y = 60; y < 70; ++y)
    for (int x = 20; x < 30; ++x) at(y, x) = (x + y) % 3 ? 45 : -2;             // beyond top, negative
  std::vector<int64_t> a(2 * (size_t)(top + 1), -1), b(a.size(), -2);
  if (mh_label_hull(lbl.data(), Y, X, top, a.data(), 0) || mh_label_hull(lbl.data(), Y, X, top, b.data(), 1)) ++bad;
  if (a != b) ++bad;
  auto rect = [](long long h, long long w) { const long long p = 2 * h, q = 2 * w - 2, r = 2 * h - 2, s = 2 * w; return p * p + q * q > r * r + s * s ? p * p + q * q : r * r + s * s; };
  if (a[2] != 77 || a[3] != rect(7, 11)) ++bad;
  if (a[4] != 30 || a[5] != 2ll * 58 * 58 + 4 * 58 + 4) ++bad;                   // (2 n - 2 + 2)^2 + (2 n - 2)^2 with n = 30: 60^2 + 58^2
  for (int l = 3; l <= 6; ++l) if (a[2 * l] != 1 || a[2 * l + 1] != 4) ++bad;
  if (a[16] != Y || a[17] != rect(Y, 1)) ++bad;
  if (a[14] < 2 || a[15] <= 4ll * (Y - 3) * (Y - 3)) ++bad;
  if (a[0] != 0 || a[1] != 0 || a[2 * 9] != 0 || a[2 * top] != 0) ++bad;
  if (mh_label_hull(nullptr, 4, 4, 1, a.data(), 0) != -1 || mh_label_hull(lbl.data(), MH_MAX_EXTENT, 1, 1, a.data(), 0) != -1) ++bad;
  printf("measure_hull harness: %s\n", bad ? "WRONG" : "ok");
  return bad ? 1 : 0;
}
#endif
