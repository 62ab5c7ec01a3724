// Host harness of stardist_amd/csrc/measure_shape.h: what csrc/measure_shape.hip does -- label tiles with a halo of 2, border bits with
// a halo of 1, the packed counters of every pixel added over runs of equal labels in a row of 64, the moment products in box-local
// coordinates -- with plain loops in place of threads.  The tiles (and the pixels of the moment pass) are visited forwards or
// backwards: the tables are integer sums and must not depend on it.  Built by tests/test_cpu_measure_shape.py (g++) as a shared
// library; with -DMEASURE_SHAPE_CHECK_MAIN it is a stand-alone program (for a sanitizer build) that runs a small scene both ways.
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../stardist_amd/csrc/measure_shape.h"

using namespace measure_shape;

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

}  // namespace

extern "C" {

int msh_tile_y() { return MSH_TILE_Y; }
int msh_tile_x() { return MSH_TILE_X; }
int msh_halo() { return MSH_HALO; }

// the table of sd_label_moment_sums_device; backwards: the pixels are visited from the last to the first
int msh_moment_sums(const int32_t* lbl, int Z, int Y, int X, int max_label, int64_t* m2, int backwards) {
  if (!lbl || !m2 || Z <= 0 || Y <= 0 || X <= 0 || max_label < 0) return -1;
  std::vector<int32_t> boxes(6 * ((size_t)max_label + 1));
  boxes_of(lbl, Z, Y, X, max_label, boxes.data());
  memset(m2, 0, 6 * ((size_t)max_label + 1) * sizeof(int64_t));
  const long long n = (long long)Z * Y * X;
  for (long long k = 0; k < n; ++k) {
    const long long i = backwards ? n - 1 - k : k;
    const int v = lbl[i];
    if (v < 1 || v > max_label) continue;
    int z0, y0, x0;
    box_start(boxes.data() + 6ll * v, Z, Y, X, &z0, &y0, &x0);
    const long long row = i / X, x = i - row * X, y = row % Y, z = row / Y;
    long long t[6];
    moment_terms(Z > 1 ? z - z0 : 0, y - y0, x - x0, t);
    for (int f = 0; f < 6; ++f) m2[6ll * v + f] += t[f];
  }
  return 0;
}

// the table of sd_label_contour_counts_device; backwards: the tiles are visited from the last to the first
int msh_contour_counts(const int32_t* lbl, int Y, int X, int max_label, int64_t* counts, int backwards) {
  if (!lbl || !counts || Y <= 0 || X <= 0 || max_label < 0) return -1;
  memset(counts, 0, (size_t)MSH_COUNTS * ((size_t)max_label + 1) * sizeof(int64_t));
  std::vector<int32_t> tile(MSH_LY * MSH_LX);
  std::vector<uint8_t> border(MSH_BY * MSH_BX);
  const int tiles_x = (X + MSH_TILE_X - 1) / MSH_TILE_X;
  const long long tiles = (long long)tiles_x * ((Y + MSH_TILE_Y - 1) / MSH_TILE_Y);
  for (long long k = 0; k < tiles; ++k) {
    const long long t = backwards ? tiles - 1 - k : k;
    const long long y0 = (t / tiles_x) * MSH_TILE_Y, x0 = (t % tiles_x) * MSH_TILE_X;
    for (int i = 0; i < MSH_LY * MSH_LX; ++i) {
      const int ly = i / MSH_LX, lx = i - ly * MSH_LX;
      tile[i] = tile_label(lbl, Y, X, max_label, 0, y0 + ly - MSH_HALO, x0 + lx - MSH_HALO);
    }
    for (int i = 0; i < MSH_BY * MSH_BX; ++i) {
      const int by = i / MSH_BX, bx = i - by * MSH_BX;
      border[i] = (uint8_t)border_bit(tile.data(), by + 1, bx + 1);
    }
    for (int ty = 0; ty < MSH_TILE_Y && y0 + ty < Y; ++ty) {
      // the packed words of a run of equal labels are added as words, as the lanes of a wave add them, and unpacked at the run's end
      unsigned long long run[MSH_WORDS] = {0, 0, 0};
      int run_label = 0;
      for (int tx = 0; tx <= MSH_TILE_X; ++tx) {
        unsigned long long w[MSH_WORDS] = {0, 0, 0};
        const int L = tx < MSH_TILE_X ? pixel_counts(tile.data(), border.data(), ty, tx, w) : 0;
        if (L != run_label || tx == MSH_TILE_X) {
          if (run_label)
            for (int f = 0; f < MSH_COUNTS; ++f) counts[(long long)MSH_COUNTS * run_label + f] += get_field(run, f);
          run[0] = run[1] = run[2] = 0;
          run_label = L;
        }
        for (int f = 0; f < MSH_WORDS; ++f) run[f] += w[f];
      }
    }
  }
  return 0;
}

}  // extern "C"

#ifdef MEASURE_SHAPE_CHECK_MAIN
#include <stdio.h>
// a frame around the whole image, squares with a hole across the tile edges, ids beyond max_label and negative ones; both visiting orders
// must give the same tables, the frame's counts are known in closed form, and sizes around the tile multiples put the halo at the border
int main() {
  int bad = 0;
  for (int dy = -2; dy <= 2; ++dy)
    for (int dx = -2; dx <= 2; ++dx) {
      const int Y = 2 * MSH_TILE_Y + dy, X = 2 * MSH_TILE_X + dx, top = 40;
      std::vector<int32_t> lbl((size_t)Y * X, 0);
      for (int y = 0; y < Y; ++y)
        for (int x = 0; x < X; ++x) {
          int32_t& v = lbl[(size_t)y * X + x];
          if (y == 0 || x == 0 || y == Y - 1 || x == X - 1) v = 1;
          else if (y % 11 < 7 && x % 13 < 9 && !(y % 11 == 3 && x % 13 == 4)) v = 2 + ((y / 11) * 10 + x / 13) % 45;   // some beyond top
          else if ((y + x) % 17 == 0) v = -3;
        }
      std::vector<int64_t> a(18 * (size_t)(top + 1)), b(a.size()), ma(6 * (size_t)(top + 1)), mb(ma.size());
      if (msh_contour_counts(lbl.data(), Y, X, top, a.data(), 0) || msh_contour_counts(lbl.data(), Y, X, top, b.data(), 1)) ++bad;
      if (msh_moment_sums(lbl.data(), 1, Y, X, top, ma.data(), 0) || msh_moment_sums(lbl.data(), 1, Y, X, top, mb.data(), 1)) ++bad;
      if (a != b || ma != mb) ++bad;
      // the frame, one pixel wide: its four corners have two border neighbours along the axes (n_1), so has every other pixel
      const long long frame = 2ll * X + 2ll * (Y - 2);
      if (a[18 + MSH_N1] != frame || a[18 + MSH_NR2] != 0 || a[18 + MSH_NH] != 0) ++bad;
      long long xx = 0;
      for (int x = 0; x < X; ++x) xx += 2ll * x * x;
      xx += (long long)(Y - 2) * (X - 1) * (X - 1);
      if (ma[6 + 5] != xx || ma[6 + 0] != 0) ++bad;
      for (int f = 0; f < 18; ++f) if (a[f] != 0) ++bad;                 // row 0
    }
  // a volume through the 3D moment path
  {
    const int Z = 3, Y = 5, X = 7;
    std::vector<int32_t> lbl((size_t)Z * Y * X, 2);
    std::vector<int64_t> m(6 * 3), r(6 * 3);
    if (msh_moment_sums(lbl.data(), Z, Y, X, 2, m.data(), 0) || msh_moment_sums(lbl.data(), Z, Y, X, 2, r.data(), 1) || m != r) ++bad;
    if (m[12] != (0 + 1 + 4) * 35 || m[12 + 5] != (1 + 4 + 9 + 16 + 25 + 36) * 15) ++bad;
  }
  printf("measure_shape harness: %s\n", bad ? "WRONG" : "ok");
  return bad ? 1 : 0;
}
#endif
